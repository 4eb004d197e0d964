# tests/cpp/walls.mk -- CPU-side test harness (never part of the product): the host side of the wall velocities
# (csrc/walls.cpp, csrc/context_walls.cpp, csrc/wall_table.h) and of their hooks in the step calls and in sfl_[batch_]set_solids,
# beside the viscosity's and the openings' units,
# run through on the CPU over the runtime that lives on the host (fake_hip.cpp) and kernels that do nothing
# (launch_stubs_ok.cpp), with launchers that log what they are handed (walls_driver.cpp).
#   make -C tests/cpp -f walls.mk && tests/cpp/walls_driver              (a plain build)
#   make -C tests/cpp -f walls.mk san && tests/cpp/walls_driver_san      (the same stand-alone program under ASan + UBSan)
# (the stubs the driver replaces with logging ones are renamed in launch_stubs_ok.cpp)
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(HERE)../../esp32-fluid-simulation_amd/csrc
CXX  ?= g++
INC  := $(HERE)../../include

HOST_SRCS := context.cpp transport.cpp sor_executor.cpp operators.cpp slab_step.cpp host_dropin.cpp slab_plan.cpp batch.cpp batch_frames.cpp \
             solve_until.cpp flow_stats.cpp history.cpp views.cpp solids.cpp context_solids.cpp context_viscous.cpp viscous.cpp openings.cpp inflow.cpp context_openings.cpp walls.cpp context_walls.cpp
CXXFLAGS_ := -std=c++17 -O1 -g -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$(CSRC) -Wall -Wno-unused-parameter -Wno-unknown-pragmas
SANFLAGS_ := -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer
RENAMED   := small_grid_fits launch_advect_vec2f launch_advect_vec3uq32 launch_advect_divergence_tiled launch_project_advect_vec3uq32 \
             launch_step_seam_tiled launch_apply_forces launch_divergence launch_subtract_gradient launch_sor_half_sweep launch_sor_fused \
             launch_zero_rows launch_small_step launch_small_solve
OBJS     := $(patsubst %.cpp,$(HERE)wl_%.o,$(HOST_SRCS)) $(HERE)wl_stubs.o $(HERE)wl_fake_hip.o $(HERE)wl_driver.o
SAN_OBJS := $(patsubst %.cpp,$(HERE)wlsan_%.o,$(HOST_SRCS)) $(HERE)wlsan_stubs.o $(HERE)wlsan_fake_hip.o $(HERE)wlsan_driver.o

all: $(HERE)walls_driver
san: $(HERE)walls_driver_san

$(HERE)wl_%.o: $(CSRC)/%.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)wl_stubs.o: $(HERE)launch_stubs_ok.cpp $(CSRC)/kernels.h
	$(CXX) $(CXXFLAGS_) $(foreach f,$(RENAMED),-D$(f)=$(f)_of_the_stubs) -c -o $@ $<
$(HERE)wl_fake_hip.o: $(HERE)fake_hip.cpp
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)wl_driver.o: $(HERE)walls_driver.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)walls_driver: $(OBJS)
	$(CXX) -o $@ $(OBJS) -lpthread

$(HERE)wlsan_%.o: $(CSRC)/%.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) $(SANFLAGS_) -c -o $@ $<
$(HERE)wlsan_stubs.o: $(HERE)launch_stubs_ok.cpp $(CSRC)/kernels.h
	$(CXX) $(CXXFLAGS_) $(SANFLAGS_) $(foreach f,$(RENAMED),-D$(f)=$(f)_of_the_stubs) -c -o $@ $<
$(HERE)wlsan_fake_hip.o: $(HERE)fake_hip.cpp
	$(CXX) $(CXXFLAGS_) $(SANFLAGS_) -c -o $@ $<
$(HERE)wlsan_driver.o: $(HERE)walls_driver.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) $(SANFLAGS_) -c -o $@ $<
$(HERE)walls_driver_san: $(SAN_OBJS)
	$(CXX) -fsanitize=address,undefined -o $@ $(SAN_OBJS) -lpthread

clean:
	rm -f $(HERE)wl_*.o $(HERE)wlsan_*.o $(HERE)walls_driver $(HERE)walls_driver_san
