# tests/cpp/context_solids.mk -- CPU-side test harness (never part of the product): the host side of sfl_set_solids and its
# companions (csrc/context_solids.cpp) and of their hooks in the step (csrc/slab_step.cpp), the operators (csrc/operators.cpp),
# the solves and the update norm (csrc/solve_until.cpp), the statistics (csrc/flow_stats.cpp), the history's sample
# (csrc/history.cpp), the views (csrc/views.cpp) and the transports (csrc/transport.cpp), run through on the CPU over the
# runtime that lives on the host (fake_hip.cpp) and kernels that do nothing (launch_stubs_ok.cpp), with launchers that log
# what they are handed, in stream order; and the tile core of the masked solve (csrc/sor_solid_tile.h) run on the host, one
# workgroup's tile after the other (context_solids_driver.cpp).  A plain build: no sanitizer.
#   make -C tests/cpp -f context_solids.mk && tests/cpp/context_solids_driver
# (the driver brings the real small_grid_fits and logging launchers of its own, so the stubs' are renamed)
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(HERE)../../esp32-fluid-simulation_amd/csrc
CXX  ?= g++
INC  := $(HERE)../../include

HOST_SRCS := context.cpp transport.cpp sor_executor.cpp operators.cpp slab_step.cpp host_dropin.cpp slab_plan.cpp batch.cpp batch_frames.cpp \
             solve_until.cpp flow_stats.cpp history.cpp views.cpp solids.cpp context_solids.cpp
CXXFLAGS_ := -std=c++17 -O1 -g -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$(CSRC) -Wall -Wno-unused-parameter -Wno-unknown-pragmas
RENAMED   := small_grid_fits launch_advect_vec2f launch_advect_vec3uq32 launch_advect_divergence_tiled launch_project_advect_vec3uq32 \
             launch_step_seam_tiled launch_apply_forces launch_divergence launch_subtract_gradient launch_sor_half_sweep launch_sor_fused \
             launch_zero_rows launch_small_step launch_small_solve
OBJS := $(patsubst %.cpp,$(HERE)cs_%.o,$(HOST_SRCS)) $(HERE)cs_stubs.o $(HERE)cs_fake_hip.o $(HERE)cs_driver.o

all: $(HERE)context_solids_driver
$(HERE)cs_%.o: $(CSRC)/%.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)cs_stubs.o: $(HERE)launch_stubs_ok.cpp $(CSRC)/kernels.h
	$(CXX) $(CXXFLAGS_) $(foreach f,$(RENAMED),-D$(f)=$(f)_of_the_stubs) -c -o $@ $<
$(HERE)cs_fake_hip.o: $(HERE)fake_hip.cpp
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)cs_driver.o: $(HERE)context_solids_driver.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)context_solids_driver: $(OBJS)
	$(CXX) -o $@ $(OBJS) -lpthread

clean:
	rm -f $(HERE)cs_*.o $(HERE)context_solids_driver
