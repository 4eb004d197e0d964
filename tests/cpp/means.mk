# tests/cpp/means.mk -- CPU-side test harness (never part of the product): the host side of the averages (csrc/means.cpp) and
# of its hooks in the step calls of the batches (csrc/batch.cpp) and of the contexts (csrc/slab_step.cpp), beside the
# histories, the loads and the friction, run through on the CPU over the runtime that lives on the host (fake_hip.cpp) and
# kernels that do nothing (launch_stubs_ok.cpp), with launchers of csrc/batch.h, of the solids, of the histories, of the loads,
# of the friction and of the averages that log what they are handed, in stream order (means_driver.cpp).
#   make -C tests/cpp -f means.mk && tests/cpp/means_driver              (a plain build)
#   make -C tests/cpp -f means.mk san && tests/cpp/means_driver_san      (the same stand-alone program under ASan + UBSan)
# (the driver brings the real small_grid_fits and logging launchers of its own for three of the stubs, which are renamed)
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(HERE)../../esp32-fluid-simulation_amd/csrc
CXX  ?= g++
INC  := $(HERE)../../include

HOST_SRCS := context.cpp transport.cpp sor_executor.cpp operators.cpp slab_step.cpp host_dropin.cpp slab_plan.cpp batch.cpp batch_frames.cpp \
             solve_until.cpp flow_stats.cpp history.cpp views.cpp solids.cpp context_solids.cpp loads.cpp friction.cpp means.cpp
CXXFLAGS_ := -std=c++17 -O1 -g -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$(CSRC) -Wall -Wno-unused-parameter -Wno-unknown-pragmas
SANFLAGS_ := -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer
RENAMED   := small_grid_fits launch_advect_vec2f launch_advect_divergence_tiled launch_step_seam_tiled
OBJS     := $(patsubst %.cpp,$(HERE)mn_%.o,$(HOST_SRCS)) $(HERE)mn_stubs.o $(HERE)mn_fake_hip.o $(HERE)mn_driver.o
SAN_OBJS := $(patsubst %.cpp,$(HERE)mnsan_%.o,$(HOST_SRCS)) $(HERE)mnsan_stubs.o $(HERE)mnsan_fake_hip.o $(HERE)mnsan_driver.o

all: $(HERE)means_driver
san: $(HERE)means_driver_san
$(HERE)mn_%.o: $(CSRC)/%.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)mn_stubs.o: $(HERE)launch_stubs_ok.cpp $(CSRC)/kernels.h
	$(CXX) $(CXXFLAGS_) $(foreach f,$(RENAMED),-D$(f)=$(f)_of_the_stubs) -c -o $@ $<
$(HERE)mn_fake_hip.o: $(HERE)fake_hip.cpp
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)mn_driver.o: $(HERE)means_driver.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)means_driver: $(OBJS)
	$(CXX) -o $@ $(OBJS) -lpthread

$(HERE)mnsan_%.o: $(CSRC)/%.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) $(SANFLAGS_) -c -o $@ $<
$(HERE)mnsan_stubs.o: $(HERE)launch_stubs_ok.cpp $(CSRC)/kernels.h
	$(CXX) $(CXXFLAGS_) $(SANFLAGS_) $(foreach f,$(RENAMED),-D$(f)=$(f)_of_the_stubs) -c -o $@ $<
$(HERE)mnsan_fake_hip.o: $(HERE)fake_hip.cpp
	$(CXX) $(CXXFLAGS_) $(SANFLAGS_) -c -o $@ $<
$(HERE)mnsan_driver.o: $(HERE)means_driver.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) $(SANFLAGS_) -c -o $@ $<
$(HERE)means_driver_san: $(SAN_OBJS)
	$(CXX) $(SANFLAGS_) -o $@ $(SAN_OBJS) -lpthread

clean:
	rm -f $(HERE)mn_*.o $(HERE)mnsan_*.o $(HERE)means_driver $(HERE)means_driver_san
