# tests/cpp/loads.mk -- CPU-side test harness (never part of the product): the host side of the loads (csrc/loads.cpp) and of
# their hooks in the step calls of the batches (csrc/batch.cpp) and of the contexts (csrc/slab_step.cpp), run through on the
# CPU over the runtime that lives on the host (fake_hip.cpp) and kernels that do nothing (launch_stubs_ok.cpp), with launchers
# of csrc/batch.h, of the solids, of the histories and of the loads that log what they are handed, in stream order
# (loads_driver.cpp).  A plain build: no sanitizer.
#   make -C tests/cpp -f loads.mk && tests/cpp/loads_driver
# (the driver brings the real small_grid_fits and logging launchers of its own for three of the stubs, which are renamed)
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(HERE)../../esp32-fluid-simulation_amd/csrc
CXX  ?= g++
INC  := $(HERE)../../include

HOST_SRCS := context.cpp transport.cpp sor_executor.cpp operators.cpp slab_step.cpp host_dropin.cpp slab_plan.cpp batch.cpp batch_frames.cpp \
             solve_until.cpp flow_stats.cpp history.cpp views.cpp solids.cpp context_solids.cpp loads.cpp
CXXFLAGS_ := -std=c++17 -O1 -g -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$(CSRC) -Wall -Wno-unused-parameter -Wno-unknown-pragmas
RENAMED   := small_grid_fits launch_advect_vec2f launch_advect_divergence_tiled launch_step_seam_tiled
OBJS := $(patsubst %.cpp,$(HERE)lo_%.o,$(HOST_SRCS)) $(HERE)lo_stubs.o $(HERE)lo_fake_hip.o $(HERE)lo_driver.o

all: $(HERE)loads_driver
$(HERE)lo_%.o: $(CSRC)/%.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)lo_stubs.o: $(HERE)launch_stubs_ok.cpp $(CSRC)/kernels.h
	$(CXX) $(CXXFLAGS_) $(foreach f,$(RENAMED),-D$(f)=$(f)_of_the_stubs) -c -o $@ $<
$(HERE)lo_fake_hip.o: $(HERE)fake_hip.cpp
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)lo_driver.o: $(HERE)loads_driver.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)loads_driver: $(OBJS)
	$(CXX) -o $@ $(OBJS) -lpthread

clean:
	rm -f $(HERE)lo_*.o $(HERE)loads_driver
