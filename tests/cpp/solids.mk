# tests/cpp/solids.mk -- CPU-side test harness (never part of the product): the host side of sfl_batch_set_solids and its
# companions (csrc/solids.cpp) and of their hooks in the step, solve and statistics calls (csrc/batch.cpp), the history's start
# (csrc/history.cpp) and the views (csrc/views.cpp), run through on the CPU over the runtime that lives on the host
# (fake_hip.cpp) and kernels that do nothing (launch_stubs_ok.cpp), with launchers of csrc/batch.h, of the statistics, the
# history's sample and the views that log what they are handed, in stream order (solids_driver.cpp).  A plain build: no sanitizer.
#   make -C tests/cpp -f solids.mk && tests/cpp/solids_driver
# (launch_stubs_ok.cpp's small_grid_fits says "no" to every shape; the driver brings the real rule, so the stub is renamed)
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(HERE)../../esp32-fluid-simulation_amd/csrc
CXX  ?= g++
INC  := $(HERE)../../include

HOST_SRCS := context.cpp transport.cpp sor_executor.cpp operators.cpp slab_step.cpp host_dropin.cpp slab_plan.cpp batch.cpp batch_frames.cpp history.cpp views.cpp solids.cpp
CXXFLAGS_ := -std=c++17 -O1 -g -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$(CSRC) -Wall -Wno-unused-parameter
RENAMED   := small_grid_fits
OBJS := $(patsubst %.cpp,$(HERE)so_%.o,$(HOST_SRCS)) $(HERE)so_stubs.o $(HERE)so_fake_hip.o $(HERE)so_driver.o

all: $(HERE)solids_driver
$(HERE)so_%.o: $(CSRC)/%.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)so_stubs.o: $(HERE)launch_stubs_ok.cpp $(CSRC)/kernels.h
	$(CXX) $(CXXFLAGS_) $(foreach f,$(RENAMED),-D$(f)=$(f)_of_the_stubs) -c -o $@ $<
$(HERE)so_fake_hip.o: $(HERE)fake_hip.cpp
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)so_driver.o: $(HERE)solids_driver.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)solids_driver: $(OBJS)
	$(CXX) -o $@ $(OBJS) -lpthread

clean:
	rm -f $(HERE)so_*.o $(HERE)solids_driver
