# tests/cpp/ensemble.mk -- CPU-side test harness (never part of the product): the host side of sfl_distance,
# sfl_batch_distance and sfl_batch_envelope* (csrc/ensemble.cpp), run through on the CPU under AddressSanitizer + UBSan over
# the runtime that lives on the host (fake_hip.cpp) and kernels that do nothing (launch_stubs_ok.cpp), with launchers of
# csrc/ensemble_kernels.h that log the pointers and strides they are handed (ensemble_driver.cpp).
#   make -C tests/cpp -f ensemble.mk && tests/cpp/ensemble_driver
# (launch_stubs_ok.cpp's small_grid_fits says "no" to every shape; the driver brings the real rule, so the stub is renamed)
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(HERE)../../esp32-fluid-simulation_amd/csrc
CXX  ?= g++
INC  := $(HERE)../../include

HOST_SRCS := context.cpp transport.cpp sor_executor.cpp operators.cpp slab_step.cpp host_dropin.cpp slab_plan.cpp batch.cpp batch_frames.cpp ensemble.cpp
SANFLAGS  := -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
             -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$(CSRC) -Wall -Wno-unused-parameter
OBJS := $(patsubst %.cpp,$(HERE)en_%.o,$(HOST_SRCS)) $(HERE)en_stubs.o $(HERE)en_fake_hip.o $(HERE)en_driver.o

all: $(HERE)ensemble_driver
$(HERE)en_%.o: $(CSRC)/%.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(SANFLAGS) -c -o $@ $<
$(HERE)en_stubs.o: $(HERE)launch_stubs_ok.cpp $(CSRC)/kernels.h
	$(CXX) $(SANFLAGS) -Dsmall_grid_fits=small_grid_fits_of_the_stubs -c -o $@ $<
$(HERE)en_fake_hip.o: $(HERE)fake_hip.cpp
	$(CXX) $(SANFLAGS) -c -o $@ $<
$(HERE)en_driver.o: $(HERE)ensemble_driver.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(SANFLAGS) -c -o $@ $<
$(HERE)ensemble_driver: $(OBJS)
	$(CXX) -fsanitize=address,undefined -o $@ $(OBJS) -lpthread

clean:
	rm -f $(HERE)en_*.o $(HERE)ensemble_driver
