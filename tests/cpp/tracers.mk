# tests/cpp/tracers.mk -- CPU-side test harness (never part of the product): the host side of sfl_tracers_* and
# sfl_batch_tracers_* (csrc/tracers.cpp) and their hook in the step calls (csrc/slab_step.cpp, csrc/batch.cpp), run through
# on the CPU under AddressSanitizer + UBSan over the runtime that lives on the host (fake_hip.cpp) and kernels that do
# nothing (launch_stubs_ok.cpp), with launchers of csrc/tracer_kernels.h, of the batches' steps and of the two kernels that
# end a context's step that log what they are handed, in stream order (tracers_driver.cpp).
#   make -C tests/cpp -f tracers.mk && tests/cpp/tracers_driver
# (launch_stubs_ok.cpp's small_grid_fits says "no" to every shape and its two step-ending launchers keep no log; the driver
# brings its own, so the stubs' are renamed)
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(HERE)../../esp32-fluid-simulation_amd/csrc
CXX  ?= g++
INC  := $(HERE)../../include

HOST_SRCS := context.cpp transport.cpp sor_executor.cpp operators.cpp slab_step.cpp host_dropin.cpp slab_plan.cpp batch.cpp batch_frames.cpp tracers.cpp
SANFLAGS  := -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
             -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$(CSRC) -Wall -Wno-unused-parameter
RENAMED   := small_grid_fits launch_project_advect_vec3uq32 launch_step_seam_tiled
OBJS := $(patsubst %.cpp,$(HERE)tr_%.o,$(HOST_SRCS)) $(HERE)tr_stubs.o $(HERE)tr_fake_hip.o $(HERE)tr_driver.o

all: $(HERE)tracers_driver
$(HERE)tr_%.o: $(CSRC)/%.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(SANFLAGS) -c -o $@ $<
$(HERE)tr_stubs.o: $(HERE)launch_stubs_ok.cpp $(CSRC)/kernels.h
	$(CXX) $(SANFLAGS) $(foreach f,$(RENAMED),-D$(f)=$(f)_of_the_stubs) -c -o $@ $<
$(HERE)tr_fake_hip.o: $(HERE)fake_hip.cpp
	$(CXX) $(SANFLAGS) -c -o $@ $<
$(HERE)tr_driver.o: $(HERE)tracers_driver.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(SANFLAGS) -c -o $@ $<
$(HERE)tracers_driver: $(OBJS)
	$(CXX) -fsanitize=address,undefined -o $@ $(OBJS) -lpthread

clean:
	rm -f $(HERE)tr_*.o $(HERE)tracers_driver
