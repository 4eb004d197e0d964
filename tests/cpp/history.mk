# tests/cpp/history.mk -- CPU-side test harness (never part of the product): the host side of sfl_history_* and
# sfl_batch_history_* (csrc/history.cpp) and their hooks in the step calls (csrc/slab_step.cpp, csrc/batch.cpp), run through on
# the CPU under AddressSanitizer + UBSan over the runtime that lives on the host (fake_hip.cpp) and kernels that do nothing
# (launch_stubs_ok.cpp), with launchers of csrc/history_kernels.h, of the batches' steps, of the recorder's render, of the
# streaming passes a context's sample is made of and of the two kernels that end a context's step that log what they are
# handed, in stream order (history_driver.cpp); and the record's layout as a C compiler sees it (history_layout.c).
#   make -C tests/cpp -f history.mk && tests/cpp/history_driver && tests/cpp/history_layout
# (launch_stubs_ok.cpp's small_grid_fits says "no" to every shape and its two step-ending launchers keep no log; the driver
# brings its own, so the stubs' are renamed)
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(HERE)../../esp32-fluid-simulation_amd/csrc
CXX  ?= g++
CC   ?= gcc
INC  := $(HERE)../../include

HOST_SRCS := context.cpp transport.cpp sor_executor.cpp operators.cpp slab_step.cpp host_dropin.cpp slab_plan.cpp batch.cpp batch_frames.cpp history.cpp
SANFLAGS  := -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
             -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$(CSRC) -Wall -Wno-unused-parameter
RENAMED   := small_grid_fits launch_project_advect_vec3uq32 launch_step_seam_tiled
OBJS := $(patsubst %.cpp,$(HERE)hi_%.o,$(HOST_SRCS)) $(HERE)hi_stubs.o $(HERE)hi_fake_hip.o $(HERE)hi_driver.o

all: $(HERE)history_driver $(HERE)history_layout
$(HERE)hi_%.o: $(CSRC)/%.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(SANFLAGS) -c -o $@ $<
$(HERE)hi_stubs.o: $(HERE)launch_stubs_ok.cpp $(CSRC)/kernels.h
	$(CXX) $(SANFLAGS) $(foreach f,$(RENAMED),-D$(f)=$(f)_of_the_stubs) -c -o $@ $<
$(HERE)hi_fake_hip.o: $(HERE)fake_hip.cpp
	$(CXX) $(SANFLAGS) -c -o $@ $<
$(HERE)hi_driver.o: $(HERE)history_driver.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(SANFLAGS) -c -o $@ $<
$(HERE)history_driver: $(OBJS)
	$(CXX) -fsanitize=address,undefined -o $@ $(OBJS) -lpthread
$(HERE)history_layout: $(HERE)history_layout.c $(INC)/sfl.h
	$(CC) -std=c99 -Wall -Werror -I$(INC) -o $@ $<

clean:
	rm -f $(HERE)hi_*.o $(HERE)history_driver $(HERE)history_layout
