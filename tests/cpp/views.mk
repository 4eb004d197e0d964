# tests/cpp/views.mk -- CPU-side test harness (never part of the product): the host side of sfl_view_*, sfl_batch_view_* and
# sfl_batch_record_view (csrc/views.cpp) and their hook in the recorder (csrc/batch_frames.cpp), run through on the CPU under
# AddressSanitizer + UBSan over the runtime that lives on the host (fake_hip.cpp) and kernels that do nothing
# (launch_stubs_ok.cpp), with launchers of csrc/view_kernels.h and of the dye's frames that log what they are handed, in stream
# order (views_driver.cpp).
#   make -C tests/cpp -f views.mk && tests/cpp/views_driver
# (launch_stubs_ok.cpp's small_grid_fits says "no" to every shape; the driver brings the real rule, so the stub is renamed)
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(HERE)../../esp32-fluid-simulation_amd/csrc
CXX  ?= g++
INC  := $(HERE)../../include

HOST_SRCS := context.cpp transport.cpp sor_executor.cpp operators.cpp slab_step.cpp host_dropin.cpp slab_plan.cpp batch.cpp batch_frames.cpp views.cpp
SANFLAGS  := -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
             -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$(CSRC) -Wall -Wno-unused-parameter
RENAMED   := small_grid_fits
OBJS := $(patsubst %.cpp,$(HERE)vw_%.o,$(HOST_SRCS)) $(HERE)vw_stubs.o $(HERE)vw_fake_hip.o $(HERE)vw_driver.o

all: $(HERE)views_driver
$(HERE)vw_%.o: $(CSRC)/%.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(SANFLAGS) -c -o $@ $<
$(HERE)vw_stubs.o: $(HERE)launch_stubs_ok.cpp $(CSRC)/kernels.h
	$(CXX) $(SANFLAGS) $(foreach f,$(RENAMED),-D$(f)=$(f)_of_the_stubs) -c -o $@ $<
$(HERE)vw_fake_hip.o: $(HERE)fake_hip.cpp
	$(CXX) $(SANFLAGS) -c -o $@ $<
$(HERE)vw_driver.o: $(HERE)views_driver.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(SANFLAGS) -c -o $@ $<
$(HERE)views_driver: $(OBJS)
	$(CXX) -fsanitize=address,undefined -o $@ $(OBJS) -lpthread

clean:
	rm -f $(HERE)vw_*.o $(HERE)views_driver
