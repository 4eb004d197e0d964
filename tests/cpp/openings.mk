# tests/cpp/openings.mk -- CPU-side test harness (never part of the product): the host side of sfl_batch_set_openings and its
# companions (csrc/openings.cpp) and of their hooks in the step, solve and statistics calls (csrc/batch.cpp), in
# sfl_batch_set_solids (csrc/solids.cpp), the history's start (csrc/history.cpp), the views (csrc/views.cpp) and
# sfl_batch_set_viscosity (csrc/viscous.cpp), run through on the CPU over the runtime that lives on the host (fake_hip.cpp) and
# kernels that do nothing (launch_stubs_ok.cpp), with launchers that log what they are handed (openings_driver.cpp).
#   make -C tests/cpp -f openings.mk && tests/cpp/openings_driver              (a plain build)
#   make -C tests/cpp -f openings.mk san && tests/cpp/openings_driver_san      (the same program under ASan + UBSan)
# (launch_stubs_ok.cpp's small_grid_fits says "no" to every shape; the driver brings the real rule, so the stub is renamed)
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(HERE)../../esp32-fluid-simulation_amd/csrc
CXX  ?= g++
INC  := $(HERE)../../include

HOST_SRCS := context.cpp transport.cpp sor_executor.cpp operators.cpp slab_step.cpp host_dropin.cpp slab_plan.cpp batch.cpp batch_frames.cpp history.cpp views.cpp solids.cpp viscous.cpp openings.cpp
CXXFLAGS_ := -std=c++17 -O1 -g -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$(CSRC) -Wall -Wno-unused-parameter
SANFLAGS_ := -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer
RENAMED   := small_grid_fits
OBJS     := $(patsubst %.cpp,$(HERE)op_%.o,$(HOST_SRCS)) $(HERE)op_stubs.o $(HERE)op_fake_hip.o $(HERE)op_driver.o
SAN_OBJS := $(patsubst %.cpp,$(HERE)opsan_%.o,$(HOST_SRCS)) $(HERE)opsan_stubs.o $(HERE)opsan_fake_hip.o $(HERE)opsan_driver.o

all: $(HERE)openings_driver
san: $(HERE)openings_driver_san
$(HERE)op_%.o: $(CSRC)/%.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)op_stubs.o: $(HERE)launch_stubs_ok.cpp $(CSRC)/kernels.h
	$(CXX) $(CXXFLAGS_) $(foreach f,$(RENAMED),-D$(f)=$(f)_of_the_stubs) -c -o $@ $<
$(HERE)op_fake_hip.o: $(HERE)fake_hip.cpp
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)op_driver.o: $(HERE)openings_driver.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)openings_driver: $(OBJS)
	$(CXX) -o $@ $(OBJS) -lpthread

$(HERE)opsan_%.o: $(CSRC)/%.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) $(SANFLAGS_) -c -o $@ $<
$(HERE)opsan_stubs.o: $(HERE)launch_stubs_ok.cpp $(CSRC)/kernels.h
	$(CXX) $(CXXFLAGS_) $(SANFLAGS_) $(foreach f,$(RENAMED),-D$(f)=$(f)_of_the_stubs) -c -o $@ $<
$(HERE)opsan_fake_hip.o: $(HERE)fake_hip.cpp
	$(CXX) $(CXXFLAGS_) $(SANFLAGS_) -c -o $@ $<
$(HERE)opsan_driver.o: $(HERE)openings_driver.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) $(SANFLAGS_) -c -o $@ $<
$(HERE)openings_driver_san: $(SAN_OBJS)
	$(CXX) $(SANFLAGS_) -o $@ $(SAN_OBJS) -lpthread

clean:
	rm -f $(HERE)op_*.o $(HERE)opsan_*.o $(HERE)openings_driver $(HERE)openings_driver_san
