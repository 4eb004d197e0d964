# tests/cpp/inflow.mk -- CPU-side test harness (never part of the product): the host side of sfl_batch_set_inflow_profile, its
# companions and sfl_batch_openings_flux (csrc/inflow.cpp), of their two hooks in csrc/openings.cpp and of the flux as
# csrc/open_flux.h states it, run through on the CPU over the runtime that lives on the host (fake_hip.cpp) and kernels that do
# nothing (launch_stubs_ok.cpp), with launchers that log what they are handed (inflow_driver.cpp).
#   make -C tests/cpp -f inflow.mk && tests/cpp/inflow_driver              (a plain build)
#   make -C tests/cpp -f inflow.mk san && tests/cpp/inflow_driver_san      (the same stand-alone program under ASan + UBSan)
# (launch_stubs_ok.cpp's small_grid_fits says "no" to every shape; the driver brings the real rule, so the stub is renamed)
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(HERE)../../esp32-fluid-simulation_amd/csrc
CXX  ?= g++
INC  := $(HERE)../../include

HOST_SRCS := context.cpp transport.cpp sor_executor.cpp operators.cpp slab_step.cpp host_dropin.cpp slab_plan.cpp batch.cpp batch_frames.cpp history.cpp views.cpp solids.cpp viscous.cpp openings.cpp inflow.cpp
CXXFLAGS_ := -std=c++17 -O1 -g -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$(CSRC) -Wall -Wno-unused-parameter
SANFLAGS_ := -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer
RENAMED   := small_grid_fits
OBJS     := $(patsubst %.cpp,$(HERE)in_%.o,$(HOST_SRCS)) $(HERE)in_stubs.o $(HERE)in_fake_hip.o $(HERE)in_driver.o
SAN_OBJS := $(patsubst %.cpp,$(HERE)insan_%.o,$(HOST_SRCS)) $(HERE)insan_stubs.o $(HERE)insan_fake_hip.o $(HERE)insan_driver.o

all: $(HERE)inflow_driver
san: $(HERE)inflow_driver_san
$(HERE)in_%.o: $(CSRC)/%.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)in_stubs.o: $(HERE)launch_stubs_ok.cpp $(CSRC)/kernels.h
	$(CXX) $(CXXFLAGS_) $(foreach f,$(RENAMED),-D$(f)=$(f)_of_the_stubs) -c -o $@ $<
$(HERE)in_fake_hip.o: $(HERE)fake_hip.cpp
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)in_driver.o: $(HERE)inflow_driver.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)inflow_driver: $(OBJS)
	$(CXX) -o $@ $(OBJS) -lpthread

$(HERE)insan_%.o: $(CSRC)/%.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) $(SANFLAGS_) -c -o $@ $<
$(HERE)insan_stubs.o: $(HERE)launch_stubs_ok.cpp $(CSRC)/kernels.h
	$(CXX) $(CXXFLAGS_) $(SANFLAGS_) $(foreach f,$(RENAMED),-D$(f)=$(f)_of_the_stubs) -c -o $@ $<
$(HERE)insan_fake_hip.o: $(HERE)fake_hip.cpp
	$(CXX) $(CXXFLAGS_) $(SANFLAGS_) -c -o $@ $<
$(HERE)insan_driver.o: $(HERE)inflow_driver.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) $(SANFLAGS_) -c -o $@ $<
$(HERE)inflow_driver_san: $(SAN_OBJS)
	$(CXX) $(SANFLAGS_) -o $@ $(SAN_OBJS) -lpthread

clean:
	rm -f $(HERE)in_*.o $(HERE)insan_*.o $(HERE)inflow_driver $(HERE)inflow_driver_san
