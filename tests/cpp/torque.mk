# tests/cpp/torque.mk -- CPU-side test harness (never part of the product): the host side of the torque (csrc/torque.cpp,
# csrc/body_recorder.h) and of its hooks in the step calls of the batches (csrc/batch.cpp) and of the contexts
# (csrc/slab_step.cpp), beside the loads (csrc/loads.cpp), the friction (csrc/friction.cpp) and the histories, run through on
# the CPU over the runtime that lives on the host (fake_hip.cpp) and kernels that do nothing (launch_stubs_ok.cpp), with
# launchers that log what they are handed, in stream order; and csrc/torque_face.h run face by face on the host
# (torque_driver.cpp; tests/test_torque.py).
#   make -C tests/cpp -f torque.mk && tests/cpp/torque_driver              (a plain build)
#   make -C tests/cpp -f torque.mk san && tests/cpp/torque_driver_san      (the same stand-alone program under ASan + UBSan)
# (the driver brings the real small_grid_fits and logging launchers of its own for three of the stubs, which are renamed)
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(HERE)../../esp32-fluid-simulation_amd/csrc
CXX  ?= g++
INC  := $(HERE)../../include

HOST_SRCS := context.cpp transport.cpp sor_executor.cpp operators.cpp slab_step.cpp host_dropin.cpp slab_plan.cpp batch.cpp batch_frames.cpp \
             solve_until.cpp flow_stats.cpp history.cpp views.cpp solids.cpp context_solids.cpp loads.cpp friction.cpp torque.cpp
CXXFLAGS_ := -std=c++17 -O1 -g -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I$(CSRC) -Wall -Wno-unused-parameter -Wno-unknown-pragmas
SANFLAGS_ := -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer
RENAMED   := small_grid_fits launch_advect_vec2f launch_advect_divergence_tiled launch_step_seam_tiled
OBJS     := $(patsubst %.cpp,$(HERE)tq_%.o,$(HOST_SRCS)) $(HERE)tq_stubs.o $(HERE)tq_fake_hip.o $(HERE)tq_driver.o
SAN_OBJS := $(patsubst %.cpp,$(HERE)tqsan_%.o,$(HOST_SRCS)) $(HERE)tqsan_stubs.o $(HERE)tqsan_fake_hip.o $(HERE)tqsan_driver.o

all: $(HERE)torque_driver
san: $(HERE)torque_driver_san
$(HERE)tq_%.o: $(CSRC)/%.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)tq_stubs.o: $(HERE)launch_stubs_ok.cpp $(CSRC)/kernels.h
	$(CXX) $(CXXFLAGS_) $(foreach f,$(RENAMED),-D$(f)=$(f)_of_the_stubs) -c -o $@ $<
$(HERE)tq_fake_hip.o: $(HERE)fake_hip.cpp
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)tq_driver.o: $(HERE)torque_driver.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) -c -o $@ $<
$(HERE)torque_driver: $(OBJS)
	$(CXX) -o $@ $(OBJS) -lpthread

$(HERE)tqsan_%.o: $(CSRC)/%.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) $(SANFLAGS_) -c -o $@ $<
$(HERE)tqsan_stubs.o: $(HERE)launch_stubs_ok.cpp $(CSRC)/kernels.h
	$(CXX) $(CXXFLAGS_) $(SANFLAGS_) $(foreach f,$(RENAMED),-D$(f)=$(f)_of_the_stubs) -c -o $@ $<
$(HERE)tqsan_fake_hip.o: $(HERE)fake_hip.cpp
	$(CXX) $(CXXFLAGS_) $(SANFLAGS_) -c -o $@ $<
$(HERE)tqsan_driver.o: $(HERE)torque_driver.cpp $(wildcard $(CSRC)/*.h) $(INC)/sfl.h
	$(CXX) $(CXXFLAGS_) $(SANFLAGS_) -c -o $@ $<
$(HERE)torque_driver_san: $(SAN_OBJS)
	$(CXX) $(SANFLAGS_) -o $@ $(SAN_OBJS) -lpthread

clean:
	rm -f $(HERE)tq_*.o $(HERE)tqsan_*.o $(HERE)torque_driver $(HERE)torque_driver_san
