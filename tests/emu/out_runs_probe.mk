# The probe of the output collector (csrc/lane_out.h): out_runs_probe.hip, one source, two stand-alone programs
# (tests only; built by tests/test_out_runs_cpu.py and tests/test_gpu_out_runs.py as
#   make -C tests/emu -f out_runs_probe.mk out_runs_probe_emu      g++, the SIMT emulator, ASan/UBSan
#   make -C tests/emu -f out_runs_probe.mk out_runs_probe_gpu      hipcc for gfx950
# ).  The sanitizers are linked into the CPU program itself: nothing is preloaded.
SRC = ../../col-bwt_amd/csrc
CXX ?= g++
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
FLAGS = -std=c++17 -g -O1 -pthread -I. -I$(SRC) -Wall -Wno-unused-result -Wno-unknown-pragmas -fno-omit-frame-pointer
# the sanitizer runtimes are linked statically: the program does not depend on the order of shared libraries
SAN ?= -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan
DEPS = out_runs_probe.hip $(SRC)/*.h

out_runs_probe_emu: $(DEPS) emu_runtime.cpp hip/hip_runtime.h
	$(CXX) $(FLAGS) $(SAN) -o $@ -x c++ out_runs_probe.hip -x c++ emu_runtime.cpp

out_runs_probe_gpu: $(DEPS)
	$(HIPCC) --offload-arch=$(ARCH) -O3 -std=c++17 -I$(SRC) -o $@ out_runs_probe.hip
