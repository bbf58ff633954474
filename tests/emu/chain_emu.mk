# Stand-alone CPU program of the chain entry points: the product's HIP sources, the SIMT emulator and
# chain_emu_main.cpp in one executable under ASan/UBSan (tests only; run by tests/test_chain_cpu.py as
#   make -C tests/emu -f chain_emu.mk
# ).  The sanitizers are linked into the program itself: nothing is preloaded.
SRC = ../../col-bwt_amd/csrc
CXX ?= g++
OUT ?= chain_emu
FLAGS = -std=c++17 -g -O1 -pthread -I. -I$(SRC) -Wall -Wno-unused-result -Wno-unknown-pragmas -fno-omit-frame-pointer
# the sanitizer runtimes are linked statically: the program does not depend on the order of shared libraries
SAN ?= -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan
HIP_SRC = $(SRC)/query_kernels.hip $(SRC)/sk_query.hip $(SRC)/sk3_query.hip $(SRC)/fat_query.hip $(SRC)/fat2_query.hip $(SRC)/gather_codec.hip $(SRC)/sk_build.hip $(SRC)/fat_build.hip $(SRC)/index_kernels.hip $(SRC)/index.hip $(SRC)/col_split.hip $(SRC)/rlbwt_build.hip $(SRC)/capi.hip
CPP_SRC = $(SRC)/fastx_reader.cpp $(SRC)/fasta_parallel.cpp $(SRC)/text_writer.cpp $(SRC)/bin_writer.cpp $(SRC)/synth.cpp $(SRC)/builder.cpp $(SRC)/rlbwt_files.cpp

$(OUT): $(HIP_SRC) $(CPP_SRC) $(SRC)/*.h ../../include/colbwt.h emu_runtime.cpp chain_emu_main.cpp hip/hip_runtime.h hipcub/hipcub.hpp
	$(CXX) $(FLAGS) $(SAN) -o $@ $(foreach f,$(HIP_SRC),-x c++ $(f)) -x c++ emu_runtime.cpp chain_emu_main.cpp $(CPP_SRC) -lz
