# CPU build of the product's HIP sources against the SIMT emulator with the trip counters compiled
# in (-DCOLBWT_COUNT_TRIPS), as a shared library that match_tail_emu.py loads into Python
# (tests only; run by tests/test_emu_match_tail.py as
#   make -C tests/emu -f match_tail_emu.mk libcolbwt_emu_trips.so
# No sanitizer: a sanitized library in a Python process needs the sanitizer's runtime preloaded,
# which this test does not do.  The same sources run under ASan/UBSan in the stand-alone emulator
# programs (docs_emu.mk and its siblings) and in libcolbwt_emu.so (Makefile).
SRC = ../../col-bwt_amd/csrc
CXX ?= g++
OUT ?= libcolbwt_emu_trips.so
FLAGS = -std=c++17 -O1 -fPIC -pthread -I. -I$(SRC) -Wall -Wno-unused-result -Wno-unknown-pragmas -fno-omit-frame-pointer \
        -DCOLBWT_COUNT_TRIPS -include match_tail_emu_shim.h
HIP_SRC = $(SRC)/query_kernels.hip $(SRC)/sk_query.hip $(SRC)/sk3_query.hip $(SRC)/fat_query.hip $(SRC)/fat2_query.hip $(SRC)/gather_codec.hip $(SRC)/sk_build.hip $(SRC)/fat_build.hip $(SRC)/index_kernels.hip $(SRC)/index.hip $(SRC)/col_split.hip $(SRC)/rlbwt_build.hip $(SRC)/capi.hip
CPP_SRC = $(SRC)/fastx_reader.cpp $(SRC)/fasta_parallel.cpp $(SRC)/text_writer.cpp $(SRC)/bin_writer.cpp $(SRC)/synth.cpp $(SRC)/builder.cpp $(SRC)/rlbwt_files.cpp

$(OUT): $(HIP_SRC) $(CPP_SRC) $(SRC)/*.h ../../include/colbwt.h emu_runtime.cpp match_tail_emu_shim.h hip/hip_runtime.h hipcub/hipcub.hpp
	$(CXX) $(FLAGS) -shared -o $@ $(foreach f,$(HIP_SRC),-x c++ $(f)) -x c++ emu_runtime.cpp $(CPP_SRC) -lz
