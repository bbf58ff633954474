// The few HIP names the -DCOLBWT_COUNT_TRIPS instrumentation of the product sources uses beyond
// what hip/hip_runtime.h (the SIMT emulator) provides.  Force-included by match_tail_emu.mk in
// front of every source.  Tests only.
#pragma once
#include "hip/hip_runtime.h"

#define HIP_SYMBOL(x) (&(x))
static inline hipError_t hipMemcpyFromSymbol(void *dst, const void *symbol, size_t n) { memcpy(dst, symbol, n); return hipSuccess; }
static inline hipError_t hipMemcpyToSymbol(void *symbol, const void *src, size_t n) { memcpy(symbol, src, n); return hipSuccess; }
static inline unsigned long long clock64() { return 0; }   // the emulator has no cycle counter: the clock stamps read 0
