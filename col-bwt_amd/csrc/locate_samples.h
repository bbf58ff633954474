// locate_samples.h -- the locate samples of the builder (include/colbwt.h, .col_loc), gathered on the
// device from the suffix array rlbwt_from_text already holds.  Included by rlbwt_build.hip only.
//   end_sa   SA at the last position of every folded run (the toeholds of a backward search)
//   phi      (SA[j], SA[j-1]) at every j >= 1 where the UNFOLDED BWT byte changes, sorted by SA[j]:
//            phi(x) = SA[ISA[x]-1] only moves with x between two such positions when the bytes on both
//            sides of the suffix-array neighbours are equal, so folded boundaries alone are not enough
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace colbwt {

constexpr int kSampleBlock = 256;

__global__ void run_end_sa_kernel(const uint32_t *sa, const uint32_t *start, uint64_t r, uint64_t n, uint32_t *end_sa) {
    for (uint64_t j = blockIdx.x * (uint64_t)kSampleBlock + threadIdx.x; j < r; j += (uint64_t)gridDim.x * kSampleBlock)
        end_sa[j] = sa[(j + 1 < r ? (uint64_t)start[j + 1] : n) - 1];
}

__global__ void phi_flags_kernel(const uint8_t *bwt, uint64_t n, uint8_t *flag) {
    for (uint64_t j = blockIdx.x * (uint64_t)kSampleBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kSampleBlock)
        flag[j] = j > 0 && bwt[j] != bwt[j - 1];
}

// at[i] = the i-th flagged j: key = SA[j], val = SA[j-1]
__global__ void phi_pairs_kernel(const uint32_t *sa, const uint32_t *at, uint64_t s, uint32_t *key, uint32_t *val) {
    for (uint64_t i = blockIdx.x * (uint64_t)kSampleBlock + threadIdx.x; i < s; i += (uint64_t)gridDim.x * kSampleBlock) {
        const uint32_t j = at[i];
        key[i] = sa[j];
        val[i] = sa[j - 1];
    }
}

}  // namespace colbwt
