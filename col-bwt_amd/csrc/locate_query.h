// locate_query.h -- text positions of each read's longest exact match (r-index toehold + phi) over
// every HBM layout of the index, gfx950, wave64.  Included by capi.hip only.
//
// The search is count_query.h's longest_suffix / search_step with kToe, and with the read's bytes <= 1
// ending it (the folded separator / terminator class: the table's LF is not the text's LF there).
// Besides the (row, offset) cursors of [sp, ep] the range then carries toe = SA[ep]:
//   ep stays in its row (the row holds c)    SA[LF(ep)] = SA[ep] - 1            toe -= 1
//   ep moves to pred(c), the last position   that position ends a folded run:  toe = toe_row[row] - 1
//   of a row that ends a run
// toe_row[j] = SA at the last position of row j of the layout in HBM for every row that ends a folded
// run (the .col_loc's end_sa, scattered to the rows; other rows hold 0 and are never read).
// Then the occurrences SA[ep], SA[ep-1], .. SA[ep-k+1] (k = min(occ, max_occ)) by phi:
//   phi(x) = SA[ISA[x] - 1] = val(a) + (x - a), a = the largest sampled position <= x,
// with the samples (SA[j], SA[j-1]) at every j >= 1 where the UNFOLDED BWT byte changes, sorted by
// SA[j].  A bucket directory dir[x >> shift] = the first sample at or after the bucket's start turns
// the search for a into one directory load and a short scan inside the bucket (shift from n / s, so
// that a bucket holds about one sample).  The walk runs in the same lane, right after the search.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "count_query.h"

namespace colbwt {

constexpr uint64_t kLocateNone = ~0ull;   // a slot of pos_out past the read's k positions

struct PhiTable {
    const uint2 *pair;       // s samples (position, phi of it), positions strictly ascending from 0
    const uint32_t *dir;     // n_buckets + 1 entries: dir[b] = first sample with position >= b << shift
    uint32_t shift;
    uint32_t last_bucket;    // n_buckets - 1: a position >= n (only from a .col_loc of another text) stays in bounds
};

// phi(x): one directory load, a binary search only when the bucket holds more than 4 samples, then a
// scan of at most 4.  pair[0] is position 0 and dir[0] = 0, so the answer is never before sample 0.
__device__ __forceinline__ uint32_t phi_step(const PhiTable &P, uint32_t x) {
    const uint32_t b = min(x >> P.shift, P.last_bucket);
    uint32_t lo = P.dir[b], hi = P.dir[b + 1];     // samples [lo, hi) lie in the bucket; the answer is in [lo - 1, hi)
    while (hi - lo > 4) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (P.pair[mid].x <= x) lo = mid + 1; else hi = mid;
    }
    while (lo < hi && P.pair[lo].x <= x) ++lo;
    const uint2 a = P.pair[lo - 1];
    return a.y + (x - a.x);
}

template <class V>
__global__ __launch_bounds__(kQueryBlock) void locate_kernel(V view, const uint32_t *__restrict__ toe_row, PhiTable phi,
                                                             const uint8_t *__restrict__ bases,
                                                             const uint64_t *__restrict__ read_off, uint64_t n_reads,
                                                             uint32_t max_occ, uint32_t *__restrict__ mlen_out,
                                                             uint64_t *__restrict__ occ_out, uint64_t *__restrict__ pos_out,
                                                             const uint32_t *__restrict__ order) {
    longest_suffix<true, true>(view, toe_row, bases, read_off, n_reads, order,
                               [&](uint64_t rd, uint64_t k, const SearchRange<V> &R) {
                                   uint64_t occ = 0;
                                   if (k > 0) occ = view.idx(R.je) + R.oe - (view.idx(R.js) + R.os) + 1;
                                   mlen_out[rd] = (uint32_t)k;
                                   occ_out[rd] = occ;
                                   const uint32_t want = (uint32_t)min(occ, (uint64_t)max_occ);
                                   uint64_t *out = pos_out + rd * max_occ;
                                   uint32_t x = R.toe;
                                   for (uint32_t t = 0; t < want; ++t) {
                                       out[t] = x;
                                       if (t + 1 < want) x = phi_step(phi, x);
                                   }
                                   for (uint32_t t = want; t < max_occ; ++t) out[t] = kLocateNone;
                               });
}

// ---- attach: the per-row toehold table of the layout in HBM -------------------------------------
constexpr uint32_t kLocBlock = 256;

inline unsigned locate_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + kLocBlock - 1) / kLocBlock, 4096); }

// flag[j] = row j ends a folded run: the next row holds another character, or j is the last row
template <class V>
__global__ void run_end_flags_kernel(V view, uint8_t *flag) {
    const uint32_t rows = view.rows();
    for (uint64_t j = blockIdx.x * (uint64_t)kLocBlock + threadIdx.x; j < rows; j += (uint64_t)gridDim.x * kLocBlock)
        flag[j] = j + 1 == rows || view.ch(view.load((uint32_t)j)) != view.ch(view.load((uint32_t)j + 1));
}

__global__ void toe_scatter_kernel(const uint32_t *sel, const uint32_t *end_sa, uint64_t r, uint32_t *toe_row) {
    for (uint64_t i = blockIdx.x * (uint64_t)kLocBlock + threadIdx.x; i < r; i += (uint64_t)gridDim.x * kLocBlock)
        toe_row[sel[i]] = end_sa[i];
}

// dir[b] = first sample with position >= b << shift, for b = 0 .. n_buckets (dir[n_buckets] = s)
__global__ void phi_dir_kernel(const uint2 *pair, uint64_t s, uint32_t shift, uint64_t n_buckets, uint32_t *dir) {
    for (uint64_t b = blockIdx.x * (uint64_t)kLocBlock + threadIdx.x; b <= n_buckets; b += (uint64_t)gridDim.x * kLocBlock) {
        const uint64_t key = b << shift;
        uint64_t lo = 0, hi = s;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (pair[mid].x < key) lo = mid + 1; else hi = mid;
        }
        dir[b] = (uint32_t)lo;
    }
}

// Row flags -> the rows that end a run, in order (d_sel, room for every row), their number in *d_count.
inline hipError_t run_end_rows(const Index &ix, uint8_t *d_flag, uint32_t *d_sel, unsigned long long *d_count, void *d_tmp,
                               size_t tmp_bytes, hipStream_t stream) {
    const uint32_t rows = (uint32_t)ix.table_rows();
    return with_view(ix, [&](auto view) {
        hipLaunchKernelGGL(run_end_flags_kernel<decltype(view)>, dim3(locate_grid(rows)), dim3(kLocBlock), 0, stream, view, d_flag);
        return hipcub::DeviceSelect::Flagged(d_tmp, tmp_bytes, hipcub::CountingInputIterator<uint32_t>(0), d_flag, d_sel, d_count,
                                             (size_t)rows, stream);
    });
}

// Locate queries over whatever layout the index holds; toe_row / phi were built for that layout.
inline void launch_locate(const Index &ix, const uint32_t *toe_row, const PhiTable &phi, const uint8_t *d_bases,
                          const uint64_t *d_read_off, uint64_t n_reads, uint32_t max_occ, uint32_t *d_mlen, uint64_t *d_occ,
                          uint64_t *d_pos, const uint32_t *d_order, hipStream_t stream) {
    if (n_reads == 0) return;
    with_view(ix, [&](auto view) {
        hipLaunchKernelGGL(locate_kernel<decltype(view)>, read_grid(n_reads), dim3(kQueryBlock), 0, stream, view, toe_row, phi,
                           d_bases, d_read_off, n_reads, max_occ, d_mlen, d_occ, d_pos, d_order);
    });
}

}  // namespace colbwt
