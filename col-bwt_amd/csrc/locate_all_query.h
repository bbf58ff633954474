// locate_all_query.h -- every occurrence of each read's longest exact match, as compressed sparse
// rows (include/colbwt.h, colbwt_locate_all_*), gfx950, wave64.  Included by capi.hip only.
//
// Three stages over a caller-provided workspace (LocAllWork), none of them with an atomic:
//   search  locate_all_search_kernel: locate_kernel's backward search (the same longest_suffix call)
//           without its walk.  Per read it leaves mlen, occ, toe = SA[ep] and the BWT position of ep.
//   plan    locate_all_width_kernel stores w (the positions the read gets) into pos_off[k + 1] and
//           ceil(w / C) into tile_off[k + 1], C = kLocAllTile; two in-place inclusive scans turn both
//           into offsets.  Entry 0 of either array is stored by the kernel.
//   walk    locate_all_walk_kernel: one lane per TILE of a read, lanes striding over the tiles of the
//           reads [read_lo, read_hi) in a fixed-size grid whose bounds come from tile_off in HBM.
//           Tile t of a read with range (lo_all, ep], lo_all = ep - w, starts at cut(t):
//             cut(0) = ep, with SA[ep] = toe;
//             cut(t) = the greatest position <= ep - t * C that is the last position of a row ending a
//                      folded run (ch(row) != ch(row + 1), or the last row) -- there SA is toe_row[row],
//                      the toehold the attach scattered for the search -- or lo_all when that
//                      position is not above lo_all (the tile is empty);
//             cut(T) = lo_all, T the read's tile count.
//           The lane derives cut(t) and cut(t + 1) itself (a binary search over idx for the row, then
//           a scan down the rows of the run), then walks p = cut(t) .. cut(t + 1) + 1 by phi and
//           stores pos[pos_off[r] + (ep - p)].  Cuts do not increase with t, so the pieces partition
//           (lo_all, ep] and every slot has one writer.  A piece is at most C + the longest run of
//           the range: inside a run there is no restart point.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "locate_query.h"

#ifndef COLBWT_LOCATE_ALL_TILE
#define COLBWT_LOCATE_ALL_TILE 256
#endif

namespace colbwt {

constexpr uint32_t kLocAllTile = COLBWT_LOCATE_ALL_TILE;
static_assert(kLocAllTile >= 1, "COLBWT_LOCATE_ALL_TILE must be at least 1");
constexpr uint32_t kLocAllBlock = 256;
constexpr uint32_t kLocAllBlocksPerCU = 8;     // 32 waves per CU: the walk is a chain of dependent loads

// The workspace of one plan, cut from a 256-byte aligned buffer of locate_all_work_bytes(n_reads) bytes.
// The walk reads ep, tile_off and toe; scan_tmp is the plan's alone.
struct LocAllWork {
    uint64_t *ep;           // n_reads: BWT position of ep
    uint64_t *tile_off;     // n_reads + 1: first tile of every read
    uint32_t *toe;          // n_reads: SA[ep]
    void *scan_tmp;
    size_t scan_tmp_bytes;
};

inline uint64_t locate_all_align(uint64_t bytes) { return (bytes + 255) & ~255ull; }
// the scans' own workspace: hipcub keeps a look-back state per block of a few thousand items
inline uint64_t locate_all_scan_tmp_bytes(uint64_t n_reads) { return locate_all_align(n_reads + (1ull << 20)); }
inline uint64_t locate_all_work_bytes(uint64_t n_reads) {
    return locate_all_align(8 * n_reads) + locate_all_align(8 * (n_reads + 1)) + locate_all_align(4 * n_reads) +
           locate_all_scan_tmp_bytes(n_reads);
}
inline LocAllWork locate_all_work(const void *d_work, uint64_t n_reads) {
    uint8_t *p = (uint8_t *)d_work;
    LocAllWork w;
    w.ep = (uint64_t *)p;
    p += locate_all_align(8 * n_reads);
    w.tile_off = (uint64_t *)p;
    p += locate_all_align(8 * (n_reads + 1));
    w.toe = (uint32_t *)p;
    p += locate_all_align(4 * n_reads);
    w.scan_tmp = p;
    w.scan_tmp_bytes = locate_all_scan_tmp_bytes(n_reads);
    return w;
}

// locate_kernel's search (count_query.h longest_suffix); what differs is what it stores afterwards.
template <class V>
__global__ __launch_bounds__(kQueryBlock) void locate_all_search_kernel(V view, const uint32_t *__restrict__ toe_row,
                                                                        const uint8_t *__restrict__ bases,
                                                                        const uint64_t *__restrict__ read_off, uint64_t n_reads,
                                                                        uint32_t *__restrict__ mlen_out, uint64_t *__restrict__ occ_out,
                                                                        uint32_t *__restrict__ toe_out, uint64_t *__restrict__ ep_out,
                                                                        const uint32_t *__restrict__ order) {
    longest_suffix<true, true>(view, toe_row, bases, read_off, n_reads, order,
                               [&](uint64_t rd, uint64_t k, const SearchRange<V> &R) {
                                   const uint64_t ep = view.idx(R.je) + R.oe;
                                   uint64_t occ = 0;
                                   if (k > 0) occ = ep - (view.idx(R.js) + R.os) + 1;
                                   mlen_out[rd] = (uint32_t)k;
                                   occ_out[rd] = occ;
                                   toe_out[rd] = R.toe;
                                   ep_out[rd] = ep;
                               });
}

// w = the positions read k gets, its tiles = ceil(w / C): the inputs of the two scans, in place
__global__ __launch_bounds__(kLocAllBlock) void locate_all_width_kernel(const uint32_t *__restrict__ mlen, const uint64_t *__restrict__ occ,
                                                                        uint64_t n_reads, uint32_t min_len, uint64_t max_per_read,
                                                                        uint64_t *__restrict__ pos_off, uint64_t *__restrict__ tile_off) {
    const uint64_t i = (uint64_t)blockIdx.x * kLocAllBlock + threadIdx.x;
    if (i >= n_reads) return;
    uint64_t w = mlen[i] >= min_len ? occ[i] : 0;
    if (max_per_read) w = min(w, max_per_read);
    pos_off[i + 1] = w;
    tile_off[i + 1] = (w + kLocAllTile - 1) / kLocAllTile;
    if (i == 0) {
        pos_off[0] = 0;
        tile_off[0] = 0;
    }
}

struct LocAllSum {
    __host__ __device__ __forceinline__ uint64_t operator()(const uint64_t &a, const uint64_t &b) const { return a + b; }
};

// The row holding BWT position q: the largest j with idx(j) <= q, searched below `hi` (idx(hi) > q, or hi == rows).
template <class V>
__device__ __forceinline__ uint32_t locate_all_row_of(const V &view, uint64_t q, uint32_t hi) {
    uint32_t lo = 0;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (view.idx(mid) <= q) lo = mid; else hi = mid;
    }
    return lo;
}

// cut: the greatest position p <= q that is the last position of a row ending a folded run, with that
// row in `row` -- or lo_all when p would not be above lo_all.  `hi` bounds the row of q from above and
// receives that row + 1 (the next cut of the lane lies below).
template <class V>
__device__ __forceinline__ int64_t locate_all_cut(const V &view, int64_t q, int64_t lo_all, uint32_t &hi, uint32_t &row) {
    const uint32_t rows = view.rows();
    const uint32_t j = locate_all_row_of(view, (uint64_t)q, hi);
    hi = j + 1;
    uint32_t above = view.ch(view.load(j));                 // the character of row k + 1 while row k is looked at
    const int64_t last_j = (int64_t)(j + 1 == rows ? view.n() : view.idx(j + 1)) - 1;
    if (last_j == q && (j + 1 == rows || view.ch(view.load(j + 1)) != above)) {
        row = j;
        return q;
    }
    for (uint32_t k = j; k-- > 0;) {
        const int64_t last = (int64_t)view.idx(k + 1) - 1;
        if (last <= lo_all) break;
        const uint32_t c = view.ch(view.load(k));
        if (c != above) {
            row = k;
            return last;
        }
        above = c;
    }
    return lo_all;
}

template <class V>
__global__ __launch_bounds__(kLocAllBlock) void locate_all_walk_kernel(V view, const uint32_t *__restrict__ toe_row, PhiTable phi,
                                                                       const uint64_t *__restrict__ pos_off,
                                                                       const uint64_t *__restrict__ tile_off,
                                                                       const uint64_t *__restrict__ ep_in, const uint32_t *__restrict__ toe_in,
                                                                       uint64_t read_lo, uint64_t read_hi, uint64_t *__restrict__ pos,
                                                                       uint64_t pos_cap) {
    const uint64_t g_hi = tile_off[read_hi], base = pos_off[read_lo];
    const uint64_t lanes = (uint64_t)gridDim.x * kLocAllBlock;
    for (uint64_t g = tile_off[read_lo] + (uint64_t)blockIdx.x * kLocAllBlock + threadIdx.x; g < g_hi; g += lanes) {
        uint64_t r = read_lo, r_hi = read_hi;              // tile_off[r] <= g < tile_off[r_hi]
        while (r_hi - r > 1) {
            const uint64_t mid = r + ((r_hi - r) >> 1);
            if (tile_off[mid] <= g) r = mid; else r_hi = mid;
        }
        const uint64_t t = g - tile_off[r], n_tiles = tile_off[r + 1] - tile_off[r];
        const uint64_t o = pos_off[r], w = pos_off[r + 1] - o;
        const int64_t ep = (int64_t)ep_in[r], lo_all = ep - (int64_t)w;
        uint32_t hi = view.rows(), row = 0, x = 0;
        int64_t p = ep;
        if (t == 0) {
            x = toe_in[r];
        } else {
            p = locate_all_cut(view, ep - (int64_t)(t * kLocAllTile), lo_all, hi, row);
            if (p > lo_all) x = toe_row[row];
        }
        int64_t stop = lo_all;
        if (t + 1 < n_tiles && p > lo_all) stop = locate_all_cut(view, ep - (int64_t)((t + 1) * kLocAllTile), lo_all, hi, row);
        uint64_t at = o - base + (uint64_t)(ep - p);
        for (; p > stop && at < pos_cap; --p, ++at) {
            pos[at] = x;
            if (p - 1 > stop) x = phi_step(phi, x);
        }
    }
}

struct LocAllArgs {
    const uint32_t *toe_row;       // the replica's locate tables
    PhiTable phi;
};

// Search and plan for a batch in HBM: d_mlen / d_occ n_reads entries, d_pos_off n_reads + 1.  d_order
// goes to the search only.
inline hipError_t launch_locate_all_plan(const Index &ix, const LocAllArgs &a, const uint8_t *d_bases, const uint64_t *d_read_off,
                                         uint64_t n_reads, uint32_t min_len, uint64_t max_per_read, uint32_t *d_mlen, uint64_t *d_occ,
                                         uint64_t *d_pos_off, void *d_work, const uint32_t *d_order, hipStream_t stream) {
    if (n_reads == 0) return hipSuccess;
    const LocAllWork w = locate_all_work(d_work, n_reads);
    with_view(ix, [&](auto view) {
        hipLaunchKernelGGL(locate_all_search_kernel<decltype(view)>, read_grid(n_reads), dim3(kQueryBlock), 0, stream, view, a.toe_row,
                           d_bases, d_read_off, n_reads, d_mlen, d_occ, w.toe, w.ep, d_order);
    });

    const dim3 grid((uint32_t)((n_reads + kLocAllBlock - 1) / kLocAllBlock)), block(kLocAllBlock);
    hipLaunchKernelGGL(locate_all_width_kernel, grid, block, 0, stream, d_mlen, d_occ, n_reads, min_len, max_per_read, d_pos_off,
                       w.tile_off);
    size_t need = 0;
    hipError_t e = hipcub::DeviceScan::InclusiveScan(nullptr, need, d_pos_off + 1, d_pos_off + 1, LocAllSum(), (size_t)n_reads, stream);
    if (e != hipSuccess) return e;
    if (need > w.scan_tmp_bytes) return hipErrorOutOfMemory;
    need = w.scan_tmp_bytes;
    e = hipcub::DeviceScan::InclusiveScan(w.scan_tmp, need, d_pos_off + 1, d_pos_off + 1, LocAllSum(), (size_t)n_reads, stream);
    if (e != hipSuccess) return e;
    need = w.scan_tmp_bytes;
    return hipcub::DeviceScan::InclusiveScan(w.scan_tmp, need, w.tile_off + 1, w.tile_off + 1, LocAllSum(), (size_t)n_reads, stream);
}

// The walk's grid: the workgroups resident at once on the device, whatever the batch holds.
inline uint32_t locate_all_fill_grid() {
    static uint32_t blocks[16] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = 0;
    if (blocks[dev] == 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 1;
        (void)hipGetLastError();
        blocks[dev] = (uint32_t)cus * kLocAllBlocksPerCU;
    }
    return blocks[dev];
}

// The walk over the reads [read_lo, read_hi) of a planned batch into d_pos[0 .. pos_cap).
inline void launch_locate_all_fill(const Index &ix, const LocAllArgs &a, uint64_t n_reads, uint64_t read_lo, uint64_t read_hi,
                                   const uint64_t *d_pos_off, uint64_t *d_pos, uint64_t pos_cap, const void *d_work, hipStream_t stream) {
    if (read_lo >= read_hi) return;
    const LocAllWork w = locate_all_work(d_work, n_reads);
    with_view(ix, [&](auto view) {
        hipLaunchKernelGGL(locate_all_walk_kernel<decltype(view)>, dim3(locate_all_fill_grid()), dim3(kLocAllBlock), 0, stream, view,
                           a.toe_row, a.phi, d_pos_off, w.tile_off, w.ep, w.toe, read_lo, read_hi, d_pos, pos_cap);
    });
}

}  // namespace colbwt
