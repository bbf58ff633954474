// locate_query.h -- text positions of each read's longest exact match (r-index toehold + phi) over
// every HBM layout of the index, gfx950, wave64.  Included by capi.hip only.
//
// The search is count_query.h's backward search, with the read's bytes <= 1 ending it (the folded
// separator / terminator class: the table's LF is not the text's LF there).  Besides the (row, offset)
// cursors of [sp, ep] the lane carries toe = SA[ep]:
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
    using Row = typename V::Row;
    __shared__ uint32_t s_rd[16][kQueryBlock];
    __shared__ uint8_t s_cmap[256];
    for (uint32_t t = threadIdx.x; t < 256; t += kQueryBlock) s_cmap[t] = view.cmap()[t];
    __syncthreads();

    const uint64_t slot = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
    if (slot >= n_reads) return;
    const uint64_t rd = order ? order[slot] : slot;
    const uint64_t off = read_off[rd];
    const uint64_t m = read_off[rd + 1] - off;

    uint32_t js = 0, je = view.rows() - 1;
    Row ws = view.load(js), we = view.load(je);
    uint64_t os = 0, oe = view.len(je, we) - 1;
    uint32_t toe = toe_row[je];   // SA[n - 1]
    uint64_t k = 0;

    SlidingWindow win;
    win.init(off + m - 1);
    for (; k < m; ++k) {
        const uint64_t g = off + m - 1 - k;
        if (__any(win.avail(g) < 1)) win.refill(s_rd, bases, g);
        const uint32_t c = win.get(s_rd, g);
        const uint32_t cidx = s_cmap[c];
        if (c <= 1 || cidx == kAbsent) break;
        uint32_t sj = js;
        uint64_t so = os;
        Row sw = ws;
        if (view.ch(ws) != c) {
            sj = view.succ(js, c, cidx, sw);
            if (sj == kNone) break;
            so = 0;
        }
        uint32_t ej = je;
        uint64_t eo = oe;
        Row ew = we;
        uint32_t te = toe;                 // SA[e]
        if (view.ch(we) != c) {
            ej = view.pred(je, c, cidx, ew);
            if (ej == kNone) break;
            eo = view.len(ej, ew) - 1;
            te = toe_row[ej];
        }
        if (sj > ej || (sj == ej && so > eo)) break;
        uint32_t nj = view.lf_row(sw);
        uint64_t nt = (uint64_t)view.lf_off(sw) + so;
        Row nw = view.load(nj);
        count_fast_forward(view, nj, nt, nw);
        uint32_t mj;
        uint64_t mt;
        Row mw;
        if (sj == ej) {
            mj = nj;
            mt = nt + (eo - so);
            mw = nw;
        } else {
            mj = view.lf_row(ew);
            mt = (uint64_t)view.lf_off(ew) + eo;
            mw = view.load(mj);
        }
        count_fast_forward(view, mj, mt, mw);
        if (nj > mj || (nj == mj && nt > mt)) break;
        js = nj; os = nt; ws = nw;
        je = mj; oe = mt; we = mw;
        toe = te - 1;
    }
    uint64_t occ = 0;
    if (k > 0) occ = view.idx(je) + oe - (view.idx(js) + os) + 1;
    mlen_out[rd] = (uint32_t)k;
    occ_out[rd] = occ;
    const uint32_t want = (uint32_t)min(occ, (uint64_t)max_occ);
    uint64_t *out = pos_out + rd * max_occ;
    uint32_t x = toe;
    for (uint32_t t = 0; t < want; ++t) {
        out[t] = x;
        if (t + 1 < want) x = phi_step(phi, x);
    }
    for (uint32_t t = want; t < max_occ; ++t) out[t] = kLocateNone;
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
template <class V>
inline hipError_t run_end_rows_view(const V &view, uint32_t rows, uint8_t *d_flag, uint32_t *d_sel,
                                    unsigned long long *d_count, void *d_tmp, size_t tmp_bytes, hipStream_t stream) {
    hipLaunchKernelGGL(run_end_flags_kernel<V>, dim3(locate_grid(rows)), dim3(kLocBlock), 0, stream, view, d_flag);
    return hipcub::DeviceSelect::Flagged(d_tmp, tmp_bytes, hipcub::CountingInputIterator<uint32_t>(0), d_flag, d_sel, d_count,
                                         (size_t)rows, stream);
}

inline hipError_t run_end_rows(const Index &ix, uint8_t *d_flag, uint32_t *d_sel, unsigned long long *d_count, void *d_tmp,
                               size_t tmp_bytes, hipStream_t stream) {
    const uint32_t rows = (uint32_t)ix.table_rows();
    if (ix.line_rows()) return run_end_rows_view(CountFatView{ix.table_fat()}, rows, d_flag, d_sel, d_count, d_tmp, tmp_bytes, stream);
    if (ix.layout() == 3) return run_end_rows_view(CountSKView<3>{ix.table_k()}, rows, d_flag, d_sel, d_count, d_tmp, tmp_bytes, stream);
    if (ix.layout() == 2) return run_end_rows_view(CountSKView<2>{ix.table_k()}, rows, d_flag, d_sel, d_count, d_tmp, tmp_bytes, stream);
    return run_end_rows_view(CountOneStepView{ix.table()}, rows, d_flag, d_sel, d_count, d_tmp, tmp_bytes, stream);
}

template <typename View>
inline void launch_locate_view(const View &view, const uint32_t *toe_row, const PhiTable &phi, const uint8_t *d_bases,
                               const uint64_t *d_read_off, uint64_t n_reads, uint32_t max_occ, uint32_t *d_mlen, uint64_t *d_occ,
                               uint64_t *d_pos, const uint32_t *d_order, hipStream_t stream) {
    const dim3 grid((uint32_t)((n_reads + kQueryBlock - 1) / kQueryBlock)), block(kQueryBlock);
    hipLaunchKernelGGL(locate_kernel<View>, grid, block, 0, stream, view, toe_row, phi, d_bases, d_read_off, n_reads, max_occ,
                       d_mlen, d_occ, d_pos, d_order);
}

// Locate queries over whatever layout the index holds; toe_row / phi were built for that layout.
inline void launch_locate(const Index &ix, const uint32_t *toe_row, const PhiTable &phi, const uint8_t *d_bases,
                          const uint64_t *d_read_off, uint64_t n_reads, uint32_t max_occ, uint32_t *d_mlen, uint64_t *d_occ,
                          uint64_t *d_pos, const uint32_t *d_order, hipStream_t stream) {
    if (n_reads == 0) return;
    if (ix.line_rows())
        launch_locate_view(CountFatView{ix.table_fat()}, toe_row, phi, d_bases, d_read_off, n_reads, max_occ, d_mlen, d_occ, d_pos,
                           d_order, stream);
    else if (ix.layout() == 3)
        launch_locate_view(CountSKView<3>{ix.table_k()}, toe_row, phi, d_bases, d_read_off, n_reads, max_occ, d_mlen, d_occ, d_pos,
                           d_order, stream);
    else if (ix.layout() == 2)
        launch_locate_view(CountSKView<2>{ix.table_k()}, toe_row, phi, d_bases, d_read_off, n_reads, max_occ, d_mlen, d_occ, d_pos,
                           d_order, stream);
    else
        launch_locate_view(CountOneStepView{ix.table()}, toe_row, phi, d_bases, d_read_off, n_reads, max_occ, d_mlen, d_occ, d_pos,
                           d_order, stream);
}

}  // namespace colbwt
