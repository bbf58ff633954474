// count_query.h -- exact-match counting (backward search) over every HBM layout of the index,
// gfx950, wave64.  Included by capi.hip only (the one translation unit that launches it).
//
// For a read P[0..m) the search starts with the whole BWT range [sp, ep] = [0, n-1] and takes the
// read's bases from the last one down.  With c = P[i]:
//   s = first position >= sp whose BWT character is c, e = last position <= ep holding c
//   (c absent from the table, or s > e: the search ends);
//   sp = LF(s), ep = LF(e) -- the move-structure step of the PML path (LF_table.hpp:251-262:
//   landing row + offset, then fast-forward); sp > ep afterwards (impossible on a real BWT,
//   possible on a synthetic table) ends the search as well, without consuming the base.
// Per read: mlen = bases consumed (the longest suffix of the read that occurs in the text),
// occ = ep - sp + 1 of the last non-empty range (0 when mlen == 0), sp = its first position
// (0 when mlen == 0).
//
// A cursor is (row, offset inside the row).  Rows partition the BWT in order and hold one
// character each, so s is (sp's row, its offset) when that row holds c, else the first row after
// it holding c at offset 0 -- succ_char of the PML path; e likewise with pred_char and the last
// offset of the row.  When s and e lie in ONE row (the common case once the range is inside a
// run) their LF images are the same landing shifted by e - s: one row fetch and one fast-forward
// serve both ends.  Positions (idx[] loads) are only formed once, at the end of the read.
//
// One lane per read, bases from the read's end, read bytes staged 64 at a time in LDS
// (lane_io.h SlidingWindow: the same d_bases padding contract as colbwt_query_device).  A
// layout enters through a View: load(j) -> Row, ch(Row), lf_row(Row), lf_off(Row), len(j, Row),
// idx(j), rows(), n(), succ / pred (row or kNone, with its image).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_layout.h"
#include "fat_layout.h"
#include "index.h"
#include "lane_io.h"
#include "lf_device.h"
#include "query_kernels.h"
#include "sk_layout.h"

namespace colbwt {

// fast-forward steps walked row by row before the walk switches to a search over idx[]: a
// landing usually stays in its row or leaves it by one or two short rows, but one-step rows may
// be longer than 65535 (the len16 escape) and a refined row's image may cover many refined rows
constexpr uint32_t kCountLinearSteps = 8;

struct CountOneStepView {
    DevTable T;
    using Row = uint4;
    __device__ __forceinline__ uint64_t n() const { return T.n; }
    __device__ __forceinline__ uint32_t rows() const { return T.r; }
    __device__ __forceinline__ uint64_t idx(uint32_t j) const { return T.idx[j]; }
    __device__ __forceinline__ const uint8_t *cmap() const { return T.cmap; }
    __device__ __forceinline__ Row load(uint32_t j) const { return T.rows[j]; }
    __device__ __forceinline__ uint32_t ch(const Row &w) const { return row_char(w); }
    __device__ __forceinline__ uint32_t lf_row(const Row &w) const { return row_interval(w); }
    __device__ __forceinline__ uint32_t lf_off(const Row &w) const { return row_offset(w); }
    __device__ __forceinline__ uint64_t len(uint32_t j, const Row &w) const { return row_len(T, j, w); }
    __device__ __forceinline__ uint32_t succ(uint32_t i, uint32_t c, uint32_t cidx, Row &w) const { return succ_char(T, i, c, cidx, w); }
    __device__ __forceinline__ uint32_t pred(uint32_t i, uint32_t c, uint32_t cidx, Row &w) const { return pred_char(T, i, c, cidx, w); }
};

template <int K>
struct CountSKView {
    SKTable T;
    using Row = SKRow<K>;
    __device__ __forceinline__ uint64_t n() const { return T.n; }
    __device__ __forceinline__ uint32_t rows() const { return T.r; }
    __device__ __forceinline__ uint64_t idx(uint32_t j) const { return T.idx[j]; }
    __device__ __forceinline__ const uint8_t *cmap() const { return T.cmap; }
    __device__ __forceinline__ Row load(uint32_t j) const { return sk_load<K>(T, j); }
    __device__ __forceinline__ uint32_t ch(const Row &w) const { return sk_char<K>(w); }
    __device__ __forceinline__ uint32_t lf_row(const Row &w) const { return sk_I<K>(w, 1); }
    __device__ __forceinline__ uint32_t lf_off(const Row &w) const { return sk_O<K>(w, 1); }
    __device__ __forceinline__ uint64_t len(uint32_t, const Row &w) const { return sk_len<K>(w); }
    __device__ __forceinline__ uint32_t succ(uint32_t i, uint32_t c, uint32_t cidx, Row &w) const { return sk_succ_char<K>(T, i, c, cidx, w); }
    __device__ __forceinline__ uint32_t pred(uint32_t i, uint32_t c, uint32_t cidx, Row &w) const { return sk_pred_char<K>(T, i, c, cidx, w); }
};

// line rows (every variant: the mismatch-line ones keep bytes [0, 80) of the row as they are)
struct CountFatView {
    FatTable T;
    struct Row {
        uint32_t i1, o1_len, ch;
    };
    __device__ __forceinline__ uint64_t n() const { return T.n; }
    __device__ __forceinline__ uint32_t rows() const { return T.r; }
    __device__ __forceinline__ uint64_t idx(uint32_t j) const { return T.idx[j]; }
    __device__ __forceinline__ const uint8_t *cmap() const { return T.cmap; }
    __device__ __forceinline__ Row load(uint32_t j) const {
        const uint32_t *p = reinterpret_cast<const uint32_t *>(T.lines + (uint64_t)j * kFatRowBytes);
        Row w;
        w.i1 = p[kFatI / 4];
        w.o1_len = fat_half(p, kFatO) | (fat_half(p, kFatLen) << 16);
        w.ch = fat_byte(p, kFatCh + 7);
        return w;
    }
    __device__ __forceinline__ uint32_t ch(const Row &w) const { return w.ch; }
    __device__ __forceinline__ uint32_t lf_row(const Row &w) const { return w.i1; }
    __device__ __forceinline__ uint32_t lf_off(const Row &w) const { return w.o1_len & 0xFFFFu; }
    __device__ __forceinline__ uint64_t len(uint32_t, const Row &w) const { return w.o1_len >> 16; }
    __device__ __forceinline__ uint32_t succ(uint32_t i, uint32_t c, uint32_t cidx, Row &w) const {
        const uint32_t s = fat_succ_char(T, i, c, cidx);
        if (s != kNone) w = load(s);
        return s;
    }
    __device__ __forceinline__ uint32_t pred(uint32_t i, uint32_t c, uint32_t cidx, Row &w) const {
        const uint32_t q = fat_pred_char(T, i, c, cidx);
        if (q != kNone) w = load(q);
        return q;
    }
};

// Fast-forward (LF_table.hpp:256-259): moves (j, t, w) on until t < len(j).  A few rows one by
// one, then a galloping + binary search for the row holding idx[j] + t (idx[rows] = n is the
// sentinel).  Never passes row rows - 1 (a validated table does not need it to).
template <class V>
__device__ __forceinline__ void count_fast_forward(const V &view, uint32_t &j, uint64_t &t, typename V::Row &w) {
    const uint32_t last = view.rows() - 1;
    for (uint32_t k = 0; k < kCountLinearSteps; ++k) {
        const uint64_t len = view.len(j, w);
        if (t < len || j >= last) return;
        t -= len;
        ++j;
        w = view.load(j);
    }
    if (t < view.len(j, w) || j >= last) return;
    const uint64_t p = view.idx(j) + t;
    uint32_t lo = j, hi = last + 1;       // idx[lo] <= p < idx[hi]
    for (uint32_t d = 1; (uint64_t)lo + d <= last; d <<= 1) {
        if (view.idx(lo + d) > p) {
            hi = lo + d;
            break;
        }
        lo += d;
        if (d >= 0x80000000u) break;
    }
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (view.idx(mid) <= p) lo = mid; else hi = mid;
    }
    j = lo;
    t = p - view.idx(lo);
    w = view.load(j);
}

// The (row, offset) cursors of [sp, ep] with the rows they lie in, and toe = SA[ep] (kToe only).
template <class V>
struct SearchRange {
    using Row = typename V::Row;
    uint32_t js, je;
    uint64_t os, oe;
    Row ws, we;
    uint32_t toe;
    // [0, n - 1]: row 0 offset 0 .. the last row at its last offset
    template <bool kToe>
    __device__ __forceinline__ void full(const V &view, const uint32_t *__restrict__ toe_row) {
        js = 0;
        je = view.rows() - 1;
        ws = view.load(js);
        we = view.load(je);
        os = 0;
        oe = view.len(je, we) - 1;
        toe = 0;
        if constexpr (kToe) toe = toe_row[je];   // SA[n - 1]
    }
};

// One backward-search step with character c (cidx = its column of the jump tables): the only copy of
// the step, called by count, locate, locate-all and anchors.  kToe: whether the toehold SA[ep]
// (locate_query.h) is carried; without it toe_row is never loaded and may be null.
// True: R is the range of c + (what R matched).  False: no such range (c does not occur in R, or LF
// left an empty range); R is unchanged.
template <bool kToe, class V>
__device__ __forceinline__ bool search_step(const V &view, const uint32_t *__restrict__ toe_row, uint32_t c, uint32_t cidx,
                                            SearchRange<V> &R) {
    using Row = typename V::Row;
    // s: first position >= sp holding c
    uint32_t sj = R.js;
    uint64_t so = R.os;
    Row sw = R.ws;
    if (view.ch(R.ws) != c) {
        sj = view.succ(R.js, c, cidx, sw);
        if (sj == kNone) return false;
        so = 0;
    }
    // e: last position <= ep holding c
    uint32_t ej = R.je;
    uint64_t eo = R.oe;
    Row ew = R.we;
    uint32_t te = R.toe;                 // SA[e]
    if (view.ch(R.we) != c) {
        ej = view.pred(R.je, c, cidx, ew);
        if (ej == kNone) return false;
        eo = view.len(ej, ew) - 1;
        if constexpr (kToe) te = toe_row[ej];
    }
    if (sj > ej || (sj == ej && so > eo)) return false;
    // LF of both ends
    uint32_t nj = view.lf_row(sw);
    uint64_t nt = (uint64_t)view.lf_off(sw) + so;
    Row nw = view.load(nj);
    count_fast_forward(view, nj, nt, nw);
    uint32_t mj;
    uint64_t mt;
    Row mw;
    if (sj == ej) {                      // one row: the image of [so, eo] is contiguous
        mj = nj;
        mt = nt + (eo - so);
        mw = nw;
    } else {
        mj = view.lf_row(ew);
        mt = (uint64_t)view.lf_off(ew) + eo;
        mw = view.load(mj);
    }
    count_fast_forward(view, mj, mt, mw);
    if (nj > mj || (nj == mj && nt > mt)) return false;   // empty range: only on synthetic tables
    R.js = nj; R.os = nt; R.ws = nw;
    R.je = mj; R.oe = mt; R.we = mw;
    R.toe = te - 1;
    return true;
}

// The longest suffix of the lane's read that occurs in the text: the frame count, locate and
// locate-all share.  The jump-table columns go to LDS, the lane takes read order[lane] (or its own),
// and the read's bases go through search_step from the last one down until one has no range.
// kStopLow: a byte <= 1 ends the search as an absent character does (count walks through them).
// A lane with a read ends in done(rd, k, R): rd = its read, k = the bases consumed, R = the last
// non-empty range (the full one when k == 0); a lane past n_reads returns without it.  The kernel's
// own epilogue is that callable and not code behind a returned k: so the lane's values and its early
// return stay in one function, and the kernels keep the registers they had with the loop written out.
// The window refill is at the top of a trip, where the wave is converged (lane_io.h).
template <bool kToe, bool kStopLow, class V, class Done>
__device__ __forceinline__ void longest_suffix(const V &view, const uint32_t *__restrict__ toe_row,
                                               const uint8_t *__restrict__ bases, const uint64_t *__restrict__ read_off,
                                               uint64_t n_reads, const uint32_t *__restrict__ order, Done &&done) {
    __shared__ uint32_t s_rd[16][kQueryBlock];
    __shared__ uint8_t s_cmap[256];
    for (uint32_t t = threadIdx.x; t < 256; t += kQueryBlock) s_cmap[t] = view.cmap()[t];
    __syncthreads();

    const uint64_t slot = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
    if (slot >= n_reads) return;
    const uint64_t rd = order ? order[slot] : slot;
    const uint64_t off = read_off[rd];
    const uint64_t m = read_off[rd + 1] - off;

    SearchRange<V> R;
    R.template full<kToe>(view, toe_row);
    uint64_t k = 0;
    SlidingWindow win;
    win.init(off + m - 1);
    for (; k < m; ++k) {
        const uint64_t g = off + m - 1 - k;
        if (__any(win.avail(g) < 1)) win.refill(s_rd, bases, g);
        const uint32_t c = win.get(s_rd, g);
        const uint32_t cidx = s_cmap[c];
        if ((kStopLow && c <= 1) || cidx == kAbsent) break;
        if (!search_step<kToe>(view, toe_row, c, cidx, R)) break;
    }
    done(rd, k, R);
}

template <class V>
__global__ __launch_bounds__(kQueryBlock) void count_kernel(V view, const uint8_t *__restrict__ bases,
                                                            const uint64_t *__restrict__ read_off, uint64_t n_reads,
                                                            uint32_t *__restrict__ mlen_out, uint64_t *__restrict__ occ_out,
                                                            uint64_t *__restrict__ sp_out, const uint32_t *__restrict__ order) {
    longest_suffix<false, false>(view, nullptr, bases, read_off, n_reads, order,
                                 [&](uint64_t rd, uint64_t k, const SearchRange<V> &R) {
                                     uint64_t occ = 0, sp = 0;
                                     if (k > 0) {
                                         sp = view.idx(R.js) + R.os;
                                         occ = view.idx(R.je) + R.oe - sp + 1;
                                     }
                                     mlen_out[rd] = (uint32_t)k;
                                     occ_out[rd] = occ;
                                     if (sp_out) sp_out[rd] = sp;
                                 });
}

// Calls f(view) with the View of the layout the index holds (exactly one of its tables is live):
// the only place that maps a layout to its View.
template <class F>
inline auto with_view(const Index &ix, F &&f) {
    if (ix.line_rows()) return f(CountFatView{ix.table_fat()});
    if (ix.layout() == 3) return f(CountSKView<3>{ix.table_k()});
    if (ix.layout() == 2) return f(CountSKView<2>{ix.table_k()});
    return f(CountOneStepView{ix.table()});
}

// one lane per read
inline dim3 read_grid(uint64_t n_reads) { return dim3((uint32_t)((n_reads + kQueryBlock - 1) / kQueryBlock)); }

// Count queries over whatever layout the index holds.
inline void launch_count(const Index &ix, const uint8_t *d_bases, const uint64_t *d_read_off, uint64_t n_reads,
                         uint32_t *d_mlen, uint64_t *d_occ, uint64_t *d_sp, const uint32_t *d_order, hipStream_t stream) {
    if (n_reads == 0) return;
    with_view(ix, [&](auto view) {
        hipLaunchKernelGGL(count_kernel<decltype(view)>, read_grid(n_reads), dim3(kQueryBlock), 0, stream, view, d_bases, d_read_off,
                           n_reads, d_mlen, d_occ, d_sp, d_order);
    });
}

}  // namespace colbwt
