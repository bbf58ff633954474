// anchors_query.h -- left-maximal exact matches along the whole read (the greedy right-to-left
// factorisation of the read against the text) over every HBM layout of the index, gfx950, wave64.
// Included by capi.hip only.
//
// locate_query.h answers for the read's longest matching suffix and stops at the first base that
// cannot extend it.  Here that base restarts the search instead: the match found so far is emitted as
// a factor (start, len, occ, toehold SA[ep]), the cursors go back to the full range [0, n - 1] and the
// SAME base is tried again from there -- it is the last base of the next factor, or, when even the
// full range has no image for it (a byte <= 1, a character absent from the table, an empty range on a
// synthetic table), a skipped base.  One loop, one trip per base attempt: a trip ends in "extended"
// (the base joins the current factor), "emitted" (the base stays) or "skipped".  The window refill and
// the row loads of the step stay at the top of a trip, where the wave is converged (lane_io.h); a
// restart inside a nested loop would run them under a divergent branch instead.
//
// The step is count_query.h's search_step, the one count and locate take too (kToe: whether the
// toehold is carried; without it no toe_row load happens, so max_occ == 0 needs no locate samples).
// The loop around it is this kernel's own: count's and locate's longest_suffix has no restart.
//
// Slots: read k owns [k * max_anchors, (k+1) * max_anchors) of start / len / occ and max_occ positions
// per slot.  During the search a kept factor's slot gets start, len, occ and pos[0] = SA[ep]; when the
// read is done the lane walks min(occ, max_occ) - 1 phi steps per stored slot (it reads back only words
// it wrote itself) and fills what is left with the NONE values.  So lanes that restart at different
// bases never wait for each other's walks during the search trips.  The summary lives in registers
// and leaves as two 16-byte stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "count_query.h"
#include "locate_query.h"

namespace colbwt {

constexpr uint32_t kAnchorNone = 0xFFFFFFFFu;   // start of a slot past the read's n_stored

struct AnchorsArgs {
    const uint32_t *toe_row;   // kPos only
    PhiTable phi;              // kPos only
    uint32_t min_len, max_anchors, max_occ;
    uint4 *summary;            // two per read: n_factors max_len skipped n_kept | cov n_unique cov_unique n_stored
    uint32_t *start, *len;     // the slot arrays: all three or none
    uint64_t *occ;
    uint64_t *pos;             // kPos: max_occ per slot
};

// kPos: positions are produced (max_occ >= 1 and slot arrays given), so the toehold is carried.
template <class V, bool kPos>
__global__ __launch_bounds__(kQueryBlock) void anchors_kernel(V view, AnchorsArgs A, const uint8_t *__restrict__ bases,
                                                              const uint64_t *__restrict__ read_off, uint64_t n_reads,
                                                              const uint32_t *__restrict__ order) {
    __shared__ uint32_t s_rd[16][kQueryBlock];
    __shared__ uint8_t s_cmap[256];
    for (uint32_t t = threadIdx.x; t < 256; t += kQueryBlock) s_cmap[t] = view.cmap()[t];
    __syncthreads();

    const uint64_t lane = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
    if (lane >= n_reads) return;
    const uint64_t rd = order ? order[lane] : lane;
    const uint64_t off = read_off[rd];
    const uint64_t m = read_off[rd + 1] - off;
    const uint64_t slot0 = rd * A.max_anchors;

    SearchRange<V> R;
    R.template full<kPos>(view, A.toe_row);
    uint32_t L = 0;          // bases of the factor being extended
    uint64_t done = 0;       // bases settled: inside a factor (the current one included) or skipped
    uint32_t n_factors = 0, max_len = 0, skipped = 0, n_kept = 0, cov = 0, n_unique = 0, cov_unique = 0;

    // the factor [start, start + L) ends here: summary, and its slot when it is kept and there is room
    auto emit = [&](uint32_t start) {
        ++n_factors;
        max_len = max(max_len, L);
        if (L < A.min_len) return;
        const uint64_t occ = view.idx(R.je) + R.oe - (view.idx(R.js) + R.os) + 1;
        if (A.start && n_kept < A.max_anchors) {
            const uint64_t s = slot0 + n_kept;
            A.start[s] = start;
            A.len[s] = L;
            A.occ[s] = occ;
            if constexpr (kPos) A.pos[s * A.max_occ] = R.toe;
        }
        ++n_kept;
        cov += L;
        if (occ == 1) {
            ++n_unique;
            cov_unique += L;
        }
    };

    SlidingWindow win;
    win.init(off + m - 1);
    while (done < m) {
        const uint64_t g = off + m - 1 - done;
        if (__any(win.avail(g) < 1)) win.refill(s_rd, bases, g);
        const uint32_t c = win.get(s_rd, g);
        const uint32_t cidx = s_cmap[c];
        if (c > 1 && cidx != kAbsent && search_step<kPos>(view, A.toe_row, c, cidx, R)) {
            ++L;
            ++done;
        } else if (L > 0) {          // the base stays: it is tried again from the full range
            emit((uint32_t)(m - done));
            R.template full<kPos>(view, A.toe_row);
            L = 0;
        } else {                     // not even the full range takes it
            ++skipped;
            ++done;
        }
    }
    if (L > 0) emit(0);

    const uint32_t n_stored = min(n_kept, A.max_anchors);
    A.summary[2 * rd] = make_uint4(n_factors, max_len, skipped, n_kept);
    A.summary[2 * rd + 1] = make_uint4(cov, n_unique, cov_unique, n_stored);
    if (!A.start) return;
    for (uint32_t t = n_stored; t < A.max_anchors; ++t) {
        A.start[slot0 + t] = kAnchorNone;
        A.len[slot0 + t] = 0;
        A.occ[slot0 + t] = 0;
    }
    if constexpr (kPos) {
        for (uint32_t t = 0; t < A.max_anchors; ++t) {
            uint64_t *out = A.pos + (slot0 + t) * A.max_occ;
            uint32_t want = 0;
            if (t < n_stored) {
                want = (uint32_t)min(A.occ[slot0 + t], (uint64_t)A.max_occ);
                uint32_t x = (uint32_t)out[0];
                for (uint32_t q = 1; q < want; ++q) {
                    x = phi_step(A.phi, x);
                    out[q] = x;
                }
            }
            for (uint32_t q = want; q < A.max_occ; ++q) out[q] = kLocateNone;
        }
    }
}

// Anchors over whatever layout the index holds.  A.pos non-null: A.toe_row / A.phi were built for that layout.
inline void launch_anchors(const Index &ix, const AnchorsArgs &A, const uint8_t *d_bases, const uint64_t *d_read_off,
                           uint64_t n_reads, const uint32_t *d_order, hipStream_t stream) {
    if (n_reads == 0) return;
    with_view(ix, [&](auto view) {
        using View = decltype(view);
        const dim3 grid = read_grid(n_reads), block(kQueryBlock);
        if (A.pos)
            hipLaunchKernelGGL((anchors_kernel<View, true>), grid, block, 0, stream, view, A, d_bases, d_read_off, n_reads, d_order);
        else
            hipLaunchKernelGGL((anchors_kernel<View, false>), grid, block, 0, stream, view, A, d_bases, d_read_off, n_reads, d_order);
    });
}

}  // namespace colbwt
