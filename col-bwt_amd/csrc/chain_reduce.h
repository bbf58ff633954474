// chain_reduce.h -- the best colinear chain of each read's anchors (include/colbwt.h, colbwt_chain_*),
// reduced on the device from the slot arrays of colbwt_anchors_* to one 32-byte record per read, gfx950,
// wave64.  Included by capi.hip only.
//
// Lanes as hits, anchors as steps.  A group of G lanes (a power of two, 8 .. 64; 64 / G reads share a wave)
// owns a read; lane g of the group holds the hits g, g + G, .. (R = ceil(max_anchors * max_occ / G) <= 4 of
// them) in registers: t, s, l, document, the best candidate so far and its predecessor.  Hit h = a * max_occ + q
// is position q of slot a, so the order of the hits is the order of the slots.
//
// A hit may only follow hits of SMALLER slots, and all hits of one slot share s and l.  So the dynamic
// program does not walk the hits one by one with a cross-lane reduction for each (max_anchors * max_occ steps
// of log2 G shuffles of a 64-bit key): it walks the SLOTS.  At step a the owners of slot a's hits have seen
// every possible predecessor, so they finalise f and publish it in the read's LDS tile (f and the predecessor
// in u32 arrays of their own, so that the lanes' stores fall on consecutive banks; beside them one 16-byte
// record per hit: t, document, s); then every lane reads the step's max_occ records and scores -- one
// address per group, so the reads are broadcasts without bank conflicts -- and offers them to its own
// later hits.  Candidates arrive in ascending j and replace the best only when strictly larger, which is the
// smallest-j tie-break; the best starts at 0, which is the "only when f(j) - drift > 0" rule.  max_anchors
// steps, each one LDS hand-over inside a wave (wave_sync: no instruction, the LDS serves a wave's requests in
// order) and max_occ * R candidate evaluations per lane, instead of max_anchors * max_occ reductions.
//
// The end of the best chain is a shuffle max-reduction over (f, inverted hit number) within the group; the
// backtrack follows the predecessors in the LDS tile (every lane of the group walks the same chain, all reads
// are broadcasts) and gives the text interval; the second pass marks the hits inside that interval dead in the
// tile (one store into the 16-byte records per pass, four lanes to a bank) and runs the same steps again over
// the same registers for score2.  doc_start is staged once per block in LDS as docs_walk_kernel stages it
// (u32, at most kDocsLds documents).
//
// No atomics, no inline assembly, no scratch (every register array is indexed by an unrolled constant);
// lane 0 of a group is the one writer of the read's record, as two 16-byte stores.  No lane leaves early:
// groups past the last read run on dead hits, so every wave_sync and shuffle is met by the whole wave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "anchors_query.h"
#include "docs_query.h"
#include "lane_io.h"

namespace colbwt {

constexpr uint32_t kChainBlock = 256;
constexpr uint32_t kChainMaxHits = 256;          // max_anchors * max_occ: 64 lanes x 4 hits
constexpr uint32_t kChainDead = 0xFFFFFFFFu;     // document of a hit that takes no part in the pass
constexpr uint32_t kChainNoPred = 0xFFFFFFFFu;

struct ChainArgs {
    const uint32_t *start, *len;   // n_reads * max_anchors
    const uint64_t *pos;           // n_reads * max_anchors * max_occ
    const uint32_t *doc_start;     // device copy, n_docs <= kDocsLds entries
    uint32_t n_docs;
    uint32_t max_anchors, max_occ, band;
    uint4 *chain;                  // two per read
};

// the document of position t: the largest d with ds[d] <= t (docs_lookup for a 64-bit position)
__device__ __forceinline__ uint32_t chain_doc(const uint32_t *ds, uint32_t n_docs, uint64_t t) {
    uint32_t lo = 0, len = n_docs;
    while (len > 1) {
        const uint32_t half = len >> 1;
        if ((uint64_t)ds[lo + half] <= t) lo += half;
        len -= half;
    }
    return lo;
}

template <uint32_t G, typename T>
__device__ __forceinline__ T chain_group_max(T v) {
#pragma unroll
    for (uint32_t m = 1; m < G; m <<= 1) {
        const T o = __shfl_xor(v, (int)m);
        v = o > v ? o : v;
    }
    return v;
}

// One pass of the dynamic program over the hits whose tile record is not kChainDead (`on`: this lane's).
// Writes f and pred of those hits into the tile and leaves f in `f` (0 for the others).
template <uint32_t G, uint32_t R>
__device__ __forceinline__ void chain_pass(const uint4 *hit, uint32_t *fs, uint32_t *pred, uint32_t g, uint32_t K, uint32_t M,
                                           uint32_t band, const uint64_t (&t)[R], const uint32_t (&s)[R], const uint32_t (&l)[R],
                                           const uint32_t (&a)[R], const uint32_t (&doc)[R], const bool (&on)[R], uint32_t (&f)[R]) {
    int64_t best[R];
    uint32_t from[R];
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) {
        best[r] = 0;
        from[r] = kChainNoPred;
        f[r] = 0;
    }
    for (uint32_t aj = 0; aj < K; ++aj) {
#pragma unroll
        for (uint32_t r = 0; r < R; ++r)
            if (on[r] && a[r] == aj) {       // every predecessor has been offered: f(i) = l_i + max(0, ..), saturated
                const int64_t v = (int64_t)l[r] + best[r];
                f[r] = v > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)v;
                fs[g + r * G] = f[r];
                pred[g + r * G] = from[r];
            }
        wave_sync();
        const uint32_t j0 = aj * M;
        const int64_t sj = (int64_t)hit[j0].w;
        for (uint32_t q = 0; q < M; ++q) {
            const uint4 hj = hit[j0 + q];
            if (hj.z == kChainDead) continue;
            const uint64_t tj = ((uint64_t)hj.y << 32) | hj.x;
            const int64_t fj = (int64_t)fs[j0 + q];
#pragma unroll
            for (uint32_t r = 0; r < R; ++r) {
                if (!on[r] || a[r] <= aj || doc[r] != hj.z) continue;
                const int64_t gr = sj - ((int64_t)s[r] + (int64_t)l[r]);
                const int64_t gt = (int64_t)(tj - (t[r] + (uint64_t)l[r]));
                if (gr < 0 || gt < 0) continue;
                const int64_t drift = gt > gr ? gt - gr : gr - gt;
                if (drift > (int64_t)band) continue;
                const int64_t cand = fj - drift;
                if (cand > best[r]) {
                    best[r] = cand;
                    from[r] = j0 + q;
                }
            }
        }
    }
    wave_sync();
}

template <uint32_t G, uint32_t R>
__global__ __launch_bounds__(kChainBlock) void chain_kernel(ChainArgs A, uint64_t n_reads) {
    constexpr uint32_t kReads = kChainBlock / G;      // reads of a block
    constexpr uint32_t kTile = G * R;                 // hit records of a read
    __shared__ uint32_t s_doc[kDocsLds];
    __shared__ uint4 s_hit[kReads * kTile];           // t (lo, hi), document or kChainDead, s
    __shared__ uint32_t s_len[kReads * kTile];
    __shared__ uint32_t s_f[kReads * kTile];          // written at every step: arrays of their own, a lane a bank
    __shared__ uint32_t s_pred[kReads * kTile];
    for (uint32_t k = threadIdx.x; k < A.n_docs; k += kChainBlock) s_doc[k] = A.doc_start[k];
    __syncthreads();

    const uint32_t g = threadIdx.x % G, grp = threadIdx.x / G;
    const uint64_t rd = (uint64_t)blockIdx.x * kReads + grp;
    const bool have = rd < n_reads;
    const uint32_t K = A.max_anchors, M = A.max_occ, H = K * M;     // H <= kTile (the launcher picks G and R)
    uint4 *hit = s_hit + grp * kTile;
    uint32_t *len = s_len + grp * kTile;
    uint32_t *fs = s_f + grp * kTile;
    uint32_t *pred = s_pred + grp * kTile;

    uint64_t t[R];
    uint32_t s[R], l[R], a[R], doc[R], f[R];
    bool on[R];
    uint32_t n_hits = 0;
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t h = g + r * G;
        a[r] = h / M;
        t[r] = 0;
        s[r] = kAnchorNone;
        l[r] = 0;
        if (have && h < H) {
            s[r] = A.start[rd * K + a[r]];
            l[r] = A.len[rd * K + a[r]];
            t[r] = A.pos[rd * H + h];
        }
        on[r] = s[r] != kAnchorNone && t[r] != kLocateNone;
        doc[r] = on[r] ? chain_doc(s_doc, A.n_docs, t[r]) : kChainDead;
        n_hits += on[r] ? 1u : 0u;
        hit[h] = make_uint4((uint32_t)t[r], (uint32_t)(t[r] >> 32), doc[r], s[r]);
        len[h] = l[r];
        fs[h] = 0;
        pred[h] = kChainNoPred;
    }
#pragma unroll
    for (uint32_t m = 1; m < G; m <<= 1) n_hits += __shfl_xor(n_hits, (int)m);

    chain_pass<G, R>(hit, fs, pred, g, K, M, A.band, t, s, l, a, doc, on, f);

    // the end of the best chain: the largest f, the smallest hit number among equals (a live key is never 0)
    uint64_t key = 0;
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) {
        const uint64_t k = on[r] ? ((uint64_t)f[r] << 32) | (0xFFFFFFFFu - (g + r * G)) : 0ull;
        key = k > key ? k : key;
    }
    key = chain_group_max<G>(key);

    uint64_t text_begin = kLocateNone;
    uint32_t text_len = 0, read_begin = 0, read_end = 0, score = 0, score2 = 0, n_chained = 0;
    if (key != 0) {
        const uint32_t e = 0xFFFFFFFFu - (uint32_t)key;
        uint32_t b = e;
        n_chained = 1;
        for (uint32_t p = pred[b]; p != kChainNoPred; p = pred[b]) {     // p < b: at most max_anchors hits
            b = p;
            ++n_chained;
        }
        const uint4 he = hit[e], hb = hit[b];
        const uint32_t lb = len[b];
        text_begin = ((uint64_t)he.y << 32) | he.x;
        const uint64_t text_end = (((uint64_t)hb.y << 32) | hb.x) + lb;
        const uint64_t span = text_end - text_begin;
        text_len = span > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)span;
        read_begin = he.w;
        read_end = hb.w + lb;
        score = (uint32_t)(key >> 32);
        // the runner-up: the same program over the hits outside [text_begin, text_end)
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) on[r] = on[r] && (t[r] + (uint64_t)l[r] <= text_begin || t[r] >= text_end);
    }
    wave_sync();     // the backtrack has read the tile: now the second pass may overwrite it
#pragma unroll
    for (uint32_t r = 0; r < R; ++r)
        if (!on[r]) hit[g + r * G].z = kChainDead;
    wave_sync();
    chain_pass<G, R>(hit, fs, pred, g, K, M, A.band, t, s, l, a, doc, on, f);
    uint32_t f2 = 0;
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) f2 = on[r] && f[r] > f2 ? f[r] : f2;
    score2 = chain_group_max<G>(f2);

    if (have && g == 0) {
        A.chain[2 * rd] = make_uint4((uint32_t)text_begin, (uint32_t)(text_begin >> 32), text_len, read_begin);
        A.chain[2 * rd + 1] = make_uint4(read_end, score, score2, n_chained | (n_hits << 16));
    }
}

// G and R of a setting: the smallest group that holds max_anchors * max_occ hits at one per lane, else 64
// lanes with 2 .. 4 hits each.
inline void chain_shape(uint32_t hits, uint32_t &G, uint32_t &R) {
    G = 8;
    while (G < 64 && G < hits) G <<= 1;
    R = (hits + G - 1) / G;
}

// The reduction for n_reads reads in HBM.  1 <= max_anchors * max_occ <= kChainMaxHits and n_docs <= kDocsLds
// (the entry points check both).
inline hipError_t launch_chain(const ChainArgs &A, uint64_t n_reads, hipStream_t stream) {
    if (n_reads == 0) return hipSuccess;
    const uint64_t hits = (uint64_t)A.max_anchors * A.max_occ;
    if (hits == 0 || hits > kChainMaxHits || A.n_docs > kDocsLds) return hipErrorInvalidValue;
    uint32_t G, R;
    chain_shape((uint32_t)hits, G, R);
    const dim3 grid((uint32_t)((n_reads + kChainBlock / G - 1) / (kChainBlock / G))), block(kChainBlock);
    if (G == 8) hipLaunchKernelGGL((chain_kernel<8, 1>), grid, block, 0, stream, A, n_reads);
    else if (G == 16) hipLaunchKernelGGL((chain_kernel<16, 1>), grid, block, 0, stream, A, n_reads);
    else if (G == 32) hipLaunchKernelGGL((chain_kernel<32, 1>), grid, block, 0, stream, A, n_reads);
    else if (R == 1) hipLaunchKernelGGL((chain_kernel<64, 1>), grid, block, 0, stream, A, n_reads);
    else if (R == 2) hipLaunchKernelGGL((chain_kernel<64, 2>), grid, block, 0, stream, A, n_reads);
    else if (R == 3) hipLaunchKernelGGL((chain_kernel<64, 3>), grid, block, 0, stream, A, n_reads);
    else hipLaunchKernelGGL((chain_kernel<64, 4>), grid, block, 0, stream, A, n_reads);
    return hipSuccess;
}

}  // namespace colbwt
