// docs_query.h -- the documents holding each read's longest exact match (include/colbwt.h,
// colbwt_docs_*), reduced on the device to a bit mask per read and a tally per batch, gfx950, wave64.
// Included by capi.hip only.
//
// Four stages on one stream, all over a caller-provided workspace (DocsWork):
//   search  launch_locate (locate_query.h) with max_occ = 1: mlen, occ and toe = SA[ep] per read
//   order   docs_key_kernel makes key = max_walk - w (w = the read's walk length, 0 below min_len) and
//           a hipcub radix sort of (key, read) over the bits of max_walk puts the longest walks first
//   walk    docs_walk_kernel: one lane per read IN SORTED ORDER, so the 64 lanes of a wave walk chains
//           of (nearly) equal length -- in the search lane a wave waits for its largest occ.  Each step
//           is phi_step (one directory load, usually one pair load), a binary search of the position in
//           doc_start, and the bit.  doc_start is staged once per block in LDS (u32, at most kDocsLds
//           documents: more are an argument error).  With one mask word the mask stays in a
//           register; otherwise the lane keeps the current word and flushes it to its own row (zeroed
//           by a memset before the launch) when the word index changes: a row has one owner, so no
//           atomics.  A lane stops once every document is hit.
//   tally   docs_tally_kernel (only when a tally array is given): grid-stride over the reads, a
//           per-block LDS histogram of 2 * n_docs u32 counters (reads per document, reads hitting
//           only that document) by LDS atomics, one global u64 atomicAdd per non-zero counter at the
//           end of the block.  Integer adds: the result does not depend on their order.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "locate_query.h"

namespace colbwt {

constexpr uint32_t kDocsBlock = 256;
constexpr uint32_t kDocsLds = 4096;          // most documents: their starts fit the block's LDS copy (16 KB)
constexpr uint32_t kDocsMaxWalk = 1u << 20;
constexpr uint32_t kDocsTallyGrid = 1024;

// The workspace of one call, cut from a 256-byte aligned buffer of docs_work_bytes(n_reads) bytes.
struct DocsWork {
    uint64_t *toe;          // n_reads: SA[ep] (the one slot of the search's max_occ = 1)
    uint32_t *key[2];       // n_reads each: the sort's double buffer of keys
    uint32_t *val[2];       // n_reads each: ... and of read numbers
    void *sort_tmp;
    size_t sort_tmp_bytes;
};

inline uint64_t docs_align(uint64_t bytes) { return (bytes + 255) & ~255ull; }
// the sort's own workspace: with double buffers hipcub needs histograms and per-block digit counts only
inline uint64_t docs_sort_tmp_bytes(uint64_t n_reads) { return docs_align(16 * n_reads + (1ull << 20)); }
inline uint64_t docs_work_bytes(uint64_t n_reads) {
    return docs_align(8 * n_reads) + 4 * docs_align(4 * n_reads) + docs_sort_tmp_bytes(n_reads);
}
inline DocsWork docs_work(void *d_work, uint64_t n_reads) {
    uint8_t *p = (uint8_t *)d_work;
    DocsWork w;
    w.toe = (uint64_t *)p;
    p += docs_align(8 * n_reads);
    for (int k = 0; k < 2; ++k) {
        w.key[k] = (uint32_t *)p;
        p += docs_align(4 * n_reads);
        w.val[k] = (uint32_t *)p;
        p += docs_align(4 * n_reads);
    }
    w.sort_tmp = p;
    w.sort_tmp_bytes = docs_sort_tmp_bytes(n_reads);
    return w;
}

// key = max_walk - w, so that the ascending sort puts the longest walks first and w = 0 last
__global__ __launch_bounds__(kDocsBlock) void docs_key_kernel(const uint32_t *__restrict__ mlen, const uint64_t *__restrict__ occ,
                                                              uint64_t n_reads, uint32_t min_len, uint32_t max_walk,
                                                              uint32_t *__restrict__ key, uint32_t *__restrict__ val) {
    const uint64_t i = (uint64_t)blockIdx.x * kDocsBlock + threadIdx.x;
    if (i >= n_reads) return;
    const uint32_t w = mlen[i] >= min_len ? (uint32_t)min(occ[i], (uint64_t)max_walk) : 0u;
    key[i] = max_walk - w;
    val[i] = (uint32_t)i;
}

// the document of position x: the largest d with ds[d] <= x (ds ascends from 0, so d = 0 at the least)
__device__ __forceinline__ uint32_t docs_lookup(const uint32_t *ds, uint32_t n_docs, uint32_t x) {
    uint32_t lo = 0, len = n_docs;
    while (len > 1) {
        const uint32_t half = len >> 1;
        if (ds[lo + half] <= x) lo += half;
        len -= half;
    }
    return lo;
}

template <bool ONE_WORD>
__global__ __launch_bounds__(kDocsBlock) void docs_walk_kernel(PhiTable phi, const uint32_t *__restrict__ doc_start, uint32_t n_docs,
                                                               uint32_t n_words, const uint32_t *__restrict__ key,
                                                               const uint32_t *__restrict__ val, const uint64_t *__restrict__ toe,
                                                               uint64_t n_reads, uint32_t max_walk, uint32_t *__restrict__ n_hit_out,
                                                               uint64_t *__restrict__ mask_out) {
    __shared__ uint32_t s_doc[kDocsLds];
    for (uint32_t t = threadIdx.x; t < n_docs; t += kDocsBlock) s_doc[t] = doc_start[t];
    __syncthreads();
    const uint32_t *ds = s_doc;

    const uint64_t slot = (uint64_t)blockIdx.x * kDocsBlock + threadIdx.x;
    if (slot >= n_reads) return;
    const uint64_t rd = val[slot];
    const uint32_t w = max_walk - key[slot];
    uint64_t *row = mask_out + rd * n_words;
    uint32_t n_hit = 0;
    uint64_t cur = 0;          // the bits of word `cw` of the row
    uint32_t cw = 0;
    if (w > 0) {
        uint32_t x = (uint32_t)toe[rd];
        for (uint32_t t = 0;;) {
            const uint32_t d = docs_lookup(ds, n_docs, x);
            if (!ONE_WORD && (d >> 6) != cw) {
                row[cw] = cur;
                cw = d >> 6;
                cur = row[cw];
            }
            const uint64_t bit = 1ull << (d & 63u);
            if (!(cur & bit)) {
                cur |= bit;
                if (++n_hit == n_docs) break;       // every document: nothing left to find
            }
            if (++t == w) break;
            x = phi_step(phi, x);
        }
    }
    if (ONE_WORD || w > 0) row[cw] = cur;           // rows of several words were zeroed before the launch
    n_hit_out[rd] = n_hit;
}

// doc_reads[d] += reads whose mask has bit d, doc_only[d] += those with n_hit == 1, through a per-block
// histogram in LDS (n_docs <= kDocsLds).
__global__ __launch_bounds__(kDocsBlock) void docs_tally_kernel(const uint64_t *__restrict__ mask, const uint32_t *__restrict__ n_hit,
                                                                uint64_t n_reads, uint32_t n_docs, uint32_t n_words,
                                                                unsigned long long *__restrict__ doc_reads,
                                                                unsigned long long *__restrict__ doc_only) {
    __shared__ uint32_t s_hist[2 * kDocsLds];
    for (uint32_t t = threadIdx.x; t < 2 * n_docs; t += kDocsBlock) s_hist[t] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * kDocsBlock + threadIdx.x; i < n_reads; i += (uint64_t)gridDim.x * kDocsBlock) {
        const uint32_t hits = n_hit[i];
        if (hits == 0) continue;
        const uint64_t *row = mask + i * n_words;
        for (uint32_t wi = 0; wi < n_words; ++wi) {
            uint64_t m = row[wi];
            while (m) {
                const uint32_t d = wi * 64u + (uint32_t)__builtin_ctzll(m);
                m &= m - 1;
                atomicAdd(&s_hist[d], 1u);
                if (hits == 1) atomicAdd(&s_hist[n_docs + d], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < n_docs; t += kDocsBlock) {
        const uint32_t a = s_hist[t], b = s_hist[n_docs + t];
        if (doc_reads && a) atomicAdd(&doc_reads[t], (unsigned long long)a);
        if (doc_only && b) atomicAdd(&doc_only[t], (unsigned long long)b);
    }
}

struct DocsArgs {
    const uint32_t *toe_row;       // the replica's locate tables
    PhiTable phi;
    const uint32_t *doc_start;     // device copy, n_docs entries
    uint32_t n_docs;
    uint32_t min_len, max_walk;
};

inline uint32_t docs_mask_words(uint32_t n_docs) { return (n_docs + 63) / 64; }

// All stages for a batch in HBM.  d_mlen / d_occ / d_n_hit n_reads entries, d_mask n_reads * W words;
// d_doc_reads / d_doc_only (nullable, n_docs u64 each) are ADDED to.  d_order goes to the search only.
// n_docs <= kDocsLds (the entry points check it).
inline hipError_t launch_docs(const Index &ix, const DocsArgs &a, const uint8_t *d_bases, const uint64_t *d_read_off,
                              uint64_t n_reads, uint32_t *d_mlen, uint64_t *d_occ, uint32_t *d_n_hit, uint64_t *d_mask,
                              uint64_t *d_doc_reads, uint64_t *d_doc_only, void *d_work, const uint32_t *d_order,
                              hipStream_t stream) {
    if (n_reads == 0) return hipSuccess;
    if (a.n_docs > kDocsLds) return hipErrorInvalidValue;
    const DocsWork w = docs_work(d_work, n_reads);
    const uint32_t n_words = docs_mask_words(a.n_docs);
    const dim3 grid((uint32_t)((n_reads + kDocsBlock - 1) / kDocsBlock)), block(kDocsBlock);

    launch_locate(ix, a.toe_row, a.phi, d_bases, d_read_off, n_reads, 1, d_mlen, d_occ, w.toe, d_order, stream);

    hipLaunchKernelGGL(docs_key_kernel, grid, block, 0, stream, d_mlen, d_occ, n_reads, a.min_len, a.max_walk, w.key[0], w.val[0]);
    int bits = 1;
    while (bits < 32 && (a.max_walk >> bits)) ++bits;      // keys are 0 .. max_walk
    hipcub::DoubleBuffer<uint32_t> keys(w.key[0], w.key[1]), vals(w.val[0], w.val[1]);
    size_t need = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, need, keys, vals, (size_t)n_reads, 0, bits, stream);
    if (e != hipSuccess) return e;
    if (need > w.sort_tmp_bytes) return hipErrorOutOfMemory;
    need = w.sort_tmp_bytes;
    e = hipcub::DeviceRadixSort::SortPairs(w.sort_tmp, need, keys, vals, (size_t)n_reads, 0, bits, stream);
    if (e != hipSuccess) return e;

    const uint32_t *sk = keys.Current(), *sv = vals.Current();
    if (n_words == 1) {
        hipLaunchKernelGGL(docs_walk_kernel<true>, grid, block, 0, stream, a.phi, a.doc_start, a.n_docs, n_words, sk, sv,
                           w.toe, n_reads, a.max_walk, d_n_hit, d_mask);
    } else {
        e = hipMemsetAsync(d_mask, 0, (size_t)n_reads * n_words * sizeof(uint64_t), stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(docs_walk_kernel<false>, grid, block, 0, stream, a.phi, a.doc_start, a.n_docs, n_words, sk, sv, w.toe,
                           n_reads, a.max_walk, d_n_hit, d_mask);
    }
    if (d_doc_reads || d_doc_only) {
        const dim3 tgrid(std::min<uint32_t>(grid.x, kDocsTallyGrid));
        unsigned long long *dr = (unsigned long long *)d_doc_reads, *dn = (unsigned long long *)d_doc_only;
        hipLaunchKernelGGL(docs_tally_kernel, tgrid, block, 0, stream, d_mask, d_n_hit, n_reads, a.n_docs, n_words, dr, dn);
    }
    return hipSuccess;
}

}  // namespace colbwt
