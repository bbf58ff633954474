// seeds_reduce.h -- per-read PML peaks ("seeds") and chain summaries reduced on the device from
// the per-base output of the query (include/colbwt.h, colbwt_seeds_*), gfx950, wave64.  Included by
// capi.hip only (the one translation unit that launches it).  Needs no index: its input is the pml /
// cid / read_off arrays of a colbwt_query_device call.
//
// Work is cut by BASES: wave w owns the reads whose first base lies in [w * chunk, (w+1) * chunk)
// (two lane-parallel 64-ary searches over read_off), i.e. the whole reads covering bases [A, B).  It
// streams that range once, from its end down, in tiles of 512 bases on 512-base boundaries: lane l
// holds the 8 bases at tile + 8l (one 16-byte load of u16 PML values, two of u32, 8 bytes of col
// ids), so a wave instruction covers consecutive lines.  Going DOWN is the order the query computes
// in: a run's seed (pos = its first base) is the last thing met of the run, by then the run's "last
// non-zero col id" is its id, and seeds come in slot order (largest pos first), so a seed's slot is
// the read's running count -- no atomics, no second pass.
//
// Per tile:
//   marks   the lanes walk the wave's read boundaries down from a wave-uniform cursor, 64 at a
//           time, and mark in LDS the LAST base of every non-empty read that ends in the tile with
//           its read number (one writer per base); empty reads get their summary right there
//   masks   a lane sees run boundaries in its own 8 values, the marks, and the one element below
//           its first (the neighbouring lane's, by ballot; lane 0 loads pml[tile - 1])
//   carries what enters a lane from the bases above it, in three rounds because each feeds the next:
//           the open run's col id and the current read (hand-over through LDS: value of the
//           nearest lane above that sets it, found in a ballot mask), then the id of the previous
//           col-carrying seed (same), then the read's counters so far (segmented wave suffix
//           scans with __shfl_down, segments closed by the lanes holding a mark; three 10-bit and
//           two 16-bit counters share a word each, a tile adds at most 512 to any of them)
//   emit    every lane walks its 8 bases once more with its carries: slots of the counting seeds,
//           the summary at the first base of a read
// Lane 0's state after the tile goes to all lanes through LDS (wave-uniform: the read that crosses
// into the next tile), so a read may be as long as the API allows; it is then one wave's work.
// Unused slots are what the launch's three memsets left.
//
// The chunk is seeds_chunk(n_bases), 2048..16384 by batch size.  COLBWT_SEEDS_CHUNK=<bases>, read at
// every launch like COLBWT_LINE_ROWS_CHUNK (fat_cursor.h), replaces it with a multiple of 512 in
// 512..16384; 512..1536 is below anything production picks and exists so that small inputs have many waves.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "lane_io.h"

namespace colbwt {

constexpr uint32_t kSeedsBlock = 256;
constexpr uint32_t kSeedsWaves = kSeedsBlock / 64;
constexpr uint32_t kSeedsTile = 512;             // bases per wave iteration: 64 lanes x 8
constexpr uint32_t kSeedsNoMark = 0xFFFFFFFFu;
constexpr uint32_t kSeedsSummaryWords = 8;       // colbwt_seed_summary

struct SeedsOut {
    uint32_t *summary;   // n_reads x 8
    uint32_t *pos;       // n_reads x max_seeds, or nullptr (then len and cid too)
    uint32_t *len;
    uint8_t *cid;
    uint32_t min_len, max_seeds;
};

struct SeedsState {
    uint32_t n_seeds, max_len, cov, resets, n_col, col_cov, asc, desc;
    uint32_t x;     // last non-zero col id of the open run
    uint32_t y;     // id of the previous col-carrying counting seed of the read
    uint32_t rid;   // the read
};

// What a lane holds of a tile.
struct SeedsLane {
    uint32_t p[8];        // PML values
    uint32_t c[8];        // col ids
    uint32_t m[8];        // read number when the base is the last of a read, else kSeedsNoMark
    uint32_t valid;       // bit j: base g0 + j belongs to the wave's range
    bool mark_below;      // base g0 - 1 is the last of a read
    bool zero_below;      // pml[g0 - 1] == 0
    uint64_t g0;
};

// first b in [0, n_entries) with off[b] >= target, n_entries when there is none; the whole wave
// calls it with the same arguments
__device__ __forceinline__ uint64_t seeds_lower_bound(const uint64_t *__restrict__ off, uint64_t n_entries, uint64_t target,
                                                      uint32_t lane) {
    uint64_t lo = 0, hi = n_entries;
    while (lo < hi) {
        const uint64_t step = (hi - lo + 63) / 64;
        const uint64_t p = lo + lane * step;
        const bool less = p < hi && off[p] < target;
        const uint32_t cnt = (uint32_t)__builtin_popcountll(__ballot(less));   // off ascends: a prefix of the lanes
        if (cnt == 0) {
            hi = lo;
        } else {
            const uint64_t last = lo + (cnt - 1) * step;
            lo = last + 1;
            hi = last + step < hi ? last + step : hi;
        }
    }
    return lo;
}

__device__ __forceinline__ void seeds_write_summary(uint32_t *__restrict__ summary, uint64_t rid, const SeedsState &s) {
    uint4 *q = reinterpret_cast<uint4 *>(summary + rid * kSeedsSummaryWords);
    q[0] = make_uint4(s.n_seeds, s.max_len, s.cov, s.resets);
    q[1] = make_uint4(s.n_col, s.col_cov, s.asc, s.desc);
}

// The lane's 8 bases from the top one down, from state `s` (what enters the lane from above).
// x_pass / y_pass: nothing in the lane set x / y (what entered is what leaves).  A mark starts a read:
// the counters restart, so what is left in `s` is the part below the lane's lowest mark.
template <bool EMIT>
__device__ __forceinline__ void seeds_walk(const SeedsLane &L, uint64_t A, const uint64_t *__restrict__ off, const SeedsOut &out,
                                           SeedsState &s, bool &x_pass, bool &y_pass) {
    x_pass = y_pass = true;
#pragma unroll
    for (int j = 7; j >= 0; --j) {
        if (!((L.valid >> j) & 1u)) continue;
        const uint64_t g = L.g0 + (uint32_t)j;
        if (L.m[j] != kSeedsNoMark) {
            s.n_seeds = s.max_len = s.cov = s.resets = s.n_col = s.col_cov = s.asc = s.desc = 0;
            s.x = s.y = 0;
            s.rid = L.m[j];
            x_pass = y_pass = false;
        }
        const uint32_t pv = L.p[j];
        const bool mark_below = j > 0 ? L.m[j > 0 ? j - 1 : 0] != kSeedsNoMark : L.mark_below;
        const bool first = g == A || mark_below;            // first base of its read
        s.max_len = max(s.max_len, pv);
        if (pv == 0) {
            ++s.resets;
            s.x = 0;
            x_pass = false;
        } else {
            if (L.c[j]) {
                s.x = L.c[j];
                x_pass = false;
            }
            const bool zero_below = j > 0 ? L.p[j > 0 ? j - 1 : 0] == 0 : L.zero_below;
            if (first || zero_below) {                      // the run's first base: its seed
                const uint32_t id = s.x;
                s.x = 0;
                x_pass = false;
                if (pv >= out.min_len) {
                    if (EMIT && out.pos && s.n_seeds < out.max_seeds && s.rid != kSeedsNoMark) {
                        const uint64_t at = (uint64_t)s.rid * out.max_seeds + s.n_seeds;
                        out.pos[at] = (uint32_t)(g - off[s.rid]);
                        out.len[at] = pv;
                        out.cid[at] = (uint8_t)id;
                    }
                    ++s.n_seeds;
                    s.cov += pv;
                    if (id) {
                        ++s.n_col;
                        s.col_cov += pv;
                        if (s.y) {                          // a = id (smaller pos), b = y
                            const uint32_t d = (s.y + 255u - id) % 255u;
                            s.asc += d >= 1 && d <= 127;
                            s.desc += d >= 128;
                        }
                        s.y = id;
                        y_pass = false;
                    }
                }
            }
        }
        if (EMIT && first && s.rid != kSeedsNoMark) seeds_write_summary(out.summary, s.rid, s);
    }
}

// Exclusive segmented suffix scan over the wave: lane l gets op over the values of lanes l+1 .. h,
// h = the nearest lane above l whose bit is set in `closed` (63 when there is none); `none` when l = 63.
template <bool MAX>
__device__ __forceinline__ uint32_t seeds_scan_above(uint32_t v, uint64_t closed, uint32_t lane, uint32_t none) {
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_down(v, (int)d);
        const bool open = lane + d < 64 && ((closed >> lane) & ((1ull << d) - 1)) == 0;   // no closing lane in [l, l + d)
        if (open) v = MAX ? max(v, t) : v + t;
    }
    const uint32_t t = __shfl_down(v, 1);
    return lane < 63 ? t : none;
}

template <typename PmlT>
__global__ __launch_bounds__(kSeedsBlock) void seeds_reduce_kernel(const PmlT *__restrict__ pml, const uint8_t *__restrict__ cid,
                                                                   const uint64_t *__restrict__ off, uint64_t n_reads,
                                                                   uint64_t n_bases, uint64_t chunk, uint64_t n_waves,
                                                                   SeedsOut out) {
    __shared__ uint32_t s_mark[kSeedsWaves][kSeedsTile];
    __shared__ uint32_t s_hand[kSeedsWaves][2][64];
    __shared__ uint32_t s_carry[kSeedsWaves][12];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t w = (uint64_t)blockIdx.x * kSeedsWaves + wv;
    if (w >= n_waves) return;

    // the wave's reads [r0, r1): those starting in its chunk of the bases (the last wave: to the end)
    uint64_t r0 = seeds_lower_bound(off, n_reads + 1, w * chunk, lane);
    uint64_t r1 = w + 1 == n_waves ? n_reads : seeds_lower_bound(off, n_reads + 1, (w + 1) * chunk, lane);
    r0 = r0 < n_reads ? r0 : n_reads;
    r1 = r1 < n_reads ? r1 : n_reads;
    if (r1 <= r0) return;
    const uint64_t A = off[r0], B = off[r1];
    const uint64_t tile_lo = A & ~(uint64_t)(kSeedsTile - 1);
    uint64_t bc = r1;          // boundaries r0+1 .. r1 (read b-1 ends at off[b]), the next one to take
    SeedsState carry{};        // wave-uniform: lane 0's state after the tile above
    carry.rid = kSeedsNoMark;
    const uint64_t above = lane < 63 ? ~0ull << (lane + 1) : 0;   // the lanes above this one
    uint32_t *mark = s_mark[wv];

    for (uint64_t tile = (B > A ? B - 1 : A) & ~(uint64_t)(kSeedsTile - 1);; tile -= kSeedsTile) {
        const bool last = tile == tile_lo;
        SeedsLane L;
        L.g0 = tile + 8u * lane;
        // ---- the lane's 8 values ----
        if (L.g0 + 8 <= n_bases) {
            if (sizeof(PmlT) == 2) {
                const uint4 v = *reinterpret_cast<const uint4 *>(pml + L.g0);
                L.p[0] = v.x & 0xFFFFu; L.p[1] = v.x >> 16; L.p[2] = v.y & 0xFFFFu; L.p[3] = v.y >> 16;
                L.p[4] = v.z & 0xFFFFu; L.p[5] = v.z >> 16; L.p[6] = v.w & 0xFFFFu; L.p[7] = v.w >> 16;
            } else {
                const uint4 v = *reinterpret_cast<const uint4 *>(pml + L.g0), u = *reinterpret_cast<const uint4 *>(pml + L.g0 + 4);
                L.p[0] = v.x; L.p[1] = v.y; L.p[2] = v.z; L.p[3] = v.w;
                L.p[4] = u.x; L.p[5] = u.y; L.p[6] = u.z; L.p[7] = u.w;
            }
            const uint2 k = *reinterpret_cast<const uint2 *>(cid + L.g0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                L.c[j] = (k.x >> (8 * j)) & 0xFFu;
                L.c[4 + j] = (k.y >> (8 * j)) & 0xFFu;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool in = L.g0 + (uint32_t)j < n_bases;
                L.p[j] = in ? (uint32_t)pml[L.g0 + (uint32_t)j] : 0;
                L.c[j] = in ? (uint32_t)cid[L.g0 + (uint32_t)j] : 0;
            }
        }
        L.valid = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) L.valid |= (uint32_t)(L.g0 + (uint32_t)j >= A && L.g0 + (uint32_t)j < B) << j;

        // ---- marks: the last base of every read that ends in the tile ----
#pragma unroll
        for (int j = 0; j < 8; ++j) mark[8 * lane + j] = kSeedsNoMark;
        wave_sync();
        for (;;) {
            const bool have = bc >= r0 + 1 + lane;
            const uint64_t b = have ? bc - lane : r0 + 1;
            const uint64_t ob = have ? off[b] : 0, oa = have ? off[b - 1] : 0;
            const bool take = have && (ob > tile || last);
            if (take) {
                if (oa == ob) {                       // an empty read
                    SeedsState z{};
                    seeds_write_summary(out.summary, b - 1, z);
                } else if (ob - 1 >= tile && ob - 1 - tile < kSeedsTile) {
                    mark[ob - 1 - tile] = (uint32_t)(b - 1);
                }
            }
            const uint32_t cnt = (uint32_t)__builtin_popcountll(__ballot(take));   // a prefix of the lanes
            bc -= cnt;
            if (cnt < 64) break;
        }
        wave_sync();
#pragma unroll
        for (int j = 0; j < 8; ++j) L.m[j] = mark[8 * lane + j];
        // the element below the lane's first: the neighbouring lane's, or (lane 0) the next tile's
        const uint64_t zero7 = __ballot(L.p[7] == 0);
        if (lane > 0) {
            L.mark_below = mark[8 * lane - 1] != kSeedsNoMark;
            L.zero_below = (zero7 >> (lane - 1)) & 1u;
        } else {
            const bool inside = tile > A;             // base tile - 1 belongs to the wave's range
            L.mark_below = inside && off[bc] == tile;  // bc: the largest boundary at or below the tile's first base
            L.zero_below = inside ? pml[tile - 1] == 0 : true;
        }
        uint32_t low_mark = kSeedsNoMark;             // the lane's lowest mark
#pragma unroll
        for (int j = 7; j >= 0; --j)
            if (L.m[j] != kSeedsNoMark) low_mark = L.m[j];
        const uint64_t closed = __ballot(low_mark != kSeedsNoMark);   // lanes where a read starts (going down)

        // ---- round 1: the open run's col id and the read entering each lane ----
        SeedsState in{};
        bool x_pass, y_pass;
        {
            SeedsState s{};
            seeds_walk<false>(L, A, off, out, s, x_pass, y_pass);
            const uint64_t x_set = __ballot(!x_pass) & above;
            s_hand[wv][0][lane] = s.x;
            s_hand[wv][1][lane] = low_mark;
            wave_sync();
            in.x = x_set ? s_hand[wv][0][__builtin_ctzll(x_set)] : carry.x;
            in.rid = (closed & above) ? s_hand[wv][1][__builtin_ctzll(closed & above)] : carry.rid;
            wave_sync();
        }
        // ---- round 2: the id of the previous col-carrying seed ----
        {
            SeedsState s{};
            s.x = in.x;
            seeds_walk<false>(L, A, off, out, s, x_pass, y_pass);
            const uint64_t y_set = __ballot(!y_pass) & above;
            s_hand[wv][0][lane] = s.y;
            wave_sync();
            in.y = y_set ? s_hand[wv][0][__builtin_ctzll(y_set)] : carry.y;
            wave_sync();
        }
        // ---- round 3: the read's counters so far ----
        {
            SeedsState s{};
            s.x = in.x;
            s.y = in.y;
            seeds_walk<false>(L, A, off, out, s, x_pass, y_pass);
            const uint32_t a = seeds_scan_above<false>(s.n_seeds | s.resets << 10 | s.n_col << 20, closed, lane, 0);
            const uint32_t c = seeds_scan_above<false>(s.asc | s.desc << 16, closed, lane, 0);
            in.n_seeds = a & 0x3FFu;
            in.resets = (a >> 10) & 0x3FFu;
            in.n_col = a >> 20;
            in.asc = c & 0xFFFFu;
            in.desc = c >> 16;
            in.cov = seeds_scan_above<false>(s.cov, closed, lane, 0);
            in.col_cov = seeds_scan_above<false>(s.col_cov, closed, lane, 0);
            in.max_len = seeds_scan_above<true>(s.max_len, closed, lane, 0);
            if (!(closed & above)) {                  // the read of the tile above reaches this lane
                in.n_seeds += carry.n_seeds;
                in.resets += carry.resets;
                in.n_col += carry.n_col;
                in.asc += carry.asc;
                in.desc += carry.desc;
                in.cov += carry.cov;
                in.col_cov += carry.col_cov;
                in.max_len = max(in.max_len, carry.max_len);
            }
        }
        // ---- emit ----
        seeds_walk<true>(L, A, off, out, in, x_pass, y_pass);
        if (last) break;
        if (lane == 0) {
            uint32_t *q = s_carry[wv];
            q[0] = in.n_seeds; q[1] = in.max_len; q[2] = in.cov; q[3] = in.resets; q[4] = in.n_col; q[5] = in.col_cov;
            q[6] = in.asc; q[7] = in.desc; q[8] = in.x; q[9] = in.y; q[10] = in.rid;
        }
        wave_sync();
        {
            const uint32_t *q = s_carry[wv];
            carry.n_seeds = q[0]; carry.max_len = q[1]; carry.cov = q[2]; carry.resets = q[3]; carry.n_col = q[4];
            carry.col_cov = q[5]; carry.asc = q[6]; carry.desc = q[7]; carry.x = q[8]; carry.y = q[9]; carry.rid = q[10];
        }
        wave_sync();
    }
}

// bases per wave: long enough to amortise the wave's two searches, short enough that a batch fills the chip
inline uint64_t seeds_chunk(uint64_t n_bases) {
    // "<bases>": the tests' way to every chunk size, and to many waves, at batch sizes they can compare in
    // full (tests/emu/seeds_emu.py depends on it); anything but a multiple of 512 in 512..16384 is ignored
    if (const char *e = getenv("COLBWT_SEEDS_CHUNK")) {
        char *end = nullptr;
        const unsigned long long v = strtoull(e, &end, 10);
        if (*e >= '0' && *e <= '9' && *end == 0 && v >= kSeedsTile && v <= 16384 && v % kSeedsTile == 0) return v;
    }
    const uint64_t per = (n_bases / 65536 + kSeedsTile - 1) / kSeedsTile * kSeedsTile;
    return per < 2048 ? 2048 : per > 16384 ? 16384 : per;
}

// The pass over buffers a query filled.  pml_bytes 2 or 4; d_pos / d_len / d_scid all null or none.
inline hipError_t launch_seeds_reduce(const void *d_pml, int pml_bytes, const uint8_t *d_cid, const uint64_t *d_read_off,
                                      uint64_t n_reads, uint64_t n_bases, uint32_t min_len, uint32_t max_seeds,
                                      uint32_t *d_summary, uint32_t *d_pos, uint32_t *d_len, uint8_t *d_scid, hipStream_t stream) {
    if (n_reads == 0) return hipSuccess;
    if (d_pos) {   // unused slots: 0xFFFFFFFF, 0, 0
        const size_t slots = (size_t)n_reads * max_seeds;
        hipError_t e = hipMemsetAsync(d_pos, 0xFF, slots * 4, stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_len, 0, slots * 4, stream);
        if (e == hipSuccess) e = hipMemsetAsync(d_scid, 0, slots, stream);
        if (e != hipSuccess) return e;
    }
    const uint64_t chunk = seeds_chunk(n_bases);
    const uint64_t n_waves = n_bases ? (n_bases + chunk - 1) / chunk : 1;
    const dim3 grid((uint32_t)((n_waves + kSeedsWaves - 1) / kSeedsWaves)), block(kSeedsBlock);
    const SeedsOut out{d_summary, d_pos, d_len, d_scid, min_len, max_seeds};
    if (pml_bytes == 2)
        hipLaunchKernelGGL(seeds_reduce_kernel<uint16_t>, grid, block, 0, stream, (const uint16_t *)d_pml, d_cid, d_read_off, n_reads,
                           n_bases, chunk, n_waves, out);
    else
        hipLaunchKernelGGL(seeds_reduce_kernel<uint32_t>, grid, block, 0, stream, (const uint32_t *)d_pml, d_cid, d_read_off, n_reads,
                           n_bases, chunk, n_waves, out);
    return hipSuccess;
}

}  // namespace colbwt
