// tests/emu/out_runs_probe.hip -- the output collector of the line-fetching kernels (csrc/lane_out.h, OutRuns) driven
// directly: every lane of a block of kQueryBlock threads plays a script of pushes, one per trip, into an OutRuns, and the
// wave flushes every fourth trip with the default 32 slots, the way fat2_query.hip does.  What arrives in the two
// output arrays is compared by tests/test_out_runs_cpu.py and tests/test_gpu_out_runs.py with the per-element formula
// of tests/out_runs_restatement.py.  TESTS ONLY; one source, two builds (out_runs_probe.mk): g++ against the SIMT
// emulator under ASan/UBSan, and hipcc for gfx950.
//
//   out_runs_probe DIR NAME...     reads DIR/NAME.case, writes DIR/NAME.pml, .cid, .lanes and .waves
//
// NAME.case (little endian; written by tests/out_runs_cases.py):
//   uint64[8]  magic, n_lanes (a multiple of kQueryBlock), n_trips, max_chunks, n_out, bias, up_to_16, n_records
//   uint64[n_lanes][2]               the lane's first record and its number of records: trips beyond them are idle
//   uint64[n_lanes][max_chunks][2]   element address (raised by bias) and length of the lane's chunks; length 0 ends the list
//   uint32[n_records][8]             n | flags << 8 (flag 1: idle, no push at all), l_new, keep, keep1, ids lo, hi, ids2 lo, hi
// The arrays hold n_out elements and are passed to the kernel lowered by `bias` elements, so that element addresses at
// and above 2^32 need no large allocation.  Both are pre-filled with a pattern.
// NAME.lanes: uint32[n_lanes][4]  largest cnt (a push the probe refused included), final cnt, finished, error
// NAME.waves: uint32[n_waves][kWaveWords]  see WaveWord
//
// The probe makes no push that the collector's contract excludes: a record that asks for more elements than the chunk
// has left, for more than the instantiation takes, or for more than the collector's 96 is refused, the lane stops and
// reports the error.  So every store of a flush lies inside a chunk, and main() checks every chunk against n_out.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "lane_out.h"

using namespace colbwt;

namespace {

constexpr uint32_t kProbeWaves = kQueryBlock / 64;
constexpr uint32_t kLdsQ = OutRuns::lds_q(32);      // the flush's working area of one wave
constexpr uint32_t kCanaryQ = 4;                    // 16 canary words behind it
constexpr uint32_t kCapacity = 96;                  // of the collector (lane_out.h)
constexpr uint64_t kMagic = 0x455341434e55524full;  // "ORUNCASE"
constexpr uint32_t kFlagIdle = 1;
enum WaveWord : uint32_t {
    kHist = 0,             // [0 .. 64]: flushes in which that many lanes of the wave emitted
    kWholeItems = 65,      // items A of exactly one block
    kRaggedItems = 66,     // the other items A, and all items B
    kMaxEmitting = 67,
    kCanaryOk = 68,
    kFlushes = 69,
    kMixedFlushes = 70,    // flushes with a whole block, a ragged item A and an item B
    kWaveWords = 72
};
enum LaneError : uint32_t { kOk = 0, kMoreThanLeft = 1, kMoreThanInstantiation = 2, kMoreThanCapacity = 3, kPushWithoutChunk = 4 };

__device__ __forceinline__ uint32_t canary_word(uint32_t wave, uint32_t i) { return 0xC0FFEE00u ^ (wave << 16) ^ i; }

template <bool kUpTo16>
__global__ __launch_bounds__(kQueryBlock)
void out_runs_probe_kernel(const uint64_t *__restrict__ lane_tab, const uint64_t *__restrict__ chunk_tab,
                           const uint32_t *__restrict__ recs, uint32_t max_chunks, uint32_t n_trips, uint16_t *pml,
                           uint8_t *cid, uint32_t *__restrict__ lane_out, uint32_t *__restrict__ wave_out) {
    __shared__ uint4 s_lds[kProbeWaves][kLdsQ + kCanaryQ];
    __shared__ uint32_t s_hist[kProbeWaves][65];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t slot = (uint64_t)blockIdx.x * kQueryBlock + threadIdx.x;
    uint32_t *const canary = reinterpret_cast<uint32_t *>(&s_lds[wave][kLdsQ]);
    for (uint32_t i = lane; i < kLdsQ; i += 64) s_lds[wave][i] = make_uint4(0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu);
    if (lane < 4 * kCanaryQ) canary[lane] = canary_word(wave, lane);
    s_hist[wave][lane] = 0;
    if (lane == 0) s_hist[wave][64] = 0;
    wave_sync();

    const uint64_t first_rec = lane_tab[2 * slot], n_rec = lane_tab[2 * slot + 1];
    const uint64_t *const chunks = chunk_tab + 2 * slot * max_chunks;
    uint32_t ci = 0;
    uint64_t base = 0, rem = 0;
    bool done = max_chunks == 0 || chunks[1] == 0;
    if (!done) { base = chunks[0]; rem = chunks[1]; }

    OutRuns acc;
    uint32_t max_cnt = 0, err = kOk;
    uint32_t whole = 0, ragged = 0, max_emit = 0, flushes = 0, mixed = 0;
    for (uint32_t trip = 0; trip < n_trips; ++trip) {
        // a lane enters its next chunk only once the flush has taken what it held (fat2_query.hip, step 1)
        if (!done && rem == 0 && acc.cnt == 0) {
            ++ci;
            if (ci < max_chunks && chunks[2 * ci + 1] != 0) { base = chunks[2 * ci]; rem = chunks[2 * ci + 1]; }
            else done = true;
        }
        if (trip < n_rec && err == kOk) {
            const uint4 *r = reinterpret_cast<const uint4 *>(recs + 8 * (first_rec + trip));
            const uint4 a = r[0], b = r[1];
            const uint32_t n = a.x & 0xFFu, flags = a.x >> 8;
            if (!(flags & kFlagIdle)) {
                if (done) err = kPushWithoutChunk;
                else if (n > rem) err = kMoreThanLeft;
                else if (n > (kUpTo16 ? 16u : 8u)) err = kMoreThanInstantiation;
                else if (acc.cnt + n > kCapacity) err = kMoreThanCapacity;
                if (!done && acc.cnt + n > max_cnt) max_cnt = acc.cnt + n;
                if (err == kOk) {
                    if constexpr (kUpTo16) acc.template push_run<true>(n, a.y, a.z, a.w, b.x, b.y, b.z, b.w);
                    else acc.push_run(n, a.y, a.z, a.w, b.x, b.y);
                    rem -= n;
                } else {
                    done = true;            // the lane stops: what it holds stays where it is
                }
            }
        }
        if ((trip & (OutRuns::kPeriod - 1)) == OutRuns::kPeriod - 1) {
            const uint64_t gl = base + rem;
            const bool final = rem == 0;
            // what this flush is about to emit, seen from outside: the same three conditions as flush_wave's
            const uint32_t below = (0u - (uint32_t)gl) & (OutRuns::kBlock - 1);
            const bool has_a = !done && below < acc.cnt;
            const bool has_b = !done && final && (below < acc.cnt ? below : acc.cnt) != 0;
            const bool whole_a = has_a && acc.cnt - below == OutRuns::kBlock;
            const uint32_t n_emit = (uint32_t)__builtin_popcountll(__ballot(has_a || has_b));
            ++flushes;
            if (lane == 0) s_hist[wave][n_emit] += 1;
            if (n_emit != 0) {
                const uint32_t n_whole = (uint32_t)__builtin_popcountll(__ballot(whole_a));
                const uint32_t n_rag_a = (uint32_t)__builtin_popcountll(__ballot(has_a && !whole_a));
                const uint32_t n_b = (uint32_t)__builtin_popcountll(__ballot(has_b));
                whole += n_whole;
                ragged += n_rag_a + n_b;
                max_emit = n_emit > max_emit ? n_emit : max_emit;
                mixed += n_whole != 0 && n_rag_a != 0 && n_b != 0;
            }
            acc.flush_wave(pml, cid, gl, !done, final, &s_lds[wave][0], lane);
        }
    }
    wave_sync();
    const bool last_chunk = ci + 1 >= max_chunks || chunks[2 * (ci + 1) + 1] == 0;
    lane_out[4 * slot + 0] = max_cnt;
    lane_out[4 * slot + 1] = acc.cnt;
    lane_out[4 * slot + 2] = err == kOk && acc.cnt == 0 && (done || (rem == 0 && last_chunk));
    lane_out[4 * slot + 3] = err;
    const bool canary_bad = lane < 4 * kCanaryQ && canary[lane] != canary_word(wave, lane);
    const bool any_bad = __any(canary_bad);
    uint32_t *const wo = wave_out + (uint64_t)(blockIdx.x * kProbeWaves + wave) * kWaveWords;
    wo[kHist + lane] = s_hist[wave][lane];
    if (lane == 0) {
        wo[kHist + 64] = s_hist[wave][64];
        wo[kWholeItems] = whole;
        wo[kRaggedItems] = ragged;
        wo[kMaxEmitting] = max_emit;
        wo[kCanaryOk] = any_bad ? 0u : 1u;
        wo[kFlushes] = flushes;
        wo[kMixedFlushes] = mixed;
        wo[71] = 0;
    }
}

#define PROBE_HIP(call)                                                                         \
    do {                                                                                        \
        const hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                                 \
            fprintf(stderr, "out_runs_probe: %s: %s\n", #call, hipGetErrorString(e_));          \
            exit(3);                                                                            \
        }                                                                                       \
    } while (0)

bool read_file(const std::string &path, std::vector<uint8_t> &out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    out.resize(size > 0 ? (size_t)size : 0);
    const bool ok = size >= 0 && fread(out.data(), 1, out.size(), f) == out.size();
    fclose(f);
    return ok;
}

bool write_file(const std::string &path, const void *data, size_t bytes) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(data, 1, bytes, f) == bytes;
    return fclose(f) == 0 && ok;
}

int fail(const std::string &name, const char *what) {
    fprintf(stderr, "out_runs_probe: %s: %s\n", name.c_str(), what);
    return 2;
}

int run_case(const std::string &dir, const std::string &name) {
    std::vector<uint8_t> file;
    if (!read_file(dir + "/" + name + ".case", file)) return fail(name, "cannot read the case file");
    if (file.size() < 64) return fail(name, "no header");
    uint64_t h[8];
    memcpy(h, file.data(), 64);
    const uint64_t n_lanes = h[1], n_trips = h[2], max_chunks = h[3], n_out = h[4], bias = h[5], up16 = h[6], n_records = h[7];
    if (h[0] != kMagic) return fail(name, "not a case file");
    if (n_lanes == 0 || n_lanes % kQueryBlock != 0 || n_lanes > (1u << 20) || n_trips > (1u << 24) || max_chunks > 4096 ||
        n_out == 0 || n_out > (1ull << 28) || n_records > (1ull << 28) || bias > (1ull << 40) || bias % 16 != 0)
        return fail(name, "header out of range");
    const size_t lane_bytes = n_lanes * 16, chunk_bytes = n_lanes * max_chunks * 16, rec_bytes = n_records * 32;
    if (file.size() != 64 + lane_bytes + chunk_bytes + rec_bytes) return fail(name, "size does not match the header");
    std::vector<uint64_t> lane_tab(n_lanes * 2), chunk_tab(n_lanes * max_chunks * 2 + 2);
    memcpy(lane_tab.data(), file.data() + 64, lane_bytes);
    memcpy(chunk_tab.data(), file.data() + 64 + lane_bytes, chunk_bytes);
    for (uint64_t l = 0; l < n_lanes; ++l)
        if (lane_tab[2 * l] > n_records || lane_tab[2 * l + 1] > n_records - lane_tab[2 * l]) return fail(name, "records out of range");
    for (uint64_t c = 0; c < n_lanes * max_chunks; ++c) {
        const uint64_t addr = chunk_tab[2 * c], len = chunk_tab[2 * c + 1];
        if (len != 0 && (addr < bias || addr - bias > n_out || len > n_out - (addr - bias))) return fail(name, "chunk outside the arrays");
    }
    std::vector<uint16_t> pml(n_out, (uint16_t)0xA5A5u);
    std::vector<uint8_t> cid(n_out, (uint8_t)0xA5u);
    const uint32_t n_waves = (uint32_t)(n_lanes / 64);
    std::vector<uint32_t> lane_out(n_lanes * 4, 0xFFFFFFFFu), wave_out((size_t)n_waves * kWaveWords, 0xFFFFFFFFu);

    uint64_t *d_lane = nullptr, *d_chunk = nullptr;
    uint32_t *d_rec = nullptr, *d_lane_out = nullptr, *d_wave_out = nullptr;
    uint16_t *d_pml = nullptr;
    uint8_t *d_cid = nullptr;
    PROBE_HIP(hipMalloc(&d_lane, lane_bytes));
    PROBE_HIP(hipMalloc(&d_chunk, chunk_bytes + 16));
    PROBE_HIP(hipMalloc(&d_rec, rec_bytes + 32));
    PROBE_HIP(hipMalloc(&d_pml, n_out * 2));
    PROBE_HIP(hipMalloc(&d_cid, n_out));
    PROBE_HIP(hipMalloc(&d_lane_out, lane_out.size() * 4));
    PROBE_HIP(hipMalloc(&d_wave_out, wave_out.size() * 4));
    PROBE_HIP(hipMemcpy(d_lane, lane_tab.data(), lane_bytes, hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy(d_chunk, chunk_tab.data(), chunk_bytes + 16, hipMemcpyHostToDevice));
    PROBE_HIP(hipMemset(d_rec, 0, rec_bytes + 32));
    PROBE_HIP(hipMemcpy(d_rec, file.data() + 64 + lane_bytes + chunk_bytes, rec_bytes, hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy(d_pml, pml.data(), n_out * 2, hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy(d_cid, cid.data(), n_out, hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy(d_lane_out, lane_out.data(), lane_out.size() * 4, hipMemcpyHostToDevice));
    PROBE_HIP(hipMemcpy(d_wave_out, wave_out.data(), wave_out.size() * 4, hipMemcpyHostToDevice));
    // element `bias` of the arrays the kernel sees is element 0 of the allocations
    uint16_t *const k_pml = reinterpret_cast<uint16_t *>(reinterpret_cast<uintptr_t>(d_pml) - 2 * (uintptr_t)bias);
    uint8_t *const k_cid = reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(d_cid) - (uintptr_t)bias);
    const dim3 grid((uint32_t)(n_lanes / kQueryBlock)), block(kQueryBlock);
    if (up16)
        hipLaunchKernelGGL(out_runs_probe_kernel<true>, grid, block, 0, 0, d_lane, d_chunk, d_rec, (uint32_t)max_chunks, (uint32_t)n_trips,
                           k_pml, k_cid, d_lane_out, d_wave_out);
    else
        hipLaunchKernelGGL(out_runs_probe_kernel<false>, grid, block, 0, 0, d_lane, d_chunk, d_rec, (uint32_t)max_chunks, (uint32_t)n_trips,
                           k_pml, k_cid, d_lane_out, d_wave_out);
    PROBE_HIP(hipGetLastError());
    PROBE_HIP(hipDeviceSynchronize());
    PROBE_HIP(hipMemcpy(pml.data(), d_pml, n_out * 2, hipMemcpyDeviceToHost));
    PROBE_HIP(hipMemcpy(cid.data(), d_cid, n_out, hipMemcpyDeviceToHost));
    PROBE_HIP(hipMemcpy(lane_out.data(), d_lane_out, lane_out.size() * 4, hipMemcpyDeviceToHost));
    PROBE_HIP(hipMemcpy(wave_out.data(), d_wave_out, wave_out.size() * 4, hipMemcpyDeviceToHost));
    PROBE_HIP(hipFree(d_lane));
    PROBE_HIP(hipFree(d_chunk));
    PROBE_HIP(hipFree(d_rec));
    PROBE_HIP(hipFree(d_pml));
    PROBE_HIP(hipFree(d_cid));
    PROBE_HIP(hipFree(d_lane_out));
    PROBE_HIP(hipFree(d_wave_out));
    const std::string stem = dir + "/" + name;
    if (!write_file(stem + ".pml", pml.data(), n_out * 2) || !write_file(stem + ".cid", cid.data(), n_out) ||
        !write_file(stem + ".lanes", lane_out.data(), lane_out.size() * 4) || !write_file(stem + ".waves", wave_out.data(), wave_out.size() * 4))
        return fail(name, "cannot write the results");
    printf("ok %s: %llu lanes, %llu trips, push_run<%s>\n", name.c_str(), (unsigned long long)n_lanes, (unsigned long long)n_trips,
           up16 ? "true" : "false");
    fflush(stdout);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: out_runs_probe DIR NAME...\n");
        return 1;
    }
    for (int i = 2; i < argc; ++i) {
        const int rc = run_case(argv[1], argv[i]);
        if (rc != 0) return rc;
    }
    printf("OUT-RUNS-PROBE-OK\n");
    return 0;
}
