// capi.hip -- the C-ABI of include/colbwt.h over the HIP engine.
// Host-side mirror of col_pml (col_bwt.hpp:386-575) and of pml_query's main
// (pml_query.cpp:92-143).  No CPU fallback anywhere: every entry point that
// computes PML/col-ids needs a HIP device and says so when there is none.
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/colbwt.h"
#include "anchors_query.h"
#include "bin_writer.h"
#include "chain_reduce.h"
#include "count_query.h"
#include "docs_query.h"
#include "fasta_parallel.h"
#include "fastx_reader.h"
#include "index.h"
#include "locate_all_query.h"
#include "locate_query.h"
#include "query_kernels.h"
#include "seeds_reduce.h"
#include "text_writer.h"

using namespace colbwt;

#define COLBWT_LAYOUT_DEFAULT_CHOICE COLBWT_LAYOUT_MISMATCH_LINES
constexpr int kDefaultLineSteps = 8;

// Device buffers, stream and events of one host-entry query, kept with the handle between calls
// (a file query makes one call per 64 Mbase batch: four hipMalloc / hipFree pairs, a stream and
// four events per call otherwise).  One caller at a time holds it; concurrent callers on the
// same replica work with a set of their own that lives for the call.
struct BatchScratch {
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    void *buf[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // bases, offsets, two result arrays, order
    size_t cap[5] = {0, 0, 0, 0, 0};
    ~BatchScratch() { release(); }
    void release() {
        for (int k = 0; k < 5; ++k) {
            if (buf[k]) (void)hipFree(buf[k]);
            buf[k] = nullptr;
            cap[k] = 0;
        }
        for (auto &e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
    }
    hipError_t ready() {   // stream + events exist
        hipError_t e = hipSuccess;
        if (!stream) e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
        for (auto &x : ev)
            if (e == hipSuccess && !x) e = hipEventCreate(&x);
        return e;
    }
    hipError_t need(int k, size_t bytes) {   // buf[k] holds at least `bytes` (grown with headroom)
        if (bytes <= cap[k]) return hipSuccess;
        if (buf[k]) (void)hipFree(buf[k]);
        buf[k] = nullptr;
        cap[k] = 0;
        const size_t want = bytes + bytes / 8 + 4096;
        const hipError_t e = hipMalloc(&buf[k], want);
        if (e == hipSuccess) cap[k] = want;
        return e;
    }
};

// Page-locked host array for the results of a batch: the device-to-host copy of 3 bytes per
// base is the largest part of the GPU stage, and runs ~4x faster into pinned memory.  Pinning
// costs about as much as a copy, so the file entry point keeps its buffers with the handle.
class PinnedBuf {
public:
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { if (p_) (void)hipHostFree(p_); }
    bool ensure(size_t bytes) {
        if (bytes <= cap_) return true;
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr;
        cap_ = 0;
        const size_t want = bytes + bytes / 8 + 4096;
        if (hipHostMalloc(&p_, want, 0) != hipSuccess) { p_ = nullptr; (void)hipGetLastError(); return false; }
        cap_ = want;
        return true;
    }
    template <typename T>
    T *as() const { return static_cast<T *>(p_); }

private:
    void *p_ = nullptr;
    size_t cap_ = 0;
};

constexpr int kFileBatches = 3;   // batches of reads in flight in colbwt_query_file

// The locate samples of one replica (colbwt_index_attach_locate): the toehold of every row of the
// layout in HBM that ends a folded run, the phi samples and their bucket directory.
struct LocateTables {
    DevPtr toe_row, pair, dir;
    DevPtr doc_dev;                     // doc_start as u32 in HBM: the walk of colbwt_docs_* looks positions up in it
    uint32_t shift = 0;
    uint64_t n_buckets = 0;
    std::vector<uint64_t> doc_start;    // host copy: positions -> (document, offset) in colbwt_locate_file
    bool ready() const { return toe_row.get() != nullptr; }
    uint64_t bytes() const { return toe_row.bytes() + pair.bytes() + dir.bytes() + doc_dev.bytes(); }
    uint32_t n_docs() const { return (uint32_t)doc_start.size(); }
    DocsArgs docs(uint32_t min_len, uint32_t max_walk) const {
        return DocsArgs{toe_row.as<const uint32_t>(), phi(), doc_dev.as<const uint32_t>(), n_docs(), min_len, max_walk};
    }
    PhiTable phi() const { return PhiTable{pair.as<const uint2>(), dir.as<const uint32_t>(), shift, (uint32_t)(n_buckets - 1)}; }
    LocAllArgs all() const { return LocAllArgs{toe_row.as<const uint32_t>(), phi()}; }
    void reset() {
        toe_row.reset();
        pair.reset();
        dir.reset();
        doc_dev.reset();
        doc_start.clear();
    }
};

struct colbwt_index {
    Index ix;
    // result arrays of colbwt_query_file's batches (one file query at a time uses them)
    std::mutex file_mu;
    PinnedBuf file_pml[kFileBatches], file_cid[kFileBatches];
    // Further replicas of the table, one per extra device (colbwt_index_open_devices): each is a
    // handle of its own kind, owned by this one.  The host entry points shard a batch over
    // [this] + more; the device entry points address the replica on the buffers' device.
    std::vector<colbwt_index *> more;
    std::mutex scratch_mu;
    BatchScratch scratch;
    // Two pinned staging buffers for results that go to pageable host memory (kept for the
    // life of the handle: pinning costs as much as a copy).  One caller at a time uses them;
    // concurrent callers fall back to the runtime's own pageable copy.
    std::mutex stage_mu;
    void *stage[2] = {nullptr, nullptr};
    size_t stage_bytes = 0;
    LocateTables loc;
    // The packed positions of a colbwt_locate_all_batch shard before they go to the host: their number
    // is only known after the plan, so they have a buffer of their own, kept between calls.  One
    // caller at a time uses it; concurrent callers allocate one for the call.
    std::mutex all_mu;
    DevPtr all_pos;
    ~colbwt_index() {
        for (colbwt_index *r : more) delete r;
        if (ix.device() >= 0) (void)hipSetDevice(ix.device());
        scratch.release();
        loc.reset();
        all_pos.reset();
        for (void *p : stage)
            if (p) (void)hipHostFree(p);
    }
};

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

const char *kNoSamples = "no locate samples attached (colbwt_index_attach_locate)";
const char *kTooManyReads = "more than 2^32-2 reads in a batch";

// kNoSamples unless every replica of the handle has its locate samples attached
const char *samples_missing(const colbwt_index *idx) {
    if (!idx->loc.ready()) return kNoSamples;
    for (const colbwt_index *r : idx->more)
        if (!r->loc.ready()) return kNoSamples;
    return nullptr;
}

// A failed HIP call `what`: its colbwt code, with "<what>: <HIP's message>" in `msg`.  Whatever the
// call queued on `stream` (nullptr: none of ours) is drained first: nothing of it may still be
// running when the caller gets its arrays (and the next caller the staging buffers) back.
int hip_failed(hipError_t e, const char *what, hipStream_t stream, std::string &msg) {
    (void)hipGetLastError();
    if (stream) (void)hipStreamSynchronize(stream);
    msg = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? COLBWT_ERR_NOMEM : COLBWT_ERR_HIP;
}

// The launch an entry point just made: COLBWT_ERR_HIP with "<entry>: <HIP's message>" when it failed.
int launch_status(const char *entry) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? COLBWT_OK : fail(COLBWT_ERR_HIP, std::string(entry) + ": " + hipGetErrorString(e));
}

#define TRY_HIP(expr, stream, msg)                                                    \
    do {                                                                              \
        const hipError_t e_ = (expr);                                                 \
        if (e_ != hipSuccess) return hip_failed(e_, #expr, stream, msg);              \
    } while (0)

bool widths_ok(const colbwt_widths *w) {
    return !w || (w->bwt_bytes == 5 && w->run_bytes == 4 && w->len_bytes == 2 && w->id_bits == 8);
}

struct MappedFile {
    const uint8_t *data = nullptr;
    uint64_t len = 0;
    int fd = -1;
    ~MappedFile() { close(); }
    void close() {
        if (data && len) munmap((void *)data, len);
        if (fd >= 0) ::close(fd);
        data = nullptr;
        len = 0;
        fd = -1;
    }
    bool open(const std::string &path) {
        close();
        fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) return false;
        len = (uint64_t)st.st_size;
        if (len == 0) return true;
        void *p = mmap(nullptr, len, PROT_READ, MAP_PRIVATE, fd, 0);
        if (p == MAP_FAILED) return false;
        data = (const uint8_t *)p;
        return true;
    }
};

// The index file of an open by name: prefix + ".col_pml" (pml_query.cpp:110-111, col_bwt.hpp:434-437),
// else the path itself.
int map_index_file(const char *prefix_or_file, MappedFile &mf) {
    if (mf.open(std::string(prefix_or_file) + ".col_pml") || mf.open(prefix_or_file)) return COLBWT_OK;
    return fail(COLBWT_ERR_IO, std::string("cannot open ") + prefix_or_file + ".col_pml (or " + prefix_or_file + ")");
}

constexpr size_t kStageBytes = 128u << 20;     // per staging buffer
constexpr size_t kStageMinTotal = 256u << 20;  // smaller results: the plain copy is as good
constexpr unsigned kStageThreads = 8;

bool is_pageable(const void *p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) == hipSuccess)                 // ROCm >= 6 knows plain host memory
        return a.type == hipMemoryTypeUnregistered;                   // else pinned / registered / device
    (void)hipGetLastError();                                          // older answer: "invalid value"
    return true;
}

void parallel_memcpy(uint8_t *dst, const uint8_t *src, size_t n) {
    if (n < (8u << 20)) {
        memcpy(dst, src, n);
        return;
    }
    std::thread ts[kStageThreads - 1];
    const size_t per = (n / kStageThreads + 4095) & ~(size_t)4095;
    for (unsigned t = 1; t < kStageThreads; ++t) {
        const size_t a = std::min(n, per * t), b = std::min(n, per * (t + 1));
        ts[t - 1] = std::thread([=] { if (b > a) memcpy(dst + a, src + a, b - a); });
    }
    memcpy(dst, src, std::min(n, per));
    for (auto &th : ts) th.join();
}

struct D2HSegment {
    uint8_t *dst;
    const uint8_t *src;
    size_t bytes;
};

// Both pinned staging buffers of the handle, or neither: a failed allocation is "not staged"
// (the caller takes the plain copy), never a half-initialised pair.
bool ensure_stage(colbwt_index *idx) {
    if (idx->stage[0] && idx->stage[1]) return true;
    for (int b = 0; b < 2; ++b)
        if (hipHostMalloc(&idx->stage[b], kStageBytes, 0) != hipSuccess) {
            (void)hipGetLastError();
            idx->stage[b] = nullptr;
            if (idx->stage[0]) (void)hipHostFree(idx->stage[0]);
            idx->stage[0] = nullptr;
            return false;
        }
    idx->stage_bytes = kStageBytes;
    return true;
}

// Device -> pageable host memory through the handle's two pinned buffers: the DMA of chunk
// k runs while host threads copy chunk k-1 out of its buffer.  Returns hipSuccess or the
// first HIP error; the stream is idle afterwards.
hipError_t staged_d2h(colbwt_index *idx, const D2HSegment *seg, int n_seg, hipStream_t stream) {
    hipError_t e = hipSuccess;
    hipEvent_t ev[2] = {nullptr, nullptr};
    for (auto &x : ev)
        if ((e = hipEventCreateWithFlags(&x, hipEventDisableTiming)) != hipSuccess) {
            for (auto &y : ev)
                if (y) (void)hipEventDestroy(y);
            return e;
        }
    struct Piece {
        uint8_t *dst;
        size_t n;
    } prev{nullptr, 0};
    int k = 0;
    for (int s = 0; s < n_seg && e == hipSuccess; ++s) {
        for (size_t o = 0; o < seg[s].bytes && e == hipSuccess; o += kStageBytes, ++k) {
            const size_t n = std::min(kStageBytes, seg[s].bytes - o);
            e = hipMemcpyAsync(idx->stage[k & 1], seg[s].src + o, n, hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipEventRecord(ev[k & 1], stream);
            if (prev.dst && e == hipSuccess) {
                e = hipEventSynchronize(ev[(k - 1) & 1]);
                if (e == hipSuccess) parallel_memcpy(prev.dst, (const uint8_t *)idx->stage[(k - 1) & 1], prev.n);
            }
            prev = Piece{seg[s].dst + o, n};
        }
    }
    if (prev.dst && e == hipSuccess) {
        e = hipEventSynchronize(ev[(k - 1) & 1]);
        if (e == hipSuccess) parallel_memcpy(prev.dst, (const uint8_t *)idx->stage[(k - 1) & 1], prev.n);
    }
    const hipError_t e2 = hipStreamSynchronize(stream);
    for (auto &x : ev) (void)hipEventDestroy(x);
    return e != hipSuccess ? e : e2;
}

// Lane order of a ragged batch: the reads by decreasing length (a counting sort over 256 length
// classes is enough: waves only need reads of SIMILAR length side by side).  Left empty when the
// batch is small or even enough for the natural order.
void length_order(const uint64_t *read_off, uint64_t n_reads, uint64_t max_len, uint64_t min_len,
                  std::vector<uint32_t> &order) {
    if (n_reads > 0xFFFFFFFFull || n_reads <= 64 || max_len <= min_len + (min_len >> 2) + 16) return;
    const uint64_t span = max_len - min_len + 1;
    uint32_t shift = 0;
    while ((span >> shift) > 4096) ++shift;
    std::vector<uint64_t> start((span >> shift) + 2, 0);
    for (uint64_t k = 0; k < n_reads; ++k) ++start[((max_len - (read_off[k + 1] - read_off[k])) >> shift) + 1];
    for (size_t b = 1; b < start.size(); ++b) start[b] += start[b - 1];
    order.resize(n_reads);
    for (uint64_t k = 0; k < n_reads; ++k)
        order[start[(max_len - (read_off[k + 1] - read_off[k])) >> shift]++] = (uint32_t)k;
}

// The three layout-dependent choices of a query: each is made here and nowhere else.
// Whether the PML kernel of the layout assigns lanes by d_order: the one- and two-step rows do;
// three-step rows (sk3_query.hip) and line rows have persistent lanes that balance by themselves.
bool pml_reads_order(const Index &ix) { return ix.layout() <= 2; }

void launch_query(const Index &ix, const uint8_t *d_bases, const uint64_t *d_read_off, uint64_t n_reads, uint64_t n_bases,
                  void *d_pml, int pml_bytes, uint8_t *d_cid, const uint32_t *d_order, hipStream_t stream) {
    if (ix.line_rows())
        launch_fat_query(ix.table_fat(), d_bases, d_read_off, n_reads, n_bases, d_pml, pml_bytes, d_cid, d_order, stream);
    else if (ix.layout() >= 2)
        launch_sk_query(ix.table_k(), d_bases, d_read_off, n_reads, n_bases, d_pml, pml_bytes, d_cid, d_order, stream);
    else
        launch_pml_query(ix.table(), d_bases, d_read_off, n_reads, d_pml, pml_bytes, d_cid, d_order, stream);
}

void launch_sampler(const Index &ix, uint64_t n_reads, uint32_t read_len, uint32_t sub_permille, uint64_t seed,
                    uint8_t *d_bases, uint64_t *d_read_off, hipStream_t stream) {
    if (ix.line_rows())
        launch_fat_synth_reads(ix.table_fat(), n_reads, read_len, sub_permille, seed, d_bases, d_read_off, stream);
    else if (ix.layout() >= 2)   // the one-step tables are gone once the K-step rows exist
        launch_sk_synth_reads(ix.table_k(), n_reads, read_len, sub_permille, seed, d_bases, d_read_off, stream);
    else
        launch_synth_reads(ix.table(), n_reads, read_len, sub_permille, seed, d_bases, d_read_off, stream);
}

// One replica's batch in HBM, in the buffers of a BatchScratch: what a caller's launch and fetch see.
struct DeviceBatch {
    uint8_t *bases;
    uint64_t *off;
    uint32_t *order;   // nullptr: lanes in read order
    void *out[2];      // the caller's two result arrays
    hipStream_t stream;
};

// One replica's part of a host-entry batch: reads [0, n_reads) of `read_off`, whose offsets are
// relative to `bases` after subtracting `off0` (a shard of a larger batch keeps the caller's
// offsets).  The replica's scratch (or, when another caller holds it, one for this call) takes the
// bases, the rebased offsets, the lane order of a ragged batch (when `ordered`) and two result
// arrays of out_bytes[0] / out_bytes[1] bytes; then `launch(batch)` enqueues the kernel and
// `fetch(batch)` copies the results back (a colbwt code; HIP failures through TRY_HIP).
template <typename Launch, typename Fetch>
int replica_batch(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t off0, uint64_t n_reads,
                  uint64_t max_len, uint64_t min_len, bool ordered, const uint64_t out_bytes[2], uint64_t alg_bytes_per_base,
                  colbwt_stats *stats, std::string &msg, Launch launch, Fetch fetch) {
    const uint64_t n_bases = read_off[n_reads] - off0;
    if (stats) memset(stats, 0, sizeof(*stats));
    int rc = select_device(idx->ix.device(), msg);
    if (rc != COLBWT_OK) return rc;

    std::unique_lock<std::mutex> lease(idx->scratch_mu, std::defer_lock);
    BatchScratch own;
    BatchScratch &S = lease.try_lock() ? idx->scratch : own;
    std::vector<uint32_t> order;   // ragged batch: lanes by decreasing read length
    if (ordered) length_order(read_off, n_reads, max_len, min_len, order);
    std::vector<uint64_t> rebased;                            // offsets from 0 for this shard
    const uint64_t *off_src = read_off;
    if (off0 != 0) {
        rebased.resize(n_reads + 1);
        for (uint64_t k = 0; k <= n_reads; ++k) rebased[k] = read_off[k] - off0;
        off_src = rebased.data();
    }
    const uint64_t bases_alloc = (n_bases + 64 + 63) & ~63ull;  // the kernel reads whole 64-byte blocks
    const uint64_t tail = std::min<uint64_t>(bases_alloc, 128);   // zeroed past the bases
    hipStream_t stream = nullptr;
    TRY_HIP(S.ready(), stream, msg);
    TRY_HIP(S.need(0, bases_alloc), stream, msg);
    TRY_HIP(S.need(1, (n_reads + 1) * sizeof(uint64_t)), stream, msg);
    TRY_HIP(S.need(2, out_bytes[0]), stream, msg);
    TRY_HIP(S.need(3, out_bytes[1]), stream, msg);
    if (!order.empty()) TRY_HIP(S.need(4, n_reads * sizeof(uint32_t)), stream, msg);
    stream = S.stream;
    const DeviceBatch b{(uint8_t *)S.buf[0], (uint64_t *)S.buf[1], order.empty() ? nullptr : (uint32_t *)S.buf[4],
                        {S.buf[2], S.buf[3]}, stream};

    TRY_HIP(hipEventRecord(S.ev[0], stream), stream, msg);
    TRY_HIP(hipMemsetAsync(b.bases + (bases_alloc - tail), 0, tail, stream), stream, msg);
    if (n_bases) TRY_HIP(hipMemcpyAsync(b.bases, bases, n_bases, hipMemcpyHostToDevice, stream), stream, msg);
    TRY_HIP(hipMemcpyAsync(b.off, off_src, (n_reads + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream), stream, msg);
    if (b.order)
        TRY_HIP(hipMemcpyAsync(b.order, order.data(), n_reads * sizeof(uint32_t), hipMemcpyHostToDevice, stream), stream, msg);
    TRY_HIP(hipEventRecord(S.ev[1], stream), stream, msg);
    launch(b);
    TRY_HIP(hipGetLastError(), stream, msg);
    TRY_HIP(hipEventRecord(S.ev[2], stream), stream, msg);
    rc = fetch(b);
    if (rc != COLBWT_OK) return rc;
    TRY_HIP(hipEventRecord(S.ev[3], stream), stream, msg);
    TRY_HIP(hipStreamSynchronize(stream), stream, msg);
    float ms[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) TRY_HIP(hipEventElapsedTime(&ms[k], S.ev[k], S.ev[k + 1]), stream, msg);
    if (stats) {
        stats->n_reads = n_reads;
        stats->n_bases = n_bases;
        stats->h2d_ms = ms[0];
        stats->kernel_ms = ms[1];
        stats->d2h_ms = ms[2];
        stats->algorithmic_bytes = n_bases * alg_bytes_per_base;
    }
    return COLBWT_OK;
}

// A batch in host memory over every replica of the handle: the reads are independent (the
// reference walks them one after the other, pml_query.cpp:74-86), so the batch is cut into
// contiguous shards of equal base count, one per replica, each run by
// `part(replica, lo, hi, max_len, min_len, stats, msg)` on a host thread of its own (the first on the
// calling thread) on its device's stream -- no exchange between devices.  Checks `read_off`, reads
// longer than `max_read_len` (message `too_long`) and, through `bad_pointers(n_bases)`, the caller's
// pointers.  Counts and bytes of the shards add up, times are the longest shard's.  A failure names
// its device when there are several replicas, or when `name_device`.
template <typename PointerCheck, typename Part>
int sharded_batch(colbwt_index *idx, const uint64_t *read_off, uint64_t n_reads, uint64_t max_read_len, const char *too_long,
                  bool name_device, colbwt_stats *stats, PointerCheck bad_pointers, Part part) {
    if (!idx) return fail(COLBWT_ERR_ARG, "null index");
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n_reads == 0) return COLBWT_OK;
    if (!read_off) return fail(COLBWT_ERR_ARG, "null read_off");
    if (read_off[0] != 0) return fail(COLBWT_ERR_ARG, "read_off[0] must be 0");
    uint64_t max_len = 0, min_len = ~0ull;
    for (uint64_t k = 0; k < n_reads; ++k) {
        if (read_off[k + 1] < read_off[k]) return fail(COLBWT_ERR_ARG, "read_off not non-decreasing");
        max_len = std::max(max_len, read_off[k + 1] - read_off[k]);
        min_len = std::min(min_len, read_off[k + 1] - read_off[k]);
    }
    const uint64_t n_bases = read_off[n_reads];
    if (max_len > max_read_len) return fail(COLBWT_ERR_ARG, too_long);
    if (const char *m = bad_pointers(n_bases)) return fail(COLBWT_ERR_ARG, m);

    std::vector<colbwt_index *> reps{idx};
    reps.insert(reps.end(), idx->more.begin(), idx->more.end());
    const size_t R = reps.size();
    // shard boundaries by base count (same rule as multi_gpu.shard_reads)
    std::vector<uint64_t> cut(R + 1, 0);
    cut[R] = n_reads;
    for (size_t r = 1; r < R; ++r) {
        const uint64_t target = n_bases / R * r + n_bases % R * r / R;
        const uint64_t k = (uint64_t)(std::lower_bound(read_off, read_off + n_reads + 1, target) - read_off);
        cut[r] = std::min(std::max(k, cut[r - 1]), n_reads);
    }
    std::vector<int> rcs(R, COLBWT_OK);
    std::vector<std::string> msgs(R);
    std::vector<colbwt_stats> sts(R);
    auto work = [&](size_t r) {
        if (cut[r + 1] > cut[r]) rcs[r] = part(reps[r], cut[r], cut[r + 1], max_len, min_len, &sts[r], msgs[r]);
    };
    std::vector<std::thread> threads;
    for (size_t r = 1; r < R; ++r) threads.emplace_back(work, r);
    work(0);
    for (auto &t : threads) t.join();
    for (size_t r = 0; r < R; ++r)
        if (rcs[r] != COLBWT_OK)
            return fail(rcs[r], R > 1 || name_device ? "device " + std::to_string(reps[r]->ix.device()) + ": " + msgs[r] : msgs[r]);
    if (stats) {
        for (size_t r = 0; r < R; ++r) {
            stats->n_reads += sts[r].n_reads;
            stats->n_bases += sts[r].n_bases;
            stats->algorithmic_bytes += sts[r].algorithmic_bytes;
            stats->h2d_ms = std::max(stats->h2d_ms, sts[r].h2d_ms);          // the devices work side by side
            stats->kernel_ms = std::max(stats->kernel_ms, sts[r].kernel_ms);
            stats->d2h_ms = std::max(stats->d2h_ms, sts[r].d2h_ms);
        }
    }
    return COLBWT_OK;
}

// col_pml::query_pml for a batch in host memory: results per base, copied straight into each
// shard's slice of the caller's arrays.
template <typename PmlT>
int query_batch_all(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, PmlT *pml,
                    uint8_t *cid, colbwt_stats *stats) {
    const bool u16 = sizeof(PmlT) == 2;
    auto bad_pointers = [&](uint64_t n_bases) -> const char * {
        return n_bases && (!bases || !pml || !cid) ? "null bases/pml/cid" : nullptr;
    };
    auto part = [&](colbwt_index *rep, uint64_t lo, uint64_t hi, uint64_t max_len, uint64_t min_len, colbwt_stats *st,
                    std::string &msg) {
        const uint64_t off0 = read_off[lo], n_bases = read_off[hi] - off0;
        if (n_bases == 0) {                                   // nothing to compute
            st->n_reads = hi - lo;
            return COLBWT_OK;
        }
        const uint64_t out_bytes[2] = {((n_bases + 15) & ~15ull) * sizeof(PmlT), (n_bases + 15) & ~15ull};
        auto launch = [&](const DeviceBatch &b) {
            launch_query(rep->ix, b.bases, b.off, hi - lo, n_bases, b.out[0], (int)sizeof(PmlT), (uint8_t *)b.out[1], b.order,
                         b.stream);
        };
        auto fetch = [&](const DeviceBatch &b) {
            PmlT *const p = pml + off0;
            uint8_t *const c = cid + off0;
            // results into pageable memory go through pinned staging buffers with several copier
            // threads (the runtime's own pageable path manages ~17 GB/s); pinned destinations and
            // small batches are copied directly
            std::unique_lock<std::mutex> stage_lock(rep->stage_mu, std::defer_lock);
            const bool staged = n_bases * (sizeof(PmlT) + 1) >= kStageMinTotal && is_pageable(p) && is_pageable(c) &&
                                stage_lock.try_lock() && ensure_stage(rep);
            if (staged) {
                const D2HSegment seg[2] = {{(uint8_t *)p, (const uint8_t *)b.out[0], n_bases * sizeof(PmlT)},
                                           {c, (const uint8_t *)b.out[1], n_bases}};
                TRY_HIP(staged_d2h(rep, seg, 2, b.stream), b.stream, msg);
            } else {
                TRY_HIP(hipMemcpyAsync(p, b.out[0], n_bases * sizeof(PmlT), hipMemcpyDeviceToHost, b.stream), b.stream, msg);
                TRY_HIP(hipMemcpyAsync(c, b.out[1], n_bases, hipMemcpyDeviceToHost, b.stream), b.stream, msg);
            }
            return COLBWT_OK;
        };
        return replica_batch(rep, bases + off0, read_off + lo, off0, hi - lo, max_len, min_len, pml_reads_order(rep->ix),
                             out_bytes, kAlgBytesPerBase, st, msg, launch, fetch);
    };
    return sharded_batch(idx, read_off, n_reads, u16 ? 65535 : 0xFFFFFFFFull,
                         u16 ? "read longer than 65535 bases: use colbwt_query_batch_u32" : "read longer than 2^32-1 bases",
                         false, stats, bad_pointers, part);
}

// Count queries (count_query.h) for a batch in host memory: results per read.  The count kernel
// assigns lanes by d_order on every layout (one lane per read).
int count_batch_all(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, uint32_t *mlen,
                    uint64_t *occ, uint64_t *sp, colbwt_stats *stats) {
    auto bad_pointers = [&](uint64_t n_bases) -> const char * {
        return (n_bases && !bases) || !mlen || !occ ? "null bases/mlen/occ" : nullptr;
    };
    auto part = [&](colbwt_index *rep, uint64_t lo, uint64_t hi, uint64_t max_len, uint64_t min_len, colbwt_stats *st,
                    std::string &msg) {
        const uint64_t n = hi - lo, off0 = read_off[lo];
        const uint64_t out_bytes[2] = {n * sizeof(uint32_t), 2 * n * sizeof(uint64_t)};   // mlen; occ, then sp
        auto launch = [&](const DeviceBatch &b) {
            uint64_t *d_occ = (uint64_t *)b.out[1];
            launch_count(rep->ix, b.bases, b.off, n, (uint32_t *)b.out[0], d_occ, sp ? d_occ + n : nullptr, b.order, b.stream);
        };
        auto fetch = [&](const DeviceBatch &b) {
            const uint64_t *d_occ = (const uint64_t *)b.out[1];
            TRY_HIP(hipMemcpyAsync(mlen + lo, b.out[0], n * sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream), b.stream, msg);
            TRY_HIP(hipMemcpyAsync(occ + lo, d_occ, n * sizeof(uint64_t), hipMemcpyDeviceToHost, b.stream), b.stream, msg);
            if (sp) TRY_HIP(hipMemcpyAsync(sp + lo, d_occ + n, n * sizeof(uint64_t), hipMemcpyDeviceToHost, b.stream), b.stream, msg);
            return COLBWT_OK;
        };
        return replica_batch(rep, bases + off0, read_off + lo, off0, n, max_len, min_len, true, out_bytes, 0, st, msg, launch,
                             fetch);
    };
    return sharded_batch(idx, read_off, n_reads, 0xFFFFFFFFull, "read longer than 2^32-1 bases", true, stats, bad_pointers,
                         part);
}

// Largest max_occ: results are n_reads x max_occ u64 slots, in host memory and in HBM.
constexpr uint32_t kLocateMaxOcc = 1u << 20;

// Locate queries (locate_query.h) for a batch in host memory: mlen and occ per read, max_occ slots
// of positions per read.  Every replica needs its samples attached.
int locate_batch_all(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, uint32_t max_occ,
                     uint32_t *mlen, uint64_t *occ, uint64_t *pos, colbwt_stats *stats) {
    if (idx && (max_occ == 0 || max_occ > kLocateMaxOcc)) return fail(COLBWT_ERR_ARG, "max_occ must be 1 .. 2^20");
    if (idx)
        if (const char *m = samples_missing(idx)) return fail(COLBWT_ERR_ARG, m);
    auto bad_pointers = [&](uint64_t n_bases) -> const char * {
        return (n_bases && !bases) || !mlen || !occ || !pos ? "null bases/mlen/occ/pos" : nullptr;
    };
    auto part = [&](colbwt_index *rep, uint64_t lo, uint64_t hi, uint64_t max_len, uint64_t min_len, colbwt_stats *st,
                    std::string &msg) {
        const uint64_t n = hi - lo, off0 = read_off[lo];
        const uint64_t out_bytes[2] = {n * sizeof(uint32_t), (n + n * max_occ) * sizeof(uint64_t)};   // mlen; occ, then pos
        auto launch = [&](const DeviceBatch &b) {
            uint64_t *d_occ = (uint64_t *)b.out[1];
            launch_locate(rep->ix, rep->loc.toe_row.as<uint32_t>(), rep->loc.phi(), b.bases, b.off, n, max_occ,
                          (uint32_t *)b.out[0], d_occ, d_occ + n, b.order, b.stream);
        };
        auto fetch = [&](const DeviceBatch &b) {
            const uint64_t *d_occ = (const uint64_t *)b.out[1];
            TRY_HIP(hipMemcpyAsync(mlen + lo, b.out[0], n * sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream), b.stream, msg);
            TRY_HIP(hipMemcpyAsync(occ + lo, d_occ, n * sizeof(uint64_t), hipMemcpyDeviceToHost, b.stream), b.stream, msg);
            TRY_HIP(hipMemcpyAsync(pos + lo * max_occ, d_occ + n, n * max_occ * sizeof(uint64_t), hipMemcpyDeviceToHost, b.stream),
                    b.stream, msg);
            return COLBWT_OK;
        };
        return replica_batch(rep, bases + off0, read_off + lo, off0, n, max_len, min_len, true, out_bytes, 0, st, msg, launch,
                             fetch);
    };
    return sharded_batch(idx, read_off, n_reads, 0xFFFFFFFFull, "read longer than 2^32-1 bases", true, stats, bad_pointers,
                         part);
}

// Largest max_anchors: slots are n_reads x max_anchors, as the seeds' are.
constexpr uint32_t kAnchorsMaxSlots = 1u << 16;
const char *kAnchorsSlotSet = "start/len/occ: all three or none; pos exactly when they are given and max_occ > 0";

const char *anchors_bad_params(uint32_t min_len, uint32_t max_anchors, uint32_t max_occ) {
    if (min_len == 0) return "min_len must be at least 1";
    if (max_anchors == 0 || max_anchors > kAnchorsMaxSlots) return "max_anchors must be 1 .. 2^16";
    if (max_occ > kLocateMaxOcc) return "max_occ must be 0 .. 2^20";
    return nullptr;
}

// Parameters, then the samples (only max_occ > 0 needs them), then the slot pointer set.
const char *anchors_bad_setup(const colbwt_index *idx, uint32_t min_len, uint32_t max_anchors, uint32_t max_occ, const void *start,
                              const void *len, const void *occ, const void *pos) {
    if (const char *m = anchors_bad_params(min_len, max_anchors, max_occ)) return m;
    if (max_occ > 0)
        if (const char *m = samples_missing(idx)) return m;
    if ((start != nullptr) != (len != nullptr) || (start != nullptr) != (occ != nullptr) ||
        (pos != nullptr) != (start != nullptr && max_occ > 0))
        return kAnchorsSlotSet;
    return nullptr;
}

AnchorsArgs anchors_args(const colbwt_index *rep, uint32_t min_len, uint32_t max_anchors, uint32_t max_occ, void *summary,
                         uint32_t *start, uint32_t *len, uint64_t *occ, uint64_t *pos) {
    AnchorsArgs A{};
    if (pos) {
        A.toe_row = rep->loc.toe_row.as<const uint32_t>();
        A.phi = rep->loc.phi();
    }
    A.min_len = min_len;
    A.max_anchors = max_anchors;
    A.max_occ = max_occ;
    A.summary = (uint4 *)summary;
    A.start = start;
    A.len = len;
    A.occ = occ;
    A.pos = pos;
    return A;
}

// Anchors (anchors_query.h) for a batch in host memory.  The first result array of the scratch holds the
// summaries, then start and len of every slot; the second occ, then the positions.
int anchors_batch_all(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, uint32_t min_len,
                      uint32_t max_anchors, uint32_t max_occ, colbwt_anchor_summary *summary, uint32_t *start, uint32_t *len,
                      uint64_t *occ, uint64_t *pos, colbwt_stats *stats) {
    if (idx) {
        if (const char *m = anchors_bad_setup(idx, min_len, max_anchors, max_occ, start, len, occ, pos)) return fail(COLBWT_ERR_ARG, m);
        if (n_reads >= 0xFFFFFFFFull) return fail(COLBWT_ERR_ARG, kTooManyReads);
    }
    const uint64_t K = max_anchors, W = pos ? max_occ : 0;
    auto bad_pointers = [&](uint64_t n_bases) -> const char * {
        return (n_bases && !bases) || !summary ? "null bases/summary" : nullptr;
    };
    auto part = [&](colbwt_index *rep, uint64_t lo, uint64_t hi, uint64_t max_len, uint64_t min_read, colbwt_stats *st,
                    std::string &msg) {
        const uint64_t n = hi - lo, off0 = read_off[lo], slots = start ? n * K : 0;
        const uint64_t out_bytes[2] = {n * 32 + 2 * slots * sizeof(uint32_t), (slots + slots * W) * sizeof(uint64_t)};
        auto launch = [&](const DeviceBatch &b) {
            uint32_t *d_start = (uint32_t *)((uint8_t *)b.out[0] + n * 32);
            uint64_t *d_occ = (uint64_t *)b.out[1];
            launch_anchors(rep->ix,
                           anchors_args(rep, min_len, max_anchors, max_occ, b.out[0], start ? d_start : nullptr,
                                        start ? d_start + slots : nullptr, start ? d_occ : nullptr, pos ? d_occ + slots : nullptr),
                           b.bases, b.off, n, b.order, b.stream);
        };
        auto fetch = [&](const DeviceBatch &b) {
            const uint32_t *d_start = (const uint32_t *)((const uint8_t *)b.out[0] + n * 32);
            const uint64_t *d_occ = (const uint64_t *)b.out[1];
            TRY_HIP(hipMemcpyAsync(summary + lo, b.out[0], n * 32, hipMemcpyDeviceToHost, b.stream), b.stream, msg);
            if (slots) {
                TRY_HIP(hipMemcpyAsync(start + lo * K, d_start, slots * sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream), b.stream, msg);
                TRY_HIP(hipMemcpyAsync(len + lo * K, d_start + slots, slots * sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream), b.stream,
                        msg);
                TRY_HIP(hipMemcpyAsync(occ + lo * K, d_occ, slots * sizeof(uint64_t), hipMemcpyDeviceToHost, b.stream), b.stream, msg);
            }
            if (slots * W)
                TRY_HIP(hipMemcpyAsync(pos + lo * K * W, d_occ + slots, slots * W * sizeof(uint64_t), hipMemcpyDeviceToHost, b.stream),
                        b.stream, msg);
            return COLBWT_OK;
        };
        return replica_batch(rep, bases + off0, read_off + lo, off0, n, max_len, min_read, true, out_bytes, 0, st, msg, launch,
                             fetch);
    };
    return sharded_batch(idx, read_off, n_reads, 0xFFFFFFFFull, "read longer than 2^32-1 bases", true, stats, bad_pointers,
                         part);
}

const char *kDocsTooMany = "more than 4096 documents";   // kDocsLds: doc_start and the tally live in a block's LDS

const char *docs_bad_params(uint32_t min_len, uint32_t max_walk) {
    if (min_len == 0) return "min_len must be at least 1";
    if (max_walk == 0 || max_walk > kDocsMaxWalk) return "max_walk must be 1 .. 2^20";
    return nullptr;
}

const char *chain_bad_params(uint32_t max_anchors, uint32_t max_occ) {
    if (max_anchors == 0) return "max_anchors must be at least 1";
    if (max_occ == 0) return "max_occ must be at least 1";
    if ((uint64_t)max_anchors * max_occ > kChainMaxHits) return "max_anchors * max_occ must be at most 256";
    return nullptr;
}

// The chain parameters, then the samples of every replica and their document count.
const char *chain_bad_setup(const colbwt_index *idx, uint32_t max_anchors, uint32_t max_occ) {
    if (const char *m = chain_bad_params(max_anchors, max_occ)) return m;
    if (const char *m = samples_missing(idx)) return m;
    if (idx->loc.n_docs() > kDocsLds) return kDocsTooMany;
    return nullptr;
}

ChainArgs chain_args(const colbwt_index *rep, const uint32_t *start, const uint32_t *len, const uint64_t *pos, uint32_t max_anchors,
                     uint32_t max_occ, uint32_t band, void *chain) {
    return ChainArgs{start, len, pos, rep->loc.doc_dev.as<const uint32_t>(), rep->loc.n_docs(), max_anchors, max_occ, band, (uint4 *)chain};
}

// The anchors' arrays of a chain call, cut from a 256-byte aligned scratch of chain_work_bytes() bytes.
struct ChainWork {
    colbwt_anchor_summary *summary;
    uint32_t *start, *len;
    uint64_t *occ, *pos;
};
uint64_t chain_work_bytes(uint64_t n_reads, uint32_t max_anchors, uint32_t max_occ) {
    const uint64_t slots = n_reads * max_anchors;
    return docs_align(32 * n_reads) + 2 * docs_align(4 * slots) + docs_align(8 * slots) + docs_align(8 * slots * max_occ);
}
ChainWork chain_work(void *d_work, uint64_t n_reads, uint32_t max_anchors, uint32_t max_occ) {
    const uint64_t slots = n_reads * max_anchors;
    uint8_t *p = (uint8_t *)d_work;
    ChainWork w;
    w.summary = (colbwt_anchor_summary *)p;
    p += docs_align(32 * n_reads);
    w.start = (uint32_t *)p;
    p += docs_align(4 * slots);
    w.len = (uint32_t *)p;
    p += docs_align(4 * slots);
    w.occ = (uint64_t *)p;
    p += docs_align(8 * slots);
    w.pos = (uint64_t *)p;
    return w;
}

// Anchors into `d_work`, then the reduction (chain_reduce.h), back to back on one stream.
hipError_t launch_chain_of_reads(const colbwt_index *rep, const uint8_t *d_bases, const uint64_t *d_read_off, uint64_t n_reads,
                                 uint32_t min_len, uint32_t max_anchors, uint32_t max_occ, uint32_t band, void *d_chain, void *d_work,
                                 const uint32_t *d_order, hipStream_t stream) {
    const ChainWork w = chain_work(d_work, n_reads, max_anchors, max_occ);
    launch_anchors(rep->ix, anchors_args(rep, min_len, max_anchors, max_occ, w.summary, w.start, w.len, w.occ, w.pos), d_bases, d_read_off,
                   n_reads, d_order, stream);
    return launch_chain(chain_args(rep, w.start, w.len, w.pos, max_anchors, max_occ, band, d_chain), n_reads, stream);
}

// Chains for a batch in host memory: the first result array of the scratch holds the records, the second
// the anchors' arrays, which never leave HBM.
int chain_batch_all(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, uint32_t min_len,
                    uint32_t max_anchors, uint32_t max_occ, uint32_t band, colbwt_chain *chain, colbwt_stats *stats) {
    if (idx) {
        if (min_len == 0) return fail(COLBWT_ERR_ARG, "min_len must be at least 1");
        if (const char *m = chain_bad_setup(idx, max_anchors, max_occ)) return fail(COLBWT_ERR_ARG, m);
        if (n_reads >= 0xFFFFFFFFull) return fail(COLBWT_ERR_ARG, kTooManyReads);
    }
    auto bad_pointers = [&](uint64_t n_bases) -> const char * { return (n_bases && !bases) || !chain ? "null bases/chain" : nullptr; };
    auto part = [&](colbwt_index *rep, uint64_t lo, uint64_t hi, uint64_t max_len, uint64_t min_read, colbwt_stats *st,
                    std::string &msg) {
        const uint64_t n = hi - lo, off0 = read_off[lo];
        const uint64_t out_bytes[2] = {n * sizeof(colbwt_chain), chain_work_bytes(n, max_anchors, max_occ)};
        hipError_t launched = hipSuccess;
        auto launch = [&](const DeviceBatch &b) {
            launched = launch_chain_of_reads(rep, b.bases, b.off, n, min_len, max_anchors, max_occ, band, b.out[0], b.out[1], b.order,
                                             b.stream);
        };
        auto fetch = [&](const DeviceBatch &b) {
            TRY_HIP(launched, b.stream, msg);
            TRY_HIP(hipMemcpyAsync(chain + lo, b.out[0], n * sizeof(colbwt_chain), hipMemcpyDeviceToHost, b.stream), b.stream, msg);
            return COLBWT_OK;
        };
        return replica_batch(rep, bases + off0, read_off + lo, off0, n, max_len, min_read, true, out_bytes, 0, st, msg, launch,
                             fetch);
    };
    return sharded_batch(idx, read_off, n_reads, 0xFFFFFFFFull, "read longer than 2^32-1 bases", true, stats, bad_pointers,
                         part);
}

// Docs (docs_query.h) for a batch in host memory: search, order, walk and tally run back to back on
// the replica's stream; positions never leave HBM.  The first result array of the scratch holds mlen,
// then n_hit; the second the workspace, occ, the masks and the shard's two tallies, which are summed
// on the host (doc_reads / doc_only receive the totals of the call).
int docs_batch_all(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, uint32_t min_len,
                   uint32_t max_walk, uint32_t *mlen, uint64_t *occ, uint32_t *n_hit, uint64_t *mask, uint64_t *doc_reads,
                   uint64_t *doc_only, colbwt_stats *stats) {
    if (idx) {
        if (const char *m = docs_bad_params(min_len, max_walk)) return fail(COLBWT_ERR_ARG, m);
        if (const char *m = samples_missing(idx)) return fail(COLBWT_ERR_ARG, m);
        if (idx->loc.n_docs() > kDocsLds) return fail(COLBWT_ERR_ARG, kDocsTooMany);
        if (n_reads >= 0xFFFFFFFFull) return fail(COLBWT_ERR_ARG, kTooManyReads);
    }
    const uint32_t n_docs = idx ? idx->loc.n_docs() : 0, n_words = docs_mask_words(n_docs);
    const bool tally = doc_reads || doc_only;
    std::vector<uint64_t> total(tally ? 2 * (size_t)n_docs : 0, 0);   // the caller's arrays are written on success only
    std::mutex tally_mu;
    auto bad_pointers = [&](uint64_t n_bases) -> const char * {
        return (n_bases && !bases) || !mlen || !occ || !n_hit || !mask ? "null bases/mlen/occ/n_hit/mask" : nullptr;
    };
    auto part = [&](colbwt_index *rep, uint64_t lo, uint64_t hi, uint64_t max_len, uint64_t min_read, colbwt_stats *st,
                    std::string &msg) {
        const uint64_t n = hi - lo, off0 = read_off[lo];
        const uint64_t work = docs_work_bytes(n), mask_bytes = n * n_words * sizeof(uint64_t);
        const uint64_t out_bytes[2] = {2 * n * sizeof(uint32_t), work + n * sizeof(uint64_t) + mask_bytes + 16ull * n_docs};
        std::vector<uint64_t> shard(tally ? 2 * (size_t)n_docs : 0);
        hipError_t launched = hipSuccess;
        auto launch = [&](const DeviceBatch &b) {
            uint32_t *d_mlen = (uint32_t *)b.out[0];
            uint64_t *d_occ = (uint64_t *)((uint8_t *)b.out[1] + work), *d_mask = d_occ + n, *d_tally = d_mask + n * n_words;
            if (tally) launched = hipMemsetAsync(d_tally, 0, 16ull * n_docs, b.stream);
            if (launched == hipSuccess)
                launched = launch_docs(rep->ix, rep->loc.docs(min_len, max_walk), b.bases, b.off, n, d_mlen, d_occ, d_mlen + n, d_mask,
                                       doc_reads ? d_tally : nullptr, doc_only ? d_tally + n_docs : nullptr, b.out[1], b.order,
                                       b.stream);
        };
        auto fetch = [&](const DeviceBatch &b) {
            TRY_HIP(launched, b.stream, msg);
            const uint32_t *d_mlen = (const uint32_t *)b.out[0];
            const uint64_t *d_occ = (const uint64_t *)((const uint8_t *)b.out[1] + work), *d_mask = d_occ + n;
            TRY_HIP(hipMemcpyAsync(mlen + lo, d_mlen, n * sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream), b.stream, msg);
            TRY_HIP(hipMemcpyAsync(n_hit + lo, d_mlen + n, n * sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream), b.stream, msg);
            TRY_HIP(hipMemcpyAsync(occ + lo, d_occ, n * sizeof(uint64_t), hipMemcpyDeviceToHost, b.stream), b.stream, msg);
            if (mask_bytes)
                TRY_HIP(hipMemcpyAsync(mask + lo * n_words, d_mask, mask_bytes, hipMemcpyDeviceToHost, b.stream), b.stream, msg);
            if (tally)
                TRY_HIP(hipMemcpyAsync(shard.data(), d_mask + n * n_words, 16ull * n_docs, hipMemcpyDeviceToHost, b.stream), b.stream,
                        msg);
            return COLBWT_OK;
        };
        const int rc = replica_batch(rep, bases + off0, read_off + lo, off0, n, max_len, min_read, true, out_bytes, 0, st, msg, launch,
                                     fetch);
        if (rc == COLBWT_OK && tally) {
            std::lock_guard<std::mutex> g(tally_mu);
            for (size_t d = 0; d < total.size(); ++d) total[d] += shard[d];
        }
        return rc;
    };
    const int rc = sharded_batch(idx, read_off, n_reads, 0xFFFFFFFFull, "read longer than 2^32-1 bases", true, stats, bad_pointers,
                                 part);
    if (rc == COLBWT_OK && doc_reads) std::copy(total.begin(), total.begin() + n_docs, doc_reads);
    if (rc == COLBWT_OK && doc_only) std::copy(total.begin() + n_docs, total.end(), doc_only);
    return rc;
}

// Where the shards of a colbwt_locate_all_batch call meet: a shard's positions start behind those of
// the reads before it, and nothing may be written unless the whole batch fits, so every shard
// publishes the number of its positions and waits for the others'.  The shards are disjoint and
// cover the batch, so "all published" is "as many reads published as the batch has".  A shard that
// fails before it publishes releases the others, which then leave without filling.
struct LocAllShards {
    struct Done {
        uint64_t lo, hi, total;
    };
    std::mutex mu;
    std::condition_variable cv;
    std::vector<Done> done;
    bool failed = false;
    uint64_t n_reads = 0;
    // -> false when a shard failed; else `base` = the positions of the reads before `lo`, `all` = the batch's
    bool publish(uint64_t lo, uint64_t hi, uint64_t total, uint64_t &base, uint64_t &all) {
        std::unique_lock<std::mutex> lk(mu);
        done.push_back(Done{lo, hi, total});
        cv.notify_all();
        for (;;) {
            if (failed) return false;
            uint64_t covered = 0;
            base = all = 0;
            for (const Done &d : done) {
                covered += d.hi - d.lo;
                all += d.total;
                if (d.hi <= lo) base += d.total;
            }
            if (covered == n_reads) return true;
            cv.wait(lk);
        }
    }
    void fail() {
        std::lock_guard<std::mutex> g(mu);
        failed = true;
        cv.notify_all();
    }
};

struct EventPair {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~EventPair() {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
    hipError_t create() {
        hipError_t r = hipSuccess;
        for (hipEvent_t &x : e)
            if (r == hipSuccess && !x) r = hipEventCreate(&x);
        return r;
    }
};

// Locate-all (locate_all_query.h) for a batch in host memory: per shard the search and the plan, then
// -- once every shard knows where its positions start and that the batch fits pos_cap -- the walk into
// a buffer of the shard's size and the copy into the caller's packed array.  mlen, occ and pos_off are
// filled whenever the search ran; pos only when pos_off[n_reads] <= pos_cap.
int locate_all_batch_all(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, uint32_t min_len,
                         uint64_t max_per_read, uint32_t *mlen, uint64_t *occ, uint64_t *pos_off, uint64_t *pos, uint64_t pos_cap,
                         colbwt_stats *stats) {
    if (idx) {
        if (min_len == 0) return fail(COLBWT_ERR_ARG, "min_len must be at least 1");
        if (const char *m = samples_missing(idx)) return fail(COLBWT_ERR_ARG, m);
        if (n_reads >= 0xFFFFFFFFull) return fail(COLBWT_ERR_ARG, kTooManyReads);
        if (n_reads == 0 && pos_off) pos_off[0] = 0;
    }
    auto bad_pointers = [&](uint64_t n_bases) -> const char * {
        if ((n_bases && !bases) || !mlen || !occ || !pos_off) return "null bases/mlen/occ/pos_off";
        return pos_cap && !pos ? "null pos with pos_cap > 0" : nullptr;
    };
    LocAllShards shards;
    shards.n_reads = n_reads;
    auto part = [&](colbwt_index *rep, uint64_t lo, uint64_t hi, uint64_t max_len, uint64_t min_read, colbwt_stats *st,
                    std::string &msg) {
        struct Guard {
            LocAllShards &s;
            bool armed = true;
            ~Guard() { if (armed) s.fail(); }
        } guard{shards};
        const uint64_t n = hi - lo, off0 = read_off[lo];
        const uint64_t work = locate_all_work_bytes(n);
        const uint64_t out_bytes[2] = {n * sizeof(uint32_t), work + (2 * n + 1) * sizeof(uint64_t)};   // mlen; workspace, occ, pos_off
        hipError_t launched = hipSuccess;
        EventPair walk;
        bool walked = false;
        auto launch = [&](const DeviceBatch &b) {
            uint64_t *d_occ = (uint64_t *)((uint8_t *)b.out[1] + work);
            launched = launch_locate_all_plan(rep->ix, rep->loc.all(), b.bases, b.off, n, min_len, max_per_read, (uint32_t *)b.out[0],
                                              d_occ, d_occ + n, b.out[1], b.order, b.stream);
        };
        auto fetch = [&](const DeviceBatch &b) {
            TRY_HIP(launched, b.stream, msg);
            const uint64_t *d_occ = (const uint64_t *)((const uint8_t *)b.out[1] + work), *d_off = d_occ + n;
            TRY_HIP(hipMemcpyAsync(mlen + lo, b.out[0], n * sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream), b.stream, msg);
            TRY_HIP(hipMemcpyAsync(occ + lo, d_occ, n * sizeof(uint64_t), hipMemcpyDeviceToHost, b.stream), b.stream, msg);
            TRY_HIP(hipMemcpyAsync(pos_off + lo + 1, d_off + 1, n * sizeof(uint64_t), hipMemcpyDeviceToHost, b.stream), b.stream, msg);
            TRY_HIP(hipStreamSynchronize(b.stream), b.stream, msg);
            const uint64_t total = pos_off[hi];          // still counted from the shard's first read
            uint64_t base = 0, all = 0;
            const bool go = shards.publish(lo, hi, total, base, all);
            guard.armed = false;
            if (!go) return COLBWT_OK;                   // the failing shard reports
            if (base)
                for (uint64_t k = lo + 1; k <= hi; ++k) pos_off[k] += base;
            if (all > pos_cap || total == 0) return COLBWT_OK;
            std::unique_lock<std::mutex> lease(rep->all_mu, std::defer_lock);
            DevPtr own;
            DevPtr &buf = lease.try_lock() ? rep->all_pos : own;
            if (buf.bytes() < total * sizeof(uint64_t)) {
                buf.reset();
                TRY_HIP(buf.alloc(total * sizeof(uint64_t) + total + 4096), b.stream, msg);
            }
            TRY_HIP(walk.create(), b.stream, msg);
            TRY_HIP(hipEventRecord(walk.e[0], b.stream), b.stream, msg);
            launch_locate_all_fill(rep->ix, rep->loc.all(), n, 0, n, d_off, buf.as<uint64_t>(), total, b.out[1], b.stream);
            TRY_HIP(hipGetLastError(), b.stream, msg);
            TRY_HIP(hipEventRecord(walk.e[1], b.stream), b.stream, msg);
            TRY_HIP(hipMemcpyAsync(pos + base, buf.get(), total * sizeof(uint64_t), hipMemcpyDeviceToHost, b.stream), b.stream, msg);
            TRY_HIP(hipStreamSynchronize(b.stream), b.stream, msg);   // the buffer's lease ends with this call
            walked = true;
            return COLBWT_OK;
        };
        const int rc = replica_batch(rep, bases + off0, read_off + lo, off0, n, max_len, min_read, true, out_bytes, 0, st, msg, launch,
                                     fetch);
        if (rc == COLBWT_OK && walked) {                  // kernel_ms: search and scans + the walk
            float ms = 0;
            TRY_HIP(hipEventElapsedTime(&ms, walk.e[0], walk.e[1]), nullptr, msg);
            st->kernel_ms += ms;
            st->d2h_ms = std::max(0.0, st->d2h_ms - ms);
        }
        return rc;
    };
    if (idx && n_reads && pos_off) pos_off[0] = 0;
    const int rc = sharded_batch(idx, read_off, n_reads, 0xFFFFFFFFull, "read longer than 2^32-1 bases", true, stats, bad_pointers,
                                 part);
    if (rc == COLBWT_OK && n_reads && pos_off[n_reads] > pos_cap)
        return fail(COLBWT_ERR_ARG, "pos_cap too small: the batch has " + std::to_string(pos_off[n_reads]) + " positions (pos_off[n_reads])");
    return rc;
}

// Largest max_seeds: results are n_reads x max_seeds slots of 9 bytes, in host memory and in HBM.
constexpr uint32_t kSeedsMaxSeeds = 1u << 16;

const char *seeds_bad_params(uint32_t min_len, uint32_t max_seeds) {
    if (min_len == 0) return "min_len must be at least 1";
    if (max_seeds == 0 || max_seeds > kSeedsMaxSeeds) return "max_seeds must be 1 .. 2^16";
    return nullptr;
}

// Seeds (seeds_reduce.h) for a batch in host memory: the query and the reduction of its output run
// back to back on the replica's stream; the per-base arrays never leave HBM.  The first result array
// of the scratch holds pml (u16, or u32 when a read is longer than 65535), then cid; the second the
// summaries, then the three slot arrays.
int seeds_batch_all(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, uint32_t min_len,
                    uint32_t max_seeds, uint32_t *summary, uint32_t *seed_pos, uint32_t *seed_len, uint8_t *seed_cid,
                    colbwt_stats *stats) {
    if (idx)
        if (const char *m = seeds_bad_params(min_len, max_seeds)) return fail(COLBWT_ERR_ARG, m);
    if (idx && n_reads >= 0xFFFFFFFFull) return fail(COLBWT_ERR_ARG, kTooManyReads);
    const bool slots = seed_pos != nullptr;
    auto bad_pointers = [&](uint64_t n_bases) -> const char * {
        if ((n_bases && !bases) || !summary) return "null bases/summary";
        if ((seed_pos != nullptr) != (seed_len != nullptr) || (seed_pos != nullptr) != (seed_cid != nullptr))
            return "seed_pos/seed_len/seed_cid: all three or none";
        return nullptr;
    };
    auto part = [&](colbwt_index *rep, uint64_t lo, uint64_t hi, uint64_t max_len, uint64_t min_read, colbwt_stats *st,
                    std::string &msg) {
        const uint64_t n = hi - lo, off0 = read_off[lo], n_bases = read_off[hi] - off0;
        const int pml_bytes = max_len > 65535 ? 4 : 2;
        const uint64_t padded = (n_bases + 63) & ~63ull, n_slots = slots ? n * max_seeds : 0;
        const uint64_t out_bytes[2] = {padded * (pml_bytes + 1) + 64, n * 32 + n_slots * 9};
        auto launch = [&](const DeviceBatch &b) {
            uint8_t *d_pml = (uint8_t *)b.out[0], *d_cid = d_pml + padded * pml_bytes;
            uint32_t *d_sum = (uint32_t *)b.out[1], *d_pos = d_sum + n * 8, *d_len = d_pos + n_slots;
            if (n_bases) launch_query(rep->ix, b.bases, b.off, n, n_bases, d_pml, pml_bytes, d_cid, b.order, b.stream);
            (void)launch_seeds_reduce(d_pml, pml_bytes, d_cid, b.off, n, n_bases, min_len, max_seeds, d_sum, slots ? d_pos : nullptr,
                                      slots ? d_len : nullptr, slots ? (uint8_t *)(d_len + n_slots) : nullptr, b.stream);
        };
        auto fetch = [&](const DeviceBatch &b) {
            const uint32_t *d_sum = (const uint32_t *)b.out[1], *d_pos = d_sum + n * 8, *d_len = d_pos + n_slots;
            TRY_HIP(hipMemcpyAsync(summary + lo * 8, d_sum, n * 32, hipMemcpyDeviceToHost, b.stream), b.stream, msg);
            if (slots) {
                TRY_HIP(hipMemcpyAsync(seed_pos + lo * max_seeds, d_pos, n_slots * 4, hipMemcpyDeviceToHost, b.stream), b.stream, msg);
                TRY_HIP(hipMemcpyAsync(seed_len + lo * max_seeds, d_len, n_slots * 4, hipMemcpyDeviceToHost, b.stream), b.stream, msg);
                TRY_HIP(hipMemcpyAsync(seed_cid + lo * max_seeds, d_len + n_slots, n_slots, hipMemcpyDeviceToHost, b.stream), b.stream,
                        msg);
            }
            return COLBWT_OK;
        };
        return replica_batch(rep, bases + off0, read_off + lo, off0, n, max_len, min_read, pml_reads_order(rep->ix), out_bytes,
                             kAlgBytesPerBase, st, msg, launch, fetch);
    };
    return sharded_batch(idx, read_off, n_reads, 0xFFFFFFFFull, "read longer than 2^32-1 bases", false, stats, bad_pointers, part);
}

// ---- .col_loc (include/colbwt.h): header, end_sa[r], phi pairs[s], doc_start[n_docs] ----
constexpr uint64_t kLocHeader = 40;
const char kLocMagic[8] = {'C', 'O', 'L', 'B', 'W', 'T', 'L', 'C'};

struct LocFile {
    uint64_t n = 0, r = 0, s = 0;
    uint32_t n_docs = 0;
    const uint32_t *end_sa = nullptr, *pair = nullptr, *doc_start = nullptr;
};

// Everything that can be checked without the device: header, length, value ranges, sorted phi positions.
int parse_loc(const uint8_t *p, uint64_t len, const Index &ix, LocFile &f, std::string &msg) {
    uint32_t version = 0;
    if (len < kLocHeader || memcmp(p, kLocMagic, 8) != 0) { msg = "not a .col_loc file (magic)"; return COLBWT_ERR_FORMAT; }
    memcpy(&version, p + 8, 4);
    memcpy(&f.n_docs, p + 12, 4);
    memcpy(&f.n, p + 16, 8);
    memcpy(&f.r, p + 24, 8);
    memcpy(&f.s, p + 32, 8);
    if (version != 1) { msg = ".col_loc version " + std::to_string(version) + " (1 expected)"; return COLBWT_ERR_FORMAT; }
    if (f.n != ix.n()) { msg = ".col_loc n = " + std::to_string(f.n) + ", the table's n = " + std::to_string(ix.n()); return COLBWT_ERR_FORMAT; }
    if (f.r != ix.bwt_r()) { msg = ".col_loc r = " + std::to_string(f.r) + ", the table's bwt_r = " + std::to_string(ix.bwt_r()); return COLBWT_ERR_FORMAT; }
    if (f.s == 0 || f.s > f.n || f.n_docs == 0 || f.n_docs > f.n) { msg = ".col_loc: bad sample or document count"; return COLBWT_ERR_FORMAT; }
    if (len != kLocHeader + 4 * f.r + 8 * f.s + 4 * (uint64_t)f.n_docs) { msg = ".col_loc: file length does not match its header"; return COLBWT_ERR_FORMAT; }
    if ((uintptr_t)p & 3) { msg = ".col_loc image must be 4-byte aligned"; return COLBWT_ERR_ARG; }
    f.end_sa = (const uint32_t *)(p + kLocHeader);
    f.pair = f.end_sa + f.r;
    f.doc_start = f.pair + 2 * f.s;
    for (uint64_t i = 0; i < f.r; ++i)
        if (f.end_sa[i] >= f.n) { msg = ".col_loc: end_sa[" + std::to_string(i) + "] >= n"; return COLBWT_ERR_FORMAT; }
    if (f.pair[0] != 0) { msg = ".col_loc: the first phi sample is not position 0"; return COLBWT_ERR_FORMAT; }
    for (uint64_t i = 0; i < f.s; ++i) {
        if (f.pair[2 * i] >= f.n || f.pair[2 * i + 1] >= f.n) { msg = ".col_loc: phi sample " + std::to_string(i) + " >= n"; return COLBWT_ERR_FORMAT; }
        if (i && f.pair[2 * i] <= f.pair[2 * i - 2]) { msg = ".col_loc: phi positions do not ascend at sample " + std::to_string(i); return COLBWT_ERR_FORMAT; }
    }
    for (uint32_t d = 0; d < f.n_docs; ++d)
        if (f.doc_start[d] >= f.n || (d ? f.doc_start[d] <= f.doc_start[d - 1] : f.doc_start[0] != 0)) {
            msg = ".col_loc: document starts must ascend from 0";
            return COLBWT_ERR_FORMAT;
        }
    return COLBWT_OK;
}

// The samples onto one replica: end_sa scattered to the layout's run-ending rows (whose number must be
// r), the phi pairs and their directory.  On failure the replica keeps no locate tables.
int attach_one(colbwt_index *rep, const LocFile &f, std::string &msg) {
    rep->loc.reset();
    int rc = select_device(rep->ix.device(), msg);
    if (rc != COLBWT_OK) return rc;
    LocateTables &L = rep->loc;
    const uint64_t rows = rep->ix.table_rows();
    // shift: buckets of 2^shift positions, 2^shift <= n / s < 2^(shift+1) -- about one sample per bucket
    // and a directory of s .. 2s entries
    uint32_t shift = 0;
    while (shift < 31 && (f.s << (shift + 1)) <= f.n) ++shift;
    const uint64_t n_buckets = ((f.n - 1) >> shift) + 1;
    DevPtr flag, sel, count, tmp, end_sa;
    size_t tmp_bytes = 0;
    TRY_HIP(hipcub::DeviceSelect::Flagged(nullptr, tmp_bytes, hipcub::CountingInputIterator<uint32_t>(0), (uint8_t *)nullptr,
                                          (uint32_t *)nullptr, (unsigned long long *)nullptr, (size_t)rows),
            nullptr, msg);
    TRY_HIP(flag.alloc(rows), nullptr, msg);
    TRY_HIP(sel.alloc(4 * rows), nullptr, msg);
    TRY_HIP(count.alloc(8), nullptr, msg);
    TRY_HIP(tmp.alloc(tmp_bytes + 256), nullptr, msg);
    TRY_HIP(end_sa.alloc(4 * f.r), nullptr, msg);
    TRY_HIP(L.toe_row.alloc(4 * rows), nullptr, msg);
    TRY_HIP(L.pair.alloc(8 * f.s), nullptr, msg);
    TRY_HIP(L.dir.alloc(4 * (n_buckets + 1)), nullptr, msg);
    TRY_HIP(L.doc_dev.alloc(4 * (uint64_t)f.n_docs), nullptr, msg);
    TRY_HIP(hipMemcpy(L.doc_dev.get(), f.doc_start, 4 * (uint64_t)f.n_docs, hipMemcpyHostToDevice), nullptr, msg);
    TRY_HIP(hipMemcpy(end_sa.get(), f.end_sa, 4 * f.r, hipMemcpyHostToDevice), nullptr, msg);
    TRY_HIP(hipMemcpy(L.pair.get(), f.pair, 8 * f.s, hipMemcpyHostToDevice), nullptr, msg);
    TRY_HIP(hipMemset(L.toe_row.get(), 0, 4 * rows), nullptr, msg);
    TRY_HIP(run_end_rows(rep->ix, flag.as<uint8_t>(), sel.as<uint32_t>(), count.as<unsigned long long>(), tmp.get(), tmp_bytes + 256,
                         nullptr),
            nullptr, msg);
    unsigned long long ends = 0;
    TRY_HIP(hipMemcpy(&ends, count.get(), 8, hipMemcpyDeviceToHost), nullptr, msg);
    if (ends != f.r) {
        L.reset();
        msg = "the table has " + std::to_string(ends) + " rows that end a run, the .col_loc " + std::to_string(f.r) + " runs";
        return COLBWT_ERR_FORMAT;
    }
    const uint32_t *p_sel = sel.as<uint32_t>(), *p_end = end_sa.as<uint32_t>();
    uint32_t *p_toe = L.toe_row.as<uint32_t>(), *p_dir = L.dir.as<uint32_t>();
    const uint2 *p_pair = L.pair.as<const uint2>();
    hipLaunchKernelGGL(toe_scatter_kernel, dim3(locate_grid(f.r)), dim3(kLocBlock), 0, nullptr, p_sel, p_end, f.r, p_toe);
    hipLaunchKernelGGL(phi_dir_kernel, dim3(locate_grid(n_buckets + 1)), dim3(kLocBlock), 0, nullptr, p_pair, f.s, shift, n_buckets,
                       p_dir);
    TRY_HIP(hipGetLastError(), nullptr, msg);
    TRY_HIP(hipDeviceSynchronize(), nullptr, msg);
    L.shift = shift;
    L.n_buckets = n_buckets;
    L.doc_start.assign(f.doc_start, f.doc_start + f.n_docs);
    return COLBWT_OK;
}

}  // namespace

namespace {

// One batch of reads on its way through the three stages of colbwt_query_file.
struct FileBatch {
    std::vector<uint8_t> bases;
    std::vector<uint64_t> off;
    std::vector<std::string> names;
    PinnedBuf own_pml, own_cid;      // u16 or u32 values / u8 col ids, one per base
    PinnedBuf *pml = &own_pml, *cid = &own_cid;   // ... or the handle's, kept across calls
    bool wide = false;
};

// Hand-over point between two stages (a few batches deep; nullptr = end of stream).
class BatchQueue {
public:
    void push(FileBatch *b) {
        std::lock_guard<std::mutex> g(mu_);
        q_.push_back(b);
        cv_.notify_one();
    }
    FileBatch *pop() {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return !q_.empty(); });
        FileBatch *b = q_.front();
        q_.pop_front();
        return b;
    }

private:
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<FileBatch *> q_;
};

}  // namespace

// The replica of a multi-device handle that lives on the device holding `d_ptr` (the first one
// when the pointer's device cannot be told or holds no replica).
static colbwt_index *replica_for(colbwt_index *idx, const void *d_ptr) {
    if (idx->more.empty()) return idx;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, d_ptr) != hipSuccess) {
        (void)hipGetLastError();
        return idx;
    }
    if (a.device == idx->ix.device()) return idx;
    for (colbwt_index *r : idx->more)
        if (r->ix.device() == a.device) return r;
    return idx;
}

// The skeleton of a device entry point: `bad_argument()` names the first bad argument (after the
// index; any pointer is fine when there are no reads), then `launch(ix, stream)` runs on the replica
// on d_bases's device.  With `stats`, the launch is timed by two events and waited for.
template <typename ArgCheck, typename Launch>
static int device_entry(colbwt_index *idx, const void *d_bases, uint64_t n_reads, uint64_t n_bases, void *hip_stream,
                        uint64_t alg_bytes_per_base, colbwt_stats *stats, ArgCheck bad_argument, Launch launch) {
    if (!idx) return fail(COLBWT_ERR_ARG, "null index");
    if (stats) memset(stats, 0, sizeof(*stats));
    if (const char *m = bad_argument()) return fail(COLBWT_ERR_ARG, m);
    if (n_reads == 0) return COLBWT_OK;
    idx = replica_for(idx, d_bases);
    const int rc = select_device(idx->ix.device(), g_err);
    if (rc != COLBWT_OK) return rc;
    const hipStream_t stream = (hipStream_t)hip_stream;
    struct Events {
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Events() {
            for (hipEvent_t x : e)
                if (x) (void)hipEventDestroy(x);
        }
    } ev;
    if (stats) {
        TRY_HIP(hipEventCreate(&ev.e[0]), nullptr, g_err);
        TRY_HIP(hipEventCreate(&ev.e[1]), nullptr, g_err);
        TRY_HIP(hipEventRecord(ev.e[0], stream), nullptr, g_err);
    }
    launch(idx->ix, stream);
    TRY_HIP(hipGetLastError(), nullptr, g_err);
    if (stats) {
        float ms = 0;
        TRY_HIP(hipEventRecord(ev.e[1], stream), nullptr, g_err);
        TRY_HIP(hipEventSynchronize(ev.e[1]), nullptr, g_err);
        TRY_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]), nullptr, g_err);
        stats->n_reads = n_reads;
        stats->n_bases = n_bases;
        stats->kernel_ms = ms;
        stats->algorithmic_bytes = n_bases * alg_bytes_per_base;
    }
    return COLBWT_OK;
}

extern "C" {

const char *colbwt_version(void) { return "colbwt-mi355x 0.2.0 (gfx950)"; }

const char *colbwt_last_error(void) { return g_err.c_str(); }

static int default_layout() {
    const char *e = getenv("COLBWT_LAYOUT");   // override: 1 = one-step, 2 / 3 = K-step rows, 4 = line rows
    if (e && e[0] >= '1' && e[0] <= '6' && e[1] == 0) return e[0] - '0';
    return COLBWT_LAYOUT_DEFAULT_CHOICE;
}

// Own steps K of a line-row open: from the layout argument, else COLBWT_LINE_ROWS_STEPS
// (experiments), else the default.
static int line_rows_steps(int layout_arg) {
    int steps = (layout_arg >> 8) & 0xFF;
    if (steps == 0) {
        steps = kDefaultLineSteps;
        const char *e = getenv("COLBWT_LINE_ROWS_STEPS");
        if (e && e[0] >= '2' && e[0] <= '8' && e[1] == 0) steps = e[0] - '0';
    }
    return steps;
}

int colbwt_index_open_memory(const void *bytes, uint64_t len, const colbwt_widths *widths, int device,
                             colbwt_index **out) {
    return colbwt_index_open_memory_layout(bytes, len, widths, device, COLBWT_LAYOUT_AUTO, out);
}

int colbwt_index_open_memory_layout(const void *bytes, uint64_t len, const colbwt_widths *widths, int device,
                                    int layout, colbwt_index **out) {
    if (!out) return fail(COLBWT_ERR_ARG, "null out");
    const bool automatic = layout == COLBWT_LAYOUT_AUTO;
    if (automatic) layout = default_layout();
    const int steps = line_rows_steps(layout);
    const bool steps_given = ((layout >> 8) & 0xFF) != 0 || getenv("COLBWT_LINE_ROWS_STEPS") != nullptr;
    layout &= 0xFF;
    if (layout < COLBWT_LAYOUT_ONE_STEP || layout > COLBWT_LAYOUT_MISMATCH_LINES_DEEP) return fail(COLBWT_ERR_ARG, "bad layout");
    if (layout >= COLBWT_LAYOUT_LINE_ROWS && !fat_steps_supported(steps))
        return fail(COLBWT_ERR_ARG, "line rows: own steps must be 4..8");
    *out = nullptr;
    if (!widths_ok(widths))
        return fail(COLBWT_ERR_ARG, "only the shipped widths BWT_BYTES=5 RUN_BYTES=4 LEN_BYTES=2 ID_BITS=8 are supported");
    colbwt_index *idx = new (std::nothrow) colbwt_index();
    if (!idx) return fail(COLBWT_ERR_NOMEM, "out of host memory");
    std::string err;
    // AUTO's first choice: mismatch lines, with deep entries when the table leaves room for batches
    const bool deep_if_room = automatic && layout == COLBWT_LAYOUT_MISMATCH_LINES && getenv("COLBWT_LAYOUT") == nullptr;
    int rc = idx->ix.load((const uint8_t *)bytes, len, device, deep_if_room ? kLayoutMismatchLinesAuto : layout, err, steps);
    if (rc == COLBWT_ERR_NOMEM && automatic) {
        // The table does not fit that way (HBM, or more than 2^32-2 refined rows): the ladder of
        // smaller layouts -- line rows at K = 8, 6, 4, three-, two-, one-step rows (the first attempt
        // already went from deep to plain mismatch entries by itself when the deep ones had no room).
        // A line-row build says at which refinement level it gave up (after that level's counting
        // pass, before anything of it was allocated): candidates that have to pass the same level
        // are not tried at all, so an index far too large for line rows costs one counting pass.
        struct Candidate { int layout, steps; };
        static const Candidate ladder[] = {{COLBWT_LAYOUT_MISMATCH_LINES_DEEP, 8}, {COLBWT_LAYOUT_MISMATCH_LINES, 8},   // (deep: only when asked for)
                                           {COLBWT_LAYOUT_LINE_ROWS, 8}, {COLBWT_LAYOUT_LINE_ROWS, 6},
                                           {COLBWT_LAYOUT_LINE_ROWS, 4},      {COLBWT_LAYOUT_THREE_STEP, 0}, {COLBWT_LAYOUT_TWO_STEP, 0},
                                           {COLBWT_LAYOUT_ONE_STEP, 0}};
        int hopeless_from = layout >= COLBWT_LAYOUT_LINE_ROWS ? idx->ix.fat_failed_level() : 0;   // steps >= this cannot be built
        for (const Candidate &c : ladder) {
            if (c.layout > layout || (c.layout == layout && (c.steps >= steps || steps_given))) continue;   // at or above the start
            if (c.layout >= COLBWT_LAYOUT_LINE_ROWS && (steps_given || (hopeless_from && c.steps >= hopeless_from))) continue;
            rc = idx->ix.load((const uint8_t *)bytes, len, device, c.layout, err, c.steps);
            if (rc != COLBWT_ERR_NOMEM) break;
            if (c.layout >= COLBWT_LAYOUT_LINE_ROWS) {
                const int f = idx->ix.fat_failed_level();
                if (f && (!hopeless_from || f < hopeless_from)) hopeless_from = f;
            }
        }
    }
    if (rc != COLBWT_OK) {
        delete idx;
        return fail(rc, err);
    }
    *out = idx;
    return COLBWT_OK;
}

int colbwt_index_open(const char *prefix_or_file, const colbwt_widths *widths, int device, colbwt_index **out) {
    return colbwt_index_open_layout(prefix_or_file, widths, device, COLBWT_LAYOUT_AUTO, out);
}

int colbwt_index_open_layout(const char *prefix_or_file, const colbwt_widths *widths, int device, int layout,
                             colbwt_index **out) {
    if (!prefix_or_file || !out) return fail(COLBWT_ERR_ARG, "null argument");
    *out = nullptr;
    MappedFile mf;
    const int rc = map_index_file(prefix_or_file, mf);
    return rc != COLBWT_OK ? rc : colbwt_index_open_memory_layout(mf.data, mf.len, widths, device, layout, out);
}

// The same table on several devices (the replacement's open takes the devices to
// use): replica k is loaded on devices[k]; every replica ends up with the layout the FIRST one
// got (AUTO falls back on the first device only, so that all replicas answer from the same kind
// of table), a device may be listed more than once (two replicas in one HBM).
int colbwt_index_open_memory_devices(const void *bytes, uint64_t len, const colbwt_widths *widths, const int *devices,
                                     int n_devices, int layout, colbwt_index **out) {
    if (!out) return fail(COLBWT_ERR_ARG, "null out");
    *out = nullptr;
    if (!devices || n_devices < 1 || n_devices > 64) return fail(COLBWT_ERR_ARG, "device list must hold 1 .. 64 devices");
    colbwt_index *first = nullptr;
    int rc = colbwt_index_open_memory_layout(bytes, len, widths, devices[0], layout, &first);
    if (rc != COLBWT_OK) return rc;
    colbwt_info info;
    (void)colbwt_index_info(first, &info);
    const int same = (int)info.layout | (info.layout >= COLBWT_LAYOUT_LINE_ROWS ? (int)(info.layout_shape >> 8) << 8 : 0);
    for (int k = 1; k < n_devices; ++k) {
        colbwt_index *rep = nullptr;
        rc = colbwt_index_open_memory_layout(bytes, len, widths, devices[k], same, &rep);
        if (rc != COLBWT_OK) {
            const std::string msg = "replica on device " + std::to_string(devices[k]) + ": " + g_err;
            delete first;
            return fail(rc, msg);
        }
        first->more.push_back(rep);
    }
    *out = first;
    return COLBWT_OK;
}

int colbwt_index_open_devices(const char *prefix_or_file, const colbwt_widths *widths, const int *devices, int n_devices,
                              int layout, colbwt_index **out) {
    if (!prefix_or_file || !out) return fail(COLBWT_ERR_ARG, "null argument");
    *out = nullptr;
    MappedFile mf;
    const int rc = map_index_file(prefix_or_file, mf);
    return rc != COLBWT_OK ? rc : colbwt_index_open_memory_devices(mf.data, mf.len, widths, devices, n_devices, layout, out);
}

void colbwt_index_close(colbwt_index *idx) { delete idx; }

int colbwt_index_info(const colbwt_index *idx, colbwt_info *out) {
    if (!idx || !out) return fail(COLBWT_ERR_ARG, "null argument");
    out->bwt_r = idx->ix.bwt_r();
    out->n = idx->ix.n();
    out->r = idx->ix.r();
    out->sigma = idx->ix.sigma();
    out->device = (uint32_t)idx->ix.device();
    out->device_bytes = idx->ix.device_bytes() + idx->loc.bytes();
    out->layout = (uint32_t)idx->ix.layout();
    out->layout_shape = idx->ix.line_rows() ? (idx->ix.table_fat().steps << 8) | kFatSlotSteps : 0;
    out->table_rows = idx->ix.table_rows();
    out->n_devices = 1 + (uint32_t)idx->more.size();
    out->tail_permille = idx->ix.line_rows() ? idx->ix.table_fat().tail_permille : 0;
    return COLBWT_OK;
}

int colbwt_query_batch(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads,
                       uint16_t *pml, uint8_t *cid, colbwt_stats *stats) {
    return query_batch_all<uint16_t>(idx, bases, read_off, n_reads, pml, cid, stats);
}

int colbwt_query_batch_u32(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads,
                           uint32_t *pml, uint8_t *cid, colbwt_stats *stats) {
    return query_batch_all<uint32_t>(idx, bases, read_off, n_reads, pml, cid, stats);
}

int colbwt_query_device(colbwt_index *idx, const uint8_t *d_bases, const uint64_t *d_read_off, uint64_t n_reads,
                        uint64_t n_bases, void *d_pml, int pml_bytes, uint8_t *d_cid, void *hip_stream,
                        colbwt_stats *stats) {
    return colbwt_query_device_ordered(idx, d_bases, d_read_off, n_reads, n_bases, d_pml, pml_bytes, d_cid, nullptr,
                                       hip_stream, stats);
}

int colbwt_query_device_ordered(colbwt_index *idx, const uint8_t *d_bases, const uint64_t *d_read_off,
                                uint64_t n_reads, uint64_t n_bases, void *d_pml, int pml_bytes, uint8_t *d_cid,
                                const uint32_t *d_order, void *hip_stream, colbwt_stats *stats) {
    auto bad_argument = [&]() -> const char * {
        if (pml_bytes != 2 && pml_bytes != 4) return "pml_bytes must be 2 or 4";
        if (n_reads == 0) return nullptr;
        if (!d_bases || !d_read_off || !d_pml || !d_cid) return "null device pointer";
        if (((uintptr_t)d_bases & 15) || ((uintptr_t)d_pml & 31) || ((uintptr_t)d_cid & 15))
            return "d_bases/d_cid must be 16-byte aligned and d_pml 32-byte aligned";
        return nullptr;
    };
    return device_entry(idx, d_bases, n_reads, n_bases, hip_stream, kAlgBytesPerBase, stats, bad_argument,
                        [&](const Index &ix, hipStream_t stream) {
                            launch_query(ix, d_bases, d_read_off, n_reads, n_bases, d_pml, pml_bytes, d_cid, d_order, stream);
                        });
}

// pml_query vec mode (pml_query.cpp:92-143) as a three-stage pipeline over batches of reads:
// a reader thread parses the FASTA/FASTQ (kseq semantics; a plain FASTA by several threads),
// the calling thread runs the GPU query (on every replica of the handle), a writer thread lays
// out and writes the two result files -- so the wall time is the slowest stage's, not the sum.
// Output bytes and order are those of the sequential loop.  `binary`: the container of
// bin_writer.h instead of the reference's text.  `count`: count queries (count_query.h) instead,
// one line per read "name\tm\tmlen\tocc\n" in pml_name (cid_name unused).  `locate_k` > 0 (with
// `count`): locate queries (locate_query.h) with max_occ = locate_k, the line followed by
// "\tdoc:offset,doc:offset,..".  `seeds_k` > 0 (with `count`): seeds (seeds_reduce.h) with min_len =
// seeds_min and max_seeds = seeds_k, one line per read as colbwt_seeds_file documents it.  `docs_w` > 0
// (with `count`): docs (docs_query.h) with min_len = docs_min and max_walk = docs_w, one line per read
// and, after the last batch, pml_name + ".tally", as colbwt_docs_file documents them.  `anch_k` > 0 (with
// `count`): anchors (anchors_query.h) with min_len = anch_min, max_anchors = anch_k and max_occ = anch_occ,
// one line per read as colbwt_anchors_file documents it; with `chain` the anchors are reduced on the device
// (chain_reduce.h, band = chain_band) and the lines are those of colbwt_chain_file.
static int query_file_impl(colbwt_index *idx, const char *pattern_path, const std::string &pml_name,
                           const std::string &cid_name, uint64_t batch_bases, colbwt_stats *stats, bool binary,
                           bool count = false, uint32_t locate_k = 0, uint32_t seeds_min = 0, uint32_t seeds_k = 0,
                           uint32_t docs_min = 0, uint32_t docs_w = 0, uint32_t anch_min = 0, uint32_t anch_k = 0,
                           uint32_t anch_occ = 0, bool chain = false, uint32_t chain_band = 0) {
    if (stats) memset(stats, 0, sizeof(*stats));
    const uint32_t docs_n = docs_w ? idx->loc.n_docs() : 0, docs_words = docs_mask_words(docs_n);
    std::vector<uint64_t> docs_tally(2 * (size_t)docs_n, 0), docs_part(2 * (size_t)docs_n, 0);   // doc_reads, then doc_only
    const size_t replicas = 1 + idx->more.size();
    if (batch_bases == 0) batch_bases = (64ull << 20) * replicas;
    ParallelFasta fasta;
    FastxReader reader;
    bool parallel = fasta.open(pattern_path);
    if (!parallel && !reader.open(pattern_path)) return fail(COLBWT_ERR_IO, std::string("cannot open pattern file ") + pattern_path);
    TextWriter wp, wc;
    BinWriter bp, bc;
    FILE *wn = nullptr;
    if (count) {
        wn = fopen(pml_name.c_str(), "wb");
        if (!wn) return fail(COLBWT_ERR_IO, "cannot create " + pml_name);
        setvbuf(wn, nullptr, _IOFBF, 4u << 20);
    } else {
        if (!(binary ? bp.open(pml_name) : wp.open(pml_name))) return fail(COLBWT_ERR_IO, "cannot create " + pml_name);
        if (!(binary ? bc.open(cid_name) : wc.open(cid_name))) return fail(COLBWT_ERR_IO, "cannot create " + cid_name);
    }
    bool count_ok = true;

    FileBatch pool[kFileBatches];
    std::unique_lock<std::mutex> pinned(idx->file_mu, std::defer_lock);
    if (pinned.try_lock())               // the handle's pinned arrays, unless another file query holds them
        for (int k = 0; k < kFileBatches; ++k) {
            pool[k].pml = &idx->file_pml[k];
            pool[k].cid = &idx->file_cid[k];
        }
    BatchQueue free_q, parsed_q, done_q;
    for (auto &b : pool) free_q.push(&b);
    std::atomic<bool> stop{false};   // a later stage failed: the reader stops feeding
    std::atomic<bool> reader_failed{false};
    const bool trace = getenv("COLBWT_TRACE") != nullptr;
    double t_parse = 0, t_gpu = 0, t_format = 0;   // busy seconds of the three stages
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_begin = now();
    const unsigned host_threads = std::min(16u, std::max(2u, std::thread::hardware_concurrency()));

    std::thread reader_thread([&] {
        bool more = true;
        while (more && !stop.load()) {
            FileBatch *b = free_q.pop();
            const double t0 = now();
            b->bases.clear();
            b->names.clear();
            b->off.assign(1, 0);
            uint64_t max_len = 0;
            if (parallel) {
                const ParallelFasta::Result r = fasta.next_batch(batch_bases, host_threads / 2, b->names, b->bases, b->off, max_len);
                if (r == ParallelFasta::kEnd) more = false;
                if (r == ParallelFasta::kNotPlainFasta) {       // FASTQ-style lines ahead: one record at a time from here
                    parallel = false;
                    if (!reader.open_at(pattern_path, fasta.position())) {
                        reader_failed.store(true);
                        more = false;
                    }
                }
            }
            if (!parallel && more) {
                std::string name;
                while (b->bases.size() < batch_bases) {  // pml_query.cpp:74 while (patterns.read())
                    if (!reader.next(name, b->bases)) {
                        more = false;
                        break;
                    }
                    b->names.push_back(name);
                    max_len = std::max<uint64_t>(max_len, b->bases.size() - b->off.back());
                    b->off.push_back(b->bases.size());
                }
            }
            b->wide = max_len > 65535;
            t_parse += now() - t0;
            if (b->names.empty()) {
                free_q.push(b);
                if (more) continue;
                break;
            }
            parsed_q.push(b);
        }
        parsed_q.push(nullptr);
    });

    std::thread writer_thread([&] {
        for (;;) {
            FileBatch *b = done_q.pop();
            if (!b) break;
            const uint64_t n_reads = b->names.size();
            const double t0 = now();
            if (seeds_k) {
                const uint32_t *sm = b->pml->as<uint32_t>();           // 8 words per read
                const uint32_t *sp = b->cid->as<uint32_t>(), *sl = sp + n_reads * seeds_k;
                const uint8_t *sc = (const uint8_t *)(sl + n_reads * seeds_k);
                for (uint64_t k = 0; k < n_reads && count_ok; ++k) {
                    const uint32_t *q = sm + 8 * k;                    // n_seeds max_len cov resets n_col col_cov asc desc
                    count_ok = fprintf(wn, "%s\t%llu\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t", b->names[k].c_str(),
                                       (unsigned long long)(b->off[k + 1] - b->off[k]), q[0], q[2], q[1], q[3], q[4], q[5], q[6],
                                       q[7]) > 0;
                    const uint64_t want = std::min<uint64_t>(q[0], seeds_k);
                    for (uint64_t t = 0; t < want && count_ok; ++t) {
                        const uint64_t at = k * seeds_k + t;
                        count_ok = fprintf(wn, t ? ",%u:%u:%u" : "%u:%u:%u", sp[at], sl[at], (unsigned)sc[at]) > 0;
                    }
                    count_ok = count_ok && fputc('\n', wn) != EOF;
                }
                t_format += now() - t0;
                free_q.push(b);
                continue;
            }
            if (chain) {
                const colbwt_chain *ch = b->pml->as<colbwt_chain>();
                const std::vector<uint64_t> &ds = idx->loc.doc_start;
                for (uint64_t k = 0; k < n_reads && count_ok; ++k) {
                    const colbwt_chain &c = ch[k];
                    count_ok = fprintf(wn, "%s\t%llu\t%u\t%u\t", b->names[k].c_str(), (unsigned long long)(b->off[k + 1] - b->off[k]),
                                       c.read_begin, c.read_end) > 0;
                    if (c.text_begin == COLBWT_LOCATE_NONE) {
                        count_ok = count_ok && fputs("*\t*", wn) != EOF;
                    } else {
                        const size_t d = (size_t)(std::upper_bound(ds.begin(), ds.end(), c.text_begin) - ds.begin()) - 1;
                        count_ok = count_ok && fprintf(wn, "%zu\t%llu", d, (unsigned long long)(c.text_begin - ds[d])) > 0;
                    }
                    count_ok = count_ok && fprintf(wn, "\t%u\t%u\t%u\t%u\t%u\n", c.text_len, c.score, c.score2, (unsigned)c.n_chained,
                                                   (unsigned)c.n_hits) > 0;
                }
                t_format += now() - t0;
                free_q.push(b);
                continue;
            }
            if (anch_k) {
                const uint32_t *sm = b->pml->as<uint32_t>();           // 8 words per read
                const uint32_t *as = sm + 8 * n_reads, *al = as + n_reads * anch_k;
                const uint64_t *ao = b->cid->as<uint64_t>(), *ap = ao + n_reads * anch_k;
                const std::vector<uint64_t> &ds = idx->loc.doc_start;
                for (uint64_t k = 0; k < n_reads && count_ok; ++k) {
                    const uint32_t *q = sm + 8 * k;                    // n_factors max_len skipped n_kept cov n_unique cov_unique n_stored
                    count_ok = fprintf(wn, "%s\t%llu\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t", b->names[k].c_str(),
                                       (unsigned long long)(b->off[k + 1] - b->off[k]), q[0], q[3], q[4], q[1], q[2], q[5], q[6]) > 0;
                    for (uint64_t t = 0; t < q[7] && count_ok; ++t) {
                        const uint64_t at = k * anch_k + t;
                        count_ok = fprintf(wn, t ? ",%u:%u:%llu" : "%u:%u:%llu", as[at], al[at], (unsigned long long)ao[at]) > 0;
                        const uint64_t want = std::min<uint64_t>(ao[at], anch_occ);
                        for (uint64_t w = 0; w < want && count_ok; ++w) {
                            const uint64_t x = ap[at * anch_occ + w];
                            const size_t d = (size_t)(std::upper_bound(ds.begin(), ds.end(), x) - ds.begin()) - 1;
                            count_ok = fprintf(wn, "@%zu:%llu", d, (unsigned long long)(x - ds[d])) > 0;
                        }
                    }
                    count_ok = count_ok && fputc('\n', wn) != EOF;
                }
                t_format += now() - t0;
                free_q.push(b);
                continue;
            }
            if (docs_w) {
                const uint32_t *ml = b->pml->as<uint32_t>(), *nh = ml + n_reads;
                const uint64_t *oc = b->cid->as<uint64_t>(), *mk = oc + n_reads;   // docs_words mask words per read
                for (uint64_t k = 0; k < n_reads && count_ok; ++k) {
                    count_ok = fprintf(wn, "%s\t%llu\t%u\t%llu\t%u\t", b->names[k].c_str(),
                                       (unsigned long long)(b->off[k + 1] - b->off[k]), ml[k], (unsigned long long)oc[k], nh[k]) > 0;
                    bool first = true;
                    for (uint32_t wi = 0; wi < docs_words && count_ok; ++wi)
                        for (uint64_t m = mk[k * docs_words + wi]; m && count_ok; m &= m - 1, first = false)
                            count_ok = fprintf(wn, first ? "%u" : ",%u", wi * 64u + (uint32_t)__builtin_ctzll(m)) > 0;
                    count_ok = count_ok && fputc('\n', wn) != EOF;
                }
                t_format += now() - t0;
                free_q.push(b);
                continue;
            }
            if (count) {
                const uint32_t *ml = b->pml->as<uint32_t>();
                const uint64_t *oc = b->cid->as<uint64_t>();
                const uint64_t *ps = oc + n_reads;          // locate: locate_k positions per read
                const std::vector<uint64_t> &ds = idx->loc.doc_start;
                for (uint64_t k = 0; k < n_reads && count_ok; ++k) {
                    count_ok = fprintf(wn, locate_k ? "%s\t%llu\t%u\t%llu\t" : "%s\t%llu\t%u\t%llu\n", b->names[k].c_str(),
                                       (unsigned long long)(b->off[k + 1] - b->off[k]), ml[k], (unsigned long long)oc[k]) > 0;
                    if (!locate_k) continue;
                    const uint64_t want = std::min<uint64_t>(oc[k], locate_k);
                    for (uint64_t t = 0; t < want && count_ok; ++t) {
                        const uint64_t x = ps[k * locate_k + t];
                        const size_t d = (size_t)(std::upper_bound(ds.begin(), ds.end(), x) - ds.begin()) - 1;
                        count_ok = fprintf(wn, t ? ",%zu:%llu" : "%zu:%llu", d, (unsigned long long)(x - ds[d])) > 0;
                    }
                    count_ok = count_ok && fputc('\n', wn) != EOF;
                }
                t_format += now() - t0;
                free_q.push(b);
                continue;
            }
            // pml_query.cpp:78-85; the two files are laid out side by side, each by several
            // host threads (same bytes, same order as the sequential loop)
            std::thread cid_thread([&] {
                if (binary) bc.batch<uint8_t>(b->names, b->off.data(), b->cid->as<uint8_t>(), n_reads, host_threads / 2);
                else wc.batch(b->names, b->off.data(), b->cid->as<uint8_t>(), n_reads, host_threads / 2);
            });
            if (binary) {
                if (b->wide) bp.batch<uint16_t>(b->names, b->off.data(), b->pml->as<uint32_t>(), n_reads, host_threads / 2);
                else bp.batch<uint16_t>(b->names, b->off.data(), b->pml->as<uint16_t>(), n_reads, host_threads / 2);
            } else {
                if (b->wide) wp.batch(b->names, b->off.data(), b->pml->as<uint32_t>(), n_reads, host_threads / 2);
                else wp.batch(b->names, b->off.data(), b->pml->as<uint16_t>(), n_reads, host_threads / 2);
            }
            cid_thread.join();
            t_format += now() - t0;
            free_q.push(b);
        }
    });

    int rc = COLBWT_OK;
    for (;;) {
        FileBatch *b = parsed_q.pop();
        if (!b) break;
        if (rc != COLBWT_OK) {           // keep draining so the reader can finish
            free_q.push(b);
            continue;
        }
        const uint64_t n_reads = b->names.size();
        const uint64_t nb = b->bases.size();
        const double t0 = now();
        colbwt_stats st{};
        rc = select_device(idx->ix.device(), g_err);
        if (rc == COLBWT_OK && seeds_k && (!b->pml->ensure(n_reads * 32) || !b->cid->ensure(n_reads * 9 * (uint64_t)seeds_k)))
            rc = fail(COLBWT_ERR_NOMEM, "cannot pin host memory for a batch of results");
        if (rc == COLBWT_OK && docs_w && (!b->pml->ensure(n_reads * 8) || !b->cid->ensure(n_reads * 8 * (1 + (uint64_t)docs_words))))
            rc = fail(COLBWT_ERR_NOMEM, "cannot pin host memory for a batch of results");
        if (rc == COLBWT_OK && chain && !b->pml->ensure(n_reads * sizeof(colbwt_chain)))
            rc = fail(COLBWT_ERR_NOMEM, "cannot pin host memory for a batch of results");
        if (rc == COLBWT_OK && anch_k && !chain &&
            (!b->pml->ensure(n_reads * (32 + 8 * (uint64_t)anch_k)) || !b->cid->ensure(n_reads * anch_k * 8 * (1 + (uint64_t)anch_occ))))
            rc = fail(COLBWT_ERR_NOMEM, "cannot pin host memory for a batch of results");
        if (rc == COLBWT_OK && count && !seeds_k && !docs_w && !anch_k && (!b->pml->ensure(n_reads * 4) || !b->cid->ensure(n_reads * 8 * (1 + (uint64_t)locate_k))))
            rc = fail(COLBWT_ERR_NOMEM, "cannot pin host memory for a batch of results");
        if (rc == COLBWT_OK && !count && (!b->cid->ensure(nb) || !b->pml->ensure(nb * (b->wide ? 4 : 2))))
            rc = fail(COLBWT_ERR_NOMEM, "cannot pin host memory for a batch of results");
        if (rc != COLBWT_OK) {
        } else if (seeds_k) {
            uint32_t *sp = b->cid->as<uint32_t>(), *sl = sp + n_reads * seeds_k;
            rc = seeds_batch_all(idx, b->bases.data(), b->off.data(), n_reads, seeds_min, seeds_k, b->pml->as<uint32_t>(), sp, sl,
                                 (uint8_t *)(sl + n_reads * seeds_k), &st);
        } else if (chain) {
            rc = chain_batch_all(idx, b->bases.data(), b->off.data(), n_reads, anch_min, anch_k, anch_occ, chain_band,
                                 b->pml->as<colbwt_chain>(), &st);
        } else if (anch_k) {
            uint32_t *as = b->pml->as<uint32_t>() + 8 * n_reads;
            uint64_t *ao = b->cid->as<uint64_t>();
            rc = anchors_batch_all(idx, b->bases.data(), b->off.data(), n_reads, anch_min, anch_k, anch_occ,
                                   b->pml->as<colbwt_anchor_summary>(), as, as + n_reads * anch_k, ao,
                                   anch_occ ? ao + n_reads * anch_k : nullptr, &st);
        } else if (docs_w) {
            rc = docs_batch_all(idx, b->bases.data(), b->off.data(), n_reads, docs_min, docs_w, b->pml->as<uint32_t>(),
                                b->cid->as<uint64_t>(), b->pml->as<uint32_t>() + n_reads, b->cid->as<uint64_t>() + n_reads,
                                docs_part.data(), docs_part.data() + docs_n, &st);
            for (size_t d = 0; rc == COLBWT_OK && d < docs_tally.size(); ++d) docs_tally[d] += docs_part[d];
        } else if (locate_k) {
            rc = locate_batch_all(idx, b->bases.data(), b->off.data(), n_reads, locate_k, b->pml->as<uint32_t>(), b->cid->as<uint64_t>(),
                                  b->cid->as<uint64_t>() + n_reads, &st);
        } else if (count) {
            rc = count_batch_all(idx, b->bases.data(), b->off.data(), n_reads, b->pml->as<uint32_t>(), b->cid->as<uint64_t>(),
                                 nullptr, &st);
        } else if (b->wide) {
            rc = colbwt_query_batch_u32(idx, b->bases.data(), b->off.data(), n_reads, b->pml->as<uint32_t>(),
                                        b->cid->as<uint8_t>(), &st);
        } else {
            rc = colbwt_query_batch(idx, b->bases.data(), b->off.data(), n_reads, b->pml->as<uint16_t>(),
                                    b->cid->as<uint8_t>(), &st);
        }
        t_gpu += now() - t0;
        if (rc != COLBWT_OK) {
            stop.store(true);
            free_q.push(b);
            continue;
        }
        if (stats) {
            stats->n_reads += st.n_reads;
            stats->n_bases += st.n_bases;
            stats->h2d_ms += st.h2d_ms;
            stats->kernel_ms += st.kernel_ms;
            stats->d2h_ms += st.d2h_ms;
            stats->algorithmic_bytes += st.algorithmic_bytes;
        }
        done_q.push(b);
    }
    done_q.push(nullptr);
    reader_thread.join();
    writer_thread.join();
    const bool okp = count ? fclose(wn) == 0 && count_ok : binary ? bp.close() : wp.close();
    const bool okc = count || (binary ? bc.close() : wc.close());
    if (trace)
        fprintf(stderr, "colbwt_query_file: wall %.3f s; busy: parse %.3f, gpu %.3f, layout+write %.3f\n",
                now() - t_begin, t_parse, t_gpu, t_format);
    if (rc != COLBWT_OK) return rc;     // message set by the failing call on this thread
    if (reader_failed.load()) return fail(COLBWT_ERR_IO, std::string("cannot re-open pattern file ") + pattern_path);
    if (!okp || !okc) return fail(COLBWT_ERR_IO, "short write on " + pml_name + " / " + cid_name);
    if (docs_w) {
        const std::string tally_name = pml_name + ".tally";
        FILE *wt = fopen(tally_name.c_str(), "wb");
        if (!wt) return fail(COLBWT_ERR_IO, "cannot create " + tally_name);
        bool ok = true;
        for (uint32_t d = 0; d < docs_n && ok; ++d)
            ok = fprintf(wt, "%u\t%llu\t%llu\n", d, (unsigned long long)docs_tally[d], (unsigned long long)docs_tally[docs_n + d]) > 0;
        if (fclose(wt) != 0 || !ok) return fail(COLBWT_ERR_IO, "short write on " + tally_name);
    }
    return COLBWT_OK;
}

int colbwt_query_file(colbwt_index *idx, const char *pattern_path, const char *pml_path, const char *cid_path,
                      uint64_t batch_bases, colbwt_stats *stats) {
    if (!idx || !pattern_path) return fail(COLBWT_ERR_ARG, "null argument");
    // pml_query.cpp:124-125
    return query_file_impl(idx, pattern_path, pml_path ? pml_path : std::string(pattern_path) + ".pml",
                           cid_path ? cid_path : std::string(pattern_path) + ".cid", batch_bases, stats, false);
}

int colbwt_query_file_binary(colbwt_index *idx, const char *pattern_path, const char *pml_bin_path, const char *cid_bin_path,
                             uint64_t batch_bases, colbwt_stats *stats) {
    if (!idx || !pattern_path) return fail(COLBWT_ERR_ARG, "null argument");
    return query_file_impl(idx, pattern_path, pml_bin_path ? pml_bin_path : std::string(pattern_path) + ".pml.bin",
                           cid_bin_path ? cid_bin_path : std::string(pattern_path) + ".cid.bin", batch_bases, stats, true);
}

int colbwt_count_batch(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, uint32_t *mlen,
                       uint64_t *occ, uint64_t *sp, colbwt_stats *stats) {
    return count_batch_all(idx, bases, read_off, n_reads, mlen, occ, sp, stats);
}

int colbwt_count_device(colbwt_index *idx, const uint8_t *d_bases, const uint64_t *d_read_off, uint64_t n_reads,
                        uint64_t n_bases, uint32_t *d_mlen, uint64_t *d_occ, uint64_t *d_sp, const uint32_t *d_order,
                        void *hip_stream, colbwt_stats *stats) {
    auto bad_argument = [&]() -> const char * {
        if (n_reads == 0) return nullptr;
        if (!d_bases || !d_read_off || !d_mlen || !d_occ) return "null device pointer";
        if (((uintptr_t)d_bases & 15) || ((uintptr_t)d_mlen & 3) || ((uintptr_t)d_occ & 7) || ((uintptr_t)d_sp & 7))
            return "d_bases must be 16-byte aligned, d_mlen 4-byte and d_occ/d_sp 8-byte aligned";
        return nullptr;
    };
    return device_entry(idx, d_bases, n_reads, n_bases, hip_stream, 0, stats, bad_argument,
                        [&](const Index &ix, hipStream_t stream) {
                            launch_count(ix, d_bases, d_read_off, n_reads, d_mlen, d_occ, d_sp, d_order, stream);
                        });
}

int colbwt_count_file(colbwt_index *idx, const char *pattern_path, const char *out_path, uint64_t batch_bases,
                      colbwt_stats *stats) {
    if (!idx || !pattern_path) return fail(COLBWT_ERR_ARG, "null argument");
    const std::string out = out_path ? out_path : std::string(pattern_path) + ".count";
    return query_file_impl(idx, pattern_path, out, out, batch_bases, stats, false, true);
}

int colbwt_seeds_batch(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, uint32_t min_len,
                       uint32_t max_seeds, colbwt_seed_summary *summary, uint32_t *seed_pos, uint32_t *seed_len, uint8_t *seed_cid,
                       colbwt_stats *stats) {
    return seeds_batch_all(idx, bases, read_off, n_reads, min_len, max_seeds, (uint32_t *)summary, seed_pos, seed_len, seed_cid,
                           stats);
}

int colbwt_seeds_reduce_device(const void *d_pml, int pml_bytes, const uint8_t *d_cid, const uint64_t *d_read_off, uint64_t n_reads,
                               uint64_t n_bases, uint32_t min_len, uint32_t max_seeds, colbwt_seed_summary *d_summary,
                               uint32_t *d_seed_pos, uint32_t *d_seed_len, uint8_t *d_seed_cid, void *hip_stream,
                               colbwt_stats *stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    if (pml_bytes != 2 && pml_bytes != 4) return fail(COLBWT_ERR_ARG, "pml_bytes must be 2 or 4");
    if (const char *m = seeds_bad_params(min_len, max_seeds)) return fail(COLBWT_ERR_ARG, m);
    if (n_reads >= 0xFFFFFFFFull) return fail(COLBWT_ERR_ARG, kTooManyReads);
    if ((d_seed_pos != nullptr) != (d_seed_len != nullptr) || (d_seed_pos != nullptr) != (d_seed_cid != nullptr))
        return fail(COLBWT_ERR_ARG, "d_seed_pos/d_seed_len/d_seed_cid: all three or none");
    if (n_reads == 0) return COLBWT_OK;
    if (!d_read_off || !d_summary || (n_bases && (!d_pml || !d_cid))) return fail(COLBWT_ERR_ARG, "null device pointer");
    if (((uintptr_t)d_pml & 15) || ((uintptr_t)d_cid & 7) || ((uintptr_t)d_summary & 15) || ((uintptr_t)d_seed_pos & 3) ||
        ((uintptr_t)d_seed_len & 3))
        return fail(COLBWT_ERR_ARG, "d_pml/d_summary must be 16-byte aligned, d_cid 8-byte, d_seed_pos/d_seed_len 4-byte");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
        (void)hipGetLastError();
        return fail(COLBWT_ERR_NO_DEVICE, "no HIP device available (the query path has no CPU fallback)");
    }
    const hipStream_t stream = (hipStream_t)hip_stream;
    struct Events {
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Events() {
            for (hipEvent_t x : e)
                if (x) (void)hipEventDestroy(x);
        }
    } ev;
    if (stats) {
        TRY_HIP(hipEventCreate(&ev.e[0]), nullptr, g_err);
        TRY_HIP(hipEventCreate(&ev.e[1]), nullptr, g_err);
        TRY_HIP(hipEventRecord(ev.e[0], stream), nullptr, g_err);
    }
    TRY_HIP(launch_seeds_reduce(d_pml, pml_bytes, d_cid, d_read_off, n_reads, n_bases, min_len, max_seeds, (uint32_t *)d_summary,
                                d_seed_pos, d_seed_len, d_seed_cid, stream),
            nullptr, g_err);
    TRY_HIP(hipGetLastError(), nullptr, g_err);
    if (stats) {
        float ms = 0;
        TRY_HIP(hipEventRecord(ev.e[1], stream), nullptr, g_err);
        TRY_HIP(hipEventSynchronize(ev.e[1]), nullptr, g_err);
        TRY_HIP(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]), nullptr, g_err);
        stats->n_reads = n_reads;
        stats->n_bases = n_bases;
        stats->kernel_ms = ms;
    }
    return COLBWT_OK;
}

int colbwt_seeds_file(colbwt_index *idx, const char *pattern_path, const char *out_path, uint32_t min_len, uint32_t max_seeds,
                      uint64_t batch_bases, colbwt_stats *stats) {
    if (!idx || !pattern_path) return fail(COLBWT_ERR_ARG, "null argument");
    if (const char *m = seeds_bad_params(min_len, max_seeds)) return fail(COLBWT_ERR_ARG, m);
    const std::string out = out_path ? out_path : std::string(pattern_path) + ".seeds";
    if (batch_bases == 0)   // the default batch of the file query, cut so that max_seeds slots per read stay ~tens of MB
        batch_bases = std::max<uint64_t>(1ull << 20, (64ull << 20) * (1 + idx->more.size()) * 16 / std::max<uint32_t>(16, max_seeds));
    return query_file_impl(idx, pattern_path, out, out, batch_bases, stats, false, true, 0, min_len, max_seeds);
}

int colbwt_index_attach_locate_memory(colbwt_index *idx, const void *col_loc_bytes, uint64_t len) {
    if (!idx || !col_loc_bytes) return fail(COLBWT_ERR_ARG, "null argument");
    const uint8_t *p = (const uint8_t *)col_loc_bytes;
    std::vector<uint32_t> aligned_copy;          // the u32 arrays are read in place
    if ((uintptr_t)p & 3) {
        aligned_copy.resize((len + 3) / 4);
        memcpy(aligned_copy.data(), p, len);
        p = (const uint8_t *)aligned_copy.data();
    }
    LocFile f;
    std::string msg;
    int rc = parse_loc(p, len, idx->ix, f, msg);
    if (rc != COLBWT_OK) return fail(rc, msg);
    std::vector<colbwt_index *> reps{idx};
    reps.insert(reps.end(), idx->more.begin(), idx->more.end());
    for (colbwt_index *rep : reps) {
        rc = attach_one(rep, f, msg);
        if (rc != COLBWT_OK) {
            if (reps.size() > 1) msg = "device " + std::to_string(rep->ix.device()) + ": " + msg;
            for (colbwt_index *x : reps) {   // all replicas or none
                if (select_device(x->ix.device(), g_err) == COLBWT_OK) x->loc.reset();
            }
            return fail(rc, msg);
        }
    }
    return COLBWT_OK;
}

int colbwt_index_attach_locate(colbwt_index *idx, const char *prefix_or_file) {
    if (!idx || !prefix_or_file) return fail(COLBWT_ERR_ARG, "null argument");
    MappedFile mf;
    if (!mf.open(std::string(prefix_or_file) + ".col_loc") && !mf.open(prefix_or_file))
        return fail(COLBWT_ERR_IO, std::string("cannot open ") + prefix_or_file + ".col_loc (or " + prefix_or_file + ")");
    if (!mf.data) return fail(COLBWT_ERR_FORMAT, "empty .col_loc file");
    return colbwt_index_attach_locate_memory(idx, mf.data, mf.len);
}

int colbwt_locate_docs(const colbwt_index *idx, uint64_t *doc_start, uint32_t cap, uint32_t *n_docs) {
    if (!idx || !n_docs) return fail(COLBWT_ERR_ARG, "null argument");
    if (!idx->loc.ready()) return fail(COLBWT_ERR_ARG, kNoSamples);
    const std::vector<uint64_t> &ds = idx->loc.doc_start;
    *n_docs = (uint32_t)ds.size();
    if (!doc_start || cap < ds.size()) return fail(COLBWT_ERR_ARG, "doc_start holds fewer than n_docs entries");
    std::copy(ds.begin(), ds.end(), doc_start);
    return COLBWT_OK;
}

int colbwt_locate_batch(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, uint32_t max_occ,
                        uint32_t *mlen, uint64_t *occ, uint64_t *pos, colbwt_stats *stats) {
    return locate_batch_all(idx, bases, read_off, n_reads, max_occ, mlen, occ, pos, stats);
}

int colbwt_locate_device(colbwt_index *idx, const uint8_t *d_bases, const uint64_t *d_read_off, uint64_t n_reads,
                         uint64_t n_bases, uint32_t max_occ, uint32_t *d_mlen, uint64_t *d_occ, uint64_t *d_pos,
                         const uint32_t *d_order, void *hip_stream, colbwt_stats *stats) {
    auto bad_argument = [&]() -> const char * {
        if (max_occ == 0 || max_occ > kLocateMaxOcc) return "max_occ must be 1 .. 2^20";
        if (const char *m = samples_missing(idx)) return m;
        if (n_reads == 0) return nullptr;
        if (!d_bases || !d_read_off || !d_mlen || !d_occ || !d_pos) return "null device pointer";
        if (((uintptr_t)d_bases & 15) || ((uintptr_t)d_mlen & 3) || ((uintptr_t)d_occ & 7) || ((uintptr_t)d_pos & 7))
            return "d_bases must be 16-byte aligned, d_mlen 4-byte and d_occ/d_pos 8-byte aligned";
        return nullptr;
    };
    return device_entry(idx, d_bases, n_reads, n_bases, hip_stream, 0, stats, bad_argument,
                        [&](const Index &ix, hipStream_t stream) {
                            const LocateTables &L = replica_for(idx, d_bases)->loc;
                            launch_locate(ix, L.toe_row.as<uint32_t>(), L.phi(), d_bases, d_read_off, n_reads, max_occ, d_mlen,
                                          d_occ, d_pos, d_order, stream);
                        });
}

int colbwt_locate_file(colbwt_index *idx, const char *pattern_path, const char *out_path, uint32_t max_occ,
                       uint64_t batch_bases, colbwt_stats *stats) {
    if (!idx || !pattern_path) return fail(COLBWT_ERR_ARG, "null argument");
    if (max_occ == 0 || max_occ > kLocateMaxOcc) return fail(COLBWT_ERR_ARG, "max_occ must be 1 .. 2^20");
    if (!idx->loc.ready()) return fail(COLBWT_ERR_ARG, kNoSamples);
    const std::string out = out_path ? out_path : std::string(pattern_path) + ".locate";
    if (batch_bases == 0)   // the default batch of the file query, cut so that max_occ slots per read stay ~tens of MB
        batch_bases = std::max<uint64_t>(1ull << 20, (64ull << 20) * (1 + idx->more.size()) * 16 / std::max<uint32_t>(16, max_occ));
    return query_file_impl(idx, pattern_path, out, out, batch_bases, stats, false, true, max_occ);
}

int colbwt_anchors_batch(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, uint32_t min_len,
                         uint32_t max_anchors, uint32_t max_occ, colbwt_anchor_summary *summary, uint32_t *anchor_start,
                         uint32_t *anchor_len, uint64_t *anchor_occ, uint64_t *anchor_pos, colbwt_stats *stats) {
    return anchors_batch_all(idx, bases, read_off, n_reads, min_len, max_anchors, max_occ, summary, anchor_start, anchor_len,
                             anchor_occ, anchor_pos, stats);
}

int colbwt_anchors_device(colbwt_index *idx, const uint8_t *d_bases, const uint64_t *d_read_off, uint64_t n_reads, uint64_t n_bases,
                          uint32_t min_len, uint32_t max_anchors, uint32_t max_occ, colbwt_anchor_summary *d_summary,
                          uint32_t *d_start, uint32_t *d_len, uint64_t *d_occ, uint64_t *d_pos, const uint32_t *d_order,
                          void *hip_stream, colbwt_stats *stats) {
    auto bad_argument = [&]() -> const char * {
        if (const char *m = anchors_bad_setup(idx, min_len, max_anchors, max_occ, d_start, d_len, d_occ, d_pos)) return m;
        if (n_reads >= 0xFFFFFFFFull) return kTooManyReads;
        if (n_reads == 0) return nullptr;
        if (!d_bases || !d_read_off || !d_summary) return "null device pointer";
        if (((uintptr_t)d_bases & 15) || ((uintptr_t)d_summary & 15) || ((uintptr_t)d_start & 3) || ((uintptr_t)d_len & 3) ||
            ((uintptr_t)d_occ & 7) || ((uintptr_t)d_pos & 7))
            return "d_bases/d_summary must be 16-byte aligned, d_start/d_len 4-byte and d_occ/d_pos 8-byte aligned";
        return nullptr;
    };
    return device_entry(idx, d_bases, n_reads, n_bases, hip_stream, 0, stats, bad_argument,
                        [&](const Index &ix, hipStream_t stream) {
                            launch_anchors(ix,
                                           anchors_args(replica_for(idx, d_bases), min_len, max_anchors, max_occ, d_summary, d_start,
                                                        d_len, d_occ, d_pos),
                                           d_bases, d_read_off, n_reads, d_order, stream);
                        });
}

int colbwt_anchors_file(colbwt_index *idx, const char *pattern_path, const char *out_path, uint32_t min_len, uint32_t max_anchors,
                        uint32_t max_occ, uint64_t batch_bases, colbwt_stats *stats) {
    if (!idx || !pattern_path) return fail(COLBWT_ERR_ARG, "null argument");
    if (const char *m = anchors_bad_params(min_len, max_anchors, max_occ)) return fail(COLBWT_ERR_ARG, m);
    if (max_occ > 0 && !idx->loc.ready()) return fail(COLBWT_ERR_ARG, kNoSamples);
    const std::string out = out_path ? out_path : std::string(pattern_path) + ".anchors";
    if (batch_bases == 0) {   // the default batch of the file query, cut by the slot bytes per read as locate cuts it by max_occ
        const uint64_t slot_bytes = (uint64_t)max_anchors * (16 + 8 * (uint64_t)max_occ);
        batch_bases = std::max<uint64_t>(1ull << 20, (64ull << 20) * (1 + idx->more.size()) * 128 / std::max<uint64_t>(128, slot_bytes));
    }
    return query_file_impl(idx, pattern_path, out, out, batch_bases, stats, false, true, 0, 0, 0, 0, 0, min_len, max_anchors, max_occ);
}

uint64_t colbwt_chain_work_bytes(uint64_t n_reads, uint32_t max_anchors, uint32_t max_occ) {
    return chain_work_bytes(n_reads, max_anchors, max_occ);
}

int colbwt_chain_reduce_device(colbwt_index *idx, const uint32_t *d_start, const uint32_t *d_len, const uint64_t *d_pos,
                               uint64_t n_reads, uint32_t max_anchors, uint32_t max_occ, uint32_t band, colbwt_chain *d_chain,
                               void *hip_stream, colbwt_stats *stats) {
    auto bad_argument = [&]() -> const char * {
        if (const char *m = chain_bad_setup(idx, max_anchors, max_occ)) return m;
        if (n_reads >= 0xFFFFFFFFull) return kTooManyReads;
        if (n_reads == 0) return nullptr;
        if (!d_start || !d_len || !d_pos || !d_chain) return "null device pointer";
        if (((uintptr_t)d_start & 3) || ((uintptr_t)d_len & 3) || ((uintptr_t)d_pos & 7) || ((uintptr_t)d_chain & 15))
            return "d_start/d_len must be 4-byte aligned, d_pos 8-byte and d_chain 16-byte aligned";
        return nullptr;
    };
    hipError_t launched = hipSuccess;
    const int rc = device_entry(idx, d_pos, n_reads, 0, hip_stream, 0, stats, bad_argument, [&](const Index &, hipStream_t stream) {
        launched = launch_chain(chain_args(replica_for(idx, d_pos), d_start, d_len, d_pos, max_anchors, max_occ, band, d_chain), n_reads,
                                stream);
    });
    if (rc == COLBWT_OK && launched != hipSuccess) return hip_failed(launched, "colbwt_chain_reduce_device", nullptr, g_err);
    return rc;
}

int colbwt_chain_device(colbwt_index *idx, const uint8_t *d_bases, const uint64_t *d_read_off, uint64_t n_reads, uint64_t n_bases,
                        uint32_t min_len, uint32_t max_anchors, uint32_t max_occ, uint32_t band, colbwt_chain *d_chain, void *d_work,
                        const uint32_t *d_order, void *hip_stream, colbwt_stats *stats) {
    auto bad_argument = [&]() -> const char * {
        if (min_len == 0) return "min_len must be at least 1";
        if (const char *m = chain_bad_setup(idx, max_anchors, max_occ)) return m;
        if (n_reads >= 0xFFFFFFFFull) return kTooManyReads;
        if (n_reads == 0) return nullptr;
        if (!d_bases || !d_read_off || !d_chain || !d_work) return "null device pointer";
        if (((uintptr_t)d_bases & 15) || ((uintptr_t)d_chain & 15)) return "d_bases/d_chain must be 16-byte aligned";
        if ((uintptr_t)d_work & 255) return "d_work must be 256-byte aligned";
        return nullptr;
    };
    hipError_t launched = hipSuccess;
    const int rc = device_entry(idx, d_bases, n_reads, n_bases, hip_stream, 0, stats, bad_argument, [&](const Index &, hipStream_t stream) {
        launched = launch_chain_of_reads(replica_for(idx, d_bases), d_bases, d_read_off, n_reads, min_len, max_anchors, max_occ, band,
                                         d_chain, d_work, d_order, stream);
    });
    if (rc == COLBWT_OK && launched != hipSuccess) return hip_failed(launched, "colbwt_chain_device", nullptr, g_err);
    return rc;
}

int colbwt_chain_batch(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, uint32_t min_len,
                       uint32_t max_anchors, uint32_t max_occ, uint32_t band, colbwt_chain *chain, colbwt_stats *stats) {
    return chain_batch_all(idx, bases, read_off, n_reads, min_len, max_anchors, max_occ, band, chain, stats);
}

int colbwt_chain_file(colbwt_index *idx, const char *pattern_path, const char *out_path, uint32_t min_len, uint32_t max_anchors,
                      uint32_t max_occ, uint32_t band, uint64_t batch_bases, colbwt_stats *stats) {
    if (!idx || !pattern_path) return fail(COLBWT_ERR_ARG, "null argument");
    if (min_len == 0) return fail(COLBWT_ERR_ARG, "min_len must be at least 1");
    if (const char *m = chain_bad_setup(idx, max_anchors, max_occ)) return fail(COLBWT_ERR_ARG, m);
    const std::string out = out_path ? out_path : std::string(pattern_path) + ".chains";
    if (batch_bases == 0) {   // colbwt_anchors_file's default: the slot bytes per read stay in HBM but still set the scratch
        const uint64_t slot_bytes = (uint64_t)max_anchors * (16 + 8 * (uint64_t)max_occ);
        batch_bases = std::max<uint64_t>(1ull << 20, (64ull << 20) * (1 + idx->more.size()) * 128 / std::max<uint64_t>(128, slot_bytes));
    }
    return query_file_impl(idx, pattern_path, out, out, batch_bases, stats, false, true, 0, 0, 0, 0, 0, min_len, max_anchors, max_occ, true,
                           band);
}

uint32_t colbwt_locate_all_tile(void) { return kLocAllTile; }

uint64_t colbwt_locate_all_work_bytes(uint64_t n_reads) { return locate_all_work_bytes(n_reads); }

int colbwt_locate_all_plan_device(colbwt_index *idx, const uint8_t *d_bases, const uint64_t *d_read_off, uint64_t n_reads,
                                  uint64_t n_bases, uint32_t min_len, uint64_t max_per_read, uint32_t *d_mlen, uint64_t *d_occ,
                                  uint64_t *d_pos_off, void *d_work, const uint32_t *d_order, void *hip_stream, uint64_t *total,
                                  colbwt_stats *stats) {
    auto bad_argument = [&]() -> const char * {
        if (min_len == 0) return "min_len must be at least 1";
        if (const char *m = samples_missing(idx)) return m;
        if (n_reads == 0) return nullptr;
        if (!d_bases || !d_read_off || !d_mlen || !d_occ) return "null device pointer";
        if (((uintptr_t)d_bases & 15) || ((uintptr_t)d_mlen & 3) || ((uintptr_t)d_occ & 7))
            return "d_bases must be 16-byte aligned, d_mlen 4-byte and d_occ 8-byte aligned";
        if (n_reads >= 0xFFFFFFFFull) return kTooManyReads;
        if (!d_pos_off || !d_work) return "null d_pos_off/d_work";
        if ((uintptr_t)d_pos_off & 7) return "d_pos_off must be 8-byte aligned";
        if ((uintptr_t)d_work & 255) return "d_work must be 256-byte aligned";
        return nullptr;
    };
    hipError_t launched = hipSuccess;
    const int rc = device_entry(idx, d_bases, n_reads, n_bases, hip_stream, 0, stats, bad_argument,
                                [&](const Index &ix, hipStream_t stream) {
                                    const LocateTables &L = replica_for(idx, d_bases)->loc;
                                    launched = launch_locate_all_plan(ix, L.all(), d_bases, d_read_off, n_reads, min_len, max_per_read,
                                                                      d_mlen, d_occ, d_pos_off, d_work, d_order, stream);
                                });
    if (rc != COLBWT_OK) return rc;
    if (launched != hipSuccess) return hip_failed(launched, "colbwt_locate_all_plan_device", nullptr, g_err);
    const hipStream_t stream = (hipStream_t)hip_stream;
    if (n_reads == 0) {                     // no reads: the offsets are the single 0
        if (d_pos_off) TRY_HIP(hipMemsetAsync(d_pos_off, 0, sizeof(uint64_t), stream), nullptr, g_err);
        if (total) {
            *total = 0;
            TRY_HIP(hipStreamSynchronize(stream), nullptr, g_err);
        }
        return COLBWT_OK;
    }
    if (total) {
        TRY_HIP(hipMemcpyAsync(total, d_pos_off + n_reads, sizeof(uint64_t), hipMemcpyDeviceToHost, stream), nullptr, g_err);
        TRY_HIP(hipStreamSynchronize(stream), nullptr, g_err);
    }
    return COLBWT_OK;
}

int colbwt_locate_all_fill_device(colbwt_index *idx, uint64_t n_reads, uint64_t read_lo, uint64_t read_hi, const uint64_t *d_pos_off,
                                  uint64_t *d_pos, uint64_t pos_cap, const void *d_work, void *hip_stream, colbwt_stats *stats) {
    auto bad_argument = [&]() -> const char * {
        if (const char *m = samples_missing(idx)) return m;
        if (read_lo > read_hi || read_hi > n_reads) return "read_lo <= read_hi <= n_reads expected";
        if (n_reads >= 0xFFFFFFFFull) return kTooManyReads;
        if (read_lo == read_hi) return nullptr;
        if (!d_pos_off || !d_work) return "null d_pos_off/d_work";
        if (pos_cap && !d_pos) return "null d_pos with pos_cap > 0";
        if (((uintptr_t)d_pos_off & 7) || ((uintptr_t)d_pos & 7)) return "d_pos_off and d_pos must be 8-byte aligned";
        if ((uintptr_t)d_work & 255) return "d_work must be 256-byte aligned";
        return nullptr;
    };
    return device_entry(idx, d_work, read_hi - read_lo, 0, hip_stream, 0, stats, bad_argument,
                        [&](const Index &ix, hipStream_t stream) {
                            const LocateTables &L = replica_for(idx, d_work)->loc;
                            launch_locate_all_fill(ix, L.all(), n_reads, read_lo, read_hi, d_pos_off, d_pos, pos_cap, d_work, stream);
                        });
}

int colbwt_locate_all_batch(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, uint32_t min_len,
                            uint64_t max_per_read, uint32_t *mlen, uint64_t *occ, uint64_t *pos_off, uint64_t *pos, uint64_t pos_cap,
                            colbwt_stats *stats) {
    return locate_all_batch_all(idx, bases, read_off, n_reads, min_len, max_per_read, mlen, occ, pos_off, pos, pos_cap, stats);
}

// One batch at a time on the handle's first replica: reader, plan, then fill / copy / write in read
// ranges of at most COLBWT_LOCATE_ALL_FILE_POSITIONS positions.
int colbwt_locate_all_file(colbwt_index *idx, const char *pattern_path, const char *out_path, uint32_t min_len, uint64_t max_per_read,
                           uint64_t batch_bases, colbwt_stats *stats) {
    if (!idx || !pattern_path) return fail(COLBWT_ERR_ARG, "null argument");
    if (min_len == 0) return fail(COLBWT_ERR_ARG, "min_len must be at least 1");
    if (!idx->loc.ready()) return fail(COLBWT_ERR_ARG, kNoSamples);
    if (stats) memset(stats, 0, sizeof(*stats));
    const std::string out = out_path ? out_path : std::string(pattern_path) + ".locate";
    if (batch_bases == 0) batch_bases = 64ull << 20;
    FastxReader reader;
    if (!reader.open(pattern_path)) return fail(COLBWT_ERR_IO, std::string("cannot open pattern file ") + pattern_path);
    int rc = select_device(idx->ix.device(), g_err);
    if (rc != COLBWT_OK) return rc;
    struct File {
        FILE *f = nullptr;
        ~File() { if (f) fclose(f); }
    } wn;
    wn.f = fopen(out.c_str(), "wb");
    if (!wn.f) return fail(COLBWT_ERR_IO, "cannot create " + out);
    setvbuf(wn.f, nullptr, _IOFBF, 4u << 20);
    struct Stream {
        hipStream_t s = nullptr;
        ~Stream() { if (s) (void)hipStreamDestroy(s); }
    } st;
    TRY_HIP(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking), nullptr, g_err);
    const hipStream_t stream = st.s;
    const uint64_t cap = COLBWT_LOCATE_ALL_FILE_POSITIONS;
    const std::vector<uint64_t> &ds = idx->loc.doc_start;

    DevPtr d_bases, d_off, d_mlen, d_occ, d_pos_off, d_work, d_pos;
    auto need = [](DevPtr &p, uint64_t bytes) { return p.bytes() >= bytes ? hipSuccess : p.alloc(bytes + bytes / 8 + 256); };
    std::vector<uint8_t> bases;
    std::vector<uint64_t> off, occ, pos_off, pos;
    std::vector<uint32_t> mlen;
    std::vector<std::string> names;
    std::string name;
    bool ok = true;
    for (bool more = true; more;) {
        bases.clear();
        names.clear();
        off.assign(1, 0);
        while (bases.size() < batch_bases && names.size() < 0xFFFFFFFEull) {
            if (!reader.next(name, bases)) {
                more = false;
                break;
            }
            if (bases.size() - off.back() > 0xFFFFFFFFull) return fail(COLBWT_ERR_ARG, "read longer than 2^32-1 bases");
            names.push_back(name);
            off.push_back(bases.size());
        }
        const uint64_t n = names.size(), nb = bases.size();
        if (n == 0) continue;
        const uint64_t bases_alloc = (nb + 64 + 63) & ~63ull;     // the search reads whole 64-byte blocks
        TRY_HIP(need(d_bases, bases_alloc), stream, g_err);
        TRY_HIP(need(d_off, 8 * (n + 1)), stream, g_err);
        TRY_HIP(need(d_mlen, 4 * n), stream, g_err);
        TRY_HIP(need(d_occ, 8 * n), stream, g_err);
        TRY_HIP(need(d_pos_off, 8 * (n + 1)), stream, g_err);
        TRY_HIP(need(d_work, locate_all_work_bytes(n)), stream, g_err);
        TRY_HIP(hipMemsetAsync(d_bases.as<uint8_t>() + nb, 0, bases_alloc - nb, stream), stream, g_err);
        if (nb) TRY_HIP(hipMemcpyAsync(d_bases.get(), bases.data(), nb, hipMemcpyHostToDevice, stream), stream, g_err);
        TRY_HIP(hipMemcpyAsync(d_off.get(), off.data(), 8 * (n + 1), hipMemcpyHostToDevice, stream), stream, g_err);
        colbwt_stats ps{}, fs{};
        uint64_t total = 0;
        rc = colbwt_locate_all_plan_device(idx, d_bases.as<uint8_t>(), d_off.as<uint64_t>(), n, nb, min_len, max_per_read,
                                           d_mlen.as<uint32_t>(), d_occ.as<uint64_t>(), d_pos_off.as<uint64_t>(), d_work.get(), nullptr,
                                           stream, &total, &ps);
        if (rc != COLBWT_OK) return rc;
        mlen.resize(n);
        occ.resize(n);
        pos_off.resize(n + 1);
        TRY_HIP(hipMemcpyAsync(mlen.data(), d_mlen.get(), 4 * n, hipMemcpyDeviceToHost, stream), stream, g_err);
        TRY_HIP(hipMemcpyAsync(occ.data(), d_occ.get(), 8 * n, hipMemcpyDeviceToHost, stream), stream, g_err);
        TRY_HIP(hipMemcpyAsync(pos_off.data(), d_pos_off.get(), 8 * (n + 1), hipMemcpyDeviceToHost, stream), stream, g_err);
        TRY_HIP(hipStreamSynchronize(stream), stream, g_err);
        const uint64_t room = std::min(total, cap);
        TRY_HIP(need(d_pos, 8 * std::max<uint64_t>(room, 1)), stream, g_err);
        pos.resize(room);
        if (stats) {
            stats->n_reads += n;
            stats->n_bases += nb;
            stats->kernel_ms += ps.kernel_ms;
        }
        for (uint64_t lo = 0; lo < n && ok;) {
            uint64_t hi = lo;
            while (hi < n && pos_off[hi + 1] - pos_off[lo] <= cap) ++hi;
            if (hi == lo)
                return fail(COLBWT_ERR_NOMEM, "read " + names[lo] + " has " + std::to_string(pos_off[lo + 1] - pos_off[lo]) +
                                                  " positions, more than colbwt_locate_all_file holds at once (" + std::to_string(cap) +
                                                  "): set max_per_read");
            const uint64_t cnt = pos_off[hi] - pos_off[lo];
            if (cnt) {
                rc = colbwt_locate_all_fill_device(idx, n, lo, hi, d_pos_off.as<uint64_t>(), d_pos.as<uint64_t>(), cnt, d_work.get(), stream,
                                                   &fs);
                if (rc != COLBWT_OK) return rc;
                TRY_HIP(hipMemcpyAsync(pos.data(), d_pos.get(), 8 * cnt, hipMemcpyDeviceToHost, stream), stream, g_err);
                TRY_HIP(hipStreamSynchronize(stream), stream, g_err);
                if (stats) stats->kernel_ms += fs.kernel_ms;
            }
            for (uint64_t k = lo; k < hi && ok; ++k) {
                ok = fprintf(wn.f, "%s\t%llu\t%u\t%llu\t", names[k].c_str(), (unsigned long long)(off[k + 1] - off[k]), mlen[k],
                             (unsigned long long)occ[k]) > 0;
                for (uint64_t t = 0, w = pos_off[k + 1] - pos_off[k]; t < w && ok; ++t) {
                    const uint64_t x = pos[pos_off[k] - pos_off[lo] + t];
                    const size_t d = (size_t)(std::upper_bound(ds.begin(), ds.end(), x) - ds.begin()) - 1;
                    ok = fprintf(wn.f, t ? ",%zu:%llu" : "%zu:%llu", d, (unsigned long long)(x - ds[d])) > 0;
                }
                ok = ok && fputc('\n', wn.f) != EOF;
            }
            lo = hi;
        }
    }
    FILE *f = wn.f;
    wn.f = nullptr;
    if (fclose(f) != 0 || !ok) return fail(COLBWT_ERR_IO, "short write on " + out);
    return COLBWT_OK;
}

uint32_t colbwt_docs_mask_words(const colbwt_index *idx) {
    return idx && idx->loc.ready() ? docs_mask_words(idx->loc.n_docs()) : 0;
}

uint64_t colbwt_docs_work_bytes(uint64_t n_reads) { return docs_work_bytes(n_reads); }

int colbwt_docs_batch(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, uint32_t min_len,
                      uint32_t max_walk, uint32_t *mlen, uint64_t *occ, uint32_t *n_hit, uint64_t *mask, uint64_t *doc_reads,
                      uint64_t *doc_only, colbwt_stats *stats) {
    return docs_batch_all(idx, bases, read_off, n_reads, min_len, max_walk, mlen, occ, n_hit, mask, doc_reads, doc_only, stats);
}

int colbwt_docs_device(colbwt_index *idx, const uint8_t *d_bases, const uint64_t *d_read_off, uint64_t n_reads, uint64_t n_bases,
                       uint32_t min_len, uint32_t max_walk, uint32_t *d_mlen, uint64_t *d_occ, uint32_t *d_n_hit, uint64_t *d_mask,
                       uint64_t *d_doc_reads, uint64_t *d_doc_only, void *d_work, const uint32_t *d_order, void *hip_stream,
                       colbwt_stats *stats) {
    auto bad_argument = [&]() -> const char * {
        if (const char *m = docs_bad_params(min_len, max_walk)) return m;
        if (const char *m = samples_missing(idx)) return m;
        if (idx->loc.n_docs() > kDocsLds) return kDocsTooMany;
        if (n_reads == 0) return nullptr;
        if (!d_bases || !d_read_off || !d_mlen || !d_occ) return "null device pointer";
        if (((uintptr_t)d_bases & 15) || ((uintptr_t)d_mlen & 3) || ((uintptr_t)d_occ & 7))
            return "d_bases must be 16-byte aligned, d_mlen 4-byte and d_occ 8-byte aligned";
        if (n_reads >= 0xFFFFFFFFull) return kTooManyReads;
        if (!d_n_hit || !d_mask || !d_work) return "null d_n_hit/d_mask/d_work";
        if (((uintptr_t)d_n_hit & 3) || ((uintptr_t)d_mask & 7) || ((uintptr_t)d_doc_reads & 7) || ((uintptr_t)d_doc_only & 7))
            return "d_n_hit must be 4-byte aligned, d_mask/d_doc_reads/d_doc_only 8-byte aligned";
        if ((uintptr_t)d_work & 255) return "d_work must be 256-byte aligned";
        return nullptr;
    };
    hipError_t launched = hipSuccess;
    const int rc = device_entry(idx, d_bases, n_reads, n_bases, hip_stream, 0, stats, bad_argument,
                                [&](const Index &ix, hipStream_t stream) {
                                    const LocateTables &L = replica_for(idx, d_bases)->loc;
                                    launched = launch_docs(ix, L.docs(min_len, max_walk), d_bases, d_read_off, n_reads, d_mlen, d_occ,
                                                           d_n_hit, d_mask, d_doc_reads, d_doc_only, d_work, d_order, stream);
                                });
    if (rc == COLBWT_OK && launched != hipSuccess) return hip_failed(launched, "colbwt_docs_device", nullptr, g_err);
    return rc;
}

int colbwt_docs_file(colbwt_index *idx, const char *pattern_path, const char *out_path, uint32_t min_len, uint32_t max_walk,
                     uint64_t batch_bases, colbwt_stats *stats) {
    if (!idx || !pattern_path) return fail(COLBWT_ERR_ARG, "null argument");
    if (const char *m = docs_bad_params(min_len, max_walk)) return fail(COLBWT_ERR_ARG, m);
    if (!idx->loc.ready()) return fail(COLBWT_ERR_ARG, kNoSamples);
    if (idx->loc.n_docs() > kDocsLds) return fail(COLBWT_ERR_ARG, kDocsTooMany);
    const std::string out = out_path ? out_path : std::string(pattern_path) + ".docs";
    if (batch_bases == 0)   // the default batch of the file query, cut so that W mask words per read stay ~tens of MB
        batch_bases = std::max<uint64_t>(1ull << 20, (64ull << 20) * (1 + idx->more.size()) * 16 /
                                                         std::max<uint32_t>(16, docs_mask_words(idx->loc.n_docs())));
    return query_file_impl(idx, pattern_path, out, out, batch_bases, stats, false, true, 0, 0, 0, min_len, max_walk);
}

int colbwt_binary_to_text(const char *bin_path, int value_bytes, const char *text_path) {
    if (!bin_path || !text_path) return fail(COLBWT_ERR_ARG, "null argument");
    std::string err;
    if (!binary_to_text(bin_path, value_bytes, text_path, err)) return fail(value_bytes == 1 || value_bytes == 2 ? COLBWT_ERR_IO : COLBWT_ERR_ARG, err);
    return COLBWT_OK;
}

int colbwt_pml_pack_device(const uint16_t *d_pml, uint64_t n_bases, uint32_t *d_mask, void *hip_stream) {
    if (!d_pml || !d_mask) return fail(COLBWT_ERR_ARG, "null argument");
    if ((uintptr_t)d_pml % 32 || (uintptr_t)d_mask % 4) return fail(COLBWT_ERR_ARG, "d_pml must be 32-byte aligned");
    launch_pml_pack(d_pml, n_bases, d_mask, (hipStream_t)hip_stream);
    return launch_status(__func__);
}

int colbwt_read_end_mask_device(const uint64_t *d_read_off, uint64_t n_reads, uint32_t *d_mask, void *hip_stream) {
    if (!d_read_off || !d_mask) return fail(COLBWT_ERR_ARG, "null argument");
    launch_read_end_mask(d_read_off, n_reads, d_mask, (hipStream_t)hip_stream);
    return launch_status(__func__);
}

int colbwt_pml_unpack_device(const uint32_t *d_zero_mask, const uint32_t *d_end_mask, uint64_t first_word,
                             uint64_t n_words, uint64_t total_words, uint16_t *d_pml, void *hip_stream) {
    if (!d_zero_mask || !d_end_mask || !d_pml) return fail(COLBWT_ERR_ARG, "null argument");
    if (first_word + n_words > total_words) return fail(COLBWT_ERR_ARG, "word range beyond the masks");
    if ((uintptr_t)d_pml % 64) return fail(COLBWT_ERR_ARG, "d_pml must be 64-byte aligned");
    launch_pml_unpack(d_zero_mask, d_end_mask, first_word, n_words, total_words, d_pml, (hipStream_t)hip_stream);
    return launch_status(__func__);
}

int colbwt_index_cid_dictionary(const colbwt_index *idx, uint8_t *ids, uint32_t *n_ids) {
    if (!idx || !ids || !n_ids) return fail(COLBWT_ERR_ARG, "null argument");
    uint32_t n = 0;
    for (uint32_t c = 0; c < 256; ++c)
        if ((idx->ix.cid_set()[c >> 5] >> (c & 31)) & 1u) ids[n++] = (uint8_t)c;
    *n_ids = n;
    return COLBWT_OK;
}

static uint32_t cid_code_bits(uint32_t n_ids) {
    uint32_t bits = 1;
    while ((1u << bits) < n_ids) ++bits;
    return bits;
}

uint32_t colbwt_cid_code_bits(uint32_t n_ids) { return n_ids >= 1 && n_ids <= 256 ? cid_code_bits(n_ids) : 0; }

int colbwt_cid_pack_device(const uint8_t *d_cid, uint64_t n_bases, const uint8_t *ids, uint32_t n_ids, uint32_t *d_planes,
                           void *hip_stream) {
    if (!d_cid || !ids || !d_planes) return fail(COLBWT_ERR_ARG, "null argument");
    if (n_ids < 1 || n_ids > 256) return fail(COLBWT_ERR_ARG, "a dictionary holds 1 .. 256 col ids");
    if ((uintptr_t)d_cid % 16) return fail(COLBWT_ERR_ARG, "d_cid must be 16-byte aligned");
    CidLut code_of;
    memset(code_of.v, 0, sizeof(code_of.v));
    for (uint32_t k = 0; k < n_ids; ++k) code_of.v[ids[k]] = (uint8_t)k;
    launch_cid_pack(d_cid, n_bases, code_of, cid_code_bits(n_ids), d_planes, (hipStream_t)hip_stream);
    return launch_status(__func__);
}

int colbwt_cid_unpack_device(const uint32_t *d_planes, uint64_t first_word, uint64_t n_words, const uint8_t *ids, uint32_t n_ids,
                             uint8_t *d_cid, void *hip_stream) {
    if (!d_planes || !ids || !d_cid) return fail(COLBWT_ERR_ARG, "null argument");
    if (n_ids < 1 || n_ids > 256) return fail(COLBWT_ERR_ARG, "a dictionary holds 1 .. 256 col ids");
    if ((uintptr_t)d_cid % 32) return fail(COLBWT_ERR_ARG, "d_cid must be 32-byte aligned");
    CidLut id_of;
    memset(id_of.v, 0, sizeof(id_of.v));
    for (uint32_t k = 0; k < n_ids; ++k) id_of.v[k] = ids[k];
    launch_cid_unpack(d_planes, first_word, n_words, id_of, cid_code_bits(n_ids), d_cid, (hipStream_t)hip_stream);
    return launch_status(__func__);
}

int colbwt_synth_reads_device(colbwt_index *idx, uint64_t n_reads, uint32_t read_len, uint32_t sub_permille,
                              uint64_t seed, uint8_t *d_bases, uint64_t *d_read_off, void *hip_stream) {
    if (!idx || !d_bases || !d_read_off || read_len == 0) return fail(COLBWT_ERR_ARG, "bad argument");
    idx = replica_for(idx, d_bases);
    int rc = select_device(idx->ix.device(), g_err);
    if (rc != COLBWT_OK) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    TRY_HIP(hipMemsetAsync(d_bases + n_reads * (uint64_t)read_len, 0, 64, stream), nullptr, g_err);
    launch_sampler(idx->ix, n_reads, read_len, sub_permille, seed, d_bases, d_read_off, stream);
    TRY_HIP(hipGetLastError(), nullptr, g_err);
    return COLBWT_OK;
}

}  // extern "C"
