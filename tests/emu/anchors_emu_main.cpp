// tests/emu/anchors_emu_main.cpp -- stand-alone driver of colbwt_anchors_* compiled with the product sources
// against the SIMT emulator under ASan/UBSan (TEST INFRASTRUCTURE ONLY; built and run by
// tests/test_anchors_cpu.py with the recipe of anchors_emu.mk).
//
//   anchors_emu DIR
// DIR/cases.txt: one case per line "case index layout min_len max_anchors max_occ reads"; DIR/<index>.col_pml is
// the index and, when max_occ > 0, DIR/<index>.col_loc its samples (max_occ == 0 runs WITHOUT samples attached);
// DIR/<reads>.fa the reads as FASTA and DIR/<reads>.bin their raw dump (u64 n_reads, u64 read_off[n_reads + 1],
// the bases).  Per case the driver runs colbwt_anchors_file on the FASTA (-> DIR/<case>.anchors), then
// colbwt_anchors_device over host arrays of the exact sizes the header asks for, filled with garbage first --
// without and with an order array (reads by decreasing length), and with the slot arrays NULL -- and
// colbwt_anchors_batch; all must agree byte for byte.  The raw outputs go to DIR/<case>.out: summary, start,
// len, occ, pos.  Then the argument errors on the first case's index.
// Prints ANCHORS-EMU-OK at the end; any mismatch ends it with exit status 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/colbwt.h"

static void die(const std::string &what) {
    fprintf(stderr, "anchors_emu: %s (last error: %s)\n", what.c_str(), colbwt_last_error());
    exit(1);
}

static std::vector<uint8_t> slurp(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) die("cannot read " + path);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

template <typename T>
static void put(FILE *f, const T *p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) die("short write");
}

// heap arrays of exactly the bytes asked for, so that ASan sees any access past them; filled with 0xAB,
// since the entry points take uninitialised buffers
struct Aligned {
    void *p = nullptr;
    size_t bytes = 0;
    Aligned(size_t align, size_t n) : bytes(n) {
        const size_t padded = (n + align - 1) / align * align;
        p = aligned_alloc(align, padded ? padded : align);
        if (!p) die("out of memory");
        memset(p, 0xAB, padded ? padded : align);
    }
    ~Aligned() { free(p); }
    template <typename T>
    T *as() const { return (T *)p; }
    bool same(const Aligned &o) const { return bytes == o.bytes && (bytes == 0 || memcmp(p, o.p, bytes) == 0); }
};

struct Reads {
    uint64_t n = 0, n_bases = 0;
    std::vector<uint64_t> off;
    std::vector<uint8_t> bases;
};

static Reads load_reads(const std::string &path) {
    const std::vector<uint8_t> raw = slurp(path);
    Reads r;
    memcpy(&r.n, raw.data(), 8);
    r.off.resize(r.n + 1);
    memcpy(r.off.data(), raw.data() + 8, 8 * (r.n + 1));
    r.n_bases = r.off[r.n];
    r.bases.assign(raw.begin() + 8 * (r.n + 2), raw.end());
    if (r.bases.size() != r.n_bases) die("bad read dump " + path);
    return r;
}

static colbwt_index *open_index(const std::string &stem, int layout, bool attach) {
    colbwt_index *h = nullptr;
    if (colbwt_index_open_layout(stem.c_str(), nullptr, 0, layout, &h) != COLBWT_OK) die("open " + stem);
    if (attach && colbwt_index_attach_locate(h, stem.c_str()) != COLBWT_OK) die("attach " + stem);
    return h;
}

static void expect(int rc, int want, const char *msg, const char *what) {
    if (rc != want || (msg && strncmp(colbwt_last_error(), msg, strlen(msg)) != 0))
        die(std::string(what) + ": got " + std::to_string(rc) + " \"" + colbwt_last_error() + "\", expected " + std::to_string(want) +
            " \"" + (msg ? msg : "") + "\"");
}

// the four slot arrays of one call, of exactly n * K (* W) entries
struct Slots {
    Aligned summary, start, len, occ, pos;
    Slots(uint64_t n, uint64_t K, uint64_t W) : summary(16, 32 * n), start(4, 4 * n * K), len(4, 4 * n * K), occ(8, 8 * n * K), pos(8, 8 * n * K * W) {}
    bool same(const Slots &o) const { return summary.same(o.summary) && start.same(o.start) && len.same(o.len) && occ.same(o.occ) && pos.same(o.pos); }
};

static void run_case(const std::string &dir, const std::string &name, const std::string &index, int layout, uint32_t min_len,
                     uint32_t K, uint32_t W, const std::string &reads_stem) {
    colbwt_index *h = open_index(dir + "/" + index, layout, W > 0);
    colbwt_stats st;
    if (colbwt_anchors_file(h, (dir + "/" + reads_stem + ".fa").c_str(), (dir + "/" + name + ".anchors").c_str(), min_len, K, W, 0, &st) !=
        COLBWT_OK)
        die("colbwt_anchors_file " + name);

    const Reads r = load_reads(dir + "/" + reads_stem + ".bin");
    const uint64_t n = r.n;
    Aligned bases(64, r.n_bases + 64), off(8, 8 * (n + 1)), order(4, 4 * n);
    memset(bases.p, 0, r.n_bases + 64);
    if (r.n_bases) memcpy(bases.p, r.bases.data(), r.n_bases);
    memcpy(off.p, r.off.data(), 8 * (n + 1));
    std::vector<uint32_t> by_len(n);
    std::iota(by_len.begin(), by_len.end(), 0u);
    std::stable_sort(by_len.begin(), by_len.end(),
                     [&](uint32_t a, uint32_t b) { return r.off[a + 1] - r.off[a] > r.off[b + 1] - r.off[b]; });
    if (n) memcpy(order.p, by_len.data(), 4 * n);

    auto device = [&](Slots &s, bool slots, const uint32_t *d_order, const char *what) {
        const int rc = colbwt_anchors_device(h, bases.as<uint8_t>(), off.as<uint64_t>(), n, r.n_bases, min_len, K, W,
                                             s.summary.as<colbwt_anchor_summary>(), slots ? s.start.as<uint32_t>() : nullptr,
                                             slots ? s.len.as<uint32_t>() : nullptr, slots ? s.occ.as<uint64_t>() : nullptr,
                                             slots && W ? s.pos.as<uint64_t>() : nullptr, d_order, nullptr, &st);
        if (rc != COLBWT_OK || st.n_reads != n) die(std::string(what) + " " + name);
    };
    Slots plain(n, K, W), ordered(n, K, W), only(n, 0, 0), host(n, K, W);
    device(plain, true, nullptr, "colbwt_anchors_device");
    device(ordered, true, order.as<uint32_t>(), "colbwt_anchors_device with d_order");
    if (!plain.same(ordered)) die("d_order changes the results of " + name);
    device(only, false, nullptr, "colbwt_anchors_device, summaries only");
    if (!only.summary.same(plain.summary)) die("summaries-only differs: " + name);
    if (colbwt_anchors_batch(h, r.bases.data(), r.off.data(), n, min_len, K, W, host.summary.as<colbwt_anchor_summary>(),
                             host.start.as<uint32_t>(), host.len.as<uint32_t>(), host.occ.as<uint64_t>(), W ? host.pos.as<uint64_t>() : nullptr,
                             &st) != COLBWT_OK || st.n_reads != n)
        die("colbwt_anchors_batch " + name);
    if (!host.same(plain)) die("colbwt_anchors_batch differs from the device form: " + name);
    {
        Slots sum_only(n, 0, 0);
        if (colbwt_anchors_batch(h, r.bases.data(), r.off.data(), n, min_len, K, W, sum_only.summary.as<colbwt_anchor_summary>(), nullptr, nullptr,
                                 nullptr, nullptr, nullptr) != COLBWT_OK || !sum_only.summary.same(plain.summary))
            die("colbwt_anchors_batch, summaries only: " + name);
    }
    FILE *f = fopen((dir + "/" + name + ".out").c_str(), "wb");
    if (!f) die("cannot create the raw output of " + name);
    put(f, plain.summary.as<uint8_t>(), 32 * n);
    put(f, plain.start.as<uint32_t>(), n * K);
    put(f, plain.len.as<uint32_t>(), n * K);
    put(f, plain.occ.as<uint64_t>(), n * K);
    put(f, plain.pos.as<uint64_t>(), n * K * W);
    fclose(f);
    colbwt_index_close(h);
    printf("ok %s: %llu reads, layout %d, min_len %u, max_anchors %u, max_occ %u\n", name.c_str(), (unsigned long long)n, layout, min_len, K, W);
}

static void arg_errors(const std::string &dir, const std::string &index, int layout, const std::string &reads_stem) {
    const char *no_samples = "no locate samples attached (colbwt_index_attach_locate)";
    const char *slot_set = "start/len/occ: all three or none; pos exactly when they are given and max_occ > 0";
    const char *aligned = "d_bases/d_summary must be 16-byte aligned, d_start/d_len 4-byte and d_occ/d_pos 8-byte aligned";
    const std::string fa = dir + "/" + reads_stem + ".fa", stem = dir + "/" + index;
    const Reads r = load_reads(dir + "/" + reads_stem + ".bin");
    const uint64_t n = r.n;
    const uint32_t K = 2, W = 2;
    colbwt_index *h = open_index(stem, layout, false);
    Aligned bases(64, r.n_bases + 64);
    memset(bases.p, 0, r.n_bases + 64);
    if (r.n_bases) memcpy(bases.p, r.bases.data(), r.n_bases);
    Slots s(n, K, W);
    const uint8_t *b = bases.as<uint8_t>();
    const uint64_t *o = r.off.data();
    colbwt_anchor_summary *sm = s.summary.as<colbwt_anchor_summary>();
    uint32_t *as = s.start.as<uint32_t>(), *al = s.len.as<uint32_t>();
    uint64_t *ao = s.occ.as<uint64_t>(), *ap = s.pos.as<uint64_t>();
    auto dev = [&](colbwt_index *x, const uint8_t *pb, uint64_t cnt, uint32_t l, uint32_t k, uint32_t w, colbwt_anchor_summary *psm,
                   uint32_t *pas, uint32_t *pal, uint64_t *pao, uint64_t *pap) {
        return colbwt_anchors_device(x, pb, o, cnt, r.n_bases, l, k, w, psm, pas, pal, pao, pap, nullptr, nullptr, nullptr);
    };
    auto bat = [&](colbwt_index *x, const uint8_t *pb, const uint64_t *po, uint64_t cnt, uint32_t l, uint32_t k, uint32_t w,
                   colbwt_anchor_summary *psm, uint32_t *pas, uint32_t *pal, uint64_t *pao, uint64_t *pap) {
        return colbwt_anchors_batch(x, pb, po, cnt, l, k, w, psm, pas, pal, pao, pap, nullptr);
    };
    expect(dev(nullptr, b, n, 1, K, W, sm, as, al, ao, ap), COLBWT_ERR_ARG, "null index", "device/null index");
    expect(bat(nullptr, b, o, n, 1, K, W, sm, as, al, ao, ap), COLBWT_ERR_ARG, "null index", "batch/null index");
    expect(colbwt_anchors_file(nullptr, fa.c_str(), nullptr, 1, K, W, 0, nullptr), COLBWT_ERR_ARG, "null argument", "file/null index");
    expect(colbwt_anchors_file(h, nullptr, nullptr, 1, K, W, 0, nullptr), COLBWT_ERR_ARG, "null argument", "file/null pattern");
    // the parameters come before the samples, the samples before anything about the pointers
    const char *min0 = "min_len must be at least 1", *bad_k = "max_anchors must be 1 .. 2^16", *bad_w = "max_occ must be 0 .. 2^20";
    expect(dev(h, b, n, 0, K, W, sm, as, al, ao, ap), COLBWT_ERR_ARG, min0, "device/min_len 0");
    expect(bat(h, b, o, n, 0, K, W, sm, as, al, ao, ap), COLBWT_ERR_ARG, min0, "batch/min_len 0");
    expect(colbwt_anchors_file(h, fa.c_str(), nullptr, 0, K, W, 0, nullptr), COLBWT_ERR_ARG, min0, "file/min_len 0");
    for (uint32_t k : {0u, (1u << 16) + 1}) {
        expect(dev(h, b, n, 1, k, W, sm, as, al, ao, ap), COLBWT_ERR_ARG, bad_k, "device/max_anchors");
        expect(bat(h, b, o, n, 1, k, W, sm, as, al, ao, ap), COLBWT_ERR_ARG, bad_k, "batch/max_anchors");
        expect(colbwt_anchors_file(h, fa.c_str(), nullptr, 1, k, W, 0, nullptr), COLBWT_ERR_ARG, bad_k, "file/max_anchors");
    }
    expect(dev(h, b, n, 1, K, (1u << 20) + 1, sm, as, al, ao, ap), COLBWT_ERR_ARG, bad_w, "device/max_occ");
    expect(bat(h, b, o, n, 1, K, (1u << 20) + 1, sm, as, al, ao, ap), COLBWT_ERR_ARG, bad_w, "batch/max_occ");
    expect(colbwt_anchors_file(h, fa.c_str(), nullptr, 1, K, (1u << 20) + 1, 0, nullptr), COLBWT_ERR_ARG, bad_w, "file/max_occ");
    expect(dev(h, nullptr, n, 1, K, W, sm, as, al, ao, ap), COLBWT_ERR_ARG, no_samples, "device/no samples");
    expect(bat(h, nullptr, o, n, 1, K, W, sm, as, al, ao, ap), COLBWT_ERR_ARG, no_samples, "batch/no samples");
    expect(dev(h, b, n, 1, K, W, sm, nullptr, nullptr, nullptr, nullptr), COLBWT_ERR_ARG, no_samples, "device/no samples, summaries only");
    expect(colbwt_anchors_file(h, fa.c_str(), (dir + "/never.anchors").c_str(), 1, K, W, 0, nullptr), COLBWT_ERR_ARG, no_samples, "file/no samples");
    // max_occ == 0 needs no samples; a position array is then one pointer too many
    expect(dev(h, b, n, 1, K, 0, sm, as, al, ao, nullptr), COLBWT_OK, nullptr, "device/max_occ 0 without samples");
    expect(dev(h, b, n, 1, K, 0, sm, as, al, ao, ap), COLBWT_ERR_ARG, slot_set, "device/pos with max_occ 0");
    expect(bat(h, b, o, n, 1, K, 0, sm, as, al, ao, ap), COLBWT_ERR_ARG, slot_set, "batch/pos with max_occ 0");
    if (colbwt_index_attach_locate(h, stem.c_str()) != COLBWT_OK) die("attach");
    // the slot pointer set
    expect(dev(h, b, n, 1, K, W, sm, as, nullptr, ao, ap), COLBWT_ERR_ARG, slot_set, "device/len missing");
    expect(dev(h, b, n, 1, K, W, sm, nullptr, al, ao, ap), COLBWT_ERR_ARG, slot_set, "device/start missing");
    expect(dev(h, b, n, 1, K, W, sm, as, al, nullptr, ap), COLBWT_ERR_ARG, slot_set, "device/occ missing");
    expect(dev(h, b, n, 1, K, W, sm, as, al, ao, nullptr), COLBWT_ERR_ARG, slot_set, "device/pos missing");
    expect(dev(h, b, n, 1, K, W, sm, nullptr, nullptr, nullptr, ap), COLBWT_ERR_ARG, slot_set, "device/pos without slots");
    expect(bat(h, b, o, n, 1, K, W, sm, as, nullptr, ao, ap), COLBWT_ERR_ARG, slot_set, "batch/len missing");
    expect(bat(h, b, o, n, 1, K, W, sm, as, al, ao, nullptr), COLBWT_ERR_ARG, slot_set, "batch/pos missing");
    expect(bat(h, b, o, n, 1, K, W, sm, nullptr, nullptr, nullptr, ap), COLBWT_ERR_ARG, slot_set, "batch/pos without slots");
    // no reads: nothing is looked at
    expect(dev(h, nullptr, 0, 1, K, W, nullptr, nullptr, nullptr, nullptr, nullptr), COLBWT_OK, nullptr, "device/no reads");
    expect(bat(h, nullptr, nullptr, 0, 1, K, W, nullptr, nullptr, nullptr, nullptr, nullptr), COLBWT_OK, nullptr, "batch/no reads");
    // pointers and alignment
    expect(dev(h, b, 0xFFFFFFFFull, 1, K, W, sm, as, al, ao, ap), COLBWT_ERR_ARG, "more than 2^32-2 reads in a batch", "device/too many reads");
    expect(bat(h, b, o, 0xFFFFFFFFull, 1, K, W, sm, as, al, ao, ap), COLBWT_ERR_ARG, "more than 2^32-2 reads in a batch", "batch/too many reads");
    expect(dev(h, nullptr, n, 1, K, W, sm, as, al, ao, ap), COLBWT_ERR_ARG, "null device pointer", "device/null bases");
    expect(dev(h, b, n, 1, K, W, nullptr, as, al, ao, ap), COLBWT_ERR_ARG, "null device pointer", "device/null summary");
    expect(dev(h, b + 1, n, 1, K, W, sm, as, al, ao, ap), COLBWT_ERR_ARG, aligned, "device/bases alignment");
    expect(dev(h, b, n, 1, K, W, (colbwt_anchor_summary *)((uint8_t *)sm + 8), as, al, ao, ap), COLBWT_ERR_ARG, aligned, "device/summary alignment");
    expect(dev(h, b, n, 1, K, W, sm, (uint32_t *)((uint8_t *)as + 2), al, ao, ap), COLBWT_ERR_ARG, aligned, "device/start alignment");
    expect(dev(h, b, n, 1, K, W, sm, as, (uint32_t *)((uint8_t *)al + 1), ao, ap), COLBWT_ERR_ARG, aligned, "device/len alignment");
    expect(dev(h, b, n, 1, K, W, sm, as, al, (uint64_t *)((uint8_t *)ao + 4), ap), COLBWT_ERR_ARG, aligned, "device/occ alignment");
    expect(dev(h, b, n, 1, K, W, sm, as, al, ao, (uint64_t *)((uint8_t *)ap + 4)), COLBWT_ERR_ARG, aligned, "device/pos alignment");
    expect(bat(h, b, nullptr, n, 1, K, W, sm, as, al, ao, ap), COLBWT_ERR_ARG, "null read_off", "batch/null read_off");
    expect(bat(h, nullptr, o, n, 1, K, W, sm, as, al, ao, ap), COLBWT_ERR_ARG, "null bases/summary", "batch/null bases");
    expect(bat(h, b, o, n, 1, K, W, nullptr, as, al, ao, ap), COLBWT_ERR_ARG, "null bases/summary", "batch/null summary");
    expect(dev(h, b, n, 1, K, W, sm, as, al, ao, ap), COLBWT_OK, nullptr, "device");
    // file form
    expect(colbwt_anchors_file(h, (dir + "/no_such_reads.fa").c_str(), (dir + "/never.anchors").c_str(), 1, K, W, 0, nullptr), COLBWT_ERR_IO,
           ("cannot open pattern file " + dir + "/no_such_reads.fa").c_str(), "file/missing pattern");
    colbwt_index_close(h);
    printf("ok argument errors of colbwt_anchors_device / _batch / _file\n");
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: anchors_emu DIR\n");
        return 2;
    }
    const std::string dir = argv[1];
    std::ifstream cases(dir + "/cases.txt");
    if (!cases) die("cannot read " + dir + "/cases.txt");
    std::string line, first_index, first_reads;
    int first_layout = 0, n_cases = 0;
    while (std::getline(cases, line)) {
        std::istringstream in(line);
        std::string name, index, reads;
        int layout = 0;
        uint32_t min_len = 0, K = 0, W = 0;
        if (!(in >> name >> index >> layout >> min_len >> K >> W >> reads)) continue;
        run_case(dir, name, index, layout, min_len, K, W, reads);
        if (n_cases++ == 0) {
            first_index = index;
            first_reads = reads;
            first_layout = layout;
        }
    }
    if (n_cases == 0) die("no cases");
    arg_errors(dir, first_index, first_layout, first_reads);
    printf("ANCHORS-EMU-OK\n");
    return 0;
}
