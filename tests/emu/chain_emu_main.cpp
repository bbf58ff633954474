// tests/emu/chain_emu_main.cpp -- stand-alone driver of colbwt_chain_* compiled with the product sources
// against the SIMT emulator under ASan/UBSan (TEST INFRASTRUCTURE ONLY; built and run by
// tests/test_chain_cpu.py with the recipe of chain_emu.mk).
//
//   chain_emu DIR
// DIR/cases.txt: one case per line "case index layout min_len max_anchors max_occ band reads"; DIR/<index>.col_pml
// is the index and DIR/<index>.col_loc its samples; DIR/<reads>.fa the reads as FASTA and DIR/<reads>.bin their raw
// dump (u64 n_reads, u64 read_off[n_reads + 1], the bases).  Per case the driver runs colbwt_chain_file on the
// FASTA (-> DIR/<case>.chains), then colbwt_chain_device over host arrays of the exact sizes the header asks for,
// filled with garbage first -- without and with an order array (reads by decreasing length) --, colbwt_chain_batch,
// and colbwt_anchors_device followed by colbwt_chain_reduce_device over its arrays; all must agree byte for byte.
// The records go to DIR/<case>.out.
// DIR/slots.txt: one handcrafted set per line "name n_reads max_anchors max_occ band"; DIR/<name>.slots holds start
// (u32), len (u32) and pos (u64) of every slot; colbwt_chain_reduce_device runs over them on the first case's index
// and the records go to DIR/<name>.out.  Then the argument errors on the first case's index and, when DIR/many.col_pml
// and .col_loc exist (an index of more than 4096 documents), that limit's.
// Prints CHAIN-EMU-OK at the end; any mismatch ends it with exit status 1.
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
    fprintf(stderr, "chain_emu: %s (last error: %s)\n", what.c_str(), colbwt_last_error());
    exit(1);
}

static std::vector<uint8_t> slurp(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) die("cannot read " + path);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
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

static void write_records(const std::string &path, const Aligned &chain) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) die("cannot create " + path);
    if (chain.bytes && fwrite(chain.p, 1, chain.bytes, f) != chain.bytes) die("short write");
    fclose(f);
}

static void run_case(const std::string &dir, const std::string &name, const std::string &index, int layout, uint32_t min_len,
                     uint32_t K, uint32_t M, uint32_t band, const std::string &reads_stem) {
    colbwt_index *h = open_index(dir + "/" + index, layout, true);
    colbwt_stats st;
    if (colbwt_chain_file(h, (dir + "/" + reads_stem + ".fa").c_str(), (dir + "/" + name + ".chains").c_str(), min_len, K, M, band, 0, &st) !=
        COLBWT_OK)
        die("colbwt_chain_file " + name);

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

    const uint64_t work_bytes = colbwt_chain_work_bytes(n, K, M);
    Aligned plain(16, 32 * n), ordered(16, 32 * n), host(16, 32 * n), reduced(16, 32 * n);
    {
        Aligned work(256, work_bytes);
        if (colbwt_chain_device(h, bases.as<uint8_t>(), off.as<uint64_t>(), n, r.n_bases, min_len, K, M, band, plain.as<colbwt_chain>(),
                                work.p, nullptr, nullptr, &st) != COLBWT_OK || st.n_reads != n)
            die("colbwt_chain_device " + name);
    }
    {
        Aligned work(256, work_bytes);
        if (colbwt_chain_device(h, bases.as<uint8_t>(), off.as<uint64_t>(), n, r.n_bases, min_len, K, M, band, ordered.as<colbwt_chain>(),
                                work.p, order.as<uint32_t>(), nullptr, &st) != COLBWT_OK || st.n_reads != n)
            die("colbwt_chain_device with d_order " + name);
    }
    if (!plain.same(ordered)) die("d_order changes the results of " + name);
    if (colbwt_chain_batch(h, r.bases.data(), r.off.data(), n, min_len, K, M, band, host.as<colbwt_chain>(), &st) != COLBWT_OK ||
        st.n_reads != n)
        die("colbwt_chain_batch " + name);
    if (!host.same(plain)) die("colbwt_chain_batch differs from the device form: " + name);
    {
        Aligned summary(16, 32 * n), start(4, 4 * n * K), len(4, 4 * n * K), occ(8, 8 * n * K), pos(8, 8 * n * K * M);
        if (colbwt_anchors_device(h, bases.as<uint8_t>(), off.as<uint64_t>(), n, r.n_bases, min_len, K, M, summary.as<colbwt_anchor_summary>(),
                                  start.as<uint32_t>(), len.as<uint32_t>(), occ.as<uint64_t>(), pos.as<uint64_t>(), nullptr, nullptr,
                                  nullptr) != COLBWT_OK)
            die("colbwt_anchors_device " + name);
        if (colbwt_chain_reduce_device(h, start.as<uint32_t>(), len.as<uint32_t>(), pos.as<uint64_t>(), n, K, M, band,
                                       reduced.as<colbwt_chain>(), nullptr, &st) != COLBWT_OK || st.n_reads != n)
            die("colbwt_chain_reduce_device " + name);
    }
    if (!reduced.same(plain)) die("colbwt_chain_reduce_device over the anchors' arrays differs from colbwt_chain_device: " + name);
    write_records(dir + "/" + name + ".out", plain);
    colbwt_index_close(h);
    printf("ok %s: %llu reads, layout %d, min_len %u, max_anchors %u, max_occ %u, band %u\n", name.c_str(), (unsigned long long)n, layout,
           min_len, K, M, band);
}

static void run_slots(const std::string &dir, colbwt_index *h, const std::string &name, uint64_t n, uint32_t K, uint32_t M, uint32_t band) {
    const std::vector<uint8_t> raw = slurp(dir + "/" + name + ".slots");
    if (raw.size() != n * K * (8 + 8 * (uint64_t)M)) die("bad slot dump " + name);
    Aligned start(4, 4 * n * K), len(4, 4 * n * K), pos(8, 8 * n * K * M), chain(16, 32 * n);
    memcpy(start.p, raw.data(), 4 * n * K);
    memcpy(len.p, raw.data() + 4 * n * K, 4 * n * K);
    memcpy(pos.p, raw.data() + 8 * n * K, 8 * n * K * M);
    if (colbwt_chain_reduce_device(h, start.as<uint32_t>(), len.as<uint32_t>(), pos.as<uint64_t>(), n, K, M, band, chain.as<colbwt_chain>(),
                                   nullptr, nullptr) != COLBWT_OK)
        die("colbwt_chain_reduce_device " + name);
    write_records(dir + "/" + name + ".out", chain);
    printf("ok %s: %llu handcrafted reads, max_anchors %u, max_occ %u, band %u\n", name.c_str(), (unsigned long long)n, K, M, band);
}

static void arg_errors(const std::string &dir, const std::string &index, int layout, const std::string &reads_stem) {
    const char *no_samples = "no locate samples attached (colbwt_index_attach_locate)";
    const char *min0 = "min_len must be at least 1", *k0 = "max_anchors must be at least 1", *m0 = "max_occ must be at least 1";
    const char *big = "max_anchors * max_occ must be at most 256", *many = "more than 2^32-2 reads in a batch";
    const std::string fa = dir + "/" + reads_stem + ".fa", stem = dir + "/" + index;
    const Reads r = load_reads(dir + "/" + reads_stem + ".bin");
    const uint64_t n = r.n;
    const uint32_t K = 3, M = 2, B = 8;
    colbwt_index *h = open_index(stem, layout, false);
    Aligned bases(64, r.n_bases + 64), start(4, 4 * n * K), len(4, 4 * n * K), pos(8, 8 * n * K * M), chain(16, 32 * n);
    Aligned work(256, colbwt_chain_work_bytes(n, K, M));
    memset(bases.p, 0, r.n_bases + 64);
    if (r.n_bases) memcpy(bases.p, r.bases.data(), r.n_bases);
    memset(start.p, 0xFF, start.bytes);          // no used slot
    const uint8_t *b = bases.as<uint8_t>();
    const uint64_t *o = r.off.data();
    uint32_t *as = start.as<uint32_t>(), *al = len.as<uint32_t>();
    uint64_t *ap = pos.as<uint64_t>();
    colbwt_chain *ch = chain.as<colbwt_chain>();
    auto red = [&](colbwt_index *x, const uint32_t *ps, const uint32_t *pl, const uint64_t *pp, uint64_t cnt, uint32_t k, uint32_t m,
                   colbwt_chain *pc) { return colbwt_chain_reduce_device(x, ps, pl, pp, cnt, k, m, B, pc, nullptr, nullptr); };
    auto dev = [&](colbwt_index *x, const uint8_t *pb, uint64_t cnt, uint32_t l, uint32_t k, uint32_t m, colbwt_chain *pc, void *pw) {
        return colbwt_chain_device(x, pb, o, cnt, r.n_bases, l, k, m, B, pc, pw, nullptr, nullptr, nullptr);
    };
    auto bat = [&](colbwt_index *x, const uint8_t *pb, const uint64_t *po, uint64_t cnt, uint32_t l, uint32_t k, uint32_t m,
                   colbwt_chain *pc) { return colbwt_chain_batch(x, pb, po, cnt, l, k, m, B, pc, nullptr); };
    auto fil = [&](colbwt_index *x, const char *p, uint32_t l, uint32_t k, uint32_t m) {
        return colbwt_chain_file(x, p, (dir + "/never.chains").c_str(), l, k, m, B, 0, nullptr);
    };
    expect(red(nullptr, as, al, ap, n, K, M, ch), COLBWT_ERR_ARG, "null index", "reduce/null index");
    expect(dev(nullptr, b, n, 1, K, M, ch, work.p), COLBWT_ERR_ARG, "null index", "device/null index");
    expect(bat(nullptr, b, o, n, 1, K, M, ch), COLBWT_ERR_ARG, "null index", "batch/null index");
    expect(fil(nullptr, fa.c_str(), 1, K, M), COLBWT_ERR_ARG, "null argument", "file/null index");
    expect(fil(h, nullptr, 1, K, M), COLBWT_ERR_ARG, "null argument", "file/null pattern");
    // the parameters come before the samples, the samples before anything about the pointers
    expect(dev(h, b, n, 0, K, M, ch, work.p), COLBWT_ERR_ARG, min0, "device/min_len 0");
    expect(bat(h, b, o, n, 0, K, M, ch), COLBWT_ERR_ARG, min0, "batch/min_len 0");
    expect(fil(h, fa.c_str(), 0, K, M), COLBWT_ERR_ARG, min0, "file/min_len 0");
    struct Bad { uint32_t k, m; const char *msg; };
    for (const Bad &bad : {Bad{0, M, k0}, Bad{K, 0, m0}, Bad{257, 1, big}, Bad{1, 257, big}, Bad{129, 2, big}, Bad{1u << 31, 2, big},
                           Bad{0xFFFFFFFFu, 0xFFFFFFFFu, big}}) {
        expect(red(h, as, al, ap, n, bad.k, bad.m, ch), COLBWT_ERR_ARG, bad.msg, "reduce/limits");
        expect(dev(h, b, n, 1, bad.k, bad.m, ch, work.p), COLBWT_ERR_ARG, bad.msg, "device/limits");
        expect(bat(h, b, o, n, 1, bad.k, bad.m, ch), COLBWT_ERR_ARG, bad.msg, "batch/limits");
        expect(fil(h, fa.c_str(), 1, bad.k, bad.m), COLBWT_ERR_ARG, bad.msg, "file/limits");
    }
    expect(red(h, nullptr, nullptr, nullptr, n, K, M, nullptr), COLBWT_ERR_ARG, no_samples, "reduce/no samples");
    expect(dev(h, nullptr, n, 1, K, M, nullptr, nullptr), COLBWT_ERR_ARG, no_samples, "device/no samples");
    expect(bat(h, nullptr, o, n, 1, K, M, nullptr), COLBWT_ERR_ARG, no_samples, "batch/no samples");
    expect(fil(h, fa.c_str(), 1, K, M), COLBWT_ERR_ARG, no_samples, "file/no samples");
    if (colbwt_index_attach_locate(h, stem.c_str()) != COLBWT_OK) die("attach");
    // no reads: nothing is looked at
    expect(red(h, nullptr, nullptr, nullptr, 0, K, M, nullptr), COLBWT_OK, nullptr, "reduce/no reads");
    expect(dev(h, nullptr, 0, 1, K, M, nullptr, nullptr), COLBWT_OK, nullptr, "device/no reads");
    expect(bat(h, nullptr, nullptr, 0, 1, K, M, nullptr), COLBWT_OK, nullptr, "batch/no reads");
    // pointers and alignment
    expect(red(h, as, al, ap, 0xFFFFFFFFull, K, M, ch), COLBWT_ERR_ARG, many, "reduce/too many reads");
    expect(dev(h, b, 0xFFFFFFFFull, 1, K, M, ch, work.p), COLBWT_ERR_ARG, many, "device/too many reads");
    expect(bat(h, b, o, 0xFFFFFFFFull, 1, K, M, ch), COLBWT_ERR_ARG, many, "batch/too many reads");
    const char *null_dev = "null device pointer";
    const char *red_al = "d_start/d_len must be 4-byte aligned, d_pos 8-byte and d_chain 16-byte aligned";
    expect(red(h, nullptr, al, ap, n, K, M, ch), COLBWT_ERR_ARG, null_dev, "reduce/null start");
    expect(red(h, as, nullptr, ap, n, K, M, ch), COLBWT_ERR_ARG, null_dev, "reduce/null len");
    expect(red(h, as, al, nullptr, n, K, M, ch), COLBWT_ERR_ARG, null_dev, "reduce/null pos");
    expect(red(h, as, al, ap, n, K, M, nullptr), COLBWT_ERR_ARG, null_dev, "reduce/null chain");
    expect(red(h, (uint32_t *)((uint8_t *)as + 2), al, ap, n, K, M, ch), COLBWT_ERR_ARG, red_al, "reduce/start alignment");
    expect(red(h, as, (uint32_t *)((uint8_t *)al + 1), ap, n, K, M, ch), COLBWT_ERR_ARG, red_al, "reduce/len alignment");
    expect(red(h, as, al, (uint64_t *)((uint8_t *)ap + 4), n, K, M, ch), COLBWT_ERR_ARG, red_al, "reduce/pos alignment");
    expect(red(h, as, al, ap, n, K, M, (colbwt_chain *)((uint8_t *)ch + 8)), COLBWT_ERR_ARG, red_al, "reduce/chain alignment");
    expect(dev(h, nullptr, n, 1, K, M, ch, work.p), COLBWT_ERR_ARG, null_dev, "device/null bases");
    expect(dev(h, b, n, 1, K, M, nullptr, work.p), COLBWT_ERR_ARG, null_dev, "device/null chain");
    expect(dev(h, b, n, 1, K, M, ch, nullptr), COLBWT_ERR_ARG, null_dev, "device/null work");
    expect(dev(h, b + 1, n, 1, K, M, ch, work.p), COLBWT_ERR_ARG, "d_bases/d_chain must be 16-byte aligned", "device/bases alignment");
    expect(dev(h, b, n, 1, K, M, (colbwt_chain *)((uint8_t *)ch + 8), work.p), COLBWT_ERR_ARG, "d_bases/d_chain must be 16-byte aligned",
           "device/chain alignment");
    expect(dev(h, b, n, 1, K, M, ch, (uint8_t *)work.p + 128), COLBWT_ERR_ARG, "d_work must be 256-byte aligned", "device/work alignment");
    expect(bat(h, b, nullptr, n, 1, K, M, ch), COLBWT_ERR_ARG, "null read_off", "batch/null read_off");
    expect(bat(h, nullptr, o, n, 1, K, M, ch), COLBWT_ERR_ARG, "null bases/chain", "batch/null bases");
    expect(bat(h, b, o, n, 1, K, M, nullptr), COLBWT_ERR_ARG, "null bases/chain", "batch/null chain");
    expect(red(h, as, al, ap, n, K, M, ch), COLBWT_OK, nullptr, "reduce");
    for (uint64_t k = 0; k < n; ++k)
        if (ch[k].text_begin != COLBWT_LOCATE_NONE || ch[k].text_len || ch[k].read_begin || ch[k].read_end || ch[k].score || ch[k].score2 ||
            ch[k].n_chained || ch[k].n_hits)
            die("a read without a used slot has a chain");
    expect(dev(h, b, n, 1, K, M, ch, work.p), COLBWT_OK, nullptr, "device");
    // file form
    expect(fil(h, (dir + "/no_such_reads.fa").c_str(), 1, K, M), COLBWT_ERR_IO,
           ("cannot open pattern file " + dir + "/no_such_reads.fa").c_str(), "file/missing pattern");
    colbwt_index_close(h);
    // DIR/many: an index of more than 4096 documents is refused right after the samples check, before any pointer
    const std::string many_stem = dir + "/many";
    if (std::ifstream(many_stem + ".col_pml")) {
        const char *too_many = "more than 4096 documents";
        colbwt_index *m = open_index(many_stem, layout, true);
        if (colbwt_docs_mask_words(m) <= 64) die("DIR/many holds no more than 4096 documents");
        expect(red(m, nullptr, al, ap, n, K, M, ch), COLBWT_ERR_ARG, too_many, "reduce/too many documents before null start");
        expect(red(m, nullptr, nullptr, nullptr, 0, K, M, nullptr), COLBWT_ERR_ARG, too_many, "reduce/too many documents, no reads");
        expect(red(m, as, al, ap, n, 257, 1, ch), COLBWT_ERR_ARG, big, "reduce/limits before too many documents");
        expect(dev(m, nullptr, n, 1, K, M, ch, work.p), COLBWT_ERR_ARG, too_many, "device/too many documents before null bases");
        expect(bat(m, b, o, n, 1, K, M, ch), COLBWT_ERR_ARG, too_many, "batch/too many documents");
        expect(fil(m, fa.c_str(), 1, K, M), COLBWT_ERR_ARG, too_many, "file/too many documents");
        colbwt_index_close(m);
        printf("ok more than 4096 documents are refused\n");
    }
    printf("ok argument errors of colbwt_chain_reduce_device / _device / _batch / _file\n");
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: chain_emu DIR\n");
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
        uint32_t min_len = 0, K = 0, M = 0, band = 0;
        if (!(in >> name >> index >> layout >> min_len >> K >> M >> band >> reads)) continue;
        run_case(dir, name, index, layout, min_len, K, M, band, reads);
        if (n_cases++ == 0) {
            first_index = index;
            first_reads = reads;
            first_layout = layout;
        }
    }
    if (n_cases == 0) die("no cases");
    std::ifstream slots(dir + "/slots.txt");
    if (slots) {
        colbwt_index *h = open_index(dir + "/" + first_index, first_layout, true);
        while (std::getline(slots, line)) {
            std::istringstream in(line);
            std::string name;
            uint64_t n = 0;
            uint32_t K = 0, M = 0, band = 0;
            if (!(in >> name >> n >> K >> M >> band)) continue;
            run_slots(dir, h, name, n, K, M, band);
        }
        colbwt_index_close(h);
    }
    arg_errors(dir, first_index, first_layout, first_reads);
    printf("CHAIN-EMU-OK\n");
    return 0;
}
