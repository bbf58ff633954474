// tests/emu/locate_all_emu_main.cpp -- stand-alone driver of colbwt_locate_all_* compiled with the product
// sources against the SIMT emulator under ASan/UBSan (TEST INFRASTRUCTURE ONLY; built and run by
// tests/test_locate_all_cpu.py with the recipe of locate_all_emu.mk, once per tile size).
//
//   locate_all_emu DIR
// DIR/cases.txt: one case per line "case index layout min_len max_per_read reads"; DIR/<index>.col_pml and
// .col_loc are the index, DIR/<reads>.fa the reads as FASTA and DIR/<reads>.bin their raw dump
// (u64 n_reads, u64 read_off[n_reads + 1], the bases).  Per case the driver runs colbwt_locate_all_file
// on the FASTA (-> DIR/<case>.locate), then plan + fill over host arrays of the exact sizes the header
// asks for -- whole, and as the two read ranges [0, n/2) and [n/2, n) into buffers of their own, which
// must hold the same positions -- and colbwt_locate_all_batch with its sizing call first.  The raw
// outputs of the whole fill go to DIR/<case>.out: mlen, occ, pos_off, pos.  Then the argument errors.
// Prints "tile <C>" first and LOCATE-ALL-EMU-OK at the end; any mismatch ends it with exit status 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/colbwt.h"

static void die(const std::string &what) {
    fprintf(stderr, "locate_all_emu: %s (last error: %s)\n", what.c_str(), colbwt_last_error());
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

// heap arrays of exactly the bytes asked for, so that ASan sees any access past them
struct Aligned {
    void *p = nullptr;
    Aligned(size_t align, size_t bytes) {
        const size_t padded = (bytes + align - 1) / align * align;
        p = aligned_alloc(align, padded ? padded : align);
        if (!p) die("out of memory");
        memset(p, 0, padded ? padded : align);
    }
    ~Aligned() { free(p); }
    template <typename T>
    T *as() const { return (T *)p; }
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

static const uint64_t kGuard = 0xABABABABABABABABull;

static void run_case(const std::string &dir, const std::string &name, const std::string &index, int layout, uint32_t min_len,
                     uint64_t max_per_read, const std::string &reads_stem) {
    colbwt_index *h = open_index(dir + "/" + index, layout, true);
    colbwt_stats st;
    if (colbwt_locate_all_file(h, (dir + "/" + reads_stem + ".fa").c_str(), (dir + "/" + name + ".locate").c_str(), min_len, max_per_read,
                               0, &st) != COLBWT_OK)
        die("colbwt_locate_all_file " + name);

    const Reads r = load_reads(dir + "/" + reads_stem + ".bin");
    const uint64_t n = r.n;
    Aligned bases(64, r.n_bases + 64), off(8, 8 * (n + 1)), mlen(4, 4 * n), occ(8, 8 * n), pos_off(8, 8 * (n + 1)),
        work(256, colbwt_locate_all_work_bytes(n));
    if (r.n_bases) memcpy(bases.p, r.bases.data(), r.n_bases);
    memcpy(off.p, r.off.data(), 8 * (n + 1));
    memset(pos_off.p, 0xAB, 8 * (n + 1));
    uint64_t total = ~0ull;
    if (colbwt_locate_all_plan_device(h, bases.as<uint8_t>(), off.as<uint64_t>(), n, r.n_bases, min_len, max_per_read, mlen.as<uint32_t>(),
                                      occ.as<uint64_t>(), pos_off.as<uint64_t>(), work.p, nullptr, nullptr, &total, &st) != COLBWT_OK)
        die("colbwt_locate_all_plan_device " + name);
    const uint64_t *po = pos_off.as<uint64_t>();
    if (st.n_reads != n || total != po[n] || po[0] != 0) die("plan: stats, total or pos_off[0] of " + name);
    // whole
    Aligned pos(8, 8 * total);
    memset(pos.p, 0xAB, 8 * total);
    if (colbwt_locate_all_fill_device(h, n, 0, n, po, pos.as<uint64_t>(), total, work.p, nullptr, &st) != COLBWT_OK)
        die("colbwt_locate_all_fill_device " + name);
    // two read ranges, each into a buffer of its own size
    const uint64_t cut[3] = {0, n / 2, n};
    for (int k = 0; k < 2; ++k) {
        const uint64_t cnt = po[cut[k + 1]] - po[cut[k]];
        Aligned part(8, 8 * cnt);
        memset(part.p, 0xAB, 8 * cnt);
        if (colbwt_locate_all_fill_device(h, n, cut[k], cut[k + 1], po, part.as<uint64_t>(), cnt, work.p, nullptr, nullptr) != COLBWT_OK)
            die("ranged colbwt_locate_all_fill_device " + name);
        if (cnt && memcmp(part.p, pos.as<uint64_t>() + po[cut[k]], 8 * cnt) != 0) die("a ranged fill differs from the whole fill: " + name);
    }
    // pos_cap below the need: nothing at or past pos_cap is written, the slots before it are the whole fill's
    if (total >= 2) {
        const uint64_t cap = total / 2;
        Aligned half(8, 8 * total);
        for (uint64_t k = 0; k < total; ++k) half.as<uint64_t>()[k] = kGuard;
        if (colbwt_locate_all_fill_device(h, n, 0, n, po, half.as<uint64_t>(), cap, work.p, nullptr, nullptr) != COLBWT_OK)
            die("capped colbwt_locate_all_fill_device " + name);
        if (memcmp(half.p, pos.p, 8 * cap) != 0) die("capped fill: slots below pos_cap differ: " + name);
        for (uint64_t k = cap; k < total; ++k)
            if (half.as<uint64_t>()[k] != kGuard) die("capped fill wrote at or past pos_cap: " + name);
    }
    // host form: the sizing call, then the call
    {
        std::vector<uint32_t> hm(n, 7);
        std::vector<uint64_t> ho(n, 7), hoff(n + 1, 7), hp(total + 1, kGuard);
        const int rc = colbwt_locate_all_batch(h, r.bases.data(), r.off.data(), n, min_len, max_per_read, hm.data(), ho.data(), hoff.data(),
                                               nullptr, 0, nullptr);
        if (total) expect(rc, COLBWT_ERR_ARG, "pos_cap too small", "batch/sizing call");
        else expect(rc, COLBWT_OK, nullptr, "batch/sizing call without positions");
        if (memcmp(hoff.data(), po, 8 * (n + 1)) != 0 || memcmp(hm.data(), mlen.p, 4 * n) != 0 || memcmp(ho.data(), occ.p, 8 * n) != 0)
            die("batch/sizing call: mlen, occ or pos_off differ from the plan's: " + name);
        if (total) {
            expect(colbwt_locate_all_batch(h, r.bases.data(), r.off.data(), n, min_len, max_per_read, hm.data(), ho.data(), hoff.data(),
                                           hp.data(), total - 1, nullptr), COLBWT_ERR_ARG, "pos_cap too small", "batch/pos_cap one short");
            if (hp[0] != kGuard) die("batch/pos_cap one short wrote positions: " + name);
        }
        expect(colbwt_locate_all_batch(h, r.bases.data(), r.off.data(), n, min_len, max_per_read, hm.data(), ho.data(), hoff.data(), hp.data(),
                                       total, &st), COLBWT_OK, nullptr, "batch");
        if (st.n_reads != n || hp[total] != kGuard || (total && memcmp(hp.data(), pos.p, 8 * total) != 0) ||
            memcmp(hoff.data(), po, 8 * (n + 1)) != 0)
            die("batch: positions differ from the device form's: " + name);
    }
    FILE *f = fopen((dir + "/" + name + ".out").c_str(), "wb");
    if (!f) die("cannot create the raw output of " + name);
    put(f, mlen.as<uint32_t>(), n);
    put(f, occ.as<uint64_t>(), n);
    put(f, po, n + 1);
    put(f, pos.as<uint64_t>(), total);
    fclose(f);
    colbwt_index_close(h);
    printf("ok %s: %llu reads, %llu positions, layout %d, min_len %u, max_per_read %llu\n", name.c_str(), (unsigned long long)n,
           (unsigned long long)total, layout, min_len, (unsigned long long)max_per_read);
}

static void arg_errors(const std::string &dir, const std::string &index, int layout, const std::string &reads_stem) {
    const char *no_samples = "no locate samples attached (colbwt_index_attach_locate)";
    const std::string fa = dir + "/" + reads_stem + ".fa", stem = dir + "/" + index;
    const Reads r = load_reads(dir + "/" + reads_stem + ".bin");
    const uint64_t n = r.n;
    colbwt_index *h = open_index(stem, layout, false);
    Aligned bases(64, r.n_bases + 64), mlen(4, 4 * n), occ(8, 8 * n), pos_off(8, 8 * (n + 1)), work(256, colbwt_locate_all_work_bytes(n));
    if (r.n_bases) memcpy(bases.p, r.bases.data(), r.n_bases);
    const uint8_t *b = bases.as<uint8_t>();
    const uint64_t *o = r.off.data();
    uint32_t *ml = mlen.as<uint32_t>();
    uint64_t *oc = occ.as<uint64_t>(), *po = pos_off.as<uint64_t>();
    uint64_t total = 0;
    auto plan = [&](colbwt_index *x, const uint8_t *pb, uint64_t cnt, uint32_t l, uint32_t *pm, uint64_t *pc, uint64_t *pp, void *pw) {
        return colbwt_locate_all_plan_device(x, pb, o, cnt, r.n_bases, l, 0, pm, pc, pp, pw, nullptr, nullptr, &total, nullptr);
    };
    if (colbwt_locate_all_tile() < 1 || colbwt_locate_all_work_bytes(n) % 256 != 0) die("tile / work bytes");
    expect(plan(nullptr, b, n, 1, ml, oc, po, work.p), COLBWT_ERR_ARG, "null index", "plan/null index");
    expect(colbwt_locate_all_fill_device(nullptr, n, 0, n, po, oc, 0, work.p, nullptr, nullptr), COLBWT_ERR_ARG, "null index", "fill/null index");
    expect(colbwt_locate_all_batch(nullptr, b, o, n, 1, 0, ml, oc, po, nullptr, 0, nullptr), COLBWT_ERR_ARG, "null index", "batch/null index");
    expect(colbwt_locate_all_file(nullptr, fa.c_str(), nullptr, 1, 0, 0, nullptr), COLBWT_ERR_ARG, "null argument", "file/null index");
    expect(colbwt_locate_all_file(h, nullptr, nullptr, 1, 0, 0, nullptr), COLBWT_ERR_ARG, "null argument", "file/null pattern");
    // min_len comes before the samples, the samples before anything about the reads
    const char *min0 = "min_len must be at least 1";
    expect(plan(h, b, n, 0, ml, oc, po, work.p), COLBWT_ERR_ARG, min0, "plan/min_len 0");
    expect(colbwt_locate_all_batch(h, b, o, n, 0, 0, ml, oc, po, nullptr, 0, nullptr), COLBWT_ERR_ARG, min0, "batch/min_len 0");
    expect(colbwt_locate_all_file(h, fa.c_str(), nullptr, 0, 0, 0, nullptr), COLBWT_ERR_ARG, min0, "file/min_len 0");
    expect(plan(h, nullptr, n, 1, ml, oc, po, work.p), COLBWT_ERR_ARG, no_samples, "plan/no samples");
    expect(colbwt_locate_all_fill_device(h, n, 0, n, po, oc, 0, work.p, nullptr, nullptr), COLBWT_ERR_ARG, no_samples, "fill/no samples");
    expect(colbwt_locate_all_batch(h, nullptr, o, n, 1, 0, ml, oc, po, nullptr, 0, nullptr), COLBWT_ERR_ARG, no_samples, "batch/no samples");
    expect(colbwt_locate_all_file(h, fa.c_str(), (dir + "/never.locate").c_str(), 1, 0, 0, nullptr), COLBWT_ERR_ARG, no_samples, "file/no samples");
    if (colbwt_index_attach_locate(h, stem.c_str()) != COLBWT_OK) die("attach");
    // no reads: the offsets are the single 0
    po[0] = 9;
    total = 9;
    expect(plan(h, nullptr, 0, 1, nullptr, nullptr, po, nullptr), COLBWT_OK, nullptr, "plan/no reads");
    if (po[0] != 0 || total != 0) die("plan/no reads: pos_off[0] and total must be 0");
    po[0] = 9;
    expect(colbwt_locate_all_batch(h, nullptr, nullptr, 0, 1, 0, nullptr, nullptr, po, nullptr, 0, nullptr), COLBWT_OK, nullptr, "batch/no reads");
    if (po[0] != 0) die("batch/no reads: pos_off[0] must be 0");
    expect(colbwt_locate_all_fill_device(h, 0, 0, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr), COLBWT_OK, nullptr, "fill/no reads");
    // pointers and alignment
    expect(plan(h, nullptr, n, 1, ml, oc, po, work.p), COLBWT_ERR_ARG, "null device pointer", "plan/null bases");
    expect(plan(h, b + 1, n, 1, ml, oc, po, work.p), COLBWT_ERR_ARG, "d_bases must be 16-byte aligned", "plan/bases alignment");
    expect(plan(h, b, 0xFFFFFFFFull, 1, ml, oc, po, work.p), COLBWT_ERR_ARG, "more than 2^32-2 reads in a batch", "plan/too many reads");
    expect(plan(h, b, n, 1, ml, oc, nullptr, work.p), COLBWT_ERR_ARG, "null d_pos_off/d_work", "plan/null pos_off");
    expect(plan(h, b, n, 1, ml, oc, po, nullptr), COLBWT_ERR_ARG, "null d_pos_off/d_work", "plan/null work");
    expect(plan(h, b, n, 1, ml, oc, (uint64_t *)((uint8_t *)po + 4), work.p), COLBWT_ERR_ARG, "d_pos_off must be 8-byte aligned", "plan/pos_off alignment");
    expect(plan(h, b, n, 1, ml, oc, po, (uint8_t *)work.p + 128), COLBWT_ERR_ARG, "d_work must be 256-byte aligned", "plan/work alignment");
    expect(plan(h, b, n, 1, ml, oc, po, work.p), COLBWT_OK, nullptr, "plan");
    expect(colbwt_locate_all_fill_device(h, n, 2, 1, po, oc, 0, work.p, nullptr, nullptr), COLBWT_ERR_ARG, "read_lo <= read_hi <= n_reads expected", "fill/range order");
    expect(colbwt_locate_all_fill_device(h, n, 0, n + 1, po, oc, 0, work.p, nullptr, nullptr), COLBWT_ERR_ARG, "read_lo <= read_hi <= n_reads expected", "fill/range end");
    expect(colbwt_locate_all_fill_device(h, n, 0, n, nullptr, oc, 0, work.p, nullptr, nullptr), COLBWT_ERR_ARG, "null d_pos_off/d_work", "fill/null pos_off");
    expect(colbwt_locate_all_fill_device(h, n, 0, n, po, nullptr, 1, work.p, nullptr, nullptr), COLBWT_ERR_ARG, "null d_pos with pos_cap > 0", "fill/null pos");
    expect(colbwt_locate_all_fill_device(h, n, 0, n, po, oc, 0, (uint8_t *)work.p + 128, nullptr, nullptr), COLBWT_ERR_ARG, "d_work must be 256-byte aligned", "fill/work alignment");
    expect(colbwt_locate_all_fill_device(h, n, 0, n, po, nullptr, 0, work.p, nullptr, nullptr), COLBWT_OK, nullptr, "fill/pos_cap 0 writes nothing");
    expect(colbwt_locate_all_fill_device(h, n, 1, 1, nullptr, nullptr, 0, nullptr, nullptr, nullptr), COLBWT_OK, nullptr, "fill/empty range");
    // host form
    expect(colbwt_locate_all_batch(h, b, nullptr, n, 1, 0, ml, oc, po, nullptr, 0, nullptr), COLBWT_ERR_ARG, "null read_off", "batch/null read_off");
    expect(colbwt_locate_all_batch(h, b, o, n, 1, 0, ml, oc, nullptr, nullptr, 0, nullptr), COLBWT_ERR_ARG, "null bases/mlen/occ/pos_off", "batch/null pos_off");
    expect(colbwt_locate_all_batch(h, b, o, n, 1, 0, ml, oc, po, nullptr, 5, nullptr), COLBWT_ERR_ARG, "null pos with pos_cap > 0", "batch/null pos");
    expect(colbwt_locate_all_batch(h, b, o, 0xFFFFFFFFull, 1, 0, ml, oc, po, nullptr, 0, nullptr), COLBWT_ERR_ARG, "more than 2^32-2 reads in a batch", "batch/too many reads");
    // file form
    expect(colbwt_locate_all_file(h, (dir + "/no_such_reads.fa").c_str(), (dir + "/never.locate").c_str(), 1, 0, 0, nullptr), COLBWT_ERR_IO,
           ("cannot open pattern file " + dir + "/no_such_reads.fa").c_str(), "file/missing pattern");
    colbwt_index_close(h);
    printf("ok argument errors of colbwt_locate_all_plan_device / _fill_device / _batch / _file\n");
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: locate_all_emu DIR\n");
        return 2;
    }
    const std::string dir = argv[1];
    printf("tile %u\n", colbwt_locate_all_tile());
    std::ifstream cases(dir + "/cases.txt");
    if (!cases) die("cannot read " + dir + "/cases.txt");
    std::string line, first_index, first_reads;
    int first_layout = 0, n_cases = 0;
    while (std::getline(cases, line)) {
        std::istringstream in(line);
        std::string name, index, reads;
        int layout = 0;
        uint32_t min_len = 0;
        uint64_t max_per_read = 0;
        if (!(in >> name >> index >> layout >> min_len >> max_per_read >> reads)) continue;
        run_case(dir, name, index, layout, min_len, max_per_read, reads);
        if (n_cases++ == 0) {
            first_index = index;
            first_reads = reads;
            first_layout = layout;
        }
    }
    if (n_cases == 0) die("no cases");
    arg_errors(dir, first_index, first_layout, first_reads);
    printf("LOCATE-ALL-EMU-OK\n");
    return 0;
}
