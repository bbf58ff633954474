// tests/emu/docs_emu_main.cpp -- stand-alone driver of colbwt_docs_* compiled with the product sources
// against the SIMT emulator under ASan/UBSan (TEST INFRASTRUCTURE ONLY; built and run by
// tests/test_docs_cpu.py with the recipe of docs_emu.mk).
//
//   docs_emu DIR
// DIR/cases.txt: one case per line "case index layout min_len max_walk reads"; DIR/<index>.col_pml and
// .col_loc are the index, DIR/<reads>.fa the reads as FASTA and DIR/<reads>.bin their raw dump
// (u64 n_reads, u64 read_off[n_reads + 1], the bases).  Per case the driver runs colbwt_docs_file on the
// FASTA (-> DIR/<case>.docs and .docs.tally) and ONE colbwt_docs_device call on host arrays of the
// exact sizes the header asks for, whose raw outputs go to DIR/<case>.out: mlen, occ, n_hit, mask,
// doc_reads, doc_only (the tallies start at kTallyStart: the device form adds).  Then the argument
// errors of the three entry points.  Prints DOCS-EMU-OK at the end; any mismatch of a return code or
// message ends it with exit status 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/colbwt.h"

static const uint64_t kTallyStart = 1000;

static void die(const std::string &what) {
    fprintf(stderr, "docs_emu: %s (last error: %s)\n", what.c_str(), colbwt_last_error());
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

static void run_case(const std::string &dir, const std::string &name, const std::string &index, int layout, uint32_t min_len,
                     uint32_t max_walk, const std::string &reads_stem) {
    colbwt_index *h = open_index(dir + "/" + index, layout, true);
    const std::string out = dir + "/" + name + ".docs";
    colbwt_stats st;
    if (colbwt_docs_file(h, (dir + "/" + reads_stem + ".fa").c_str(), out.c_str(), min_len, max_walk, 0, &st) != COLBWT_OK)
        die("colbwt_docs_file " + name);

    const Reads r = load_reads(dir + "/" + reads_stem + ".bin");
    uint32_t n_docs = 0;
    colbwt_locate_docs(h, nullptr, 0, &n_docs);
    const uint32_t W = colbwt_docs_mask_words(h);
    if (W != (n_docs + 63) / 64) die("colbwt_docs_mask_words");
    Aligned bases(64, r.n_bases + 64), off(8, 8 * (r.n + 1)), mlen(4, 4 * r.n), occ(8, 8 * r.n), n_hit(4, 4 * r.n),
        mask(8, 8 * r.n * W), doc_reads(8, 8 * (size_t)n_docs), doc_only(8, 8 * (size_t)n_docs),
        work(256, colbwt_docs_work_bytes(r.n));
    if (r.n_bases) memcpy(bases.p, r.bases.data(), r.n_bases);
    memcpy(off.p, r.off.data(), 8 * (r.n + 1));
    memset(mask.p, 0xAB, 8 * r.n * W);                     // the call owns every word of the masks
    memset(n_hit.p, 0xAB, 4 * r.n);
    for (uint32_t d = 0; d < n_docs; ++d) ((uint64_t *)doc_reads.p)[d] = ((uint64_t *)doc_only.p)[d] = kTallyStart;
    if (colbwt_docs_device(h, (const uint8_t *)bases.p, (const uint64_t *)off.p, r.n, r.n_bases, min_len, max_walk, (uint32_t *)mlen.p,
                           (uint64_t *)occ.p, (uint32_t *)n_hit.p, (uint64_t *)mask.p, (uint64_t *)doc_reads.p, (uint64_t *)doc_only.p,
                           work.p, nullptr, nullptr, &st) != COLBWT_OK)
        die("colbwt_docs_device " + name);
    if (st.n_reads != r.n) die("stats of colbwt_docs_device " + name);
    FILE *f = fopen((dir + "/" + name + ".out").c_str(), "wb");
    if (!f) die("cannot create the raw output of " + name);
    put(f, (const uint32_t *)mlen.p, r.n);
    put(f, (const uint64_t *)occ.p, r.n);
    put(f, (const uint32_t *)n_hit.p, r.n);
    put(f, (const uint64_t *)mask.p, r.n * W);
    put(f, (const uint64_t *)doc_reads.p, n_docs);
    put(f, (const uint64_t *)doc_only.p, n_docs);
    fclose(f);
    colbwt_index_close(h);
    printf("ok %s: %llu reads, %u documents, layout %d, min_len %u, max_walk %u\n", name.c_str(), (unsigned long long)r.n, n_docs,
           layout, min_len, max_walk);
}

static void expect(int rc, int want, const char *msg, const char *what) {
    if (rc != want || (msg && strcmp(colbwt_last_error(), msg) != 0))
        die(std::string(what) + ": got " + std::to_string(rc) + " \"" + colbwt_last_error() + "\", expected " + std::to_string(want) +
            " \"" + (msg ? msg : "") + "\"");
}

// Code and message of every argument error, in the order the entry points check them: locate's checks
// (parameter range, samples, pointers, alignment) first, the new ones after them.
static void arg_errors(const std::string &dir, const std::string &index, int layout, const std::string &reads_stem) {
    const char *no_samples = "no locate samples attached (colbwt_index_attach_locate)";
    const std::string fa = dir + "/" + reads_stem + ".fa", stem = dir + "/" + index;
    const Reads r = load_reads(dir + "/" + reads_stem + ".bin");
    colbwt_index *h = open_index(stem, layout, false);
    if (colbwt_docs_mask_words(h) != 0 || colbwt_docs_mask_words(nullptr) != 0) die("mask words without samples");
    Aligned bases(64, r.n_bases + 64), mlen(4, 4 * r.n), occ(8, 8 * r.n), n_hit(4, 4 * r.n), mask(8, 8 * r.n * 4),
        work(256, colbwt_docs_work_bytes(r.n));
    const uint8_t *b = (const uint8_t *)bases.p;
    const uint64_t *o = r.off.data();
    uint32_t *ml = (uint32_t *)mlen.p, *nh = (uint32_t *)n_hit.p;
    uint64_t *oc = (uint64_t *)occ.p, *mk = (uint64_t *)mask.p;
    auto dev = [&](colbwt_index *x, const uint8_t *pb, const uint64_t *po, uint64_t n, uint32_t l, uint32_t w, uint32_t *pm, uint64_t *pc,
                   uint32_t *ph, uint64_t *pk, uint64_t *pr, uint64_t *pn, void *pw) {
        return colbwt_docs_device(x, pb, po, n, r.n_bases, l, w, pm, pc, ph, pk, pr, pn, pw, nullptr, nullptr, nullptr);
    };
    // the parameter range comes before the samples, the samples before anything about the reads
    expect(colbwt_docs_batch(nullptr, b, o, r.n, 1, 1, ml, oc, nh, mk, nullptr, nullptr, nullptr), COLBWT_ERR_ARG, "null index", "batch/null index");
    expect(dev(nullptr, b, o, r.n, 1, 1, ml, oc, nh, mk, nullptr, nullptr, work.p), COLBWT_ERR_ARG, "null index", "device/null index");
    expect(colbwt_docs_file(nullptr, fa.c_str(), nullptr, 1, 1, 0, nullptr), COLBWT_ERR_ARG, "null argument", "file/null index");
    expect(colbwt_docs_file(h, nullptr, nullptr, 1, 1, 0, nullptr), COLBWT_ERR_ARG, "null argument", "file/null pattern");
    for (int form = 0; form < 3; ++form) {
        auto call = [&](uint32_t l, uint32_t w) {
            if (form == 0) return colbwt_docs_batch(h, b, o, r.n, l, w, ml, oc, nh, mk, nullptr, nullptr, nullptr);
            if (form == 1) return dev(h, b, o, r.n, l, w, ml, oc, nh, mk, nullptr, nullptr, work.p);
            return colbwt_docs_file(h, fa.c_str(), nullptr, l, w, 0, nullptr);
        };
        expect(call(0, 0), COLBWT_ERR_ARG, "min_len must be at least 1", "min_len 0");
        expect(call(1, 0), COLBWT_ERR_ARG, "max_walk must be 1 .. 2^20", "max_walk 0");
        expect(call(1, (1u << 20) + 1), COLBWT_ERR_ARG, "max_walk must be 1 .. 2^20", "max_walk 2^20 + 1");
        expect(call(1, 1u << 20), COLBWT_ERR_ARG, no_samples, "no samples");
    }
    if (colbwt_index_attach_locate(h, stem.c_str()) != COLBWT_OK) die("attach");
    // no reads: any pointer is fine, the host form still writes its (zero) totals
    uint32_t n_docs = 0;
    colbwt_locate_docs(h, nullptr, 0, &n_docs);
    std::vector<uint64_t> tally_v(2 * (size_t)n_docs + 1, 9);
    uint64_t *tally = tally_v.data();
    expect(colbwt_docs_batch(h, nullptr, nullptr, 0, 1, 1, nullptr, nullptr, nullptr, nullptr, tally, tally + n_docs, nullptr), COLBWT_OK, nullptr, "batch/no reads");
    for (uint32_t d = 0; d < 2 * n_docs; ++d)
        if (tally[d] != 0) die("the host form must write the totals of an empty call");
    if (tally[2 * n_docs] != 9) die("the host form wrote past its tallies");
    expect(dev(h, nullptr, nullptr, 0, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), COLBWT_OK, nullptr, "device/no reads");
    // host form; a failing call leaves the caller's tallies as they were
    for (uint32_t d = 0; d < 2 * n_docs; ++d) tally[d] = 7;
    expect(colbwt_docs_batch(h, b, nullptr, r.n, 1, 1, ml, oc, nh, mk, tally, tally + n_docs, nullptr), COLBWT_ERR_ARG, "null read_off", "batch/null read_off");
    expect(colbwt_docs_batch(h, b, o, r.n, 1, 1, ml, oc, nh, nullptr, tally, tally + n_docs, nullptr), COLBWT_ERR_ARG, "null bases/mlen/occ/n_hit/mask", "batch/null mask with tallies");
    for (uint32_t d = 0; d < 2 * n_docs; ++d)
        if (tally[d] != 7) die("a failing colbwt_docs_batch changed the caller's tallies");
    expect(colbwt_docs_batch(h, nullptr, o, r.n, 1, 1, ml, oc, nh, mk, nullptr, nullptr, nullptr), COLBWT_ERR_ARG, "null bases/mlen/occ/n_hit/mask", "batch/null bases");
    expect(colbwt_docs_batch(h, b, o, r.n, 1, 1, ml, oc, nullptr, mk, nullptr, nullptr, nullptr), COLBWT_ERR_ARG, "null bases/mlen/occ/n_hit/mask", "batch/null n_hit");
    expect(colbwt_docs_batch(h, b, o, r.n, 1, 1, ml, oc, nh, nullptr, nullptr, nullptr, nullptr), COLBWT_ERR_ARG, "null bases/mlen/occ/n_hit/mask", "batch/null mask");
    expect(colbwt_docs_batch(h, b, o, 0xFFFFFFFFull, 1, 1, ml, oc, nh, mk, nullptr, nullptr, nullptr), COLBWT_ERR_ARG, "more than 2^32-2 reads in a batch", "batch/too many reads");
    // device form: locate's pointer and alignment checks, then the new ones
    const char *null_ptr = "null device pointer", *align1 = "d_bases must be 16-byte aligned, d_mlen 4-byte and d_occ 8-byte aligned";
    const char *null_new = "null d_n_hit/d_mask/d_work", *align2 = "d_n_hit must be 4-byte aligned, d_mask/d_doc_reads/d_doc_only 8-byte aligned";
    expect(dev(h, nullptr, o, r.n, 1, 1, ml, oc, nullptr, mk, nullptr, nullptr, work.p), COLBWT_ERR_ARG, null_ptr, "device/null bases before null n_hit");
    expect(dev(h, b, o, r.n, 1, 1, nullptr, oc, nh, mk, nullptr, nullptr, work.p), COLBWT_ERR_ARG, null_ptr, "device/null mlen");
    expect(dev(h, b + 1, o, r.n, 1, 1, ml, oc, nh, nullptr, nullptr, nullptr, work.p), COLBWT_ERR_ARG, align1, "device/bases alignment before null mask");
    expect(dev(h, b, o, r.n, 1, 1, ml, (uint64_t *)((uint8_t *)oc + 4), nh, mk, nullptr, nullptr, work.p), COLBWT_ERR_ARG, align1, "device/occ alignment");
    expect(dev(h, b, o, 0xFFFFFFFFull, 1, 1, ml, oc, nullptr, mk, nullptr, nullptr, work.p), COLBWT_ERR_ARG, "more than 2^32-2 reads in a batch", "device/too many reads before null n_hit");
    expect(dev(h, b, o, r.n, 1, 1, ml, oc, nullptr, mk, nullptr, nullptr, work.p), COLBWT_ERR_ARG, null_new, "device/null n_hit");
    expect(dev(h, b, o, r.n, 1, 1, ml, oc, nh, nullptr, nullptr, nullptr, work.p), COLBWT_ERR_ARG, null_new, "device/null mask");
    expect(dev(h, b, o, r.n, 1, 1, ml, oc, nh, mk, nullptr, nullptr, nullptr), COLBWT_ERR_ARG, null_new, "device/null work");
    expect(dev(h, b, o, r.n, 1, 1, ml, oc, (uint32_t *)((uint8_t *)nh + 2), mk, nullptr, nullptr, (uint8_t *)work.p + 8), COLBWT_ERR_ARG, align2, "device/n_hit alignment before work alignment");
    expect(dev(h, b, o, r.n, 1, 1, ml, oc, nh, (uint64_t *)((uint8_t *)mk + 4), nullptr, nullptr, work.p), COLBWT_ERR_ARG, align2, "device/mask alignment");
    expect(dev(h, b, o, r.n, 1, 1, ml, oc, nh, mk, (uint64_t *)((uint8_t *)tally + 4), nullptr, work.p), COLBWT_ERR_ARG, align2, "device/doc_reads alignment");
    expect(dev(h, b, o, r.n, 1, 1, ml, oc, nh, mk, nullptr, (uint64_t *)((uint8_t *)tally + 4), work.p), COLBWT_ERR_ARG, align2, "device/doc_only alignment");
    expect(dev(h, b, o, r.n, 1, 1, ml, oc, nh, mk, nullptr, nullptr, (uint8_t *)work.p + 128), COLBWT_ERR_ARG, "d_work must be 256-byte aligned", "device/work alignment");
    // file form
    expect(colbwt_docs_file(h, (dir + "/no_such_reads.fa").c_str(), (dir + "/never.docs").c_str(), 1, 1, 0, nullptr), COLBWT_ERR_IO,
           ("cannot open pattern file " + dir + "/no_such_reads.fa").c_str(), "file/missing pattern");
    colbwt_index_close(h);
    // DIR/many: an index of more than 4096 documents is refused right after the samples check
    const std::string many = dir + "/many";
    if (std::ifstream(many + ".col_pml")) {
        const char *too_many = "more than 4096 documents";
        colbwt_index *m = open_index(many, layout, true);
        if (colbwt_docs_mask_words(m) <= 64) die("DIR/many holds no more than 4096 documents");
        expect(colbwt_docs_batch(m, b, o, r.n, 1, 1, ml, oc, nh, mk, nullptr, nullptr, nullptr), COLBWT_ERR_ARG, too_many, "batch/too many documents");
        expect(colbwt_docs_batch(m, b, o, r.n, 1, 0, ml, oc, nh, mk, nullptr, nullptr, nullptr), COLBWT_ERR_ARG, "max_walk must be 1 .. 2^20", "batch/max_walk before too many documents");
        expect(dev(m, nullptr, o, r.n, 1, 1, ml, oc, nh, mk, nullptr, nullptr, work.p), COLBWT_ERR_ARG, too_many, "device/too many documents before null bases");
        expect(dev(m, nullptr, nullptr, 0, 1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), COLBWT_ERR_ARG, too_many, "device/too many documents, no reads");
        expect(colbwt_docs_file(m, fa.c_str(), (dir + "/never.docs").c_str(), 1, 1, 0, nullptr), COLBWT_ERR_ARG, too_many, "file/too many documents");
        colbwt_index_close(m);
        printf("ok more than 4096 documents are refused\n");
    }
    printf("ok argument errors of colbwt_docs_batch / _device / _file\n");
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: docs_emu DIR\n");
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
        uint32_t min_len = 0, max_walk = 0;
        if (!(in >> name >> index >> layout >> min_len >> max_walk >> reads)) continue;
        run_case(dir, name, index, layout, min_len, max_walk, reads);
        if (n_cases++ == 0) {
            first_index = index;
            first_reads = reads;
            first_layout = layout;
        }
    }
    if (n_cases == 0) die("no cases");
    arg_errors(dir, first_index, first_layout, first_reads);
    printf("DOCS-EMU-OK\n");
    return 0;
}
