"""GPU tier at pangenome scale: construction, count, locate and PML queries on one collection whose
text (with reverse complements) holds more than 2^25 characters, checked against the fast numpy
reference (tests/sa_reference.py, itself pinned to oracle/rlbwt_oracle.py by
tests/test_sa_reference.py) and, for the suffix array, against the text itself.

The collection (fixed seed): 33 documents of about 520 kbp, copies of one base sequence with 0.1 %
substitutions and a few short indels; documents 0 and 1 identical (LCPs of about the document
length: 18+ doubling rounds and as many rank levels); some documents of several records
(separators inside a document); a 120 kbp homopolymer in one document (a BWT run longer than
65535, the len16 escape of the table); a 5 kbp run of N in one and short ones in others (runs of
a rare character millions of positions apart: the block path of the threshold pass); 33 > 32
documents (a second word of document flags per multi-MUM window).

Measured on an MI355X host: the whole module in 41 s, 33 s of it the CPU reference (n = 34 320 163,
r = 1 018 246 runs, 18 doubling rounds, longest run 119 989, 11 774 multi-MUMs, largest occ of a
read without separators 119 982).  The first run found runs longer than the 16-bit offset field of
the table cut by the builder.
"""
import os
import sys

import numpy as np
import pytest

import helpers
import sa_reference as sr
import seeds_restatement as seeds_rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import rlbwt_oracle as ro  # noqa: E402

pytestmark = pytest.mark.gpu

LAYOUTS = (1, 2, 3, 4, 5, 6, 0)
ACGT = np.frombuffer(b"ACGT", np.uint8)
N_DOCS = 33
DOC_LEN = 520_000
MIN_MUM = 20
POLY_DOC, POLY_AT, POLY_LEN = 4, 200_000, 120_000      # documents of one record (d % 3 != 2)
NRUN_DOC, NRUN_AT, NRUN_LEN = 9, 300_000, 5_000


def pangenome_docs(seed=2025):
    """-> list of documents, each a list of records (bytes)."""
    rng = np.random.default_rng(seed)
    base = rng.choice(ACGT, size=DOC_LEN)
    docs = []
    for d in range(N_DOCS):
        if d == 1:
            docs.append(list(docs[0]))                              # identical to document 0
            continue
        s = base.copy()
        mut = rng.random(DOC_LEN) < 0.001
        s[mut] = rng.choice(ACGT, size=int(mut.sum()))
        if d == POLY_DOC:
            s[POLY_AT:POLY_AT + POLY_LEN] = ord("A")
        if d == NRUN_DOC:
            s[NRUN_AT:NRUN_AT + NRUN_LEN] = ord("N")
        elif d % 4 == 3:
            for at in rng.integers(0, DOC_LEN - 50, size=3):
                s[at:at + int(rng.integers(1, 40))] = ord("N")
        s = s.tobytes()
        for _ in range(int(rng.integers(1, 4))):                    # a few short indels, away from the homopolymer
            at = int(rng.integers(0, 150_000))
            if rng.random() < 0.5:
                s = s[:at] + s[at + int(rng.integers(1, 6)):]
            else:
                s = s[:at] + rng.choice(ACGT, size=int(rng.integers(1, 6))).tobytes() + s[at:]
        records = int(rng.integers(1, 4)) if d % 3 == 2 else 1
        cuts = sorted(rng.choice(np.arange(1000, len(s) - 1000), size=records - 1, replace=False).tolist())
        docs.append([s[a:b] for a, b in zip([0] + cuts, cuts + [len(s)])])
    return docs


def _reads(text, doc_start, docs, seed=7):
    """About 3000 reads: exact substrings, 1 % substitutions, the homopolymer and its edges, the N
    stretch and separators, the identical pair."""
    rng = np.random.default_rng(seed)
    t = np.frombuffer(text, np.uint8)
    n = t.size

    def sub(a, m):
        a = int(min(max(a, 0), n - 1 - m))
        return t[a:a + m].tobytes()
    reads = [sub(rng.integers(0, n), int(rng.integers(20, 301))) for _ in range(1200)]
    for _ in range(800):
        r = np.frombuffer(sub(rng.integers(0, n), int(rng.integers(20, 301))), np.uint8).copy()
        mut = rng.random(r.size) < 0.01
        r[mut] = rng.choice(ACGT, size=int(mut.sum()))
        reads.append(r.tobytes())
    poly = text.find(b"A" * POLY_LEN)
    assert poly >= doc_start[POLY_DOC]
    for _ in range(300):
        m = int(rng.integers(20, 301))
        reads.append(sub(poly + rng.integers(0, POLY_LEN - m), m))                  # inside: occ ~ 1e5
    for edge in (poly, poly + POLY_LEN):
        for _ in range(100):
            m = int(rng.integers(20, 301))
            reads.append(sub(edge - rng.integers(1, m), m))                        # across an edge
    nrun = text.find(b"N" * NRUN_LEN)
    assert nrun >= doc_start[NRUN_DOC]
    for edge in (nrun, nrun + NRUN_LEN):
        for _ in range(100):
            m = int(rng.integers(20, 301))
            reads.append(sub(edge - rng.integers(-m // 2, m), m))                  # ending in or crossing the Ns
    seps = np.flatnonzero(t <= 1)
    for at in rng.choice(seps[:-1], size=200):
        m = int(rng.integers(20, 301))
        reads.append(sub(at - rng.integers(-m // 2, m), m))                        # ending in or crossing a separator
    for at in rng.choice(seps[:-1], size=20):
        reads.append(sub(at - 29, 30))                                            # ending with one: mlen 0
    pair = doc_start[1] - doc_start[0]
    for _ in range(200):
        m = int(rng.integers(20, 301))
        reads.append(sub(rng.integers(0, pair - m), m))                           # from the identical pair
    return reads


@pytest.fixture(scope="module")
def pan(tmp_path_factory):
    docs = pangenome_docs()
    text, doc_start = ro.build_text(docs, revcomp=True)
    assert len(text) >= 1 << 25
    ref = sr.build(text, doc_start, MIN_MUM)
    ref["docs"] = docs
    ref["loc"] = sr.samples(text, ref["sa"], doc_start)
    ref["dir"] = tmp_path_factory.mktemp("pangenome")
    reads = _reads(text, doc_start, docs)
    ref["reads"] = reads
    loc = sr.Locator(text, ref["sa"])
    ref["want"], ref["want_sp"] = [], []
    for r in reads:
        mlen, sp, ep1 = loc.search(r)
        ref["want"].append((mlen, ep1 - sp, ref["sa"][max(sp, ep1 - 1000):ep1][::-1].tolist()))
        ref["want_sp"].append(sp)
    return ref


def _check_construction(got, ref):
    assert got["n"] == len(ref["text"])
    assert np.array_equal(got["heads"], ref["heads"])
    assert np.array_equal(got["lens"], ref["lens"])
    bad = np.flatnonzero(got["thr"] != ref["thr"].astype(np.uint64))
    assert bad.size == 0, ("thr", bad[:5], got["thr"][bad[:5]], ref["thr"][bad[:5]])
    mums = list(zip(got["mum_len"].tolist(), got["mum_pos"].tolist()))
    assert len(mums) == len(ref["mums"]) and mums == ref["mums"]


def test_construction_from_text(pkg, pan):
    path = str(pan["dir"] / "text.col_loc")
    got = pkg.rlbwt_from_text(pan["text"], pan["doc_start"], min_mum=MIN_MUM, locate_path=path)
    _check_construction(got, pan)
    assert open(path, "rb").read() == pan["loc"]
    # the collection is what it claims to be
    assert got["rounds"] == pan["rounds"] and got["rounds"] >= 15, got["rounds"]
    assert int(got["lens"].max()) > 65535
    assert got["n_docs"] == N_DOCS > 32
    assert len(pan["mums"]) > 1000
    print(f"\npangenome: n {got['n']} r {got['heads'].size} rounds {got['rounds']} longest run {int(got['lens'].max())} "
          f"mums {len(pan['mums'])} phi samples {(len(pan['loc']) - 40 - 4 * got['heads'].size - 4 * N_DOCS) // 8}")


def test_construction_from_fasta_files(pkg, pan):
    paths = []
    for d, records in enumerate(pan["docs"]):
        p = str(pan["dir"] / f"doc{d}.fa")
        helpers.write_fasta(p, [np.frombuffer(r, np.uint8) for r in records], [f"doc{d}_{k}" for k in range(len(records))], width=80)
        paths.append(p)
    prefix = str(pan["dir"] / "files")
    got = pkg.rlbwt_from_fastas(paths, prefix, min_mum=MIN_MUM, revcomp=True, locate=True)
    _check_construction(got, pan)
    for ext, want in zip((".bwt.heads", ".bwt.len", ".thr_pos", ".col_mums"), ro.file_bytes(pan, N_DOCS)):
        assert open(prefix + ext, "rb").read() == want, ext
    assert open(prefix + ".col_loc", "rb").read() == pan["loc"]


def test_reference_suffix_array_against_the_text(pan):
    """About 1e5 random neighbouring suffixes: the reference LCP bytes are equal, the next one ascends."""
    text, sa, lcp = pan["text"], pan["sa"], pan["lcp"]
    rng = np.random.default_rng(5)
    ks = rng.integers(1, len(text), size=100_000)
    ks = np.concatenate((ks, np.argsort(lcp)[-200:]))                # and the longest LCPs
    for k in ks.tolist():
        a, b, l = int(sa[k - 1]), int(sa[k]), int(lcp[k])
        assert text[a:a + l] == text[b:b + l], k
        assert b + l < len(text) and (a + l == len(text) or text[a + l] < text[b + l]), k
    assert int(lcp.max()) >= 500_000


@pytest.fixture(scope="module")
def image(pkg, oracle, pan):
    """col_split + build_col_pml on the device / host product == the C oracle: the index image."""
    heads, lens = pan["heads"].astype(np.uint8), pan["lens"].astype(np.uint64)
    mlen = np.array([m[0] for m in pan["mums"]], np.uint64)
    mpos = np.array([m[1] for m in pan["mums"]], np.uint64)
    pos, ids, n = pkg.col_split_arrays(heads, lens, mlen, mpos, N_DOCS, "tunnels", 2)
    epos, eids, en, _ = oracle.col_split(heads, lens, mlen, mpos, N_DOCS, "tunnels", 2)
    assert n == en == len(pan["text"])
    assert np.array_equal(pos, epos) and np.array_equal(ids, eids)
    img = pkg.build_col_pml_arrays(heads, lens, ids, pos, pan["thr"].astype(np.uint64))
    assert np.array_equal(img, oracle.build_col_pml(heads, lens, eids, epos, pan["thr"].astype(np.uint64)))
    return img


def _check_positions(text, read, mlen, pos):
    """Every reported position starts the read's last mlen bytes (independent of any suffix array)."""
    if not mlen or not len(pos):
        return True
    t = np.frombuffer(text, np.uint8)
    tail = np.frombuffer(read[len(read) - mlen:], np.uint8)
    at = np.asarray(pos, np.int64)[:, None] + np.arange(mlen)
    return bool((at < t.size).all() and (t[np.minimum(at, t.size - 1)] == tail).all())


def test_count_and_locate_every_layout(pkg, pan, image):
    reads, want = pan["reads"], pan["want"]
    bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
    clean = np.array([len(r) > 0 and min(r) > 1 for r in reads])
    w_mlen = np.array([w[0] for w in want], np.uint32)
    w_occ = np.array([w[1] for w in want], np.uint64)
    w_sp = np.array(pan["want_sp"], np.uint64)
    assert int(w_occ[clean].max()) >= 100_000 and (w_mlen == 0).any() and (~clean).any()
    print(f"\nreads {len(reads)}, largest occ {int(w_occ.max())}, of a read without separators {int(w_occ[clean].max())}")
    for layout in LAYOUTS:
        tbl = pkg.ColPml.from_bytes(image, layout=layout)
        tbl.attach_locate(data=pan["loc"])
        mlen, occ, sp, _ = tbl.count_batch(bases, off, want_sp=True)
        for name, g, w in (("mlen", mlen, w_mlen), ("occ", occ, w_occ), ("sp", sp, w_sp)):
            bad = np.flatnonzero(clean & (g != w))
            assert bad.size == 0, (layout, "count", name, bad[:5], g[bad[:5]], w[bad[:5]])
        for k in (1, 16, 1000):
            mlen, occ, pos, _ = tbl.locate_batch(bases, off, k)
            assert np.array_equal(mlen, w_mlen), (layout, k, np.flatnonzero(mlen != w_mlen)[:5])
            assert np.array_equal(occ, w_occ), (layout, k, np.flatnonzero(occ != w_occ)[:5])
            for i, (wm, wo, wp) in enumerate(want):
                q = min(wo, k)
                assert pos[i, :q].tolist() == wp[:q], (layout, k, i, pos[i, :q][:8], wp[:8])
                assert (pos[i, q:] == pkg.LOCATE_NONE).all(), (layout, k, i)
                assert _check_positions(pan["text"], reads[i], wm, pos[i, :q]), (layout, k, i)
        tbl.close()


def test_pml_every_layout(pkg, oracle, pan, image):
    reads = [r for r in pan["reads"] if len(r) and min(r) > 1][::2][:1000]
    bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
    ep, ec = oracle.OracleIndex(image).query_batch(bases, off)
    assert int(ep.max()) >= 200
    for layout in LAYOUTS:
        tbl = pkg.ColPml.from_bytes(image, layout=layout)
        p, c, _ = tbl.query_batch(bases, off)
        tbl.close()
        assert np.array_equal(p, ep), (layout, np.flatnonzero(p != ep)[:5])
        assert np.array_equal(c, ec), (layout, np.flatnonzero(c != ec)[:5])


def test_seeds_every_layout(pkg, oracle, pan, image):
    """seeds_batch on the reads of test_pml_every_layout == the restatement applied to the oracle's PML
    and col ids, in every layout.  The col ids of this index come from real multi-MUM chains, so the
    chain fields (n_col, asc, desc) see ids no synthetic table gives them."""
    reads = [r for r in pan["reads"] if len(r) and min(r) > 1][::2][:1000]
    bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
    ep, ec = oracle.OracleIndex(image).query_batch(bases, off)
    params = ((1, 1000), (20, 8), (16, 16))
    wants = {p: seeds_rs.seeds(ep, ec, off, *p) for p in params}
    for p in params:
        seeds_rs.check_invariants(*wants[p][:3], off, *p)
    for field, name in ((4, "n_col"), (6, "asc"), (7, "desc")):
        assert any((wants[p][0][:, field] > 0).any() for p in params), f"{name} > 0 occurs in the sample"
    s = wants[(16, 16)][0]
    print(f"\nseeds (16, 16): reads with n_col > 0 {int((s[:, 4] > 0).sum())}, asc > 0 {int((s[:, 6] > 0).sum())}, "
          f"desc > 0 {int((s[:, 7] > 0).sum())} of {len(reads)}")
    for layout in LAYOUTS:
        tbl = pkg.ColPml.from_bytes(image, layout=layout)
        for p in params:
            summary, pos, ln, sc, st = tbl.seeds_batch(bases, off, *p)
            assert st.n_reads == len(reads) and st.n_bases == int(off[-1])
            for name, g, w in zip(("summary", "seed_pos", "seed_len", "seed_cid"), (summary.view(np.uint32).reshape(-1, 8), pos, ln, sc),
                                  wants[p]):
                bad = np.argwhere(g != w)
                assert bad.size == 0, (layout, p, name, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
        tbl.close()
