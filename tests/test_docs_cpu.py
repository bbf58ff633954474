"""CPU tier of docs (include/colbwt.h colbwt_docs_*): the restatement (tests/docs_restatement.py)
against a scan of the text, and the three entry points compiled with the product sources against the
SIMT emulator into a stand-alone program under ASan/UBSan (tests/emu/docs_emu_main.cpp, built by
tests/emu/docs_emu.mk), whose outputs are compared with the restatement byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

import docs_restatement as dr
import helpers
import locate_restatement as lr

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import rlbwt_oracle  # noqa: E402

LINE_ROWS_4 = 4 | (4 << 8)          # include/colbwt.h COLBWT_LAYOUT_LINE_ROWS_STEPS(4)


def _scan_docs(text, doc_start, pattern):
    """{d : some p in document d has text[p:p+len(pattern)] == pattern}, by scanning the text."""
    found = set()
    p = text.find(pattern)
    while p >= 0:
        found.add(max(d for d, s in enumerate(doc_start) if s <= p))
        p = text.find(pattern, p + 1)
    return sorted(found)


def _check_against_scan(text, doc_start, reads, min_len):
    ref = dr.Docs(text, doc_start)
    got = ref.batch(reads, min_len, 1 << 30)
    mlen, occ, n_hit, mask, doc_reads, doc_only = got
    want_reads = np.zeros(len(doc_start), np.uint64)
    want_only = np.zeros(len(doc_start), np.uint64)
    for k, rd in enumerate(reads):
        rd = bytes(rd)
        L = int(mlen[k])
        want = _scan_docs(text, doc_start, rd[len(rd) - L:]) if L >= max(min_len, 1) else []
        assert dr.mask_docs(mask[k]) == want, (k, rd[:40])
        assert int(n_hit[k]) == len(want)
        if L:
            assert int(occ[k]) == sum(1 for p in range(len(text)) if text[p:p + L] == rd[len(rd) - L:])
        for d in want:
            want_reads[d] += np.uint64(1)
            if len(want) == 1:
                want_only[d] += np.uint64(1)
    assert np.array_equal(doc_reads, want_reads) and np.array_equal(doc_only, want_only)
    assert mask.shape == (len(reads), (len(doc_start) + 63) // 64)
    return got


@pytest.mark.parametrize("revcomp", [False, True])
def test_restatement_equals_scan_on_a_multi_document_text(revcomp):
    rng = np.random.default_rng(31)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    base = rng.choice(acgt, size=160)
    docs = []
    for d in range(4):
        recs = []
        for j in range(2):
            s = base[j * 30:j * 30 + 90 + 10 * d].copy()
            mut = rng.random(s.size) < 0.03
            s[mut] = rng.choice(acgt, size=int(mut.sum()))
            recs.append(s.tobytes())
        docs.append(recs)
    text, starts = rlbwt_oracle.build_text(docs, revcomp=revcomp)
    reads = [bytes(r) for r in helpers.reads_from_text(text, 80, (1, 50), 0.02, seed=8, extra=b"N")]
    reads += [docs[1][0], b"", b"N", docs[2][1][:20] + b"\x01" + docs[2][1][20:30]]
    for min_len in (1, 12):
        got = _check_against_scan(text, starts, reads, min_len)
    assert int(got[2].max()) >= 2          # reads shared by several documents are among them


@pytest.mark.parametrize("n_docs", [1, 5, 64, 65, 130])
def test_restatement_equals_scan_with_invented_documents(n_docs):
    rng = np.random.default_rng(5)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    a = rng.choice(acgt, size=300).tobytes()
    img, text = helpers.true_bwt_index([a, a[50:200], b"ACGT" * 20, a[:60]], seed=1)
    starts = dr.invented_cuts(len(text), n_docs, seed=n_docs)
    assert len(starts) == n_docs and starts[0] == 0 and len(set(starts)) == n_docs
    reads = [bytes(r) for r in helpers.reads_from_text(text, 60, (1, 40), 0.02, seed=9, extra=b"N")]
    reads += [text[:-1], b"", b"ACGT" * 21, b"A"]
    got = _check_against_scan(text, starts, reads, 1)
    assert int(got[2].max()) >= min(n_docs, 3)
    # formatting: ascending document numbers, an empty last field without hits
    line = dr.docs_line("r", 4, 2, 7, [0, 3, 64])
    assert line == "r\t4\t2\t7\t3\t0,3,64" and dr.docs_line("e", 0, 0, 0, []) == "e\t0\t0\t0\t0\t"
    assert dr.tally_file([3, 0], [1, 0]) == "0\t3\t1\n1\t0\t0\n"


def _emu_inputs(tmp):
    """Index images, sample files, FASTA files and raw read dumps of the emulator cases -> the case list."""
    rng = np.random.default_rng(2)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    a = rng.choice(acgt, size=260).tobytes()
    seqs = [a, a[60:200], rng.choice(acgt, size=150).tobytes(), b"ACGT" * 25, a[:70]]
    img, text = helpers.true_bwt_index(seqs, seed=6, extra_splits=40)
    body = text[:-1]
    starts = {5: [int(x) for x in np.cumsum([0] + [len(s) for s in seqs[:-1]])], 130: dr.invented_cuts(len(text), 130, seed=3)}
    sa = lr.suffix_array(text)
    refs = {}
    for n_docs, ds in starts.items():
        stem = os.path.join(tmp, f"d{n_docs}")
        open(stem + ".col_pml", "wb").write(bytes(img))
        open(stem + ".col_loc", "wb").write(lr.samples(text, sa, ds))
        refs[n_docs] = dr.Docs(text, ds, sa)
    special = [body,                                       # the whole text
               b"",                                        # empty
               b"N" + body[:6], body[10:30] + b"N",        # N at either end
               body[:5] + b"\x01" + body[5:25],            # a byte <= 1 ends the search
               body[3:9] + b"\x00",                        # ... also as the last byte
               b"ACGT" * 26, body[-8:], b"A"]
    sampled = [bytes(r) for r in helpers.reads_from_text(text, 248, (1, 60), 0.02, seed=4, extra=b"N")]
    read_sets = {257: sampled + special, 63: special + sampled[:54], 1: [body[100:140]]}
    fasta_sets = {}
    for n, reads in read_sets.items():
        assert len(reads) == n
        bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
        with open(os.path.join(tmp, f"reads{n}.bin"), "wb") as f:
            f.write(np.uint64(n).tobytes() + off.tobytes() + bases.tobytes())
        fasta_sets[n] = [(f"r{k}", r) for k, r in enumerate(reads) if all(b >= 32 for b in r)]   # what a FASTA line can hold
        helpers.write_fasta(os.path.join(tmp, f"reads{n}.fa"), [np.frombuffer(r, np.uint8) for _, r in fasta_sets[n]],
                            [nm for nm, _ in fasta_sets[n]])
    cases = []
    for layout in (2, LINE_ROWS_4):
        for n_docs in (5, 130):
            for min_len in (1, 12):
                for max_walk in (1, 3, 1000):
                    cases.append((layout, n_docs, min_len, max_walk, 257))
    for layout, n_docs in ((2, 130), (LINE_ROWS_4, 5)):
        for n in (1, 63):
            for max_walk in (3, 1000):
                cases.append((layout, n_docs, 1, max_walk, n))
    # more than 4096 documents: an argument error (the driver looks for DIR/many)
    unit = rng.choice(acgt, size=1500).tobytes()
    img_m, text_m = helpers.true_bwt_index_large([unit, unit[:1400], unit[100:1500], rng.choice(acgt, size=1000).tobytes()], seed=2)
    open(os.path.join(tmp, "many.col_pml"), "wb").write(bytes(img_m))
    open(os.path.join(tmp, "many.col_loc"), "wb").write(lr.samples(text_m, doc_start=dr.invented_cuts(len(text_m), 4097, seed=1)))
    with open(os.path.join(tmp, "cases.txt"), "w") as f:
        for k, (layout, n_docs, min_len, max_walk, n) in enumerate(cases):
            f.write(f"c{k} d{n_docs} {layout} {min_len} {max_walk} reads{n}\n")
    return cases, refs, read_sets, fasta_sets


def test_emulated_docs_equal_restatement_under_asan(tmp_path):
    """colbwt_docs_file and one colbwt_docs_device call per case in a stand-alone sanitized program:
    layouts 2 and 4, min_len 1 / 12, max_walk 1 / 3 / 1000, 5 and 130 documents, reads with N, a byte
    <= 1, an empty read and the whole text, 1 / 63 / 257 reads; then the argument errors, an index
    of 4097 documents among them."""
    tmp = str(tmp_path)
    exe = os.path.join(HERE, "emu", "docs_emu")
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu"), "-f", "docs_emu.mk", "docs_emu"], stdout=subprocess.DEVNULL)
    cases, refs, read_sets, fasta_sets = _emu_inputs(tmp)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe, tmp], env=env, capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and "DOCS-EMU-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert "ok more than 4096 documents are refused" in out.stdout
    assert (refs[130].batch(read_sets[257], 1, 1000)[3][:, 1:] != 0).any()   # words past the first are in use
    for k, (layout, n_docs, min_len, max_walk, n) in enumerate(cases):
        ref, label = refs[n_docs], f"c{k} {(layout, n_docs, min_len, max_walk, n)}"
        mlen, occ, n_hit, mask, doc_reads, doc_only = ref.batch(read_sets[n], min_len, max_walk)
        want = mlen.tobytes() + occ.tobytes() + n_hit.tobytes() + mask.tobytes() + (doc_reads + np.uint64(1000)).tobytes() \
            + (doc_only + np.uint64(1000)).tobytes()
        assert open(os.path.join(tmp, f"c{k}.out"), "rb").read() == want, label
        names, reads = [nm for nm, _ in fasta_sets[n]], [r for _, r in fasta_sets[n]]
        res = ref.batch(reads, min_len, max_walk)
        assert open(os.path.join(tmp, f"c{k}.docs")).read() == dr.docs_file(names, reads, res), label
        assert open(os.path.join(tmp, f"c{k}.docs.tally")).read() == dr.tally_file(res[4], res[5]), label
