"""GPU tier of locate (include/colbwt.h colbwt_locate_*): the locate kernel on the MI355X against a
brute-force locator over sorted suffixes (tests/locate_restatement.py) on real BWT indexes in every
layout, through every entry point, and the whole chain `col-bwt build --locate` -> `col-bwt locate`."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import locate_restatement as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = (1, 2, 3, 4, 5, 6, 0)

pytestmark = pytest.mark.gpu


def _check(label, reads, got, want, max_occ, none):
    mlen, occ, pos = got
    for i, (wm, wo, wp) in enumerate(want):
        k = min(int(occ[i]), max_occ)
        g = (int(mlen[i]), int(occ[i]), [int(x) for x in pos[i, :k]])
        assert g == (wm, wo, wp), f"{label}: read {i} {bytes(reads[i])[:40]!r}: {g} != {(wm, wo, wp)}"
        assert (pos[i, k:] == none).all(), f"{label}: read {i}: slots past k"


def _true_index(seed, size=700):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    a = rng.choice(acgt, size=size).tobytes()
    seqs = [a, a[200:500], rng.choice(acgt, size=500).tobytes(), b"ACGT" * 30, a[:100]]
    return helpers.true_bwt_index(seqs, seed=seed, extra_splits=80)


def _reads(text, seed):
    body = text[:-1]
    reads = [bytes(r) for r in helpers.reads_from_text(text, 150, (1, 120), 0.01, seed=seed, extra=b"Nn")]
    reads += [body, b"", b"N", b"ACGT" * 31, body[:7] + b"\x01" + body[7:20], body[-40:]]
    return reads


def test_locate_equals_brute_force_every_layout(pkg):
    img, text = _true_index(2)
    loc = lr.samples(text)
    ref = lr.Locator(text)
    reads = _reads(text, 5)
    bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
    for layout in LAYOUTS:
        tbl = pkg.ColPml.from_bytes(img, layout=layout)
        tbl.attach_locate(data=loc)
        cm, co, _, _ = tbl.count_batch(bases, off)
        for k in (1, 3, 1000):
            mlen, occ, pos, _ = tbl.locate_batch(bases, off, k)
            _check(f"L{layout}/k{k}", reads, (mlen, occ, pos), [ref.locate(r, k) for r in reads], k, pkg.LOCATE_NONE)
            clean = np.array([all(b > 1 for b in r) for r in reads])
            assert np.array_equal(mlen[clean], cm[clean]) and np.array_equal(occ[clean], co[clean])
        assert tbl.locate(text[:-1], 4)[:2] == (len(text) - 1, 1)
        tbl.close()


def test_locate_large_text_with_repeats(pkg):
    """~1 Mchar text of repeats (occ in the hundreds), a seeded sample of reads, AUTO layout."""
    rng = np.random.default_rng(17)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    unit = rng.choice(acgt, size=4000)
    parts = []
    for _ in range(250):
        s = unit.copy()
        mut = rng.random(s.size) < 0.003
        s[mut] = rng.choice(acgt, size=int(mut.sum()))
        parts.append(s.tobytes())
    img, text = helpers.true_bwt_index_large(parts, seed=3)
    sa = lr.suffix_array(text)
    loc = lr.samples(text, sa)
    ref = lr.Locator(text, sa)
    reads = [bytes(r) for r in helpers.reads_from_text(text, 300, (10, 150), 0.002, seed=19)]
    bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
    tbl = pkg.ColPml.from_bytes(img)
    tbl.attach_locate(data=loc)
    for k in (1, 64, 1000):
        mlen, occ, pos, _ = tbl.locate_batch(bases, off, k)
        _check(f"large/k{k}", reads, (mlen, occ, pos), [ref.locate(r, k) for r in reads], k, pkg.LOCATE_NONE)
    assert int(occ.max()) >= 100, int(occ.max())
    tbl.close()


def test_locate_device_with_and_without_order(pkg):
    import torch
    dev = torch.device("cuda", 0)
    img, text = _true_index(4, size=1500)
    reads = [np.frombuffer(bytes(r), np.uint8) for r in helpers.reads_from_text(text, 300, (0, 300), 0.005, seed=6)]
    bases, off = helpers.concat_reads(reads)
    lens = np.diff(off.astype(np.int64))
    d_bases = torch.zeros(len(bases) + 128, dtype=torch.uint8, device=dev)
    d_bases[:len(bases)] = torch.from_numpy(bases)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    order = torch.from_numpy(np.argsort(-lens, kind="stable").astype(np.int32)).to(dev)
    k = 8
    for layout in (1, 3, 5, 0):
        tbl = pkg.ColPml.from_bytes(img, layout=layout)
        tbl.attach_locate(data=lr.samples(text))
        want = tbl.locate_batch(bases, off, k)[:3]
        for d_order in (None, order.data_ptr()):
            d_mlen = torch.zeros(len(reads), dtype=torch.int32, device=dev)
            d_occ = torch.zeros(len(reads), dtype=torch.int64, device=dev)
            d_pos = torch.zeros(len(reads) * k, dtype=torch.int64, device=dev)
            st = tbl.locate_device(d_bases.data_ptr(), d_off.data_ptr(), len(reads), len(bases), k, d_mlen.data_ptr(),
                                   d_occ.data_ptr(), d_pos.data_ptr(), d_order, timed=True)
            assert st.n_reads == len(reads)
            got = (d_mlen.cpu().numpy().view(np.uint32), d_occ.cpu().numpy().view(np.uint64),
                   d_pos.cpu().numpy().view(np.uint64).reshape(len(reads), k))
            for g, w in zip(got, want):
                assert np.array_equal(g, w), (layout, d_order is not None)
        tbl.close()


def test_locate_two_replicas_match_one(pkg):
    img, text = _true_index(9)
    reads = [np.frombuffer(bytes(r), np.uint8) for r in helpers.reads_from_text(text, 2000, (1, 100), 0.01, seed=2)]
    reads += [np.zeros(0, np.uint8)] * 3
    bases, off = helpers.concat_reads(reads)
    loc = lr.samples(text)
    one = pkg.ColPml.from_bytes(img)
    two = pkg.ColPml.from_bytes(img, devices=[0, 0])
    one.attach_locate(data=loc)
    two.attach_locate(data=loc)
    a = one.locate_batch(bases, off, 5)
    b = two.locate_batch(bases, off, 5)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    assert b[3].n_reads == len(reads)
    one.close()
    two.close()


def test_col_bwt_build_locate_then_locate_equals_brute_force(tmp_path):
    """`col-bwt build -r --locate` on three FASTA documents of two records, then `col-bwt locate`:
    every line equals the brute-force locator over the collection's text as oracle/rlbwt_oracle.py
    lays it out, doc:offset strings included; the build without --locate writes no .col_loc and
    leaves the index byte-identical."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import rlbwt_oracle as ro
    rng = np.random.default_rng(12)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    base = rng.choice(acgt, size=1500)
    docs, paths = [], []
    for k in range(3):
        recs = []
        for j in range(2):
            s = base[j * 300:j * 300 + 900].copy()
            mut = rng.random(s.size) < 0.02
            s[mut] = rng.choice(acgt, size=int(mut.sum()))
            recs.append(s)
        docs.append([r.tobytes() for r in recs])
        paths.append(str(tmp_path / f"g{k}.fa"))
        helpers.write_fasta(paths[-1], recs, [f"g{k}_{j}" for j in range(2)])
    launcher = [sys.executable, os.path.join(ROOT, "col-bwt_amd", "col-bwt")]
    outp = str(tmp_path / "coll")
    out = subprocess.run(launcher + ["build", "-r", "--locate", "-l", "20", "-o", outp] + paths, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    plain = str(tmp_path / "plain")
    out = subprocess.run(launcher + ["build", "-r", "-l", "20", "-o", plain] + paths, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert not os.path.exists(plain + ".col_loc")
    assert open(plain + ".col_pml", "rb").read() == open(outp + ".col_pml", "rb").read()
    text, starts = ro.build_text(docs, revcomp=True)
    assert open(outp + ".col_loc", "rb").read() == lr.samples(text, doc_start=starts)
    ref = lr.Locator(text)
    reads = [bytes(r) for r in helpers.reads_from_text(text, 200, (5, 150), 0.01, seed=13)]
    reads += [docs[0][0][:300], docs[1][1][-200:][::-1], b"NNNN"]
    names = [f"p{k}" for k in range(len(reads))]
    fa = str(tmp_path / "reads.fa")
    helpers.write_fasta(fa, [np.frombuffer(r, np.uint8) for r in reads], names)
    out = subprocess.run(launcher + ["locate", "-p", fa, "-k", "5", outp], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = open(fa + ".locate").read().split("\n")
    assert lines[-1] == "" and len(lines) == len(reads) + 1
    for line, rd, nm in zip(lines, reads, names):
        mlen, occ, pos = ref.locate(rd, 5)
        hits = ",".join("%d:%d" % lr.doc_offset(p, starts) for p in pos)
        assert line == f"{nm}\t{len(rd)}\t{mlen}\t{occ}\t{hits}", line
    bad = subprocess.run(launcher + ["locate", "-p", fa, plain], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0            # no samples beside that index


def test_locate_calls_do_not_leak_hbm(pkg):
    import torch
    img, text = _true_index(11)
    loc = lr.samples(text)
    reads = [np.frombuffer(bytes(r), np.uint8) for r in helpers.reads_from_text(text, 500, (1, 100), 0.01, seed=3)]
    bases, off = helpers.concat_reads(reads)
    tbl = pkg.ColPml.from_bytes(img)
    tbl.attach_locate(data=loc)
    tbl.locate_batch(bases, off, 16)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        tbl.attach_locate(data=loc)
        tbl.locate_batch(bases, off, 16)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] >= free0 - (64 << 20)
    tbl.close()
