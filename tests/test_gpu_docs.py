"""GPU tier of docs (include/colbwt.h colbwt_docs_*): search, order, walk and tally on the MI355X
against the restatement (tests/docs_restatement.py) on real BWT indexes in every layout, through every
entry point, and the whole chain `col-bwt build --locate` -> `col-bwt docs`."""
import os
import subprocess
import sys

import numpy as np
import pytest

import docs_restatement as dr
import helpers
import locate_restatement as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = (1, 2, 3, 4, 5, 6, 0)

pytestmark = pytest.mark.gpu


def _true_index(seed, size=700):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    a = rng.choice(acgt, size=size).tobytes()
    seqs = [a, a[200:500], rng.choice(acgt, size=500).tobytes(), b"ACGT" * 30, a[:100]]
    img, text = helpers.true_bwt_index(seqs, seed=seed, extra_splits=80)
    return img, text, [int(x) for x in np.cumsum([0] + [len(s) for s in seqs[:-1]])]


def _reads(text, seed, n=150):
    body = text[:-1]
    reads = [bytes(r) for r in helpers.reads_from_text(text, n, (1, 120), 0.01, seed=seed, extra=b"Nn")]
    reads += [body, b"", b"N", b"ACGT" * 31, body[:7] + b"\x01" + body[7:20], body[-40:]]
    return reads


def _check(label, got, want):
    for name, g, w in zip(("mlen", "occ", "n_hit", "mask", "doc_reads", "doc_only"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (label, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1)) if g.size else []
        assert len(bad) == 0, f"{label}: {name} differs at {list(bad[:5])}: {g[bad[:3]]} != {w[bad[:3]]}"


def test_docs_equal_restatement_every_layout(pkg):
    img, text, five = _true_index(2)
    sa = lr.suffix_array(text)
    reads = _reads(text, 5)
    bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
    clean = np.array([all(b > 1 for b in r) for r in reads])
    for starts in (five, dr.invented_cuts(len(text), 130, seed=7)):
        loc = lr.samples(text, sa, starts)
        ref = dr.Docs(text, starts, sa)
        for layout in LAYOUTS:
            tbl = pkg.ColPml.from_bytes(img, layout=layout)
            tbl.attach_locate(data=loc)
            assert tbl.docs_mask_words() == (len(starts) + 63) // 64
            cm, co, _, _ = tbl.count_batch(bases, off)
            for min_len in (1, 12):
                for max_walk in (1, 3, 1000):
                    got = tbl.docs_batch(bases, off, min_len, max_walk)
                    _check(f"L{layout}/d{len(starts)}/l{min_len}/w{max_walk}", got[:6], ref.batch(reads, min_len, max_walk))
                    assert np.array_equal(got[0][clean], cm[clean]) and np.array_equal(got[1][clean], co[clean])
                    assert got[6].n_reads == len(reads)
            assert tbl.docs(text[:-1], 1, 4) == (len(text) - 1, 1, [0])
            tbl.close()


@pytest.mark.parametrize("n_docs", [64, 65])
def test_docs_word_boundary(pkg, n_docs):
    """Documents 63 and 64 share a repeat: with 64 documents the last one takes both copies and the
    mask is one word, with 65 the second copy sets bit 0 of a second word; no bit at or above n_docs."""
    rng = np.random.default_rng(13)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    rep = rng.choice(acgt, size=40).tobytes()
    seqs = [rng.choice(acgt, size=12).tobytes() for _ in range(63)] + [rep + b"C", rep + b"G"]
    img, text = helpers.true_bwt_index(seqs, seed=1)
    starts = [int(x) for x in np.cumsum([0] + [len(s) for s in seqs[:-1]])][:n_docs]
    ref = dr.Docs(text, starts)
    reads = [rep, rep[5:], rep + b"G", seqs[0], seqs[62] + rep[:20], b"", text[:-1]]
    reads += [bytes(r) for r in helpers.reads_from_text(text, 100, (1, 30), 0.01, seed=3)]
    bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
    tbl = pkg.ColPml.from_bytes(img)
    tbl.attach_locate(data=lr.samples(text, doc_start=starts))
    for max_walk in (1, 1000):
        got = tbl.docs_batch(bases, off, 1, max_walk)
        _check(f"d{n_docs}/w{max_walk}", got[:6], ref.batch(reads, 1, max_walk))
        mask = got[3]
        assert mask.shape[1] == (2 if n_docs == 65 else 1)
        if n_docs % 64:
            assert not (mask[:, -1] >> np.uint64(n_docs % 64)).any()          # bits at or above n_docs
    assert dr.mask_docs(mask[0]) == ([63, 64] if n_docs == 65 else [63])
    assert tbl.docs(rep, 1, 1000)[2] == dr.mask_docs(mask[0])
    tbl.close()


def test_docs_heavy_ragged_walks(pkg):
    """60 mutated copies of a 2000-base unit, one document each: occ spreads from 1 to the number of
    copies, so the sorted walk has lanes of every length; max_walk 16 truncates the sets."""
    rng = np.random.default_rng(17)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    unit = rng.choice(acgt, size=2000)
    parts = []
    for _ in range(60):
        s = unit.copy()
        mut = rng.random(s.size) < 0.002
        s[mut] = rng.choice(acgt, size=int(mut.sum()))
        parts.append(s.tobytes())
    img, text = helpers.true_bwt_index_large(parts, seed=3)
    starts = [2000 * d for d in range(60)]
    sa = lr.suffix_array(text)
    ref = dr.Docs(text, starts, sa)
    reads = [bytes(r) for r in helpers.reads_from_text(text, 990, (10, 150), 0.004, seed=19)]
    reads += [b""] * 4 + [b"ACGTA", b"GATTACA", bytes(parts[7][:12]), b"N" * 20, bytes(parts[0]), b"T"]
    assert len(reads) == 1000
    bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
    tbl = pkg.ColPml.from_bytes(img)
    tbl.attach_locate(data=lr.samples(text, sa, starts))
    for max_walk in (16, 1000):
        got = tbl.docs_batch(bases, off, 16, max_walk)
        want = ref.batch(reads, 16, max_walk)
        _check(f"heavy/w{max_walk}", got[:6], want)
        if max_walk == 16:
            assert int(got[2].max()) <= 16 and (got[1] > 16).any()              # truncated sets
    assert int(got[1].max()) >= 50, int(got[1].max())
    assert (got[0] < 16).any() and (got[2][got[0] < 16] == 0).all()         # reads below min_len: searched, not walked
    assert int(got[2].max()) >= 50 and len(np.unique(got[2])) >= 20         # walks of many lengths, up to (nearly) every document
    tbl.close()


def test_docs_device_with_and_without_order_and_accumulating_tallies(pkg):
    import torch
    dev = torch.device("cuda", 0)
    img, text, starts = _true_index(4, size=1500)
    starts130 = dr.invented_cuts(len(text), 130, seed=2)
    sa = lr.suffix_array(text)
    reads = [np.frombuffer(bytes(r), np.uint8) for r in helpers.reads_from_text(text, 300, (0, 300), 0.005, seed=6)]
    bases, off = helpers.concat_reads(reads)
    n = len(reads)
    lens = np.diff(off.astype(np.int64))
    d_bases = torch.zeros(len(bases) + 128, dtype=torch.uint8, device=dev)
    d_bases[:len(bases)] = torch.from_numpy(bases)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    order = torch.from_numpy(np.argsort(-lens, kind="stable").astype(np.int32)).to(dev)
    assert pkg.docs_work_bytes(n) % 256 == 0 and pkg.docs_work_bytes(n) >= 24 * n
    d_work = torch.zeros(pkg.docs_work_bytes(n), dtype=torch.uint8, device=dev)
    assert d_work.data_ptr() % 256 == 0
    for layout, ds in ((1, starts), (3, starts130), (5, starts130), (0, starts)):
        tbl = pkg.ColPml.from_bytes(img, layout=layout)
        tbl.attach_locate(data=lr.samples(text, doc_start=ds))
        words = tbl.docs_mask_words()
        want = dr.Docs(text, ds, sa).batch([bytes(r) for r in reads], 12, 8)
        _check(f"L{layout}/host", tbl.docs_batch(bases, off, 12, 8)[:6], want)
        d_reads = torch.zeros(len(ds), dtype=torch.int64, device=dev)
        d_only = torch.zeros(len(ds), dtype=torch.int64, device=dev)
        calls = 0
        for d_order in (None, order.data_ptr()):
            d_mlen = torch.full((n,), -1, dtype=torch.int32, device=dev)
            d_occ = torch.full((n,), -1, dtype=torch.int64, device=dev)
            d_hit = torch.full((n,), -1, dtype=torch.int32, device=dev)
            d_mask = torch.full((n * words,), -1, dtype=torch.int64, device=dev)
            st = tbl.docs_device(d_bases.data_ptr(), d_off.data_ptr(), n, len(bases), 12, 8, d_mlen.data_ptr(), d_occ.data_ptr(),
                                 d_hit.data_ptr(), d_mask.data_ptr(), d_work.data_ptr(), d_reads.data_ptr(), d_only.data_ptr(),
                                 d_order, timed=True)
            calls += 1
            assert st.n_reads == n and st.kernel_ms > 0
            got = (d_mlen.cpu().numpy().view(np.uint32), d_occ.cpu().numpy().view(np.uint64), d_hit.cpu().numpy().view(np.uint32),
                   d_mask.cpu().numpy().view(np.uint64).reshape(n, words), d_reads.cpu().numpy().view(np.uint64),
                   d_only.cpu().numpy().view(np.uint64))
            _check(f"L{layout}/order{d_order is not None}", got,
                   want[:4] + (want[4] * np.uint64(calls), want[5] * np.uint64(calls)))     # the device form adds
        # without tallies and untimed: asynchronous on the default stream
        d_hit = torch.zeros(n, dtype=torch.int32, device=dev)
        tbl.docs_device(d_bases.data_ptr(), d_off.data_ptr(), n, len(bases), 12, 8, d_mlen.data_ptr(), d_occ.data_ptr(),
                        d_hit.data_ptr(), d_mask.data_ptr(), d_work.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_hit.cpu().numpy().view(np.uint32), want[2])
        tbl.close()


def test_docs_refuse_more_than_4096_documents(pkg):
    """4096 documents are served (64 mask words, the whole LDS copy of doc_start); 4097 are an argument
    error of the host and the device form, and the index keeps locating."""
    rng = np.random.default_rng(23)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    unit = rng.choice(acgt, size=1500).tobytes()
    img, text = helpers.true_bwt_index_large([unit, unit[:1400], unit[100:1500], rng.choice(acgt, size=1000).tobytes()], seed=2)
    sa = lr.suffix_array(text)
    reads = [bytes(r) for r in helpers.reads_from_text(text, 120, (1, 80), 0.01, seed=4)] + [b"", text[:-1]]
    bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
    tbl = pkg.ColPml.from_bytes(img)
    starts = dr.invented_cuts(len(text), 4096, seed=1)
    tbl.attach_locate(data=lr.samples(text, sa, starts))
    assert tbl.docs_mask_words() == 64
    for max_walk in (2, 1000):
        _check(f"d4096/w{max_walk}", tbl.docs_batch(bases, off, 1, max_walk)[:6], dr.Docs(text, starts, sa).batch(reads, 1, max_walk))
    tbl.attach_locate(data=lr.samples(text, sa, dr.invented_cuts(len(text), 4097, seed=1)))
    with pytest.raises(pkg.ColbwtError) as ei:
        tbl.docs_batch(bases, off, 1, 4)
    assert ei.value.code == -1 and "more than 4096 documents" in str(ei.value)
    with pytest.raises(pkg.ColbwtError) as ei:
        tbl.docs_device(256, 256, 1, 1, 1, 4, 256, 256, 256, 256, 256)
    assert ei.value.code == -1 and "more than 4096 documents" in str(ei.value)
    assert tbl.locate(text[:-1], 2)[:2] == (len(text) - 1, 1)
    tbl.close()


def test_docs_two_replicas_match_one(pkg):
    img, text, starts = _true_index(9)
    reads = [np.frombuffer(bytes(r), np.uint8) for r in helpers.reads_from_text(text, 2000, (1, 100), 0.01, seed=2)]
    reads += [np.zeros(0, np.uint8)] * 3
    bases, off = helpers.concat_reads(reads)
    loc = lr.samples(text, doc_start=starts)
    one = pkg.ColPml.from_bytes(img)
    two = pkg.ColPml.from_bytes(img, devices=[0, 0])
    one.attach_locate(data=loc)
    two.attach_locate(data=loc)
    a = one.docs_batch(bases, off, 10, 5)
    b = two.docs_batch(bases, off, 10, 5)
    _check("replicas", b[:6], a[:6])
    assert b[6].n_reads == len(reads) and int(a[4].sum()) > 0
    one.close()
    two.close()


def test_col_bwt_build_locate_then_docs_equals_restatement(tmp_path):
    """`col-bwt build -r --locate` on three FASTA documents of two records, then `col-bwt docs`: every
    line and the tally equal the restatement over the collection's text as oracle/rlbwt_oracle.py lays
    it out; an index without samples makes `col-bwt docs` fail."""
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
    text, starts = ro.build_text(docs, revcomp=True)
    ref = dr.Docs(text, starts)
    reads = [bytes(r) for r in helpers.reads_from_text(text, 200, (5, 150), 0.01, seed=13)]
    reads += [docs[0][0][:300], docs[1][1][-200:][::-1], b"NNNN"]
    names = [f"p{k}" for k in range(len(reads))]
    fa = str(tmp_path / "reads.fa")
    helpers.write_fasta(fa, [np.frombuffer(r, np.uint8) for r in reads], names)
    out = subprocess.run(launcher + ["docs", "-p", fa, "-l", "14", "-w", "4", outp], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    want = ref.batch(reads, 14, 4)
    assert open(fa + ".docs").read() == dr.docs_file(names, reads, want)
    assert open(fa + ".docs.tally").read() == dr.tally_file(want[4], want[5])
    assert int(want[2].max()) >= 2
    os.remove(outp + ".col_loc")
    bad = subprocess.run(launcher + ["docs", "-p", fa, outp], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0            # no samples beside that index


def test_docs_calls_do_not_leak_hbm(pkg):
    import torch
    img, text, starts = _true_index(11)
    loc = lr.samples(text, doc_start=starts)
    reads = [np.frombuffer(bytes(r), np.uint8) for r in helpers.reads_from_text(text, 500, (1, 100), 0.01, seed=3)]
    bases, off = helpers.concat_reads(reads)
    tbl = pkg.ColPml.from_bytes(img)
    tbl.attach_locate(data=loc)
    tbl.docs_batch(bases, off, 16, 64)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        tbl.attach_locate(data=loc)
        tbl.docs_batch(bases, off, 16, 64)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] >= free0 - (64 << 20)
    tbl.close()
