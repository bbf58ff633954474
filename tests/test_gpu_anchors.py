"""GPU tier of anchors (include/colbwt.h colbwt_anchors_*): the anchors kernel on the MI355X against the
plain-Python restatement (tests/anchors_restatement.py) on real BWT indexes in every layout, against locate
through the public API alone, through every entry point, and the chain `col-bwt build` -> `col-bwt anchors`."""
import os
import subprocess
import sys

import numpy as np
import pytest

import anchors_restatement as ar
import helpers
import locate_restatement as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = (1, 2, 3, 4, 5, 6, 0)
SETTINGS = ((1, 16, 4), (12, 2, 1), (1, 16, 0))     # (min_len, max_anchors, max_occ)

pytestmark = pytest.mark.gpu


def _true_index(seed, size=700):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    a = rng.choice(acgt, size=size).tobytes()
    seqs = [a, a[200:500], rng.choice(acgt, size=500).tobytes(), b"ACGT" * 30, a[:100]]
    return helpers.true_bwt_index(seqs, seed=seed, extra_splits=80)


def _reads(text, seed, n=200):
    body = text[:-1]
    rng = np.random.default_rng(seed)
    reads = [r for r, _ in ar.planted_reads(text, n, seed=seed)]
    reads += [body, b"", b"N", b"NNN", b"ACGT" * 31, body[:7] + b"\x01" + body[7:20], body[-40:], body[30:60] + b"\x00",
              b"N" + body[100:140] + b"NN" + body[900:960] + b"N", rng.choice(np.frombuffer(b"ACGT", np.uint8), size=220).tobytes()]
    return reads


def _same(label, got, want):
    for name, g, w in zip(("summary", "start", "len", "occ", "pos"), got, want):
        if w is None:
            assert g is None, (label, name)
        else:
            assert np.array_equal(g.view(w.dtype).reshape(w.shape), w), (label, name)


def _batch(tbl, bases, off, setting, **kw):
    summary, start, ln, occ, pos, st = tbl.anchors_batch(bases, off, *setting, **kw)
    return (summary.view(np.uint32).reshape(-1, 8), start, ln, occ, pos), st


def test_anchors_equal_restatement_every_layout(pkg):
    img, text = _true_index(2)
    loc = lr.samples(text)
    ref = ar.Anchors(text)
    reads = _reads(text, 5)
    bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
    want = {s: ref.batch(reads, *s) for s in SETTINGS}
    assert int(want[SETTINGS[0]][0][:, 0].max()) > 16 and (want[SETTINGS[0]][0][:, 2] > 0).sum() >= 20
    assert (want[SETTINGS[1]][0][:, 3] > 2).any() and (want[SETTINGS[0]][3] > 4).any()
    for layout in LAYOUTS:
        tbl = pkg.ColPml.from_bytes(img, layout=layout)
        tbl.attach_locate(data=loc)
        for s in SETTINGS:
            got, st = _batch(tbl, bases, off, s)
            assert st.n_reads == len(reads)
            _same(f"L{layout}/{s}", got, want[s])
        summary, factors = tbl.anchors(reads[0], 1, 16, 4)
        assert summary == dict(zip(ar.SUMMARY, (int(x) for x in want[SETTINGS[0]][0][0])))
        assert factors == [(f[0], f[1], f[2], f[3][:4]) for f in ref.factors(reads[0])[0][:16]]
        tbl.close()


def test_anchors_against_locate_through_the_public_api(pkg):
    """Slot 0 is locate's answer for every read with mlen > 0, and iterating locate_batch on the truncated reads
    reproduces every stored anchor; the summaries follow from the slots."""
    img, text = _true_index(3)
    reads = _reads(text, 7, n=150)
    arrs = [np.frombuffer(r, np.uint8) for r in reads]
    bases, off = helpers.concat_reads(arrs)
    K, W = 128, 3
    tbl = pkg.ColPml.from_bytes(img)
    tbl.attach_locate(data=lr.samples(text))
    (summary, start, ln, occ, pos), _ = _batch(tbl, bases, off, (1, K, W))
    mlen, locc, lpos, _ = tbl.locate_batch(bases, off, W)
    assert (summary[:, 0] <= K).all()
    has = mlen > 0
    lens = np.diff(off.astype(np.int64))
    assert np.array_equal(start[has, 0], (lens[has] - mlen[has]).astype(np.uint32)) and np.array_equal(ln[has, 0], mlen[has])
    assert np.array_equal(occ[has, 0], locc[has]) and np.array_equal(pos[has, 0], lpos[has])
    # the loop of the header, one locate_batch per round over the prefixes still to be parsed
    end = lens - 1
    slot = np.zeros(len(reads), np.int64)
    skipped = np.zeros(len(reads), np.int64)
    while (end >= 0).any():
        live = np.flatnonzero(end >= 0)
        pb, po = helpers.concat_reads([arrs[k][:end[k] + 1] for k in live])
        m2, o2, p2, _ = tbl.locate_batch(pb, po, W)
        for j, k in enumerate(live):
            L = int(m2[j])
            if L == 0:
                skipped[k] += 1
                end[k] -= 1
                continue
            t = slot[k]
            assert (int(start[k, t]), int(ln[k, t]), int(occ[k, t])) == (end[k] - L + 1, L, int(o2[j])), (k, t)
            assert np.array_equal(pos[k, t], p2[j]), (k, t)
            slot[k] += 1
            end[k] -= L
    assert np.array_equal(slot, summary[:, 0]) and np.array_equal(slot, summary[:, 7]) and np.array_equal(skipped, summary[:, 2])
    assert (start[np.arange(K)[None, :] >= slot[:, None]] == pkg.ANCHOR_NONE).all()
    tbl.close()


def test_anchors_without_samples_equal_the_run_with_samples(pkg):
    img, text = _true_index(4)
    reads = _reads(text, 9)
    bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
    for layout in (1, 3, 0):
        bare = pkg.ColPml.from_bytes(img, layout=layout)
        full = pkg.ColPml.from_bytes(img, layout=layout)
        full.attach_locate(data=lr.samples(text))
        for min_len, K in ((1, 16), (12, 2)):
            a, _ = _batch(bare, bases, off, (min_len, K, 0))
            b, _ = _batch(full, bases, off, (min_len, K, 0))
            c, _ = _batch(full, bases, off, (min_len, K, 2))
            assert a[4] is None and b[4] is None
            _same(f"L{layout} bare/with samples", a[:4], b[:4])
            _same(f"L{layout} max_occ 0/2", a[:4], c[:4])
            s, _ = _batch(full, bases, off, (min_len, K, 2), want_slots=False)
            assert s[1] is None and np.array_equal(s[0], a[0])
        with pytest.raises(pkg.ColbwtError) as ei:
            bare.anchors_batch(bases, off, 1, 16, 1)
        assert ei.value.code == -1 and "no locate samples attached" in str(ei.value)
        bare.close()
        full.close()


def test_anchors_device_with_and_without_order(pkg):
    import torch
    dev = torch.device("cuda", 0)
    img, text = _true_index(4, size=1500)
    reads = [np.frombuffer(bytes(r), np.uint8) for r in helpers.reads_from_text(text, 300, (0, 300), 0.02, seed=6, extra=b"N")]
    bases, off = helpers.concat_reads(reads)
    lens = np.diff(off.astype(np.int64))
    n = len(reads)
    d_bases = torch.zeros(len(bases) + 128, dtype=torch.uint8, device=dev)
    d_bases[:len(bases)] = torch.from_numpy(bases)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    order = torch.from_numpy(np.argsort(-lens, kind="stable").astype(np.int32)).to(dev)
    for layout in (1, 3, 5, 0):
        tbl = pkg.ColPml.from_bytes(img, layout=layout)
        tbl.attach_locate(data=lr.samples(text))
        for min_len, K, W in SETTINGS:
            want, _ = _batch(tbl, bases, off, (min_len, K, W))
            for d_order in (None, order.data_ptr()):
                # garbage first: the kernel initialises every slot itself
                d_sum = torch.full((n * 8,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
                d_start = torch.full((n * K,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
                d_len = torch.full((n * K,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
                d_occ = torch.full((n * K,), 0x5A5A5A5A5A5A, dtype=torch.int64, device=dev)
                d_pos = torch.full((n * K * max(W, 1),), 0x5A5A5A5A5A5A, dtype=torch.int64, device=dev)
                st = tbl.anchors_device(d_bases.data_ptr(), d_off.data_ptr(), n, len(bases), min_len, K, W, d_sum.data_ptr(),
                                        d_start.data_ptr(), d_len.data_ptr(), d_occ.data_ptr(), d_pos.data_ptr() if W else None,
                                        d_order, timed=True)
                assert st.n_reads == n
                got = (d_sum.cpu().numpy().view(np.uint32).reshape(n, 8), d_start.cpu().numpy().view(np.uint32).reshape(n, K),
                       d_len.cpu().numpy().view(np.uint32).reshape(n, K), d_occ.cpu().numpy().view(np.uint64).reshape(n, K),
                       d_pos.cpu().numpy().view(np.uint64).reshape(n, K, W) if W else None)
                _same(f"L{layout}/{(min_len, K, W)}/order {d_order is not None}", got, want)
            d_sum = torch.full((n * 8,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
            tbl.anchors_device(d_bases.data_ptr(), d_off.data_ptr(), n, len(bases), min_len, K, W, d_sum.data_ptr(), timed=True)
            assert np.array_equal(d_sum.cpu().numpy().view(np.uint32).reshape(n, 8), want[0]), "summaries only"
        tbl.close()


def test_anchors_two_replicas_match_one(pkg):
    img, text = _true_index(9)
    reads = [np.frombuffer(r, np.uint8) for r, _ in ar.planted_reads(text, 2000, seed=2, max_len=100)]
    reads += [np.zeros(0, np.uint8)] * 3
    bases, off = helpers.concat_reads(reads)
    loc = lr.samples(text)
    one = pkg.ColPml.from_bytes(img)
    two = pkg.ColPml.from_bytes(img, devices=[0, 0])
    one.attach_locate(data=loc)
    two.attach_locate(data=loc)
    for s in SETTINGS:
        a, _ = _batch(one, bases, off, s)
        b, st = _batch(two, bases, off, s)
        _same(f"replicas {s}", b, a)
        assert st.n_reads == len(reads)
    one.close()
    two.close()


def test_col_bwt_build_then_anchors_equals_restatement(tmp_path):
    """`col-bwt build -r --locate` on three FASTA documents of two records, then `col-bwt anchors`: every line equals
    the restatement's formatter over the collection's text; `col-bwt anchors -n 0` runs on the index built without
    --locate, and the default -n on that index exits non-zero."""
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
    outp, plain = str(tmp_path / "coll"), str(tmp_path / "plain")
    for cmd in (["build", "-r", "--locate", "-l", "20", "-o", outp], ["build", "-r", "-l", "20", "-o", plain]):
        out = subprocess.run(launcher + cmd + paths, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
    assert not os.path.exists(plain + ".col_loc")
    text, starts = ro.build_text(docs, revcomp=True)
    ref = ar.Anchors(text, starts)
    reads = [r for r, _ in ar.planted_reads(text, 150, seed=13)] + [docs[0][0][:300], docs[1][1][-200:][::-1], b"NNNN"]
    names = [f"p{k}" for k in range(len(reads))]
    fa = str(tmp_path / "reads.fa")
    helpers.write_fasta(fa, [np.frombuffer(r, np.uint8) for r in reads], names)
    out = subprocess.run(launcher + ["anchors", "-p", fa, "-l", "12", "-k", "3", "-n", "2", outp], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(fa + ".anchors").read() == ref.file(names, reads, 12, 3, 2)
    out = subprocess.run(launcher + ["anchors", "-p", fa, outp], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(fa + ".anchors").read() == ref.file(names, reads, 16, 16, 1)
    os.remove(fa + ".anchors")
    out = subprocess.run(launcher + ["anchors", "-p", fa, "-n", "0", plain], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(fa + ".anchors").read() == ref.file(names, reads, 16, 16, 0)
    os.remove(fa + ".anchors")
    bad = subprocess.run(launcher + ["anchors", "-p", fa, plain], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "col_loc" in bad.stderr            # no samples beside that index
    assert not os.path.exists(fa + ".anchors")


def test_anchors_calls_do_not_leak_hbm(pkg):
    import torch
    img, text = _true_index(11)
    loc = lr.samples(text)
    reads = [np.frombuffer(r, np.uint8) for r, _ in ar.planted_reads(text, 500, seed=3, max_len=100)]
    bases, off = helpers.concat_reads(reads)
    tbl = pkg.ColPml.from_bytes(img)
    tbl.attach_locate(data=loc)
    tbl.anchors_batch(bases, off, 1, 16, 4)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        tbl.anchors_batch(bases, off, 1, 16, 4)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] >= free0 - (64 << 20)
    tbl.close()
