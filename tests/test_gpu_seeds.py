"""GPU tier of the seeds reduction (include/colbwt.h colbwt_seeds_*): the reduction kernel on the
MI355X against the plain-Python restatement (tests/seeds_restatement.py) applied to the same
handle's query output and to the oracle's, through every entry point.  Every comparison is exact."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import seeds_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = (1, 2, 3, 4, 5, 6, 0)
PARAMS = ((1, 1000), (3, 3), (8, 1), (16, 16), (20, 8))

pytestmark = pytest.mark.gpu


def _summary(summary):
    return summary.view(np.uint32).reshape(-1, 8)


def _same(label, got, want):
    for name, g, w in zip(("summary", "seed_pos", "seed_len", "seed_cid"), got, want):
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{label}: {name} differs at {bad[:5].tolist()}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}"


def _true_bwt(seed=2, size=900, extra_splits=120):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    a = rng.choice(acgt, size=size).tobytes()
    seqs = [a, a[200:500], rng.choice(acgt, size=size // 2).tobytes(), b"ACGT" * 30]
    return helpers.true_bwt_index(seqs, seed=seed, extra_splits=extra_splits)


def _reduce_on_device(pkg, pml, cid, off, min_len, max_seeds, slots=True, stream=None):
    """colbwt_seeds_reduce_device over host arrays copied to the device -> host results."""
    import torch
    dev = torch.device("cuda", 0)
    nr, nb = len(off) - 1, len(pml)
    pml = np.ascontiguousarray(pml)
    d_pml = torch.from_numpy(pml.view(np.uint8).copy()).to(dev) if nb else torch.zeros(16, dtype=torch.uint8, device=dev)
    d_cid = torch.from_numpy(np.ascontiguousarray(cid, np.uint8)).to(dev) if nb else torch.zeros(16, dtype=torch.uint8, device=dev)
    d_off = torch.from_numpy(np.asarray(off).astype(np.int64)).to(dev)
    d_sum = torch.full((nr * 8,), 0x2B2B2B2B, dtype=torch.int32, device=dev)
    d_pos = torch.full((nr * max_seeds,), 7, dtype=torch.int32, device=dev)
    d_len = torch.full((nr * max_seeds,), 7, dtype=torch.int32, device=dev)
    d_sc = torch.full((nr * max_seeds,), 7, dtype=torch.uint8, device=dev)
    ptr = (lambda t: t.data_ptr()) if slots else (lambda t: None)
    torch.cuda.synchronize()
    pkg.seeds_reduce_device(d_pml.data_ptr(), d_cid.data_ptr(), d_off.data_ptr(), nr, nb, min_len, max_seeds, d_sum.data_ptr(),
                            ptr(d_pos), ptr(d_len), ptr(d_sc), pml_bytes=pml.dtype.itemsize,
                            stream=stream.cuda_stream if stream is not None else 0)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    if not slots:
        assert bool((d_pos == 7).all()) and bool((d_len == 7).all()) and bool((d_sc == 7).all())
    return (d_sum.cpu().numpy().view(np.uint32).reshape(nr, 8), d_pos.cpu().numpy().view(np.uint32).reshape(nr, max_seeds),
            d_len.cpu().numpy().view(np.uint32).reshape(nr, max_seeds), d_sc.cpu().numpy().reshape(nr, max_seeds))


def test_seeds_every_layout_against_own_query_and_oracle(pkg, oracle):
    img, text = _true_bwt()
    reads = helpers.reads_from_text(text, 400, (1, 300), 0.03, seed=5, extra=b"Nn")
    reads += [np.frombuffer(text[:-1], np.uint8), np.zeros(0, np.uint8), np.frombuffer(b"A", np.uint8), np.zeros(0, np.uint8)]
    reads = [np.zeros(0, np.uint8)] + reads
    bases, off = helpers.concat_reads(reads)
    epml, ecid = oracle.OracleIndex(bytes(img)).query_batch(bases, off)
    assert ecid.any(), "the index carries col ids"
    wants = {p: sr.seeds(epml, ecid, off, *p) for p in PARAMS}
    for p in PARAMS:
        sr.check_invariants(*wants[p][:3], off, *p)
    for layout in LAYOUTS:
        tbl = pkg.ColPml.from_bytes(img, layout=layout)
        pml, cid, _ = tbl.query_batch(bases, off)
        for p in PARAMS:
            summary, pos, ln, sc, st = tbl.seeds_batch(bases, off, *p)
            assert st.n_reads == len(reads) and st.n_bases == int(off[-1])
            _same(f"L{layout} {p} vs oracle", (_summary(summary), pos, ln, sc), wants[p])
            _same(f"L{layout} {p} vs own query", (_summary(summary), pos, ln, sc), sr.seeds(pml, cid, off, *p))
        only, p0, l0, c0, _ = tbl.seeds_batch(bases, off, 3, 3, want_seeds=False)
        assert p0 is None and np.array_equal(_summary(only), wants[(3, 3)][0])
        s, where = tbl.seeds(bytes(reads[5]), min_len=1, max_seeds=1000)
        assert s["cov"] + s["resets"] == len(reads[5]) and len(where) == s["n_seeds"]
        tbl.close()


def test_seeds_reduce_device_crafted_arrays_and_alignments(pkg):
    rng = np.random.default_rng(11)

    def both(label, pml, cid, off, params=((1, 4), (3, 2), (8, 1), (20, 1000))):
        pml, cid, off = np.asarray(pml), np.asarray(cid, np.uint8), np.asarray(off, np.uint64)
        for min_len, max_seeds in params:
            want = sr.seeds(pml, cid, off, min_len, max_seeds)
            _same(f"{label}/l{min_len}/k{max_seeds}", _reduce_on_device(pkg, pml, cid, off, min_len, max_seeds), want)
        got = _reduce_on_device(pkg, pml, cid, off, *params[0], slots=False)
        assert np.array_equal(got[0], sr.seeds(pml, cid, off, *params[0])[0]), f"{label}: summaries only"

    n = 3000
    even = np.arange(0, n + 1, 100)
    both("all-zero pml", np.zeros(n, np.uint16), rng.integers(0, 256, n), even)
    ramp = np.tile(np.arange(100, 0, -1), n // 100).astype(np.uint16)
    both("col ids everywhere", ramp, rng.integers(1, 256, n), even)
    both("col ids nowhere", ramp, np.zeros(n), even)
    both("one read, u32", ramp.astype(np.uint32), rng.integers(0, 3, n), [0, n])
    for edge in (8, 64, 512):
        for shift in (-1, 0, 1):
            pml = np.zeros(1200, np.uint16)
            e = edge + shift
            pml[e - 5:e] = np.arange(5, 0, -1)
            pml[e + 1:e + 31] = np.arange(30, 0, -1)
            pml[1024 - 40:1024] = np.arange(40, 0, -1)
            cid = np.where(rng.random(1200) < 0.1, rng.integers(1, 256, 1200), 0)
            both(f"run end at {e}", pml, cid, [0, 1200], params=((1, 8), (8, 2), (20, 1)))
            both(f"read end at {e}", pml, cid, [0, e, 1200], params=((1, 8), (8, 2)))
    for a in range(16):
        lens = [a + 16, 1, 0, 37, 600, 2, 0, 0, 9]
        off = np.concatenate(([0], np.cumsum(lens)))
        nb = int(off[-1])
        pml = rng.integers(0, 4, nb).astype(np.uint16)
        cid = np.where(rng.random(nb) < 0.3, rng.integers(1, 256, nb), 0)
        both(f"alignment {a}", pml, cid, off, params=((1, 3), (3, 1000)))
    lens = np.concatenate(([0, 0], rng.integers(0, 6, 5000), [0, 0, 0]))
    off = np.concatenate(([0], np.cumsum(lens)))
    nb = int(off[-1])
    both("tiny reads", rng.integers(0, 3, nb).astype(np.uint16), rng.integers(0, 3, nb), off, params=((1, 2), (2, 5)))
    both("only empty reads", np.zeros(0, np.uint16), np.zeros(0), np.zeros(70, np.uint64), params=((1, 2),))
    lens = rng.integers(0, 3000, 300)
    off = np.concatenate(([0], np.cumsum(lens)))
    nb = int(off[-1])
    pml = np.where(rng.random(nb) < 0.05, 0, rng.integers(1, 2 ** 32, nb)).astype(np.uint32)
    both("u32 arbitrary", pml, np.where(rng.random(nb) < 0.02, rng.integers(1, 256, nb), 0), off, params=((1, 3), (1 << 31, 1000)))


def test_seeds_long_reads_and_u32_path(pkg, oracle):
    """10-kbp reads (each spans ~20 wave iterations) and one read > 65535 bases (u32 PML)."""
    img, text = _true_bwt(seed=6, size=4000, extra_splits=400)
    rng = np.random.default_rng(3)
    src = np.frombuffer(text[:-1], np.uint8)

    def long_read(m):
        rd = np.tile(src, m // src.size + 2)[int(rng.integers(0, src.size)):][:m].copy()
        hit = rng.integers(0, m, m // 40)
        rd[hit] = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=hit.size)
        return rd

    reads = [long_read(10_000) for _ in range(40)] + [np.zeros(0, np.uint8), long_read(7)]
    for name, batch, wide in (("10 kbp", reads, False), ("u32", [reads[0][:900], long_read(70_000), reads[1][:33]], True)):
        bases, off = helpers.concat_reads(batch)
        epml, ecid = oracle.OracleIndex(bytes(img)).query_batch(bases, off, wide=wide)
        for layout in (0, 3) if wide else (0, 1, 3, 5):
            tbl = pkg.ColPml.from_bytes(img, layout=layout)
            for p in ((1, 1000), (20, 8)):
                want = sr.seeds(epml, ecid, off, *p)
                sr.check_invariants(*want[:3], off, *p)
                summary, pos, ln, sc, _ = tbl.seeds_batch(bases, off, *p)
                _same(f"{name} L{layout} {p}", (_summary(summary), pos, ln, sc), want)
            tbl.close()


def test_seeds_c2_shape_sample_in_full_and_on_a_stream(pkg, c2_image):
    """The C2 index (AUTO layout), 120 000 x 150 bp reads from the device sampler: query_device then
    seeds_reduce_device on a non-default stream, every read compared with the restatement applied
    to that query output; seeds_batch on the same reads gives the same."""
    import torch
    dev = torch.device("cuda", 0)
    tbl = pkg.ColPml.from_bytes(c2_image)
    n_reads, m, min_len, max_seeds = 120_000, 150, 20, 8
    nb = n_reads * m
    d_bases = torch.zeros(nb + 128, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(n_reads + 1, dtype=torch.int64, device=dev)
    tbl.synth_reads_device(n_reads, m, 10, 77, d_bases.data_ptr(), d_off.data_ptr())
    d_pml = torch.zeros(nb + 64, dtype=torch.int16, device=dev)
    d_cid = torch.zeros(nb + 64, dtype=torch.uint8, device=dev)
    d_sum = torch.zeros(n_reads * 8, dtype=torch.int32, device=dev)
    d_pos = torch.zeros(n_reads * max_seeds, dtype=torch.int32, device=dev)
    d_len = torch.zeros(n_reads * max_seeds, dtype=torch.int32, device=dev)
    d_sc = torch.zeros(n_reads * max_seeds, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    tbl.query_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, nb, d_pml.data_ptr(), d_cid.data_ptr(), stream=stream.cuda_stream)
    tbl.seeds_reduce_device(d_pml.data_ptr(), d_cid.data_ptr(), d_off.data_ptr(), n_reads, nb, min_len, max_seeds, d_sum.data_ptr(),
                            d_pos.data_ptr(), d_len.data_ptr(), d_sc.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    st = tbl.seeds_reduce_device(d_pml.data_ptr(), d_cid.data_ptr(), d_off.data_ptr(), n_reads, nb, min_len, max_seeds,
                                 d_sum.data_ptr(), d_pos.data_ptr(), d_len.data_ptr(), d_sc.data_ptr(), timed=True)
    assert st.kernel_ms > 0 and st.n_reads == n_reads
    pml = d_pml[:nb].cpu().numpy().view(np.uint16)
    cid = d_cid[:nb].cpu().numpy()
    off = d_off.cpu().numpy().astype(np.uint64)
    got = (d_sum.cpu().numpy().view(np.uint32).reshape(n_reads, 8), d_pos.cpu().numpy().view(np.uint32).reshape(n_reads, max_seeds),
           d_len.cpu().numpy().view(np.uint32).reshape(n_reads, max_seeds), d_sc.cpu().numpy().reshape(n_reads, max_seeds))
    want = sr.seeds(pml, cid, off, min_len, max_seeds)
    assert want[0][:, 0].sum() > n_reads // 4, "the sample holds seeds"
    _same("C2 sample, device entry point", got, want)
    sr.check_invariants(*want[:3], off, min_len, max_seeds)
    bases = d_bases[:nb].cpu().numpy()
    summary, pos, ln, sc, st = tbl.seeds_batch(bases, off, min_len, max_seeds)
    assert st.kernel_ms > 0 and st.d2h_ms >= 0
    _same("C2 sample, seeds_batch", (_summary(summary), pos, ln, sc), want)
    tbl.close()


def test_seeds_two_replicas_match_one(pkg):
    image = pkg.synth_index(300_000, mean_len=8, split_permille=100, seed=9)
    reads = helpers.backward_walk_reads(image, 3000, 120, 0.01, seed=2)
    reads += [np.zeros(0, np.uint8)] + [r[:k] for k, r in zip(range(1, 200), reads)]
    bases, off = helpers.concat_reads(reads)
    one = pkg.ColPml.from_bytes(image)
    two = pkg.ColPml.from_bytes(image, devices=[0, 0])
    a, b = one.seeds_batch(bases, off, 8, 4), two.seeds_batch(bases, off, 8, 4)
    _same("two replicas", (_summary(b[0]),) + b[1:4], (_summary(a[0]),) + a[1:4])
    one.close()
    two.close()


def test_seeds_argument_errors(pkg):
    img, _ = _true_bwt()
    tbl = pkg.ColPml.from_bytes(img)
    bases, off = helpers.concat_reads([np.frombuffer(b"ACGT", np.uint8)])
    for min_len, max_seeds in ((0, 4), (1, 0), (1, (1 << 16) + 1)):
        with pytest.raises(pkg.ColbwtError) as e:
            tbl.seeds_batch(bases, off, min_len, max_seeds)
        assert e.value.code == -1
    tbl.close()


def test_col_bwt_build_then_seeds_equals_restatement(pkg, tmp_path):
    """`col-bwt build -r` on a small collection, then `col-bwt seeds`: every line equals the Python
    formatting of the restatement applied to the built index's query output; seeds_file on FASTQ
    and .gz in several batches gives the same bytes."""
    rng = np.random.default_rng(12)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    base = rng.choice(acgt, size=3000)
    paths, docs = [], []
    for k in range(3):
        s = base.copy()
        mut = rng.random(s.size) < 0.02
        s[mut] = rng.choice(acgt, size=int(mut.sum()))
        docs.append(s)
        paths.append(str(tmp_path / f"g{k}.fa"))
        helpers.write_fasta(paths[-1], [s], [f"g{k}"])
    launcher = [sys.executable, os.path.join(ROOT, "col-bwt_amd", "col-bwt")]
    outp = str(tmp_path / "coll")
    out = subprocess.run(launcher + ["build", "-r", "-l", "20", "-s", "1", "-o", outp] + paths, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    reads = []
    for k in range(300):
        d = docs[k % 3]
        lo = int(rng.integers(0, d.size - 400))
        rd = d[lo:lo + int(rng.integers(1, 400))].copy()
        hit = rng.random(rd.size) < 0.02
        rd[hit] = rng.choice(acgt, size=int(hit.sum()))
        reads.append(rd)
    reads.append(np.zeros(0, np.uint8))
    names = [f"p{k}" for k in range(len(reads))]
    fa = str(tmp_path / "reads.fa")
    helpers.write_fasta(fa, reads, names)
    tbl = pkg.ColPml.load(outp)
    bases, off = helpers.concat_reads(reads)
    pml, cid, _ = tbl.query_batch(bases, off)
    assert cid.any(), "the built index carries col ids"
    for min_len, max_seeds, flags in ((16, 16, []), (5, 2, ["-l", "5", "-k", "2"])):
        want = sr.format_lines(names, off, *sr.seeds(pml, cid, off, min_len, max_seeds), max_seeds)
        out = subprocess.run(launcher + ["seeds", "-p", fa] + flags + [outp], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert open(fa + ".seeds", "rb").read() == want
    fq = str(tmp_path / "reads.fq")
    with open(fq, "wb") as f:
        for nm, rd in zip(names, reads):
            f.write(b"@" + nm.encode() + b" comment\n" + bytes(rd) + b"\n+\n" + b"I" * len(rd) + b"\n")
    gz = fq + ".gz"
    with open(fq, "rb") as src, gzip.open(gz, "wb") as dst:
        dst.write(src.read())
    for path in (fq, gz):
        st = tbl.seeds_file(path, min_len=5, max_seeds=2, batch_bases=9_000)
        assert st.n_reads == len(reads)
        assert open(path + ".seeds", "rb").read() == want, path
    tbl.close()
    bad = subprocess.run(launcher + ["seeds", "-p", fa, "-k", "0", outp], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0
