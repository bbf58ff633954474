"""GPU tier of exact-match counting (include/colbwt.h colbwt_count_*): the count kernel on the
MI355X against brute-force substring counting on real BWT indexes and against the plain-Python
restatement (tests/count_restatement.py) on synthetic tables, through every entry point."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import count_restatement
import helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = (1, 2, 3, 4, 5, 6, 0)

pytestmark = pytest.mark.gpu


def _expect(rows):
    return (np.array([w[0] for w in rows], np.uint32), np.array([w[1] for w in rows], np.uint64),
            np.array([w[2] for w in rows], np.uint64))


def _assert_counts(label, got, want):
    for name, g, w in zip(("mlen", "occ", "sp"), got, want):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{label}: {name} differs at reads {bad[:5]}: {g[bad[:5]]} != {w[bad[:5]]}"


def test_count_equals_brute_force_on_true_bwt_every_layout(pkg):
    rng = np.random.default_rng(31)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    a = rng.choice(acgt, size=700).tobytes()
    seqs = [a, a[200:500], rng.choice(acgt, size=500).tobytes(), b"ACGT" * 30]
    img, text = helpers.true_bwt_index(seqs, seed=2, extra_splits=80)
    reads = [bytes(r) for r in helpers.reads_from_text(text, 150, (1, 120), 0.01, seed=5, extra=b"Nn")]
    reads += [text[:-1], b"", b"N", b"ACGT" * 31, a[-40:] + b"T"]
    want = _expect([count_restatement.brute_force(text, rd) for rd in reads])
    bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
    for layout in LAYOUTS:
        tbl = pkg.ColPml.from_bytes(img, layout=layout)
        mlen, occ, sp, _ = tbl.count_batch(bases, off, want_sp=True)
        _assert_counts(f"L{layout}", (mlen, occ, sp), want)
        assert tbl.count(text[:-1])[:2] == (len(text) - 1, 1)
        tbl.close()


def test_count_synthetic_long_rows_and_splits_every_layout(pkg):
    for seed in range(4):
        rng = np.random.default_rng(100 + seed)
        alpha = (b"ACGT", b"AC", b"ACGTN", b"ACGT")[seed]
        r = int(rng.integers(2000, 20000))
        img = helpers.random_table(rng, r, alphabet=alpha, max_len=(9, 40, 300, 9)[seed], split_prob=(0.1, 0.5, 0, 0.2)[seed])
        if seed % 2 == 0:     # a few rows beyond the 16-bit length field (the len16 escape)
            t = helpers.unpack_col_pml(img)
            lens = np.diff(np.append(t["idx"].astype(np.int64), t["n"]))
            lens[rng.integers(0, r, size=3)] = rng.integers(65536, 200000, size=3)
            idx = np.concatenate(([0], np.cumsum(lens)[:-1]))
            n = int(lens.sum())
            interval, offset = helpers.lf_columns(t["char"], idx, n)
            img = helpers.pack_col_pml(int(t["bwt_r"]), n, t["char"], idx, interval, offset, t["cid"], t["thr"])
        reads = [rng.choice(np.frombuffer(alpha + b"Z", np.uint8), size=int(m)) for m in rng.integers(0, 80, size=150)]
        reads += helpers.backward_walk_reads(img, 150, 60, 0.0, seed)
        want = _expect(count_restatement.count_reads(img, reads))
        bases, off = helpers.concat_reads(reads)
        for layout in LAYOUTS:
            tbl = pkg.ColPml.from_bytes(img, layout=layout)
            mlen, occ, sp, _ = tbl.count_batch(bases, off, want_sp=True)
            _assert_counts(f"seed {seed} L{layout}", (mlen, occ, sp), want)
            tbl.close()


def test_count_device_c2_shape_sample(pkg, c2_image):
    """The C2 index (AUTO layout), reads from the device sampler; first, middle, last and a seeded
    sample of reads against the restatement; with and without d_order, with d_sp NULL."""
    import torch
    dev = torch.device("cuda", 0)
    tbl = pkg.ColPml.from_bytes(c2_image)
    n_reads, m = 200_000, 150
    d_bases = torch.zeros(n_reads * m + 128, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(n_reads + 1, dtype=torch.int64, device=dev)
    tbl.synth_reads_device(n_reads, m, 10, 77, d_bases.data_ptr(), d_off.data_ptr())
    d_mlen = torch.zeros(n_reads, dtype=torch.int32, device=dev)
    d_occ = torch.zeros(n_reads, dtype=torch.int64, device=dev)
    d_sp = torch.zeros(n_reads, dtype=torch.int64, device=dev)
    st = tbl.count_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, n_reads * m, d_mlen.data_ptr(), d_occ.data_ptr(),
                          d_sp.data_ptr(), timed=True)
    assert st.kernel_ms > 0
    mlen = d_mlen.cpu().numpy().view(np.uint32)
    occ = d_occ.cpu().numpy().view(np.uint64)
    sp = d_sp.cpu().numpy().view(np.uint64)
    bases = d_bases.cpu().numpy()
    pick = sorted({0, n_reads // 2, n_reads - 1} | set(np.random.default_rng(3).choice(n_reads, 40, replace=False).tolist()))
    t = count_restatement.Table(c2_image)
    for k in pick:
        assert (int(mlen[k]), int(occ[k]), int(sp[k])) == t.count(bases[k * m:(k + 1) * m]), f"read {k}"
    assert (mlen == m).mean() > 0.1 and (occ[mlen > 0] > 0).all()
    # reversed lane order and no d_sp: the same values
    order = torch.arange(n_reads - 1, -1, -1, dtype=torch.int32, device=dev)
    d_mlen2 = torch.zeros_like(d_mlen)
    d_occ2 = torch.zeros_like(d_occ)
    tbl.count_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, n_reads * m, d_mlen2.data_ptr(), d_occ2.data_ptr(),
                     None, order.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(d_mlen2, d_mlen) and torch.equal(d_occ2, d_occ)
    tbl.close()


def test_count_device_ragged_with_order(pkg):
    import torch
    dev = torch.device("cuda", 0)
    img, text = helpers.true_bwt_index([np.random.default_rng(4).choice(np.frombuffer(b"ACGT", np.uint8), size=1500).tobytes()],
                                       seed=4)
    reads = helpers.reads_from_text(text, 300, (0, 500), 0.005, seed=6)
    bases, off = helpers.concat_reads(reads)
    want = _expect(count_restatement.count_reads(img, reads))
    lens = np.diff(off.astype(np.int64))
    d_bases = torch.zeros(len(bases) + 128, dtype=torch.uint8, device=dev)
    d_bases[:len(bases)] = torch.from_numpy(bases)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    order = torch.from_numpy(np.argsort(-lens, kind="stable").astype(np.int32)).to(dev)
    for layout in (1, 3, 5):
        tbl = pkg.ColPml.from_bytes(img, layout=layout)
        for d_order in (None, order.data_ptr()):
            d_mlen = torch.zeros(len(reads), dtype=torch.int32, device=dev)
            d_occ = torch.zeros(len(reads), dtype=torch.int64, device=dev)
            d_sp = torch.zeros(len(reads), dtype=torch.int64, device=dev)
            tbl.count_device(d_bases.data_ptr(), d_off.data_ptr(), len(reads), len(bases), d_mlen.data_ptr(),
                             d_occ.data_ptr(), d_sp.data_ptr(), d_order)
            torch.cuda.synchronize()
            got = (d_mlen.cpu().numpy().view(np.uint32), d_occ.cpu().numpy().view(np.uint64), d_sp.cpu().numpy().view(np.uint64))
            _assert_counts(f"L{layout} order={d_order is not None}", got, want)
        tbl.close()


def test_count_two_replicas_match_one(pkg):
    image = pkg.synth_index(300_000, mean_len=8, split_permille=100, seed=9)
    reads = helpers.backward_walk_reads(image, 3000, 120, 0.01, seed=2)
    reads += [np.zeros(0, np.uint8)] + [r[:k] for k, r in zip(range(1, 200), reads)]
    bases, off = helpers.concat_reads(reads)
    one = pkg.ColPml.from_bytes(image)
    two = pkg.ColPml.from_bytes(image, devices=[0, 0])
    assert two.info().n_devices == 2
    a = one.count_batch(bases, off, want_sp=True)
    b = two.count_batch(bases, off, want_sp=True)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    assert b[3].n_reads == len(reads)
    one.close()
    two.close()


def _write_inputs(d, reads, names):
    fa = os.path.join(d, "r.fa")
    helpers.write_fasta(fa, reads, names)
    fq = os.path.join(d, "r.fq")
    with open(fq, "wb") as f:
        for nm, rd in zip(names, reads):
            f.write(b"@" + nm.encode() + b" comment\n" + bytes(rd) + b"\n+\n" + b"I" * len(rd) + b"\n")
    gz = os.path.join(d, "r.fa.gz")
    with open(fa, "rb") as src, gzip.open(gz, "wb") as dst:
        dst.write(src.read())
    return fa, fq, gz


def test_count_file_and_cli_match_count_batch(pkg, tmp_path):
    img, text = helpers.true_bwt_index([np.random.default_rng(8).choice(np.frombuffer(b"ACGT", np.uint8), size=2000).tobytes()],
                                       seed=8)
    prefix = str(tmp_path / "idx")
    with open(prefix + ".col_pml", "wb") as f:
        f.write(img)
    reads = helpers.reads_from_text(text, 500, (0, 200), 0.01, seed=9, extra=b"N")
    names = [f"q{k}" for k in range(len(reads))]
    tbl = pkg.ColPml.load(prefix)
    bases, off = helpers.concat_reads(reads)
    mlen, occ, _, _ = tbl.count_batch(bases, off)
    want = "".join(f"{names[k]}\t{len(reads[k])}\t{mlen[k]}\t{occ[k]}\n" for k in range(len(reads))).encode()
    d = str(tmp_path)
    for path in _write_inputs(d, reads, names):
        st = tbl.count_file(path, batch_bases=20_000)
        assert st.n_reads == len(reads)
        assert open(path + ".count", "rb").read() == want, path
        os.remove(path + ".count")
        out = subprocess.run([sys.executable, os.path.join(ROOT, "col-bwt_amd", "col-bwt"), "count", "-p", path, prefix],
                             capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert open(path + ".count", "rb").read() == want, path
    tbl.close()
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "col-bwt_amd", "col-bwt"), "count", "-p", path,
                          str(tmp_path / "missing")], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0


def test_col_bwt_build_then_count_equals_brute_force(tmp_path):
    """`col-bwt build -r` on a small collection, then `col-bwt count`: mlen / occ of every read equal
    substring counting over the collection's text as oracle/rlbwt_oracle.py lays it out."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import rlbwt_oracle as ro
    rng = np.random.default_rng(12)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    base = rng.choice(acgt, size=1500)
    docs, paths = [], []
    for k in range(3):
        s = base.copy()
        mut = rng.random(s.size) < 0.02
        s[mut] = rng.choice(acgt, size=int(mut.sum()))
        docs.append([s.tobytes()])
        paths.append(str(tmp_path / f"g{k}.fa"))
        helpers.write_fasta(paths[-1], [s], [f"g{k}"])
    launcher = [sys.executable, os.path.join(ROOT, "col-bwt_amd", "col-bwt")]
    outp = str(tmp_path / "coll")
    out = subprocess.run(launcher + ["build", "-r", "-l", "20", "-o", outp] + paths, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    text, _ = ro.build_text(docs, revcomp=True)
    reads = [bytes(r) for r in helpers.reads_from_text(text, 200, (5, 150), 0.01, seed=13)]
    reads += [docs[0][0][:300], docs[1][0][-200:][::-1]]
    names = [f"p{k}" for k in range(len(reads))]
    fa = str(tmp_path / "reads.fa")
    helpers.write_fasta(fa, [np.frombuffer(r, np.uint8) for r in reads], names)
    out = subprocess.run(launcher + ["count", "-p", fa, outp], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = open(fa + ".count").read().splitlines()
    assert len(lines) == len(reads)
    for line, rd, nm in zip(lines, reads, names):
        name, m, mlen, occ = line.split("\t")
        want = count_restatement.brute_force(text, rd, with_sp=False)
        assert (name, int(m), int(mlen), int(occ)) == (nm, len(rd), want[0], want[1]), line


def test_count_calls_do_not_leak_hbm(pkg):
    import torch
    image = pkg.synth_index(1_000_000, mean_len=8, split_permille=0, seed=5)
    reads = helpers.backward_walk_reads(image, 2000, 100, 0.01, seed=1)
    bases, off = helpers.concat_reads(reads)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    tbl = pkg.ColPml.from_bytes(image)
    for _ in range(20):
        tbl.count_batch(bases, off, want_sp=True)
    tbl.close()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert free0 - free1 < 64 << 20, f"HBM leak: {free0 - free1} bytes"
