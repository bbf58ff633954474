#!/usr/bin/env python3
"""CPU-tier check of the seeds reduction (csrc/seeds_reduce.h) and its host plumbing compiled
against the SIMT emulator (tests/emu/hip/hip_runtime.h), against the plain-Python restatement
(tests/seeds_restatement.py) applied to the oracle's pml / cid.  Run by tests/test_seeds_cpu.py in a
subprocess with libasan preloaded, so every out-of-bounds access is fatal.  Prints SEEDS-EMU-OK at
the end."""
import gzip
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from __graft_entry__ import load_oracle, load_package  # noqa: E402
import helpers  # noqa: E402
import seeds_restatement as sr  # noqa: E402

pkg = load_package()
pkg.LIB_PATH = os.path.join(HERE, "libcolbwt_emu.so")   # emulated build instead of the HIP one
oracle = load_oracle()

LINE_ROWS_4 = 4 | (4 << 8)          # include/colbwt.h COLBWT_LAYOUT_LINE_ROWS_STEPS(4)
LAYOUTS = (1, 2, 3, LINE_ROWS_4)


def summary_array(summary):
    return summary.view(np.uint32).reshape(-1, 8)


def same(label, got, want):
    for name, g, w in zip(("summary", "seed_pos", "seed_len", "seed_cid"), got, want):
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{label}: {name} differs at {bad[:5].tolist()}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}"


def aligned(n, dt, fill=0):
    """An array of n items, all `fill`, that starts on a 64-byte boundary."""
    size = n * np.dtype(dt).itemsize
    raw = np.zeros(size + 64, np.uint8)
    o = (-raw.ctypes.data) % 64
    a = raw[o:o + size].view(dt)
    a[...] = fill
    return a


def reduce_device(pml, cid, off, min_len, max_seeds, slots=True):
    """colbwt_seeds_reduce_device over host arrays (the emulated device is host memory)."""
    nr, nb = len(off) - 1, len(pml)
    d_pml = aligned(nb, pml.dtype)
    d_pml[:] = pml
    d_cid = aligned(nb, np.uint8)
    d_cid[:] = cid
    d_off = aligned(nr + 1, np.uint64)
    d_off[:] = off
    d_sum = aligned(nr * 8, np.uint32, 0xAB)
    d_pos, d_len, d_sc = aligned(nr * max_seeds, np.uint32, 7), aligned(nr * max_seeds, np.uint32, 7), aligned(nr * max_seeds, np.uint8, 7)
    ptr = (lambda a: a.ctypes.data) if slots else (lambda a: None)
    st = pkg.seeds_reduce_device(d_pml.ctypes.data, d_cid.ctypes.data, d_off.ctypes.data, nr, nb, min_len, max_seeds,
                                 d_sum.ctypes.data, ptr(d_pos), ptr(d_len), ptr(d_sc), pml_bytes=pml.dtype.itemsize, timed=True)
    assert st.n_reads == nr and st.n_bases == nb
    if not slots:
        assert (d_pos == 7).all() and (d_len == 7).all() and (d_sc == 7).all(), "slot arrays touched though omitted"
    return d_sum.reshape(nr, 8), d_pos.reshape(nr, max_seeds), d_len.reshape(nr, max_seeds), d_sc.reshape(nr, max_seeds)


def check_index(image, reads, label, layouts=LAYOUTS, params=((1, 1000), (3, 3), (8, 1), (20, 3))):
    image = bytes(image)
    bases, off = helpers.concat_reads(reads)
    wide = max((len(r) for r in reads), default=0) > 65535
    epml, ecid = oracle.OracleIndex(image).query_batch(bases, off, wide=wide)
    for layout in layouts:
        tbl = pkg.ColPml.from_bytes(image, layout=layout)
        for min_len, max_seeds in params:
            want = sr.seeds(epml, ecid, off, min_len, max_seeds)
            sr.check_invariants(*want[:3], off, min_len, max_seeds)
            summary, pos, ln, sc, st = tbl.seeds_batch(bases, off, min_len, max_seeds)
            assert st.n_reads == len(reads) and st.n_bases == int(off[-1])
            same(f"{label}/L{layout}/l{min_len}/k{max_seeds}", (summary_array(summary), pos, ln, sc), want)
        only, p0, l0, c0, _ = tbl.seeds_batch(bases, off, 3, 3, want_seeds=False)      # the slot arrays omitted
        assert p0 is None and l0 is None and c0 is None
        assert np.array_equal(summary_array(only), sr.seeds(epml, ecid, off, 3, 3)[0]), f"{label}/L{layout}: summaries only"
        tbl.close()
    print(f"ok {label}: {len(reads)} reads, {int(off[-1])} bases, layouts {layouts}")


def check_crafted():
    """colbwt_seeds_reduce_device on arrays no query would produce."""
    rng = np.random.default_rng(11)

    def both(label, pml, cid, off, params=((1, 4), (3, 2), (8, 1), (20, 1000))):
        pml, cid, off = np.asarray(pml), np.asarray(cid, np.uint8), np.asarray(off, np.uint64)
        for min_len, max_seeds in params:
            want = sr.seeds(pml, cid, off, min_len, max_seeds)
            same(f"{label}/l{min_len}/k{max_seeds}", reduce_device(pml, cid, off, min_len, max_seeds), want)
        got = reduce_device(pml, cid, off, *params[0], slots=False)
        assert np.array_equal(got[0], sr.seeds(pml, cid, off, *params[0])[0]), f"{label}: summaries only"

    n = 1500
    even = np.arange(0, n + 1, 100)
    both("all-zero pml", np.zeros(n, np.uint16), rng.integers(0, 256, n), even)
    ramp = np.tile(np.arange(100, 0, -1), n // 100).astype(np.uint16)     # every read one run
    both("col ids everywhere", ramp, rng.integers(1, 256, n), even)
    both("col ids nowhere", ramp, np.zeros(n), even)
    both("one read, u32", ramp.astype(np.uint32), rng.integers(0, 3, n), [0, n])
    # runs that end exactly on 8-, 64- and 512-element boundaries (and one past / one short of them)
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
    # read-start alignments 0..15: a few reads after a first read of a + 16 bases
    for a in range(16):
        lens = [a + 16, 1, 0, 37, 600, 2, 0, 0, 9]
        off = np.concatenate(([0], np.cumsum(lens)))
        nb = int(off[-1])
        pml = rng.integers(0, 4, nb).astype(np.uint16)
        cid = np.where(rng.random(nb) < 0.3, rng.integers(1, 256, nb), 0)
        both(f"alignment {a}", pml, cid, off, params=((1, 3), (3, 1000)))
    # arbitrary arrays, many tiny reads (several read starts per lane), empty reads at both ends
    lens = np.concatenate(([0, 0], rng.integers(0, 6, 700), [0, 0, 0]))
    off = np.concatenate(([0], np.cumsum(lens)))
    nb = int(off[-1])
    both("tiny reads", rng.integers(0, 3, nb).astype(np.uint16), rng.integers(0, 3, nb), off, params=((1, 2), (2, 5)))
    both("only empty reads", np.zeros(0, np.uint16), np.zeros(0), np.zeros(70, np.uint64), params=((1, 2),))
    # several waves and blocks (the pass cuts the bases into chunks of at least 2048), large values
    lens = rng.integers(0, 900, 40)
    off = np.concatenate(([0], np.cumsum(lens)))
    nb = int(off[-1])
    pml = np.where(rng.random(nb) < 0.05, 0, rng.integers(1, 2 ** 32, nb)).astype(np.uint32)
    both("u32 arbitrary, several waves", pml, np.where(rng.random(nb) < 0.02, rng.integers(1, 256, nb), 0), off,
         params=((1, 3), (1 << 31, 1000)))
    print("ok crafted arrays through seeds_reduce_device")


def check_file(image, reads):
    """colbwt_seeds_file on FASTA, FASTQ and .gz == a Python formatting of the restatement."""
    image = bytes(image)
    tbl = pkg.ColPml.from_bytes(image, layout=2)
    bases, off = helpers.concat_reads(reads)
    epml, ecid = oracle.OracleIndex(image).query_batch(bases, off)
    names = [f"read_{k}" for k in range(len(reads))]
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "r.fa")
        helpers.write_fasta(fa, reads, names)
        fq = os.path.join(d, "r.fq")
        with open(fq, "wb") as f:
            for nm, rd in zip(names, reads):
                f.write(b"@" + nm.encode() + b" extra words\n" + bytes(rd) + b"\n+\n" + b"I" * len(rd) + b"\n")
        gz = os.path.join(d, "r.fq.gz")
        with open(fq, "rb") as src, gzip.open(gz, "wb") as dst:
            dst.write(src.read())
        for min_len, max_seeds in ((1, 3), (8, 16)):
            want = sr.format_lines(names, off, *sr.seeds(epml, ecid, off, min_len, max_seeds), max_seeds)
            for path in (fa, fq, gz):
                tbl.seeds_file(path, min_len=min_len, max_seeds=max_seeds, batch_bases=997)      # several batches
                got = open(path + ".seeds", "rb").read()
                assert got == want, f"seeds_file {os.path.basename(path)}: {got[:300]!r} != {want[:300]!r}"
        tbl.seeds_file(fa, os.path.join(d, "elsewhere.txt"), min_len=8, max_seeds=16)
        assert open(os.path.join(d, "elsewhere.txt"), "rb").read() == want
    tbl.close()
    print(f"ok seeds_file: {len(reads)} reads, FASTA / FASTQ / .gz")


def check_replicas(image, reads):
    image = bytes(image)
    bases, off = helpers.concat_reads(reads)
    one = pkg.ColPml.from_bytes(image, layout=2)
    two = pkg.ColPml.from_bytes(image, layout=2, devices=[0, 0])
    assert two.info().n_devices == 2
    a, b = one.seeds_batch(bases, off, 3, 4), two.seeds_batch(bases, off, 3, 4)
    same("two replicas", (summary_array(b[0]),) + b[1:4], (summary_array(a[0]),) + a[1:4])
    assert b[4].n_reads == len(reads) and b[4].n_bases == int(off[-1])
    one.close(), two.close()
    print(f"ok two replicas == one: {len(reads)} reads")


def check_errors(image):
    tbl = pkg.ColPml.from_bytes(bytes(image), layout=1)
    bases, off = helpers.concat_reads([np.frombuffer(b"ACGT", np.uint8)])
    for min_len, max_seeds in ((0, 4), (1, 0), (1, (1 << 16) + 1)):
        try:
            tbl.seeds_batch(bases, off, min_len, max_seeds)
        except pkg.ColbwtError as e:
            assert e.code == -1, e
        else:
            raise AssertionError(f"min_len {min_len} max_seeds {max_seeds} accepted")
    s, where = tbl.seeds(b"ACGTACGT", min_len=1, max_seeds=4)
    assert s["cov"] + s["resets"] == 8 and len(where) == min(s["n_seeds"], 4)
    tbl.close()
    print("ok argument errors")


def main():
    rng = np.random.default_rng(5)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    seqs = [rng.choice(acgt, size=300).tobytes() for _ in range(3)]
    seqs.append(seqs[0][50:200])
    img, text = helpers.true_bwt_index(seqs, seed=3, extra_splits=60)
    reads = helpers.reads_from_text(text, 90, (1, 160), 0.03, seed=4, extra=b"Nn")
    reads += [np.frombuffer(text[:-1], np.uint8), np.zeros(0, np.uint8), np.frombuffer(b"A", np.uint8),
              np.frombuffer(b"N", np.uint8), np.zeros(0, np.uint8)]
    reads = [np.zeros(0, np.uint8)] + reads
    check_index(img, reads, "true-bwt ragged")
    # reads longer than one wave iteration (512 bases), with substitutions so that they hold many runs
    long_text = np.frombuffer(text[:-1], np.uint8)
    longs = []
    for k in range(6):
        rd = np.concatenate([long_text[(37 * k) % 200:], long_text[: 300 + 50 * k]])
        rd = rd.copy()
        rd[rng.integers(0, rd.size, rd.size // 25)] = ord("T")
        longs.append(rd)
    check_index(img, longs + [np.zeros(0, np.uint8)] + reads[:20], "reads > 512 bases", params=((1, 1000), (8, 3)))
    # synthetic table
    trng = np.random.default_rng(2)
    simg = helpers.random_table(trng, 2500, alphabet=b"ACGT", max_len=9, split_prob=0.1)
    sreads = helpers.backward_walk_reads(simg, 60, 120, 0.03, 2) + [trng.choice(acgt, size=int(m)) for m in trng.integers(0, 80, 40)]
    check_index(simg, sreads, "random table", layouts=(1, LINE_ROWS_4), params=((1, 1000), (3, 3)))
    # one read > 65535 bases: the u32 path
    giant = np.tile(long_text, 66000 // long_text.size + 1)[:66000].copy()
    giant[rng.integers(0, giant.size, 900)] = ord("G")
    check_index(img, [reads[3], giant, reads[5]], "read > 65535 bases", layouts=(3,), params=((8, 1000), (1, 3)))
    check_crafted()
    check_file(img, reads[:40] + [np.zeros(0, np.uint8)])
    check_replicas(img, reads)
    check_errors(img)
    print("SEEDS-EMU-OK")


if __name__ == "__main__":
    main()
