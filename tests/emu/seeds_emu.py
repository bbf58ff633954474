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


KNOB = helpers.SEEDS_KNOB
WAVE_CHUNKS = (512, 1024, 2048, 2560, 16384)


class knob:
    """COLBWT_SEEDS_CHUNK=`chunk` for the launches inside (the library reads it at every launch)."""

    def __init__(self, chunk):
        self.chunk = chunk

    def __enter__(self):
        os.environ[KNOB] = str(self.chunk)

    def __exit__(self, *exc):
        del os.environ[KNOB]


def lens_from_cuts(cuts, n_bases):
    """Read lengths of a batch of n_bases bases cut at the positions `cuts`, in any order (a position
    given n times: n - 1 empty reads there; 0 and n_bases are cuts already, so n times means n)."""
    cuts = sorted([0] + [int(v) for v in cuts])
    return np.diff(np.asarray(cuts + [n_bases], np.int64))


def check_wave_boundaries():
    """Which wave owns a read (csrc/seeds_reduce.h: the one whose chunk [w c, (w+1) c) holds the read's
    first base; the last wave to the end), with the chunk c forced to 512, 1024, 2048, 2560 and 16384:
    read starts and runs of empty reads placed on, one before and one after k c, a read over several
    whole chunks, batches of exactly k c bases with and without trailing empty reads.  Every read of
    every batch against the restatement, u16 and u32, with the slot arrays and without."""
    rng = np.random.default_rng(23)
    runs = {"launches": 0, "bases": 0}

    def arrays(nb, dt, nonzero=(), zero=()):
        """Random pml (about 15 % zeros) and col ids (about 20 % non-zero); `nonzero` / `zero`: ranges forced."""
        pml = np.where(rng.random(nb) < 0.15, 0, rng.integers(1, 60, nb)).astype(dt)
        if dt is np.uint32:
            big = rng.random(nb) < 0.3
            pml[big & (pml > 0)] += np.uint32(1 << 31)
        for lo, hi in nonzero:
            pml[max(lo, 0):min(hi, nb)] = 7
        for lo, hi in zero:
            pml[max(lo, 0):min(hi, nb)] = 0
        cid = np.where(rng.random(nb) < 0.2, rng.integers(1, 256, nb), 0).astype(np.uint8)
        return pml, cid

    def run(label, c, lens, nonzero=(), zero=(), waves=None):
        lens = np.asarray(lens, np.int64)
        off = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
        nb = int(off[-1])
        assert helpers.seeds_chunk(nb, os.environ) == c, (label, c)
        if waves is not None:
            assert helpers.seeds_waves(nb, c) == waves, (label, nb, c, waves)
        for dt, params in ((np.uint16, ((1, 4), (3, 2))), (np.uint32, ((1, 3), (1 << 31, 5)))):
            pml, cid = arrays(nb, dt, nonzero, zero)
            for k, (min_len, max_seeds) in enumerate(params):
                want = sr.seeds(pml, cid, off, min_len, max_seeds)
                name = f"chunk {c}: {label}/{np.dtype(dt).name}/l{min_len}/k{max_seeds}"
                same(name, reduce_device(pml, cid, off, min_len, max_seeds), want)
                if k == 0:
                    got = reduce_device(pml, cid, off, min_len, max_seeds, slots=False)
                    assert np.array_equal(got[0], want[0]), f"{name}: summaries only"
                    runs["launches"] += 1
                runs["launches"] += 1
                runs["bases"] += nb
        return off

    def fill(lo, hi, top):
        """Read starts strictly inside (lo, hi), reads of up to about `top` bases."""
        n = max((hi - lo) // max(top // 2, 1), 1)
        return np.unique(rng.integers(lo + 1, hi, n)).tolist() if hi - lo > 1 else []

    for c in WAVE_CHUNKS:
        top = 300 if c < 16384 else 2500
        with knob(c):
            # read starts at c - 1 (the read, and a PML run inside it, span the boundary), 2c, 3c + 1 (base 3c
            # is the last of the previous read and of its run), and one-base reads at 4c - 1, 4c, 4c + 1
            cuts = [c - 1, 2 * c, 3 * c + 1, 4 * c - 1, 4 * c, 4 * c + 1]
            for a, b in ((0, c - 1), (c + 40, 2 * c), (2 * c, 3 * c - 40), (3 * c + 1, 4 * c - 1), (4 * c + 2, 4 * c + 90)):
                cuts += fill(a, b, top)
            off = run("read starts", c, lens_from_cuts(cuts, 4 * c + 90), waves=5,
                      nonzero=((c - 4, c + 5), (3 * c - 3, 3 * c + 1), (2 * c - 2, 2 * c + 3)), zero=((3 * c + 1, 3 * c + 2),))
            for want_start in (c - 1, 2 * c, 3 * c + 1, 4 * c - 1, 4 * c, 4 * c + 1):
                assert want_start in off
            assert not ((off > c - 1) & (off <= c + 5)).any()
            # runs of empty reads exactly at k c: at 0 (before the first read: nothing ends there), at c (after a
            # read that ends there and before one that starts there), at 2c = n_bases (after the last read:
            # nothing starts there).  More than 64 boundaries: the mark loop's second round.
            for n_e in (1, 63, 64, 65, 200):
                cuts = [0] * n_e + [c] * (n_e + 1) + [2 * c] * n_e + fill(0, c, top) + fill(c, 2 * c, top)
                run(f"{n_e} empty reads at 0, c, 2c", c, lens_from_cuts(cuts, 2 * c), waves=2)
            # the same run one base off the boundary on either side: the other wave owns it
            cuts = [c - 1] * 66 + [2 * c + 1] * 66 + fill(0, c - 1, top) + fill(c, 2 * c, top) + fill(2 * c + 2, 2 * c + 60, top)
            run("65 empty reads at c - 1 and 2c + 1", c, lens_from_cuts(cuts, 2 * c + 60), waves=3)
            # one read of 3c + 17 bases from c - 5: the waves of [c, 4c) own nothing; tiny reads on both sides
            tiny = rng.integers(0, 6, 4 * c)
            left = tiny[:np.searchsorted(np.cumsum(tiny), c - 5, side="right")]
            left = np.concatenate((left, [c - 5 - left.sum()]))
            right = tiny[2 * c:2 * c + 150]
            lens = np.concatenate((left, [3 * c + 17], right))
            off = run("read over three whole chunks", c, lens, nonzero=((2 * c - 9, 2 * c + 9),), zero=((3 * c, 3 * c + 1),))
            assert int(off[len(left)]) == c - 5 and int(off[len(left) + 1]) == 4 * c + 12
            assert not ((off >= c) & (off < 4 * c)).any() and int(off[-1]) > 4 * c + 12
            # n_bases an exact multiple of c
            body = fill(0, 3 * c, top) + [c, 2 * c - 1]
            run("n_bases 3c, the last read ends there", c, lens_from_cuts(body, 3 * c), waves=3)
            for n_e in (1, 64, 70):
                run(f"n_bases 2c and {n_e} trailing empty reads", c, lens_from_cuts(fill(0, 2 * c, top) + [2 * c] * n_e, 2 * c), waves=2)
            for n_e in (3, 70):
                cuts = [v for v in fill(0, c, top)] + [c - 7] + [2 * c] * n_e      # the last non-empty read: [c - 7, 2c)
                cuts = [v for v in cuts if v <= c - 7 or v == 2 * c]
                run(f"a read over the whole last chunk and {n_e} trailing empty reads", c, lens_from_cuts(cuts, 2 * c), waves=2)
            run("n_bases c in one read", c, [c], waves=1)
            run("n_bases c in one read, empty reads around", c, [0, 0, c, 0], waves=1)
            if c == 16384:
                # one wave, 32 tiles, about 6000 read ends (more than 64 in most tiles), one read of 600 bases
                tiny = rng.integers(0, 6, 8000)
                half = tiny[:np.searchsorted(np.cumsum(tiny), (c - 600) // 2)]
                rest = tiny[4000:4000 + np.searchsorted(np.cumsum(tiny[4000:]), c - 600 - half.sum(), side="right")]
                lens = np.concatenate((half, [600], rest, [c - 600 - half.sum() - rest.sum()]))
                off = run("one wave of reads of 0..5 bases", c, lens, waves=1)
                assert len(lens) > 5500 and int(off[-1]) == c
                ends = np.bincount((off[1:][lens > 0] - 1).astype(np.int64) // 512, minlength=32)
                assert (ends > 64).sum() >= 20, ends
        print(f"ok wave boundaries at chunk {c}")
    assert KNOB not in os.environ
    print(f"ok wave boundaries: {runs['launches']} launches, {runs['bases']} bases compared")


def check_batch_under_knob(image, reads):
    """seeds_batch (the query, then the pass over the shard's rebased read_off) with the chunk forced
    to 512 (many waves per shard) and to 16384 (one), one replica and two."""
    for c in (512, 16384):
        with knob(c):
            assert helpers.seeds_chunk(int(sum(len(r) for r in reads)), os.environ) == c
            check_index(image, reads, f"seeds_batch at chunk {c}", layouts=(2, LINE_ROWS_4), params=((1, 1000), (8, 3)))
            check_replicas(image, reads)


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
    assert helpers.SEEDS_KNOB not in os.environ       # everything above ran with the product's own chunk
    check_wave_boundaries()
    check_batch_under_knob(img, reads)
    print("SEEDS-EMU-OK")


if __name__ == "__main__":
    main()
