#!/usr/bin/env python3
"""CPU-tier check of the count kernel (csrc/count_query.h) and its host plumbing compiled
against the SIMT emulator (tests/emu/hip/hip_runtime.h), against the plain-Python restatement
(tests/count_restatement.py).  Run by tests/test_count_cpu.py in a subprocess with libasan
preloaded, so every out-of-bounds access is fatal.  Prints COUNT-EMU-OK at the end."""
import gzip
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from __graft_entry__ import load_package  # noqa: E402
import count_restatement  # noqa: E402
import helpers  # noqa: E402

pkg = load_package()
pkg.LIB_PATH = os.path.join(HERE, "libcolbwt_emu.so")   # emulated build instead of the HIP one

LINE_ROWS_4 = 4 | (4 << 8)          # include/colbwt.h COLBWT_LAYOUT_LINE_ROWS_STEPS(4)
LAYOUTS = (1, 2, 3, LINE_ROWS_4)


def check(image, reads, label, layouts=LAYOUTS):
    image = bytes(image)
    want = count_restatement.count_reads(image, reads)
    wm = np.array([w[0] for w in want], np.uint32)
    wo = np.array([w[1] for w in want], np.uint64)
    ws = np.array([w[2] for w in want], np.uint64)
    bases, off = helpers.concat_reads(reads)
    for layout in layouts:
        tbl = pkg.ColPml.from_bytes(image, layout=layout)
        assert tbl.info().layout == layout & 0xFF
        mlen, occ, sp, _ = tbl.count_batch(bases, off, want_sp=True)
        for name, got, exp in (("mlen", mlen, wm), ("occ", occ, wo), ("sp", sp, ws)):
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, f"{label}/L{layout}: {name} differs at reads {bad[:5]}: {got[bad[:5]]} != {exp[bad[:5]]}"
        mlen2, occ2, sp2, _ = tbl.count_batch(bases, off)           # without sp
        assert sp2 is None and np.array_equal(mlen2, wm) and np.array_equal(occ2, wo), f"{label}/L{layout}: no-sp form"
        tbl.close()
    print(f"ok {label}: {len(reads)} reads, {int(off[-1])} bases, whole-read matches {int((wm == [len(r) for r in reads]).sum())}")


def rand_reads(rng, n, lo, hi, alphabet=b"ACGT"):
    return [rng.choice(np.frombuffer(alphabet, np.uint8), size=int(m)) for m in rng.integers(lo, hi + 1, size=n)]


def check_file(image, reads):
    """colbwt_count_file on FASTA, FASTQ and .gz == a Python formatting of count_batch."""
    tbl = pkg.ColPml.from_bytes(bytes(image), layout=2)
    bases, off = helpers.concat_reads(reads)
    mlen, occ, _, _ = tbl.count_batch(bases, off)
    names = [f"read_{k}" for k in range(len(reads))]
    want = "".join(f"{names[k]}\t{len(reads[k])}\t{mlen[k]}\t{occ[k]}\n" for k in range(len(reads))).encode()
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
        for path in (fa, fq, gz):
            tbl.count_file(path, batch_bases=997)                 # several batches
            got = open(path + ".count", "rb").read()
            assert got == want, f"count_file {os.path.basename(path)}: {got[:200]!r} != {want[:200]!r}"
    tbl.close()
    print(f"ok count_file: {len(reads)} reads, FASTA / FASTQ / .gz")


def main():
    rng = np.random.default_rng(5)
    # true-BWT tables (several alphabets, repeats)
    seqs = [rng.choice(np.frombuffer(b"ACGT", np.uint8), size=300).tobytes() for _ in range(3)]
    seqs.append(seqs[0][50:200])                                  # repeats
    img, text = helpers.true_bwt_index(seqs, seed=3, extra_splits=60)
    reads = helpers.reads_from_text(text, 120, (1, 90), 0.01, seed=4, extra=b"Nn")
    reads += [np.frombuffer(text[:-1], np.uint8), np.zeros(0, np.uint8), np.frombuffer(b"NNAC", np.uint8)]
    check(img, reads, "true-bwt ACGT")
    img, text = helpers.true_bwt_index([bytes(rng.choice(np.frombuffer(b"ab", np.uint8), size=500))], seed=5)
    check(img, helpers.reads_from_text(text, 80, (1, 40), 0.0, seed=6, alphabet=b"ab"), "true-bwt sigma 2")
    img, text = helpers.true_bwt_index([bytes(rng.choice(np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8), size=600))],
                                       seed=7)
    check(img, helpers.reads_from_text(text, 80, (1, 30), 0.02, seed=8, alphabet=b"ACDEFGHIKLMNPQRSTVWY"),
          "true-bwt protein")
    # synthetic tables: sub-run splits, several alphabets, and long rows (> 65535: the len16 escape)
    for seed, alpha, max_len, split, r in ((1, b"ACGT", 9, 0.1, 3000), (2, b"AC", 5, 0.3, 2000),
                                           (3, b"ACGTNX", 30, 0.05, 2500), (4, b"ACGT", 90000, 0.2, 40)):
        trng = np.random.default_rng(seed)
        img = helpers.random_table(trng, r, alphabet=alpha, max_len=max_len, split_prob=split)
        reads = rand_reads(trng, 100, 0, 60, alpha + b"Z")
        reads += helpers.backward_walk_reads(img, 60, 40, 0.0, seed)
        check(img, reads, f"random table sigma {len(alpha)} max_len {max_len}")
    # one long run whose image covers thousands of one-position rows: the fast-forward leaves the
    # row-by-row walk for its search over idx[]
    trng = np.random.default_rng(6)
    chars = np.concatenate(([ord("C")], trng.choice(np.frombuffer(b"ACGT", np.uint8), size=6000)))
    lens = np.concatenate(([5000], np.ones(6000, np.int64)))
    idx = np.concatenate(([0], np.cumsum(lens)[:-1]))
    n = int(lens.sum())
    interval, offset = helpers.lf_columns(chars, idx, n)
    img = helpers.pack_col_pml(int((np.diff(chars) != 0).sum()) + 1, n, chars, idx, interval, offset,
                               np.zeros(len(chars), np.uint8), idx)
    reads = rand_reads(trng, 100, 1, 30) + helpers.backward_walk_reads(img, 100, 30, 0.0, 6)
    reads += [np.frombuffer(b"C" * k, np.uint8) for k in (1, 2, 3, 50)]
    check(img, reads, "long run over short rows")
    # ragged batch of > 64 reads: the host entry point orders the lanes
    img, text = helpers.true_bwt_index(seqs, seed=9)
    ragged = helpers.reads_from_text(text, 200, (1, 400), 0.0, seed=10)
    check(img, ragged, "ragged batch", layouts=(1, 2))
    check_file(img, ragged[:50] + [np.zeros(0, np.uint8)])
    check_replicas(img, ragged + [np.zeros(0, np.uint8)] * 2)
    check_device(img, ragged[:120] + [np.zeros(0, np.uint8)] * 2)
    print("COUNT-EMU-OK")


def aligned(n, dt, pad=0):
    """A zeroed array of n items (+ pad spare bytes) that starts on a 64-byte boundary."""
    size = n * np.dtype(dt).itemsize
    raw = np.zeros(size + pad + 64, np.uint8)
    o = (-raw.ctypes.data) % 64
    return raw[o:o + size].view(dt)


def check_replicas(image, reads):
    """Two replicas (one shard each) == one replica, with sp; their stats add up."""
    image = bytes(image)
    bases, off = helpers.concat_reads(reads)
    one = pkg.ColPml.from_bytes(image, layout=2)
    two = pkg.ColPml.from_bytes(image, layout=2, devices=[0, 0])
    assert two.info().n_devices == 2
    m1, o1, s1, st1 = one.count_batch(bases, off, want_sp=True)
    m2, o2, s2, st2 = two.count_batch(bases, off, want_sp=True)
    assert np.array_equal(m1, m2) and np.array_equal(o1, o2) and np.array_equal(s1, s2)
    for st in (st1, st2):
        assert st.n_reads == len(reads) and st.n_bases == int(off[-1]) and st.algorithmic_bytes == 0, st.as_dict()
    one.close(), two.close()
    print(f"ok two replicas == one: {len(reads)} reads, {int(off[-1])} bases")


def check_device(image, reads):
    """colbwt_count_device with and without d_order (and d_sp) == colbwt_count_batch, layouts 1, 2, 3, 5."""
    image = bytes(image)
    bases, off = helpers.concat_reads(reads)
    nr, nb = len(reads), int(off[-1])
    d_bases = aligned(nb, np.uint8, pad=64)
    d_bases[:nb] = bases
    d_off = aligned(nr + 1, np.uint64)
    d_off[:] = off
    d_order = aligned(nr, np.uint32)
    d_order[:] = np.argsort(-np.diff(off.astype(np.int64)), kind="stable")
    for layout in (1, 2, 3, 5):
        tbl = pkg.ColPml.from_bytes(image, layout=layout)
        mlen, occ, sp, _ = tbl.count_batch(bases, off, want_sp=True)
        for order in (None, d_order.ctypes.data):
            d_mlen, d_occ, d_sp = aligned(nr, np.uint32), aligned(nr, np.uint64), aligned(nr, np.uint64)
            st = tbl.count_device(d_bases.ctypes.data, d_off.ctypes.data, nr, nb, d_mlen.ctypes.data, d_occ.ctypes.data,
                                  d_sp.ctypes.data, order, timed=True)
            assert st.n_reads == nr and st.n_bases == nb and st.algorithmic_bytes == 0
            assert np.array_equal(d_mlen, mlen) and np.array_equal(d_occ, occ) and np.array_equal(d_sp, sp), (layout, order)
            d_mlen[:], d_occ[:] = 0, 0
            tbl.count_device(d_bases.ctypes.data, d_off.ctypes.data, nr, nb, d_mlen.ctypes.data, d_occ.ctypes.data,
                             None, order)
            assert np.array_equal(d_mlen, mlen) and np.array_equal(d_occ, occ), (layout, order, "no sp")
        tbl.close()
    print(f"ok count_device == count_batch: {nr} reads, layouts 1, 2, 3, 5, with / without order and sp")


if __name__ == "__main__":
    main()
