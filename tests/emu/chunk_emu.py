#!/usr/bin/env python3
"""CPU-tier check of the persistent lanes' MULTI-READ chunks (csrc/fat_cursor.h ChunkPlan /
ReadCursor, the wave collectors of csrc/lane_out.h and csrc/lane_io.h) on ragged batches: the
three persistent-lane kernels (layouts 3, 4, 5 and 6) compiled against the SIMT emulator, every
base of every read against the oracle.  Run by tests/test_emu_chunks.py in a subprocess with
libasan preloaded.  Prints CHUNK-EMU-OK at the end.

A workgroup takes chunks of `big` >= 2 reads only when its share of the batch exceeds 2 x 256
reads, and the product chooses big >= 2 only for millions of reads, so the batches here have
1000-2100 reads on the emulator's two workgroups and set COLBWT_LINE_ROWS_CHUNK
("<big>[,<tail permille>]", read at every launch).  Every case states the geometry it is meant to
run with (shares, big chunks per workgroup) and asserts it from helpers.ChunkPlan, the Python
restatement of the plan, so a later change of the plan cannot quietly turn it into a case of
single reads.

The tests pin results, not scheduling: which lane takes which chunk is free.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from __graft_entry__ import load_oracle, load_package  # noqa: E402
import helpers  # noqa: E402

pkg = load_package()
pkg.LIB_PATH = os.path.join(HERE, "libcolbwt_emu.so")   # emulated build instead of the HIP one
oracle = load_oracle()

KNOB = "COLBWT_LINE_ROWS_CHUNK"
RESIDENT = 2            # workgroups the emulated device keeps resident: 2 CUs x 1 block (hip/hip_runtime.h)
PAT16, PAT8 = 0xA5C3, 0x5A                             # what untouched output memory holds

# (reads, setting, the shares of the two workgroups, their big chunks).  Together: big chunks in
# both workgroups; more big chunks than lanes (269 > 256: big chunks are CLAIMED from the LDS
# counter, not only taken as the lanes' own first chunks); shares of exactly 512, 513,
# 512 + big - 1 (no big chunk yet) and 512 + big reads; n_reads % 2 of 0 and 1 (the two branches of
# read_lo); tail permille 0, 100 and 1000 (single reads only: the control); big 2, 3, 8.
GEOMETRIES = (
    (1400, "3,100", (700, 700), (62, 62)),
    (1400, "8,0", (700, 700), (23, 23)),
    (1401, "2,1000", (701, 700), (0, 0)),
    (1025, "3,100", (513, 512), (0, 0)),
    (1029, "3", (515, 514), (1, 0)),
    (2101, "2,0", (1051, 1050), (269, 269)),
)
# the emulator's time goes with the bases: the lengths from 95 up are drawn half as often as the others
WEIGHTS = [0.5 if m >= 95 else 1.0 for m in helpers.EDGE_LENGTHS]
KINDS = ("first_empty", "last_empty", "all_empty", "small_then_wide", "middle_empty")
seen = {k: 0 for k in KINDS}                            # placements over all cases, checked at the end
seen.update(claimed=0, launches=0)


def layouts(case):
    """All three kernels and the deep entries, look-ahead depth 4 .. 8 varying with the case."""
    k = [(4 + (case + d) % 5) << 8 for d in range(3)]
    return (3, 4 | k[0], 5 | k[1], 6 | k[2])


def plans_of(n_reads, setting, shares=None, n_big=None):
    big, permille = helpers.chunk_setting(setting)
    plans = helpers.chunk_plans(n_reads, RESIDENT, big, permille)
    if shares is not None:
        got = tuple(p.n for p in plans), tuple(p.n_big for p in plans)
        assert got == (tuple(shares), tuple(n_big)), f"{n_reads} reads at {setting}: plan gives {got}"
    return plans


def place(lens, plans, rng):
    """Deliberate placements in a batch of lengths (changed in place).  Returns the placed chunks
    as (kind, block, chunk) and the mask of reads whose length is now fixed."""
    n = len(lens)
    fixed = np.zeros(n, bool)
    placed = []

    def put(reads, values):
        assert not fixed[reads].any()
        lens[reads] = values
        fixed[reads] = True

    for b, p in enumerate(plans):
        # workgroup 0 starts with its chunk 0 (read 0 of the batch is empty), the others leave their
        # first read to the share boundary below
        first = 0 if b == 0 else 1
        step = max(2, p.n_big // 12)
        starts = list(range(first, p.n_big, step))
        starts += [c for c in range(256, p.n_big - 1, 2)][:5]           # claimed big chunks
        at = 0
        for c in starts:
            kind = KINDS[at % len(KINDS)]
            if kind == "middle_empty" and p.big < 3:
                at += 1
                kind = KINDS[at % len(KINDS)]
            if kind == "small_then_wide" and c + 1 >= p.n_big:
                kind = "last_empty"
            f, l = p.first_read(c), p.last_read(c)
            reads = np.arange(f, l + 1 + (p.big if kind == "small_then_wide" else 0))
            if fixed[reads].any():
                continue
            at += 1
            v = np.where(lens[reads] == 0, 9, lens[reads])             # nonempty unless the kind says so
            if kind == "first_empty":
                v[0] = 0
            elif kind == "last_empty":
                v[-1] = 0
            elif kind == "middle_empty":
                v[len(v) // 2] = 0
            elif kind == "all_empty":
                v[:] = 0
            else:   # fewer than 64 bases in all, then a chunk over several 64-element blocks
                v[:p.big] = rng.choice([1, 2, 3, 7], size=p.big)
                v[p.big:] = rng.choice([97, 129, 200], size=p.big)
            put(reads, v)
            placed.append((kind, b, c))
    if not fixed[0]:
        put(np.array([0]), 0)
    assert lens[0] == 0                                                # empty reads at both ends of the batch
    put(np.array([n - 1]), 0)
    for p in plans[1:]:                                                # ragged reads on both sides of a share boundary
        put(np.array([p.read_lo - 1, p.read_lo]), [13, 27])
    return placed, fixed


def nudge(lens, fixed, read, delta):
    """Moves the first base of `read` up by delta: the nearest read below it whose length is free grows."""
    k = read - 1
    while fixed[k]:
        k -= 1
    lens[k] += delta
    fixed[k] = True


def align(lens, fixed, plans, placed, base=0):
    """Small chunks get no block boundary inside, share boundaries fall inside a 16-byte piece (so
    inside a 64-element block too): lengths below them grow by a few bases, in address order."""
    events = [(plans[b].first_read(c), plans[b].last_read(c)) for kind, b, c in placed if kind == "small_then_wide"]
    events += [(p.read_lo, None) for p in plans[1:]]
    for f, l in sorted(events):
        lo = base + int(lens[:f].sum())
        if l is None:
            if lo % 16 == 0:
                nudge(lens, fixed, f - 1, 5)
        elif lo // 64 != (lo + int(lens[f:l + 1].sum()) - 1) // 64:
            nudge(lens, fixed, f, 64 - lo % 64)


def verify_placements(off, plans, placed, base_read=0):
    """What the case claims about its batch, from the plan and the final offsets."""
    ln = np.diff(off.astype(np.int64))[base_read:]
    o = off.astype(np.int64)[base_read:]
    small_ok = 0
    for kind, b, c in placed:
        p = plans[b]
        assert c < p.n_big and p.last_read(c) - p.first_read(c) + 1 == p.big >= 2
        f, l = p.first_read(c), p.last_read(c)
        v = ln[f:l + 1]
        if kind == "first_empty":
            assert v[0] == 0 and (v[1:] > 0).all()
        elif kind == "last_empty":
            assert v[-1] == 0 and (v[:-1] > 0).all()
        elif kind == "middle_empty":
            assert p.big >= 3 and v[len(v) // 2] == 0 and v[0] > 0 and v[-1] > 0
        elif kind == "all_empty":
            assert (v == 0).all()
        else:
            assert 0 < v.sum() < 64 and o[f] // 64 == (o[l + 1] - 1) // 64, (b, c, o[f], o[l + 1])
            f2, l2 = p.first_read(c + 1), p.last_read(c + 1)
            assert c + 1 < p.n_big and f2 == l + 1 and (o[l2 + 1] - 1) // 64 - o[f2] // 64 >= 2
            small_ok += 1
        seen[kind] += 1
        seen["claimed"] += c >= helpers.QUERY_BLOCK
    assert ln[0] == 0 and ln[plans[-1].read_lo + plans[-1].n - 1] == 0
    for p in plans[1:]:
        assert ln[p.read_lo - 1] % 8 and ln[p.read_lo] % 8 and o[p.read_lo] % 16, "share boundary"
    return small_ok


def make_index(case):
    """(image, source of match-heavy reads) -- a different kind of table per case."""
    rng = np.random.default_rng(1000 + case)
    kind = case % 4
    if kind == 0:
        img = pkg.synth_index(3000, mean_len=6, split_permille=50, seed=60 + case)
    elif kind == 1:
        base = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=400)
        seqs = []
        for _ in range(4):
            s = base.copy()
            mut = rng.random(400) < 0.03
            s[mut] = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(mut.sum()))
            seqs.append(bytes(s))
        img, text = helpers.true_bwt_index(seqs, seed=case, extra_splits=60)
        return bytes(img), text
    elif kind == 2:
        img = helpers.random_table(rng, 1500, alphabet=b"\x01ACGNTac")   # sigma 8: characters without a slot
    else:
        img = pkg.synth_index(2500, mean_len=6, split_permille=50, seed=60 + case, thr_mode=1)
    img = bytes(img)
    walks = helpers.backward_walk_reads(img, 6, 1500, 0.0, seed=case)
    return img, b"".join(bytes(w) for w in walks)


def make_batch(case, n_reads, setting, shares=None, n_big=None, before=0, after=0, source=None, giant=0):
    """A ragged batch with the placements for `setting`, preceded / followed by `before` / `after`
    reads that are not part of the launch.  giant: length of one read put into a big chunk."""
    rng = np.random.default_rng(case)
    plans = plans_of(n_reads, setting, shares, n_big)
    lens = helpers.ragged_lengths(rng, n_reads, n_long=4, weights=WEIGHTS)
    placed, fixed = place(lens, plans, rng)
    pre = helpers.ragged_lengths(rng, before, weights=WEIGHTS)
    if before:
        pre[-1] += (int(pre.sum()) % 64 == 0) * 3 + (int(pre.sum()) % 16 == 0)     # the launch does not start on a block boundary
    if giant:
        p = plans[0]
        c = p.n_big // 2
        while fixed[p.first_read(c):p.last_read(c) + 1].any():
            c += 1
        assert c < p.n_big
        lens[p.first_read(c) + 1] = giant
        fixed[p.first_read(c) + 1] = True
    align(lens, fixed, plans, placed, base=int(pre.sum()))
    all_lens = np.concatenate((pre, lens, helpers.ragged_lengths(rng, after, weights=WEIGHTS)))
    bases, off = helpers.ragged_reads(source, all_lens, rng)
    small = verify_placements(off, plans, placed, base_read=before)
    return bases, off, plans, placed, small


def run_host(case, n_reads, setting, shares, n_big, wide=False, giant=0, source_len=0):
    t0 = time.time()
    img, source = make_index(case)
    if source_len:
        source = bytes(helpers.backward_walk_reads(img, 1, source_len, 0.0005, seed=case)[0])
    bases, off, plans, placed, small = make_batch(case, n_reads, setting, shares, n_big, source=source, giant=giant)
    epml, ecid = oracle.OracleIndex(img).query_batch(bases, off, wide=wide)
    os.environ[KNOB] = setting
    for layout in layouts(case):
        tbl = pkg.ColPml.from_bytes(img, layout=layout)
        assert tbl.info().layout == layout & 0xFF
        pml, cid, _ = tbl.query_batch(bases, off, wide=wide)
        seen["launches"] += 1
        assert np.array_equal(pml, epml), f"case {case} {setting} L{layout:#x}: PML differs at {np.flatnonzero(pml != epml)[:8]}"
        assert np.array_equal(cid, ecid), f"case {case} {setting} L{layout:#x}: col ids differ at {np.flatnonzero(cid != ecid)[:8]}"
        tbl.close()
    del os.environ[KNOB]
    kinds = sorted({k for k, _, _ in placed})
    print(f"ok case {case}: {n_reads} reads, {int(off[-1])} bases, {KNOB}={setting}, {'u32' if wide else 'u16'}, shares "
          f"{[p.n for p in plans]}, big chunks {[p.n_big for p in plans]}, placed {len(placed)} {kinds}, "
          f"{time.time() - t0:.1f} s", flush=True)


def aligned(n, dt, fill):
    """An array of n items that starts on a 64-byte boundary, filled with `fill`."""
    size = n * np.dtype(dt).itemsize
    raw = np.zeros(size + 64, np.uint8)
    o = (-raw.ctypes.data) % 64
    out = raw[o:o + size].view(dt)
    out[:] = fill
    return out


def run_device(case, n_reads, setting, shares, n_big, before, after, orders):
    """colbwt_query_device[_ordered] on caller memory: the launch covers reads [before, before +
    n_reads) of a larger batch through a d_read_off that points into the middle of its offsets
    (absolute offsets: the first read does not start at base 0, nor on a block boundary), and must
    write exactly its own bases -- everything else in the output arrays, a guard behind the last
    base included, keeps its pattern."""
    t0 = time.time()
    img, source = make_index(case)
    bases, off, plans, placed, _ = make_batch(case, n_reads, setting, shares, n_big, before, after, source)
    nb_all = int(off[-1])
    lo, hi = int(off[before]), int(off[before + n_reads])
    assert (lo % 64 != 0) == (before != 0)
    epml, ecid = oracle.OracleIndex(img).query_batch(bases, off)
    guard = 256
    d_bases = aligned(nb_all + 64, np.uint8, 0)              # the kernels read whole 64-byte blocks
    d_bases[:nb_all] = bases
    d_off = aligned(len(off), np.uint64, 0)
    d_off[:] = off
    d_order = aligned(n_reads, np.uint32, 0)
    d_order[:] = np.argsort(-np.diff(off[before:before + n_reads + 1].astype(np.int64)), kind="stable")
    os.environ[KNOB] = setting
    for layout in layouts(case):
        tbl = pkg.ColPml.from_bytes(img, layout=layout)
        for order in orders:
            d_pml, d_cid = aligned(nb_all + guard, np.uint16, PAT16), aligned(nb_all + guard, np.uint8, PAT8)
            tbl.query_device(d_bases.ctypes.data, d_off.ctypes.data + 8 * before, n_reads, hi - lo, d_pml.ctypes.data,
                             d_cid.ctypes.data, d_order=d_order.ctypes.data if order else None)
            seen["launches"] += 1
            where = f"case {case} {setting} L{layout:#x} order {order}"
            assert np.array_equal(d_pml[lo:hi], epml[lo:hi]), f"{where}: PML differs at {lo + np.flatnonzero(d_pml[lo:hi] != epml[lo:hi])[:8]}"
            assert np.array_equal(d_cid[lo:hi], ecid[lo:hi]), f"{where}: col ids differ at {lo + np.flatnonzero(d_cid[lo:hi] != ecid[lo:hi])[:8]}"
            for name, arr, pat in (("PML", d_pml, PAT16), ("col ids", d_cid, PAT8)):
                out = np.concatenate((arr[:lo], arr[hi:]))
                assert (out == pat).all(), f"{where}: {name} written outside the launch's bases [{lo}, {hi})"
        tbl.close()
    del os.environ[KNOB]
    print(f"ok case {case}: device entry point, reads [{before}, {before + n_reads}) of {len(off) - 1}, bases [{lo}, {hi}) of "
          f"{nb_all}, {KNOB}={setting}, orders {orders}, big chunks {[p.n_big for p in plans]}, {time.time() - t0:.1f} s", flush=True)


def main():
    t0 = time.time()
    os.environ.pop(KNOB, None)
    # 1. every geometry on every layout, ragged reads with the placements, u16, host entry point
    for case, (n_reads, setting, shares, n_big) in enumerate(GEOMETRIES):
        run_host(case, n_reads, setting, shares, n_big)
    # 2. u32 output: the kernels store per base and a lane enters its next chunk without waiting for
    #    a flush.  Tail permille 800 is the only one here above the floor of 512 reads (560).  The
    #    long read inside a big chunk has 3 000 bases: one beyond the u16 range (66 000 bases) took
    #    the emulator 190 s more for the four launches, a quarter of the test's whole allowance.
    run_host(20, 1400, "3,800", (700, 700), (46, 46), wide=True)
    run_host(21, 1400, "8,0", (700, 700), (23, 23), wide=True, giant=3_000, source_len=4_000)
    # 3. the device entry points: with and without a lane order from base 0; into the middle of a
    #    larger batch
    run_device(28, 1400, "8,0", (700, 700), (23, 23), 0, 0, orders=(False, True))
    run_device(31, 1400, "3,100", (700, 700), (62, 62), 37, 21, orders=(False,))
    # what the cases above were written to contain
    for kind in KINDS:
        assert seen[kind] >= 8, seen
    assert seen["claimed"] >= 4, seen
    print(f"placements {seen}, {time.time() - t0:.0f} s")
    print("CHUNK-EMU-OK")


if __name__ == "__main__":
    main()
