"""The cases of the match-tail tests (fat_layout.h: a K = 8 row of a mismatch-line layout carries the
steps 9 .. 16 of its leading positions; fat2_query.hip walks 16 matching bases in one trip), shared
by the emulated tier (tests/emu/match_tail_emu.py) and the GPU tier (tests/test_gpu_match_tail.py).

Every case is a table, a batch of reads, the layouts to open the table with and, optionally, a
setting of COLBWT_LINE_ROWS_CHUNK.  `check_case` opens each layout twice, with COLBWT_MATCH_TAIL=1
and =0 (read at open), and wants both bit-equal to the oracle, hence to each other.
"""
import os

import numpy as np

import helpers

SWITCH = "COLBWT_MATCH_TAIL"
CHUNK_KNOB = "COLBWT_LINE_ROWS_CHUNK"
K8 = 8 << 8
TAIL_LAYOUTS = (5 | K8, 6 | K8)                       # mismatch lines / deep entries at K = 8: the rows with a tail


def tables(pkg):
    """name -> image.  The four synth tables of the issue, one with a fifth character in its text
    (some tails cannot be coded: TSPAN = 0) and one with thresholds between the runs."""
    out = {}
    for rows in (3_000, 60_000):
        for split in (0, 50):
            out[f"synth{rows}_s{split}"] = bytes(pkgsynth(pkg, rows, split, 0))
    rng = np.random.default_rng(77)
    out["five_chars"] = bytes(helpers.random_table(rng, 3_000, alphabet=b"ACGTN", max_len=15, split_prob=0.05))
    out["thr_mode1"] = bytes(pkgsynth(pkg, 3_000, 50, 1))
    return out


def pkgsynth(pkg, rows, split, thr_mode):
    return pkg.synth_index(rows, mean_len=8, split_permille=split, seed=11 + rows % 97 + split, thr_mode=thr_mode)


def exact_reads(image, seed, per_length=10, n_150=800):
    """Backward-walk reads without substitutions, lengths 1 .. 40 (all the edges: 15, 16, 17, 23, 24,
    25, 31, 32, 33) and 150: after its first bases such a read matches to its end, so every row trip
    with 16 bases left wants the tail.  Most reads have 150 bases: a row trip of a read shorter than
    24 can never take the tail, and with 25 reads per short length only 48 % of the full-match trips
    did.  1 200 reads: in the emulator's two workgroups that is more than the 512 reads of a share's
    single-read tail, so COLBWT_LINE_ROWS_CHUNK puts them into multi-read chunks."""
    reads = []
    for m in range(1, 41):
        reads += helpers.backward_walk_reads(image, per_length, m, 0.0, seed=seed + m)
    reads += helpers.backward_walk_reads(image, n_150, 150, 0.0, seed=seed + 150)
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(reads))                # ragged: the lengths mixed
    return helpers.concat_reads([reads[k] for k in order])


def bench_like_reads(image, seed, n=2_000):
    return helpers.concat_reads(helpers.backward_walk_reads(image, n, 150, 0.01, seed=seed))


def guard_reads(image, seed):
    """64 exact reads of 2 000 bases: every trip wants the tail, and the lanes meet the collector's
    guard at every count and phase."""
    return helpers.concat_reads(helpers.backward_walk_reads(image, 64, 2_000, 0.0, seed=seed))


def cases(tbls):
    """(name, table name, (bases, off), layouts, chunk setting).  Reads are made per table."""
    out = []
    for t in ("synth3000_s0", "synth3000_s50", "synth60000_s0", "synth60000_s50"):
        img = tbls[t]
        exact = exact_reads(img, 5)
        out.append((f"exact/{t}", t, exact, TAIL_LAYOUTS, None))
        out.append((f"bench_like/{t}", t, bench_like_reads(img, 6), TAIL_LAYOUTS, None))
        out.append((f"guard/{t}", t, guard_reads(img, 7), TAIL_LAYOUTS, None))
        if t in ("synth3000_s50", "synth60000_s0"):
            out.append((f"chunk8/{t}", t, exact, TAIL_LAYOUTS, "8"))
            out.append((f"chunk2_singles/{t}", t, exact, TAIL_LAYOUTS, "2,1000"))
    for t in ("five_chars", "thr_mode1"):
        out.append((f"exact/{t}", t, exact_reads(tbls[t], 8), TAIL_LAYOUTS, None))
        out.append((f"bench_like/{t}", t, bench_like_reads(tbls[t], 9, n=600), TAIL_LAYOUTS, None))
    # shapes that must not change: K = 6 rows have no tail, layout 4 has in-row slots
    out.append(("unchanged/synth3000_s50", "synth3000_s50", exact_reads(tbls["synth3000_s50"], 5), (6 | (6 << 8), 4 | K8), None))
    return out


def check_table(pkg, image, layouts, items, expect, after_query=None, before_query=None):
    """The same checks with ONE open per (layout, switch) for all cases of a table -- where an open is
    slow (the emulator).  items: [(name, reads, chunk)]; expect: name -> the oracle's (pml, cid);
    before_query() / after_query(name, layout, switch, info) bracket every launch (trip counters).
    Returns {layout: tail per mille}."""
    permille = {}
    saved = {k: os.environ.get(k) for k in (SWITCH, CHUNK_KNOB)}
    try:
        for layout in layouts:
            for switch in ("1", "0"):
                os.environ[SWITCH] = switch
                os.environ.pop(CHUNK_KNOB, None)
                tbl = pkg.ColPml.from_bytes(image, layout=layout)
                info = tbl.info()
                assert info.layout == layout & 0xFF and info.layout_shape >> 8 == layout >> 8, (layout,)
                permille[layout] = int(info.tail_permille)
                for name, reads, chunk in items:
                    if chunk is None:
                        os.environ.pop(CHUNK_KNOB, None)
                    else:
                        os.environ[CHUNK_KNOB] = chunk                # read at every launch
                    if before_query:
                        before_query()
                    pml, cid, _ = tbl.query_batch(*reads)
                    if after_query:
                        after_query(name, layout, switch, info)
                    epml, ecid = expect[name]
                    tag = f"{name} layout {layout:#x} {SWITCH}={switch}"
                    assert np.array_equal(pml, epml), f"{tag}: PML differs at {np.flatnonzero(pml != epml)[:8]}"
                    assert np.array_equal(cid, ecid), f"{tag}: col ids differ at {np.flatnonzero(cid != ecid)[:8]}"
                tbl.close()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return permille


def check_case(pkg, image, reads, layouts, chunk, expect, where):
    """Opens `image` with each layout, the tail on and off; both must equal `expect` = the oracle's
    (pml, cid).  Returns {layout: tail per mille}."""
    return check_table(pkg, image, layouts, [(where, reads, chunk)], {where: expect})
