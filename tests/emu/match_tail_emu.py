#!/usr/bin/env python3
"""CPU-tier check of the match tail (csrc/fat_layout.h, fat_build.hip, fat2_query.hip, lane_out.h):
the product's HIP sources compiled against the SIMT emulator with the trip counters in
(match_tail_emu.mk: libcolbwt_emu_trips.so, no sanitizer, nothing preloaded), the cases of
tests/match_tail_cases.py against the oracle with COLBWT_MATCH_TAIL=1 and =0.  Run by
tests/test_emu_match_tail.py in a subprocess.  Prints MATCH-TAIL-EMU-OK at the end.

An emulated open of a 60 000-row table takes a minute and a half (every kernel launch of the
table build starts an OS thread per GPU thread), four opens per case an hour in all.  So a table
is opened ONCE per layout and switch for all of its cases, and the 60 000-row tables are left to
the GPU tier (tests/test_gpu_match_tail.py runs every case on both of them and both layouts) and
to --full, which adds the split-0 one with layout 6 and is how the recorded trip counts
(profiles/*_match_tail_emu_trips.json) are taken: three and a half minutes more.

So that the cases cannot pass without the tail being walked:
  * every K = 8 table used reports a non-zero tail per mille (colbwt_index_info);
  * in the run of the exact reads the match-tail trips are more than half of the row trips whose 8
    bases all match; and on the table with a fifth character -- the only one where mismatches are
    resolved by a run-time threshold scan, which consumes the landing row's own base on the way --
    some match-tail trips consume 15 bases;
  * on the benchmark-like reads (2 000 x 150 bp, 1 % substitutions; 3 000 rows, with --full 60 000
    as well) row trips per read fall by at least a quarter of the full-match trips when the tail is
    switched on, and entry trips do not change.

    python tests/emu/match_tail_emu.py [--full [--record FILE]]   # FILE: the 60 000-row trip counts as JSON
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from __graft_entry__ import load_oracle, load_package  # noqa: E402
import match_tail_cases as mt  # noqa: E402

pkg = load_package()
pkg.LIB_PATH = os.path.join(HERE, "libcolbwt_emu_trips.so")   # emulated build instead of the HIP one
oracle = load_oracle()

NAMES = ("row_trips", "fast_forward", "entry_trips", "scan", "absent", "idle", "row_to_entry", "tail_trips", "full_match_trips",
         "tail_trips_15")


def read_stats(reset=True):
    out = (C.c_ulonglong * 16)()
    assert pkg.lib().colbwt_debug_fat2_stats(out, 1 if reset else 0) == 0
    return {k: int(v) for k, v in zip(NAMES, out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", action="store_true", help="the 60 000-row table (split 0, layout 6) as well")
    ap.add_argument("--record", help="with --full: write its benchmark-like trip counts (tail off / on) to this JSON file")
    a = ap.parse_args()
    assert a.full or not a.record
    t0 = time.time()
    tbls = mt.tables(pkg)
    by_table = {}
    for name, t, reads, layouts, chunk in mt.cases(tbls):
        if t == "synth60000_s50" or (t == "synth60000_s0" and not a.full):
            continue                                                     # GPU tier only (see above)
        if t == "synth60000_s0":
            layouts = (6 | mt.K8,)
        by_table.setdefault((t, layouts), []).append((name, reads, chunk))
    stats = {}                                                           # (case, layout, switch) -> counters of its launch
    permille_of = {}
    for (t, layouts), items in by_table.items():
        t1 = time.time()
        ref = oracle.OracleIndex(tbls[t])
        expect = {}
        for name, reads, _ in items:
            same = [n for n, r, _ in items if r is reads and n in expect]
            expect[name] = expect[same[0]] if same else ref.query_batch(*reads)

        def after(name, layout, switch, info):
            stats[(name, layout, switch)] = read_stats()

        permille = mt.check_table(pkg, tbls[t], layouts, items, expect, after_query=after, before_query=read_stats)
        permille_of.setdefault(t, {}).update(permille)
        for layout, pm in permille.items():
            assert (pm > 0) == (layout in mt.TAIL_LAYOUTS), f"{t}: layout {layout:#x} reports tail per mille {pm}"
        print(f"ok {t}: {[n for n, _, _ in items]}, layouts {[hex(x) for x in layouts]}, tail per mille {permille}, "
              f"{time.time() - t1:.1f} s", flush=True)

    # ---- the tail is walked: exact reads
    walked = [("synth3000_s0", mt.TAIL_LAYOUTS), ("synth3000_s50", mt.TAIL_LAYOUTS)] + ([("synth60000_s0", (6 | mt.K8,))] if a.full else [])
    for t, layouts in walked:
        for layout in layouts:
            on, off = stats[(f"exact/{t}", layout, "1")], stats[(f"exact/{t}", layout, "0")]
            print(f"exact reads {t} layout {layout:#x}: on {on}\n    off {off}", flush=True)
            assert off["tail_trips"] == 0 and off["tail_trips_15"] == 0
            assert 2 * on["tail_trips"] > on["full_match_trips"] > 0, (t, layout, on)
            assert on["entry_trips"] == off["entry_trips"], (t, layout, on, off)
    for layout in mt.TAIL_LAYOUTS:
        on = stats[("exact/five_chars", layout, "1")]
        print(f"exact reads five_chars layout {layout:#x}: on {on}", flush=True)
        assert on["scan"] > 0 and on["tail_trips_15"] > 0, (layout, on)
    # ---- and it saves trips on reads like the benchmark's: 2 000 x 150 bp at 1 %
    n = 2_000
    for t, layouts in walked:
        for layout in layouts:
            on, off = stats[(f"bench_like/{t}", layout, "1")], stats[(f"bench_like/{t}", layout, "0")]
            saved = off["row_trips"] - on["row_trips"]
            record = {"table": t, "rows": int(t[5:].split("_")[0]), "reads": n, "read_len": 150, "sub_permille": 10,
                      "layout": layout & 0xFF, "steps": 8, "tail_permille": permille_of[t][layout], "off": off, "on": on,
                      "per_read_off": {k: round(v / n, 3) for k, v in off.items()},
                      "per_read_on": {k: round(v / n, 3) for k, v in on.items()},
                      "row_trips_saved_per_read": round(saved / n, 3)}
            print(f"benchmark-like {t} layout {layout:#x}: per read off {record['per_read_off']}\n    on {record['per_read_on']}\n"
                  f"    row trips saved per read {saved / n:.3f}", flush=True)
            assert on["entry_trips"] == off["entry_trips"], (on, off)
            assert 4 * saved >= off["full_match_trips"] > 0, (on, off)
            if a.record and t == "synth60000_s0":
                with open(a.record, "w") as f:
                    json.dump(record, f, indent=1)
                    f.write("\n")
    print(f"{time.time() - t0:.0f} s")
    print("MATCH-TAIL-EMU-OK")


if __name__ == "__main__":
    main()
