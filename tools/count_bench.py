#!/usr/bin/env python3
"""Exact-match counting (colbwt_count_device) on the C2 index: 200 M synthetic rows (SURVEY.md
8(d) recipe, seed 42, AUTO layout), reads sampled on the device by backward walk.  Three read sets:
  exact   10 M x 150 bp, no substitutions
  c2      10 M x 150 bp, the C2 substitution rate (1 %)
  long    1 M x 10 kbp, the C2 substitution rate
Each set: one warm-up launch, then --reps launches timed with HIP events.  One JSON line per set:
processed bases (sum of mlen: the bases the search consumed) per second, reads per second, ms per
launch (median, min, max over the reps) and the layout.  For the two 150-bp sets the PML query
(colbwt_query_device) on the same reads is timed the same way, as the yardstick of the estimate in
DESIGN.md section 8."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from __graft_entry__ import load_package  # noqa: E402

SETS = {"exact": (10_000_000, 150, 0), "c2": (10_000_000, 150, 10), "long": (1_000_000, 10_000, 10)}


def timed(fn, reps):
    fn()                                              # warm-up
    ms = [fn().kernel_ms for _ in range(reps)]
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sets", default="exact,c2,long")
    ap.add_argument("--layout", type=int, default=0, help="include/colbwt.h COLBWT_LAYOUT_* (0 = AUTO)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("count_bench.py needs a HIP device (no CPU fallback)")
    dev = torch.device("cuda", 0)
    pkg = load_package()
    t0 = time.time()
    tbl = pkg.ColPml.from_bytes(pkg.synth_index(args.rows, mean_len=8, split_permille=0, seed=42), layout=args.layout)
    t_open = time.time() - t0
    info = tbl.info()
    for name in args.sets.split(","):
        n_reads, m, sub = SETS[name]
        n_bases = n_reads * m
        d_bases = torch.zeros(n_bases + 128, dtype=torch.uint8, device=dev)
        d_off = torch.zeros(n_reads + 1, dtype=torch.int64, device=dev)
        tbl.synth_reads_device(n_reads, m, sub, 43, d_bases.data_ptr(), d_off.data_ptr())
        d_mlen = torch.zeros(n_reads, dtype=torch.int32, device=dev)
        d_occ = torch.zeros(n_reads, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        med, lo, hi = timed(lambda: tbl.count_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, n_bases,
                                                     d_mlen.data_ptr(), d_occ.data_ptr(), timed=True), args.reps)
        mlen = d_mlen.to(torch.int64)
        processed = int(mlen.sum().item())
        out = {"set": name, "reads": n_reads, "read_len": m, "sub_permille": sub, "layout": int(info.layout),
               "layout_shape": int(info.layout_shape), "rows": int(info.r), "reps": args.reps,
               "ms_per_launch": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
               "processed_bases": processed, "processed_bases_per_s": processed / (med * 1e-3),
               "reads_per_s": n_reads / (med * 1e-3), "mean_mlen": processed / n_reads,
               "whole_read_fraction": float((mlen == m).double().mean().item()), "open_s": round(t_open, 1)}
        if name != "long":
            d_pml = torch.zeros(n_bases + 16, dtype=torch.int16, device=dev)
            d_cid = torch.zeros(n_bases + 16, dtype=torch.uint8, device=dev)
            pmed, plo, phi = timed(lambda: tbl.query_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, n_bases,
                                                            d_pml.data_ptr(), d_cid.data_ptr(), 2, 0, timed=True), args.reps)
            out.update({"pml_ms_per_launch": round(pmed, 3), "pml_ms_min": round(plo, 3), "pml_ms_max": round(phi, 3),
                        "pml_bases_per_s": n_bases / (pmed * 1e-3)})
            del d_pml, d_cid
        print(json.dumps(out), flush=True)
        del d_bases, d_off, d_mlen, d_occ
        torch.cuda.empty_cache()
    tbl.close()


if __name__ == "__main__":
    main()
