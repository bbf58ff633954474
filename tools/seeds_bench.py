#!/usr/bin/env python3
"""The seeds reduction (colbwt_seeds_reduce_device) on the C2 index: 200 M synthetic rows (SURVEY.md
8(d) recipe, seed 42, AUTO layout), reads sampled on the device by backward walk at the C2
substitution rate.  Two read sets:
  c2      10 M x 150 bp
  long    1 M x 10 kbp
Each set: the query launch (colbwt_query_device) and the reduction pass over its output, each one
warm-up launch and then --reps launches timed with HIP events (median, min, max).  One JSON line per
set: both times, the pass's bytes (3 per base in, 32 + 9 * max_seeds per read out) per second,
and the selectivity (seeds per read, mean cov / m) at min_len 1, 8, 16 and 20.  With --host the c2
set also goes through the host entry points (seeds_batch against query_batch on a tenth of the
reads: h2d / kernel / d2h from colbwt_stats and wall time, PCIe inclusive)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from __graft_entry__ import load_package  # noqa: E402

SETS = {"c2": (10_000_000, 150, 10), "long": (1_000_000, 10_000, 10)}


def timed(fn, reps):
    fn()                                              # warm-up
    ms = [fn().kernel_ms for _ in range(reps)]
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sets", default="c2,long")
    ap.add_argument("--layout", type=int, default=0, help="include/colbwt.h COLBWT_LAYOUT_* (0 = AUTO)")
    ap.add_argument("--min-len", type=int, default=20)
    ap.add_argument("--max-seeds", type=int, default=8)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of each set's reads")
    ap.add_argument("--host", action="store_true", help="also time seeds_batch against query_batch (c2 set)")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("seeds_bench.py needs a HIP device (no CPU fallback)")
    dev = torch.device("cuda", 0)
    pkg = load_package()
    tbl = pkg.ColPml.from_bytes(pkg.synth_index(args.rows, mean_len=8, split_permille=0, seed=42), layout=args.layout)
    info = tbl.info()
    k = args.max_seeds
    for name in args.sets.split(","):
        n_reads, m, sub = SETS[name]
        n_reads = max(1, int(n_reads * args.scale))
        n_bases = n_reads * m
        d_bases = torch.zeros(n_bases + 128, dtype=torch.uint8, device=dev)
        d_off = torch.zeros(n_reads + 1, dtype=torch.int64, device=dev)
        tbl.synth_reads_device(n_reads, m, sub, 43, d_bases.data_ptr(), d_off.data_ptr())
        d_pml = torch.zeros(n_bases + 64, dtype=torch.int16, device=dev)
        d_cid = torch.zeros(n_bases + 64, dtype=torch.uint8, device=dev)
        d_sum = torch.zeros(n_reads * 8, dtype=torch.int32, device=dev)
        d_pos = torch.zeros(n_reads * k, dtype=torch.int32, device=dev)
        d_len = torch.zeros(n_reads * k, dtype=torch.int32, device=dev)
        d_sc = torch.zeros(n_reads * k, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        qmed, qlo, qhi = timed(lambda: tbl.query_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, n_bases, d_pml.data_ptr(),
                                                        d_cid.data_ptr(), 2, 0, timed=True), args.reps)

        def reduce(min_len, slots=True):
            return pkg.seeds_reduce_device(d_pml.data_ptr(), d_cid.data_ptr(), d_off.data_ptr(), n_reads, n_bases, min_len, k,
                                           d_sum.data_ptr(), d_pos.data_ptr() if slots else None, d_len.data_ptr() if slots else None,
                                           d_sc.data_ptr() if slots else None, timed=True)

        smed, slo, shi = timed(lambda: reduce(args.min_len), args.reps)
        omed, olo, ohi = timed(lambda: reduce(args.min_len, slots=False), args.reps)
        moved = 3 * n_bases + 8 * (n_reads + 1) + n_reads * (32 + 9 * k)
        out = {"set": name, "reads": n_reads, "read_len": m, "sub_permille": sub, "layout": int(info.layout),
               "layout_shape": int(info.layout_shape), "rows": int(info.r), "reps": args.reps, "min_len": args.min_len,
               "max_seeds": k, "query_ms": round(qmed, 3), "query_ms_min": round(qlo, 3), "query_ms_max": round(qhi, 3),
               "seeds_ms": round(smed, 3), "seeds_ms_min": round(slo, 3), "seeds_ms_max": round(shi, 3),
               "seeds_summaries_only_ms": round(omed, 3), "seeds_summaries_only_ms_min": round(olo, 3),
               "seeds_summaries_only_ms_max": round(ohi, 3), "seeds_over_query": round(smed / qmed, 3),
               "seeds_bytes": moved, "seeds_bytes_per_s": moved / (smed * 1e-3), "selectivity": {}}
        for min_len in (1, 8, 16, 20):
            reduce(min_len, slots=False)
            s = d_sum.view(n_reads, 8).to(torch.float64)
            out["selectivity"][str(min_len)] = {"seeds_per_read": float(s[:, 0].mean().item()),
                                                "mean_cov_over_m": float((s[:, 2] / m).mean().item()),
                                                "col_seeds_per_read": float(s[:, 4].mean().item())}
        if args.host and name == "c2":
            n_host = max(1, n_reads // 10)
            bases = d_bases[:n_host * m].cpu().numpy()
            off = (np.arange(n_host + 1, dtype=np.uint64) * m)
            host = {}
            for label, fn in (("query_batch", lambda: tbl.query_batch(bases, off)[2]),
                              ("seeds_batch", lambda: tbl.seeds_batch(bases, off, args.min_len, k)[4])):
                fn()                                  # warm-up: the handle's device and staging buffers
                rows = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    st = fn()
                    rows.append(((time.perf_counter() - t0) * 1e3, st.h2d_ms, st.kernel_ms, st.d2h_ms))
                rows.sort()
                wall, h2d, kern, d2h = rows[len(rows) // 2]
                host[label] = {"reads": n_host, "wall_ms": round(wall, 3), "wall_ms_min": round(rows[0][0], 3),
                               "wall_ms_max": round(rows[-1][0], 3), "h2d_ms": round(h2d, 3), "kernel_ms": round(kern, 3),
                               "d2h_ms": round(d2h, 3), "bases_per_s": n_host * m / (wall * 1e-3)}
            out["host"] = host
        print(json.dumps(out), flush=True)
        del d_bases, d_off, d_pml, d_cid, d_sum, d_pos, d_len, d_sc
        torch.cuda.empty_cache()
    tbl.close()


if __name__ == "__main__":
    main()
