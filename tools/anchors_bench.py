#!/usr/bin/env python3
"""Anchors (colbwt_anchors_device) against locate (colbwt_locate_device, max_occ = 1) on the same reads, on the
FASTA-built index of tools/locate_bench.py: --docs copies of one random genome of --length bases with
--divergence substitutions, `col-bwt build -r --locate`, AUTO layout; --reads reads of --read-len bases drawn
from the documents, at each of the --errors substitution rates.  In one process the two kernels are launched
alternately, event-timed: a warm-up launch of each, then --reps pairs.  Prints one JSON line per rate: median,
min and max ms of both, the anchors / locate ratio, locate's own launch-to-launch spread, the factor statistics,
and the wall time of colbwt_anchors_batch against colbwt_locate_batch (host arrays in, host arrays out).
The anchors call is `-l 16 -k 16 -n 1` (--min-len, --max-anchors, --max-occ)."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from __graft_entry__ import load_package  # noqa: E402
from bench_pipeline import write_fasta  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)


def spread(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=32)
    ap.add_argument("--length", type=int, default=8_000_000)
    ap.add_argument("--divergence", type=float, default=0.002)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--errors", default="0,0.01,0.05")
    ap.add_argument("--min-len", type=int, default=16)
    ap.add_argument("--max-anchors", type=int, default=16)
    ap.add_argument("--max-occ", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch-reps", type=int, default=3)
    ap.add_argument("--tmp", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("anchors_bench.py needs a HIP device (no CPU fallback)")
    pkg = load_package()
    rng = np.random.default_rng(1)
    tmp = tempfile.mkdtemp(dir=a.tmp)
    try:
        base = rng.choice(ACGT, size=a.length)
        seqs, paths = [], []
        for d in range(a.docs):
            s = base.copy()
            mut = rng.random(a.length) < a.divergence
            s[mut] = rng.choice(ACGT, size=int(mut.sum()))
            seqs.append(s)
            paths.append(os.path.join(tmp, f"hap{d}.fa"))
            write_fasta(paths[-1], b"hap%d" % d, s)
        prefix = os.path.join(tmp, "idx")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "col-bwt_amd", "col-bwt"), "build", "-r", "--locate", "-o", prefix]
                           + paths, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"col-bwt build failed: {r.stdout[-2000:]}{r.stderr[-2000:]}")
        tbl = pkg.ColPml.load(prefix)
        tbl.attach_locate(prefix)
        info = tbl.info()
        common = {"docs": a.docs, "length": a.length, "divergence": a.divergence, "n": int(info.n), "layout": int(info.layout),
                  "table_rows": int(info.table_rows), "min_len": a.min_len, "max_anchors": a.max_anchors, "max_occ": a.max_occ,
                  "reps": a.reps}
        n, m, K, W = a.reads, a.read_len, a.max_anchors, a.max_occ
        stacked = np.stack(seqs)
        dev = torch.device("cuda", 0)
        d_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * m
        d_mlen = torch.zeros(n, dtype=torch.int32, device=dev)
        d_locc = torch.zeros(n, dtype=torch.int64, device=dev)
        d_lpos = torch.zeros(n, dtype=torch.int64, device=dev)
        d_sum = torch.zeros(n * 8, dtype=torch.int32, device=dev)
        d_start = torch.zeros(n * K, dtype=torch.int32, device=dev)
        d_len = torch.zeros(n * K, dtype=torch.int32, device=dev)
        d_occ = torch.zeros(n * K, dtype=torch.int64, device=dev)
        d_pos = torch.zeros(n * K * max(W, 1), dtype=torch.int64, device=dev)
        off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(m))
        for err in [float(x) for x in a.errors.split(",")]:
            which = rng.integers(0, a.docs, size=n)
            starts = rng.integers(0, a.length - m, size=n)
            reads = stacked[which[:, None], starts[:, None] + np.arange(m)[None, :]]
            mut = rng.random(reads.shape) < err
            orig = reads[mut]
            reads[mut] = ACGT[(np.searchsorted(ACGT, orig) + rng.integers(1, 4, size=orig.size)) % 4]   # always another base
            d_bases = torch.zeros(n * m + 128, dtype=torch.uint8, device=dev)
            d_bases[:n * m] = torch.from_numpy(reads.reshape(-1)).to(dev)

            def anchors():
                return tbl.anchors_device(d_bases.data_ptr(), d_off.data_ptr(), n, n * m, a.min_len, K, W, d_sum.data_ptr(),
                                          d_start.data_ptr(), d_len.data_ptr(), d_occ.data_ptr(), d_pos.data_ptr() if W else None,
                                          timed=True).kernel_ms

            def locate():
                return tbl.locate_device(d_bases.data_ptr(), d_off.data_ptr(), n, n * m, 1, d_mlen.data_ptr(), d_locc.data_ptr(),
                                         d_lpos.data_ptr(), timed=True).kernel_ms

            anchors()
            locate()
            a_ms, l_ms = [], []
            for _ in range(a.reps):
                a_ms.append(anchors())
                l_ms.append(locate())
            summary = d_sum.cpu().numpy().view(np.uint32).reshape(n, 8)
            mlen = d_mlen.cpu().numpy()
            # the host entry points: wall time of a call, results included
            flat = reads.reshape(-1)
            walls = {"anchors_batch": [], "locate_batch": []}
            for _ in range(a.batch_reps + 1):
                t0 = time.perf_counter()
                tbl.anchors_batch(flat, off, a.min_len, K, W)
                walls["anchors_batch"].append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                tbl.locate_batch(flat, off, 1)
                walls["locate_batch"].append((time.perf_counter() - t0) * 1e3)
            am, lm = statistics.median(a_ms), statistics.median(l_ms)
            out = dict(common, error=err, reads=n, read_len=m, anchors_ms=spread(a_ms), locate_ms=spread(l_ms),
                       anchors_over_locate=round(am / lm, 3), locate_spread=round((max(l_ms) - min(l_ms)) / lm, 4),
                       trips_per_base=round(float((summary[:, 0].sum() + n * m)) / (n * m), 4),
                       locate_steps_per_base=round(float(mlen.sum() + n) / (n * m), 4),
                       mean_factors=round(float(summary[:, 0].mean()), 2), mean_kept=round(float(summary[:, 3].mean()), 2),
                       mean_cov=round(float(summary[:, 4].mean()), 1), mean_skipped=round(float(summary[:, 2].mean()), 3),
                       mean_unique=round(float(summary[:, 5].mean()), 2), mean_locate_mlen=round(float(mlen.mean()), 1),
                       anchors_batch_wall_ms=spread(walls["anchors_batch"][1:]), locate_batch_wall_ms=spread(walls["locate_batch"][1:]))
            print(json.dumps(out), flush=True)
            del d_bases
            torch.cuda.empty_cache()
        tbl.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
