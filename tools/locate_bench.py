#!/usr/bin/env python3
"""Locate (colbwt_locate_device) on a FASTA-built index of the bench_pipeline kind: --docs copies of
one random genome of --length bases with --divergence substitutions, `col-bwt build -r --locate`,
AUTO layout; --reads reads of --read-len bases drawn from the documents with --error substitutions.
Prints one JSON line per max_occ: attach time and HBM bytes of the samples, locate ms per launch
(median of --reps after a warm-up launch, min, max), positions reported per second, and count ms on
the same reads and layout (colbwt_count_device, timed the same way)."""
import argparse
import json
import os
import shutil
import statistics
import struct
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


def timed(fn, reps):
    fn()                                              # warm-up
    ms = [fn().kernel_ms for _ in range(reps)]
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=32)
    ap.add_argument("--length", type=int, default=8_000_000)
    ap.add_argument("--divergence", type=float, default=0.002)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--max-occ", default="1,16,64")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tmp", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("locate_bench.py needs a HIP device (no CPU fallback)")
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
        t0 = time.time()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "col-bwt_amd", "col-bwt"), "build", "-r", "--locate", "-o", prefix]
                           + paths, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"col-bwt build failed: {r.stdout[-2000:]}{r.stderr[-2000:]}")
        build_s = time.time() - t0
        tbl = pkg.ColPml.load(prefix)
        info = tbl.info()
        before = int(info.device_bytes)
        t0 = time.time()
        tbl.attach_locate(prefix)
        attach_s = time.time() - t0
        loc_bytes = int(tbl.info().device_bytes) - before
        with open(prefix + ".col_loc", "rb") as f:
            s = struct.unpack_from("<QQQ", f.read(40), 16)[2]       # include/colbwt.h .col_loc header: n, r, s
        common = {"docs": a.docs, "length": a.length, "divergence": a.divergence, "n": int(info.n), "bwt_r": int(info.bwt_r),
                  "phi_samples": int(s), "layout": int(info.layout), "table_rows": int(info.table_rows),
                  "index_GB": round(before / 1e9, 2), "build_s": round(build_s, 1), "attach_s": round(attach_s, 3),
                  "attach_bytes": loc_bytes, "attach_bytes_per_row": round(loc_bytes / info.table_rows, 2)}

        n, m = a.reads, a.read_len
        which = rng.integers(0, a.docs, size=n)
        starts = rng.integers(0, a.length - m, size=n)
        reads = np.stack(seqs)[which[:, None], starts[:, None] + np.arange(m)[None, :]]
        mut = rng.random(reads.shape) < a.error
        reads[mut] = rng.choice(ACGT, size=int(mut.sum()))
        dev = torch.device("cuda", 0)
        d_bases = torch.zeros(n * m + 128, dtype=torch.uint8, device=dev)
        d_bases[:n * m] = torch.from_numpy(reads.reshape(-1)).to(dev)
        d_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * m
        d_mlen = torch.zeros(n, dtype=torch.int32, device=dev)
        d_occ = torch.zeros(n, dtype=torch.int64, device=dev)
        cmed, clo, chi = timed(lambda: tbl.count_device(d_bases.data_ptr(), d_off.data_ptr(), n, n * m, d_mlen.data_ptr(),
                                                        d_occ.data_ptr(), timed=True), a.reps)
        occ = d_occ.cpu().numpy()
        mlen = d_mlen.cpu().numpy()
        common.update(reads=n, read_len=m, error=a.error, mean_mlen=round(float(mlen.mean()), 1),
                      mean_occ=round(float(occ.mean()), 1), count_ms=round(cmed, 3), count_ms_min=round(clo, 3),
                      count_ms_max=round(chi, 3))
        for k in [int(x) for x in a.max_occ.split(",")]:
            d_pos = torch.zeros(n * k, dtype=torch.int64, device=dev)
            med, lo, hi = timed(lambda: tbl.locate_device(d_bases.data_ptr(), d_off.data_ptr(), n, n * m, k, d_mlen.data_ptr(),
                                                          d_occ.data_ptr(), d_pos.data_ptr(), timed=True), a.reps)
            positions = int(np.minimum(d_occ.cpu().numpy(), k).sum())
            out = dict(common, max_occ=k, reps=a.reps, locate_ms=round(med, 3), locate_ms_min=round(lo, 3),
                       locate_ms_max=round(hi, 3), positions=positions, positions_per_s=positions / (med * 1e-3),
                       locate_over_count=round(med / cmed, 2))
            print(json.dumps(out), flush=True)
            del d_pos
            torch.cuda.empty_cache()
        tbl.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
