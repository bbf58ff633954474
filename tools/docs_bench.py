#!/usr/bin/env python3
"""Docs (colbwt_docs_device) against locate (colbwt_locate_device) on the index and reads of
tools/locate_bench.py: --docs copies of one random genome of --length bases with --divergence
substitutions, `col-bwt build -r --locate`, AUTO layout; --reads reads of --read-len bases drawn from
the documents with --error substitutions.  Prints one JSON line per measurement: docs ms per launch at
every --max-walk with and without the tally (median of --reps after a warm-up launch, min, max),
locate ms at every --max-occ on the same reads, and with --host the host entry points' wall time and
bytes coming back per read (colbwt_docs_batch against colbwt_locate_batch)."""
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


def timed(fn, reps):
    fn()                                              # warm-up
    ms = [fn().kernel_ms for _ in range(reps)]
    return round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)


def wall(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        st = fn()
        out.append(((time.perf_counter() - t0) * 1e3, st))
    ms = [x for x, _ in out]
    st = out[len(out) // 2][1]
    return round(statistics.median(ms), 2), round(min(ms), 2), round(max(ms), 2), st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=32)
    ap.add_argument("--length", type=int, default=8_000_000)
    ap.add_argument("--divergence", type=float, default=0.002)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--min-len", type=int, default=16)
    ap.add_argument("--max-walk", default="16,64,256,1024")
    ap.add_argument("--max-occ", default="16,64")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host", action="store_true", help="also time the host entry points")
    ap.add_argument("--tmp", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("docs_bench.py needs a HIP device (no CPU fallback)")
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
        n_docs = int(tbl.locate_docs().size)
        words = tbl.docs_mask_words()

        n, m = a.reads, a.read_len
        which = rng.integers(0, a.docs, size=n)
        starts = rng.integers(0, a.length - m, size=n)
        reads = np.stack(seqs)[which[:, None], starts[:, None] + np.arange(m)[None, :]]
        mut = rng.random(reads.shape) < a.error
        reads[mut] = rng.choice(ACGT, size=int(mut.sum()))
        del seqs
        dev = torch.device("cuda", 0)
        d_bases = torch.zeros(n * m + 128, dtype=torch.uint8, device=dev)
        d_bases[:n * m] = torch.from_numpy(reads.reshape(-1)).to(dev)
        d_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * m
        d_mlen = torch.zeros(n, dtype=torch.int32, device=dev)
        d_occ = torch.zeros(n, dtype=torch.int64, device=dev)
        d_hit = torch.zeros(n, dtype=torch.int32, device=dev)
        d_mask = torch.zeros(n * words, dtype=torch.int64, device=dev)
        d_tally = torch.zeros(2 * n_docs, dtype=torch.int64, device=dev)
        d_work = torch.zeros(pkg.docs_work_bytes(n), dtype=torch.uint8, device=dev)
        b, o = d_bases.data_ptr(), d_off.data_ptr()
        common = {"docs": n_docs, "mask_words": words, "n": int(info.n), "layout": int(info.layout), "reads": n, "read_len": m,
                  "error": a.error, "min_len": a.min_len, "reps": a.reps, "work_bytes_per_read": pkg.docs_work_bytes(n) / n}
        cnt = timed(lambda: tbl.count_device(b, o, n, n * m, d_mlen.data_ptr(), d_occ.data_ptr(), timed=True), a.reps)
        occ = d_occ.cpu().numpy()
        common.update(mean_occ=round(float(occ.mean()), 1), max_occ_seen=int(occ.max()), count_ms=cnt)
        for k in [int(x) for x in a.max_occ.split(",")]:
            d_pos = torch.zeros(n * k, dtype=torch.int64, device=dev)
            loc = timed(lambda: tbl.locate_device(b, o, n, n * m, k, d_mlen.data_ptr(), d_occ.data_ptr(), d_pos.data_ptr(), timed=True),
                        a.reps)
            print(json.dumps(dict(common, what="locate_device", max_occ=k, ms=loc,
                                  positions=int(np.minimum(d_occ.cpu().numpy(), k).sum()))), flush=True)
            del d_pos
            torch.cuda.empty_cache()
        for w in [int(x) for x in a.max_walk.split(",")]:
            def run(tally):
                return tbl.docs_device(b, o, n, n * m, a.min_len, w, d_mlen.data_ptr(), d_occ.data_ptr(), d_hit.data_ptr(),
                                       d_mask.data_ptr(), d_work.data_ptr(), d_tally.data_ptr() if tally else None,
                                       d_tally.data_ptr() + 8 * n_docs if tally else None, timed=True)
            plain = timed(lambda: run(False), a.reps)
            full = timed(lambda: run(True), a.reps)
            ml, oc = d_mlen.cpu().numpy(), d_occ.cpu().numpy()
            walked = int(np.minimum(oc, w)[ml >= a.min_len].sum())
            hit = d_hit.cpu().numpy()
            print(json.dumps(dict(common, what="docs_device", max_walk=w, ms_no_tally=plain, ms=full,
                                  tally_ms=round(full[0] - plain[0], 3), walked_positions=walked, mean_n_hit=round(float(hit.mean()), 2),
                                  complete=float(((oc <= w) | (hit == n_docs)).mean()))), flush=True)
        if a.host:
            bases, off = reads.reshape(-1), (np.arange(n + 1, dtype=np.uint64) * np.uint64(m))
            for k in [int(x) for x in a.max_occ.split(",")]:
                med, lo, hi, st = wall(lambda: tbl.locate_batch(bases, off, k)[3], a.reps)
                print(json.dumps(dict(common, what="locate_batch", max_occ=k, wall_ms=(med, lo, hi), bytes_back_per_read=12 + 8 * k,
                                      h2d_ms=round(st.h2d_ms, 2), kernel_ms=round(st.kernel_ms, 2), d2h_ms=round(st.d2h_ms, 2))),
                      flush=True)
            for w in [int(x) for x in a.max_walk.split(",")]:
                med, lo, hi, st = wall(lambda: tbl.docs_batch(bases, off, a.min_len, w)[6], a.reps)
                print(json.dumps(dict(common, what="docs_batch", max_walk=w, wall_ms=(med, lo, hi),
                                      bytes_back_per_read=16 + 8 * words, h2d_ms=round(st.h2d_ms, 2),
                                      kernel_ms=round(st.kernel_ms, 2), d2h_ms=round(st.d2h_ms, 2))), flush=True)
        tbl.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
