#!/usr/bin/env python3
"""The chain reduction (colbwt_chain_reduce_device) next to the anchors launch that feeds it
(colbwt_anchors_device), on the FASTA-built index of tools/anchors_bench.py: --docs copies of one random genome
of --length bases with --divergence substitutions, `col-bwt build -r --locate`, AUTO layout; --reads reads of
--read-len bases drawn from the documents, at each of the --errors substitution rates, for each max_occ of
--max-occ (a comma list: the index is built once).  In one process the two kernels are launched alternately,
event-timed: a warm-up launch of each, then --reps pairs.  Prints one JSON line per (max_occ, rate): median, min
and max ms of both, the reduction / anchors ratio, the anchors launch's own spread, the share of reads with a
chain, the mean n_chained, the share with score2 == 0, and the wall time of colbwt_chain_batch against
colbwt_anchors_batch (host arrays in, host arrays out) called alternately on the same reads.  With --anchors-lib
the colbwt_anchors_batch of that comparison comes from another build of the library (the commit before chain
existed), loaded beside this one with a handle of its own on the same index.
The calls are `-l 16 -k 16 -b 16` (--min-len, --max-anchors, --band)."""
import argparse
import ctypes as C
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


class OtherLibrary:
    """colbwt_anchors_batch of another build of libcolbwt.so on a handle of its own."""

    def __init__(self, path, prefix):
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        self.lib = C.CDLL(path)
        self.lib.colbwt_last_error.restype = C.c_char_p
        self.lib.colbwt_index_open.argtypes = [C.c_char_p, vp, C.c_int, C.POINTER(vp)]
        self.lib.colbwt_index_attach_locate.argtypes = [vp, C.c_char_p]
        self.lib.colbwt_anchors_batch.argtypes = [vp, vp, vp, u64, u32, u32, u32, vp, vp, vp, vp, vp, vp]
        self.lib.colbwt_index_close.argtypes = [vp]
        self.h = vp()
        if self.lib.colbwt_index_open(os.fsencode(prefix), None, 0, C.byref(self.h)) != 0 or \
                self.lib.colbwt_index_attach_locate(self.h, os.fsencode(prefix)) != 0:
            raise SystemExit("--anchors-lib: " + self.lib.colbwt_last_error().decode())

    def anchors_batch(self, bases, off, min_len, K, W):
        n = off.size - 1
        summary = np.zeros((n, 8), np.uint32)
        start, ln = np.zeros((n, K), np.uint32), np.zeros((n, K), np.uint32)
        occ, pos = np.zeros((n, K), np.uint64), np.zeros((n, K, W), np.uint64)
        if self.lib.colbwt_anchors_batch(self.h, bases.ctypes.data, off.ctypes.data, n, min_len, K, W, summary.ctypes.data,
                                         start.ctypes.data, ln.ctypes.data, occ.ctypes.data, pos.ctypes.data, None) != 0:
            raise SystemExit("--anchors-lib: " + self.lib.colbwt_last_error().decode())
        return summary, start, ln, occ, pos

    def close(self):
        self.lib.colbwt_index_close(self.h)


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
    ap.add_argument("--max-occ", default="4,1")
    ap.add_argument("--band", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch-reps", type=int, default=3)
    ap.add_argument("--anchors-lib", default=None)
    ap.add_argument("--tmp", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("chain_bench.py needs a HIP device (no CPU fallback)")
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
        other = OtherLibrary(a.anchors_lib, prefix) if a.anchors_lib else None
        info = tbl.info()
        n, m, K = a.reads, a.read_len, a.max_anchors
        stacked = np.stack(seqs)
        dev = torch.device("cuda", 0)
        d_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * m
        off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(m))
        read_sets = []
        for err in [float(x) for x in a.errors.split(",")]:
            which = rng.integers(0, a.docs, size=n)
            starts = rng.integers(0, a.length - m, size=n)
            reads = stacked[which[:, None], starts[:, None] + np.arange(m)[None, :]]
            mut = rng.random(reads.shape) < err
            orig = reads[mut]
            reads[mut] = ACGT[(np.searchsorted(ACGT, orig) + rng.integers(1, 4, size=orig.size)) % 4]   # always another base
            read_sets.append((err, reads))
        for W in [int(x) for x in a.max_occ.split(",")]:
            common = {"docs": a.docs, "length": a.length, "divergence": a.divergence, "n": int(info.n), "layout": int(info.layout),
                      "min_len": a.min_len, "max_anchors": K, "max_occ": W, "band": a.band, "reps": a.reps,
                      "anchors_batch_from": "another build" if other else "this build"}
            d_sum = torch.zeros(n * 8, dtype=torch.int32, device=dev)
            d_start = torch.zeros(n * K, dtype=torch.int32, device=dev)
            d_len = torch.zeros(n * K, dtype=torch.int32, device=dev)
            d_occ = torch.zeros(n * K, dtype=torch.int64, device=dev)
            d_pos = torch.zeros(n * K * W, dtype=torch.int64, device=dev)
            d_chain = torch.zeros(n * 4, dtype=torch.int64, device=dev)
            for err, reads in read_sets:
                d_bases = torch.zeros(n * m + 128, dtype=torch.uint8, device=dev)
                d_bases[:n * m] = torch.from_numpy(reads.reshape(-1)).to(dev)

                def anchors():
                    return tbl.anchors_device(d_bases.data_ptr(), d_off.data_ptr(), n, n * m, a.min_len, K, W, d_sum.data_ptr(),
                                              d_start.data_ptr(), d_len.data_ptr(), d_occ.data_ptr(), d_pos.data_ptr(),
                                              timed=True).kernel_ms

                def reduce():
                    return tbl.chain_reduce_device(d_start.data_ptr(), d_len.data_ptr(), d_pos.data_ptr(), n, K, W, a.band,
                                                   d_chain.data_ptr(), timed=True).kernel_ms

                anchors()
                reduce()
                a_ms, c_ms = [], []
                for _ in range(a.reps):
                    a_ms.append(anchors())
                    c_ms.append(reduce())
                chain = d_chain.cpu().numpy().view(pkg.CHAIN)
                has = chain["text_begin"] != np.uint64(pkg.LOCATE_NONE)
                # the host entry points: wall time of a call, results included
                flat = reads.reshape(-1)
                walls = {"chain_batch": [], "anchors_batch": []}
                for _ in range(a.batch_reps + 1):
                    t0 = time.perf_counter()
                    host, _ = tbl.chain_batch(flat, off, a.min_len, K, W, a.band)
                    walls["chain_batch"].append((time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    if other:
                        other.anchors_batch(flat, off, a.min_len, K, W)
                    else:
                        tbl.anchors_batch(flat, off, a.min_len, K, W)
                    walls["anchors_batch"].append((time.perf_counter() - t0) * 1e3)
                if host.tobytes() != chain.tobytes():
                    raise SystemExit("colbwt_chain_batch and colbwt_chain_reduce_device disagree")
                am, cm = statistics.median(a_ms), statistics.median(c_ms)
                cb, ab = walls["chain_batch"][1:], walls["anchors_batch"][1:]
                out = dict(common, error=err, reads=n, read_len=m, anchors_ms=spread(a_ms), reduce_ms=spread(c_ms),
                           reduce_over_anchors=round(cm / am, 4), anchors_spread=round((max(a_ms) - min(a_ms)) / am, 4),
                           with_chain=round(float(has.mean()), 4), mean_n_chained=round(float(chain["n_chained"][has].mean()), 3),
                           mean_n_hits=round(float(chain["n_hits"].mean()), 2), score2_zero=round(float((chain["score2"][has] == 0).mean()), 4),
                           mean_score=round(float(chain["score"][has].mean()), 1),
                           chain_batch_wall_ms=spread(cb), anchors_batch_wall_ms=spread(ab),
                           anchors_batch_spread=round((max(ab) - min(ab)) / statistics.median(ab), 4))
                print(json.dumps(out), flush=True)
                del d_bases
                torch.cuda.empty_cache()
        if other:
            other.close()
        tbl.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
