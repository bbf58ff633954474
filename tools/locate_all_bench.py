#!/usr/bin/env python3
"""Locate-all (colbwt_locate_all_plan_device / _fill_device / _batch) on the index and reads of
tools/locate_bench.py: --docs copies of one random genome of --length bases with --divergence
substitutions, `col-bwt build -r --locate`, AUTO layout; --reads reads of --read-len bases drawn from the
documents with --error substitutions.  One process; every time is the median of --reps launches after a
warm-up, with min and max.  Prints one JSON line per measurement:
  device   plan and fill ms at --min-len, uncapped, positions per second; beside them colbwt_locate_device
           at max_occ 64 on the same reads, and whether the two return the same positions
  heavy    the batch at min_len 1 with and without one extra read of --heavy-len bases (occ in the
           millions): the time that read adds, against ONE lane walking 2^20 of its positions
           (colbwt_locate_device on that read alone at max_occ 2^20)
  host     colbwt_locate_all_batch (sizing call + call, as ColPml.locate_all_batch does) and
           colbwt_locate_batch at max_occ 64: wall ms"""
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
    return round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=32)
    ap.add_argument("--length", type=int, default=8_000_000)
    ap.add_argument("--divergence", type=float, default=0.002)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--min-len", type=int, default=16)
    ap.add_argument("--heavy-len", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--prefix", default=None, help="keep the index here and reuse it when it is there (the documents are "
                    "regenerated from the seed either way)")
    ap.add_argument("--only", default="device,heavy,host", help="which measurements to run")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("locate_all_bench.py needs a HIP device (no CPU fallback)")
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
        prefix = a.prefix or os.path.join(tmp, "idx")
        t0 = time.time()
        if not (os.path.exists(prefix + ".col_pml") and os.path.exists(prefix + ".col_loc")):
            for d, s in enumerate(seqs):
                write_fasta(paths[d], b"hap%d" % d, s)
            r = subprocess.run([sys.executable, os.path.join(ROOT, "col-bwt_amd", "col-bwt"), "build", "-r", "--locate", "-o", prefix]
                               + paths, capture_output=True, text=True)
            if r.returncode != 0:
                raise SystemExit(f"col-bwt build failed: {r.stdout[-2000:]}{r.stderr[-2000:]}")
        build_s = time.time() - t0
        only = set(a.only.split(","))
        tbl = pkg.ColPml.load(prefix)
        tbl.attach_locate(prefix)
        info = tbl.info()
        tile = pkg.LOCATE_ALL_TILE
        common = {"docs": a.docs, "length": a.length, "n": int(info.n), "bwt_r": int(info.bwt_r), "layout": int(info.layout),
                  "table_rows": int(info.table_rows), "build_s": round(build_s, 1), "tile": tile, "reps": a.reps}

        n, m = a.reads, a.read_len
        which = rng.integers(0, a.docs, size=n)
        starts = rng.integers(0, a.length - m, size=n)
        reads = np.stack(seqs)[which[:, None], starts[:, None] + np.arange(m)[None, :]]
        mut = rng.random(reads.shape) < a.error
        reads[mut] = rng.choice(ACGT, size=int(mut.sum()))
        heavy = seqs[0][1000:1000 + a.heavy_len].copy()
        dev = torch.device("cuda", 0)

        def upload(flat, off):
            d_b = torch.zeros(len(flat) + 128, dtype=torch.uint8, device=dev)
            d_b[:len(flat)] = torch.from_numpy(flat).to(dev)
            return d_b, torch.from_numpy(off.astype(np.int64)).to(dev)

        flat = reads.reshape(-1)
        off = np.arange(n + 1, dtype=np.uint64) * m
        flat_h = np.concatenate([flat, heavy])
        off_h = np.append(off, off[-1] + a.heavy_len).astype(np.uint64)

        def plan_fill(d_b, d_o, cnt, nb, min_len):
            """-> (plan ms, fill ms, total, occ, pos_off, pos tensor) over --reps timed repetitions"""
            d_mlen = torch.zeros(cnt, dtype=torch.int32, device=dev)
            d_occ = torch.zeros(cnt, dtype=torch.int64, device=dev)
            d_po = torch.zeros(cnt + 1, dtype=torch.int64, device=dev)
            d_work = torch.zeros(pkg.locate_all_work_bytes(cnt), dtype=torch.uint8, device=dev)
            plan = lambda: tbl.locate_all_plan_device(d_b.data_ptr(), d_o.data_ptr(), cnt, nb, min_len, 0, d_mlen.data_ptr(),  # noqa: E731
                                                      d_occ.data_ptr(), d_po.data_ptr(), d_work.data_ptr(), timed=True)
            total, _ = plan()
            d_pos = torch.zeros(max(total, 1), dtype=torch.int64, device=dev)
            fill = lambda: tbl.locate_all_fill_device(cnt, 0, cnt, d_po.data_ptr(), d_pos.data_ptr(), total, d_work.data_ptr(),  # noqa: E731
                                                      timed=True)
            fill()
            p_ms = [plan()[1].kernel_ms for _ in range(a.reps)]
            f_ms = [fill().kernel_ms for _ in range(a.reps)]
            return p_ms, f_ms, total, d_occ.cpu().numpy(), d_po.cpu().numpy(), d_pos

        d_b, d_o = upload(flat, off)

        def device_part():
            # plan + fill against locate at max_occ 64
            p_ms, f_ms, total, occ, po, d_pos = plan_fill(d_b, d_o, n, n * m, a.min_len)
            d_mlen = torch.zeros(n, dtype=torch.int32, device=dev)
            d_occ = torch.zeros(n, dtype=torch.int64, device=dev)
            d_p64 = torch.zeros(n * 64, dtype=torch.int64, device=dev)
            loc = lambda: tbl.locate_device(d_b.data_ptr(), d_o.data_ptr(), n, n * m, 64, d_mlen.data_ptr(), d_occ.data_ptr(),  # noqa: E731
                                            d_p64.data_ptr(), timed=True)
            loc()
            l_ms = [loc().kernel_ms for _ in range(a.reps)]
            p64 = d_p64.cpu().numpy().reshape(n, 64)
            pos = d_pos.cpu().numpy()
            w = np.diff(po)
            same = all(np.array_equal(pos[po[k]:po[k] + min(w[k], 64)], p64[k, :min(w[k], 64)]) for k in range(0, n, max(n // 5000, 1)))
            pm, fm = statistics.median(p_ms), statistics.median(f_ms)
            print(json.dumps(dict(common, what="device", reads=n, read_len=m, min_len=a.min_len, positions=int(total),
                                  max_occ_in_batch=int(occ.max()), tiles=int((-(-w // tile)).sum()), plan_ms=spread(p_ms),
                                  fill_ms=spread(f_ms), plan_plus_fill_ms=round(pm + fm, 3), positions_per_s=total / ((pm + fm) * 1e-3),
                                  locate64_ms=spread(l_ms), locate64_positions=int(np.minimum(occ, 64).sum()),
                                  first_64_equal_locate=bool(same))), flush=True)
            del d_p64, d_pos
            torch.cuda.empty_cache()

        def heavy_part():
            # the batch at min_len 1, without and with one read of occ in the millions
            p0, f0, total0, _, _, d_pos = plan_fill(d_b, d_o, n, n * m, 1)
            del d_pos
            torch.cuda.empty_cache()
            d_bh, d_oh = upload(flat_h, off_h)
            p1, f1, total1, occ1, _, d_pos = plan_fill(d_bh, d_oh, n + 1, n * m + a.heavy_len, 1)
            del d_pos
            torch.cuda.empty_cache()
            d_b1, d_o1 = upload(heavy, np.array([0, a.heavy_len], np.uint64))
            k1 = 1 << 20
            d_m1 = torch.zeros(1, dtype=torch.int32, device=dev)
            d_c1 = torch.zeros(1, dtype=torch.int64, device=dev)
            d_p1 = torch.zeros(k1, dtype=torch.int64, device=dev)
            lane = lambda: tbl.locate_device(d_b1.data_ptr(), d_o1.data_ptr(), 1, a.heavy_len, k1, d_m1.data_ptr(), d_c1.data_ptr(),  # noqa: E731
                                             d_p1.data_ptr(), timed=True)
            lane()
            lane_ms = [lane().kernel_ms for _ in range(3)]
            heavy_occ = int(occ1[-1])
            walked = min(heavy_occ, k1)
            added = (statistics.median(p1) + statistics.median(f1)) - (statistics.median(p0) + statistics.median(f0))
            one_lane_all = statistics.median(lane_ms) / walked * heavy_occ
            print(json.dumps(dict(common, what="heavy", min_len=1, heavy_read=heavy.tobytes().decode(), heavy_occ=heavy_occ,
                                  batch_positions=int(total0), batch_plan_ms=spread(p0), batch_fill_ms=spread(f0),
                                  with_heavy_positions=int(total1), with_heavy_plan_ms=spread(p1), with_heavy_fill_ms=spread(f1),
                                  added_ms=round(added, 3), one_lane_ms_for_2p20=spread(lane_ms), one_lane_positions=walked,
                                  one_lane_ns_per_step=round(statistics.median(lane_ms) * 1e6 / walked, 1),
                                  one_lane_ms_for_all=round(one_lane_all, 1), added_over_one_lane=added / one_lane_all)), flush=True)
            del d_p1, d_bh, d_oh
            torch.cuda.empty_cache()

        def host_part():
            # host entry points: wall time
            def wall(fn):
                fn()
                ms = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    fn()
                    ms.append((time.perf_counter() - t0) * 1e3)
                return ms
            h_all = wall(lambda: tbl.locate_all_batch(flat, off, a.min_len, 0))
            h_64 = wall(lambda: tbl.locate_batch(flat, off, 64))
            st = tbl.locate_all_batch(flat, off, a.min_len, 0)[4]
            print(json.dumps(dict(common, what="host", min_len=a.min_len, locate_all_batch_wall_ms=spread(h_all),
                                  locate_all_batch_last_call=dict(h2d_ms=round(st.h2d_ms, 3), kernel_ms=round(st.kernel_ms, 3),
                                                                  d2h_ms=round(st.d2h_ms, 3)),
                                  locate_batch64_wall_ms=spread(h_64))), flush=True)

        for part, fn in (("device", device_part), ("heavy", heavy_part), ("host", host_part)):
            if part in only:
                fn()
        tbl.close()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
