"""GPU tier of locate-all (include/colbwt.h colbwt_locate_all_*): search, plan and the tiled walk on the
MI355X against the restatement (tests/locate_all_restatement.py) on real BWT indexes in every layout,
through every entry point, and the whole chain `col-bwt build --locate` -> `col-bwt locate --all`."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import locate_all_restatement as la
import locate_restatement as lr
import test_gpu_locate as tgl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = (1, 2, 3, 4, 5, 6, 0)

pytestmark = pytest.mark.gpu


def _check(label, got, want):
    for name, g, w in zip(("mlen", "occ", "pos_off", "pos"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (label, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, f"{label}: {name} differs at {list(bad[:5])}: {g[bad[:3]]} != {w[bad[:3]]}"


def test_locate_all_equals_restatement_every_layout(pkg):
    img, text = tgl._true_index(2)
    sa = lr.suffix_array(text)
    loc = lr.samples(text, sa)
    ref = la.LocateAll(text, sa=sa)
    reads = tgl._reads(text, 5) + [b"A", b"AC"]
    bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
    assert pkg.LOCATE_ALL_TILE >= 1
    for layout in LAYOUTS:
        tbl = pkg.ColPml.from_bytes(img, layout=layout)
        tbl.attach_locate(data=loc)
        lm, lo, lp, _ = tbl.locate_batch(bases, off, 5)
        for min_len, cap in ((1, 0), (12, 0), (1, 3)):
            got = tbl.locate_all_batch(bases, off, min_len, cap)
            _check(f"L{layout}/l{min_len}/k{cap}", got[:4], ref.batch(reads, min_len, cap))
            assert got[4].n_reads == len(reads)
            mlen, occ, pos_off, pos = got[:4]
            assert np.array_equal(mlen, lm) and np.array_equal(occ, lo)
            for k in range(len(reads)):                      # the first min(w, 5) positions are locate's
                w = int(pos_off[k + 1] - pos_off[k])
                assert np.array_equal(pos[int(pos_off[k]):int(pos_off[k]) + min(w, 5)], lp[k, :min(w, 5)]), (layout, k)
            assert not (pos == pkg.LOCATE_NONE).any()
        assert tbl.locate_all(text[:-1]) == (len(text) - 1, 1, [0])
        tbl.close()


def _large():
    """The 264 k text of the tile and cut checks: 120 k random characters, ACGT x 6000 and 40 near-copies of
    a 3 kb unit; its index with sub-run splits, its suffix array and the reads."""
    rng = np.random.default_rng(41)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    unit = rng.choice(acgt, size=3000)
    parts = [rng.choice(acgt, size=120000).tobytes(), b"ACGT" * 6000]
    for _ in range(40):
        s = unit.copy()
        mut = rng.random(s.size) < 0.003
        s[mut] = rng.choice(acgt, size=int(mut.sum()))
        parts.append(s.tobytes())
    img, text = helpers.true_bwt_index_large(parts, seed=5, extra_splits=3000)
    sa = lr.suffix_array(text)
    reads = [b"A", b"AC", b"ACG", b"ACGTACGT", b"ACGT" * 10, unit[100:160].tobytes(), unit[2000:2025].tobytes()]
    reads += [bytes(r) for r in helpers.reads_from_text(text, 200, (5, 150), 0.004, seed=43)]
    return img, text, sa, reads


def test_locate_all_tiles_and_cuts_at_the_product_tile(pkg):
    """Ranges of tens of thousands of positions: hundreds of tiles per read, cuts that fall inside long
    folded runs and inside rows, reads with many run ends per tile and with almost none."""
    img, text, sa, reads = _large()
    tile = pkg.LOCATE_ALL_TILE
    ref = la.LocateAll(text, sa=sa)
    t = np.frombuffer(text, np.uint8)
    bwt = np.maximum(t[(sa - 1) % len(t)], 1)                       # folded: bytes <= 1 are one character
    is_end = np.append(bwt[1:] != bwt[:-1], True)
    ends_per_tile = []
    for rd in reads[:7]:
        mlen, sp, ep = ref.range(rd)
        assert mlen == len(rd)
        ends_per_tile.append(float(is_end[sp:ep].sum()) / -(-(ep - sp + 1) // tile))
    assert min(ends_per_tile) < 2 and max(ends_per_tile) > 2, ends_per_tile
    bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
    want = ref.batch(reads, 1, 0)
    for k, rd in enumerate(reads):                                  # the restatement's lists are SA[ep..sp]
        mlen, sp, ep = ref.range(rd)
        if mlen:
            assert np.array_equal(want[3][int(want[2][k]):int(want[2][k + 1])], sa[sp:ep + 1][::-1].astype(np.uint64))
    loc = lr.samples(text, sa)
    for layout in (0, 1):
        tbl = pkg.ColPml.from_bytes(img, layout=layout)
        tbl.attach_locate(data=loc)
        got = tbl.locate_all_batch(bases, off, 1, 0)
        assert int(got[1].max()) >= 64 * tile, int(got[1].max())
        _check(f"large/L{layout}", got[:4], want)
        _check(f"large/L{layout}/k1000", tbl.locate_all_batch(bases, off, 20, 1000)[:4], ref.batch(reads, 20, 1000))
        tbl.close()


def test_locate_all_device_plan_fill_whole_and_in_ranges(pkg):
    import torch
    dev = torch.device("cuda", 0)
    img, text = tgl._true_index(4, size=1500)
    reads = [np.frombuffer(bytes(r), np.uint8) for r in helpers.reads_from_text(text, 300, (0, 300), 0.005, seed=6)]
    reads += [np.frombuffer(b"A", np.uint8), np.frombuffer(b"CG", np.uint8)]
    bases, off = helpers.concat_reads(reads)
    n = len(reads)
    lens = np.diff(off.astype(np.int64))
    d_bases = torch.zeros(len(bases) + 128, dtype=torch.uint8, device=dev)
    d_bases[:len(bases)] = torch.from_numpy(bases)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    order = torch.from_numpy(np.argsort(-lens, kind="stable").astype(np.int32)).to(dev)
    work_bytes = pkg.locate_all_work_bytes(n)
    assert work_bytes % 256 == 0 and work_bytes >= 20 * n
    guard = 0x5A5A5A5A5A5A5A5A
    for layout in (1, 3, 5, 0):
        tbl = pkg.ColPml.from_bytes(img, layout=layout)
        tbl.attach_locate(data=lr.samples(text))
        for min_len, cap in ((1, 0), (12, 7)):
            want = tbl.locate_all_batch(bases, off, min_len, cap)[:4]
            for d_order in (None, order.data_ptr()):
                label = (layout, min_len, cap, d_order is not None)
                d_work = torch.zeros(work_bytes, dtype=torch.uint8, device=dev)
                assert d_work.data_ptr() % 256 == 0
                d_mlen = torch.full((n,), -1, dtype=torch.int32, device=dev)
                d_occ = torch.full((n,), -1, dtype=torch.int64, device=dev)
                d_pos_off = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
                total, st = tbl.locate_all_plan_device(d_bases.data_ptr(), d_off.data_ptr(), n, len(bases), min_len, cap,
                                                       d_mlen.data_ptr(), d_occ.data_ptr(), d_pos_off.data_ptr(), d_work.data_ptr(),
                                                       d_order, timed=True)
                assert st.n_reads == n and st.kernel_ms > 0 and total == int(want[2][-1])
                assert np.array_equal(d_mlen.cpu().numpy().view(np.uint32), want[0]), label
                assert np.array_equal(d_occ.cpu().numpy().view(np.uint64), want[1]), label
                assert np.array_equal(d_pos_off.cpu().numpy().view(np.uint64), want[2]), label
                # whole, with guard words behind pos_cap
                d_pos = torch.full((total + 64,), guard, dtype=torch.int64, device=dev)
                st = tbl.locate_all_fill_device(n, 0, n, d_pos_off.data_ptr(), d_pos.data_ptr(), total, d_work.data_ptr(), timed=True)
                assert st.n_reads == n
                got = d_pos.cpu().numpy().view(np.uint64)
                assert np.array_equal(got[:total], want[3]), label
                assert (got[total:] == np.uint64(guard)).all(), label
                # two read ranges into buffers of their own, both in flight at once
                cuts = (0, n // 3, n)
                parts = []
                for a, b in zip(cuts[:-1], cuts[1:]):
                    cnt = int(want[2][b] - want[2][a])
                    d_part = torch.full((cnt + 64,), guard, dtype=torch.int64, device=dev)
                    tbl.locate_all_fill_device(n, a, b, d_pos_off.data_ptr(), d_part.data_ptr(), cnt, d_work.data_ptr())
                    parts.append((a, b, cnt, d_part))
                torch.cuda.synchronize()
                for a, b, cnt, d_part in parts:
                    got = d_part.cpu().numpy().view(np.uint64)
                    assert np.array_equal(got[:cnt], want[3][int(want[2][a]):int(want[2][b])]), (label, a, b)
                    assert (got[cnt:] == np.uint64(guard)).all(), (label, a, b)
                # pos_cap below the need: the slots below it are filled, nothing at or past it is written
                half = total // 2
                d_half = torch.full((total + 64,), guard, dtype=torch.int64, device=dev)
                tbl.locate_all_fill_device(n, 0, n, d_pos_off.data_ptr(), d_half.data_ptr(), half, d_work.data_ptr())
                torch.cuda.synchronize()
                got = d_half.cpu().numpy().view(np.uint64)
                assert np.array_equal(got[:half], want[3][:half]) and (got[half:] == np.uint64(guard)).all(), label
        tbl.close()


def test_locate_all_two_replicas_match_one(pkg):
    img, text = tgl._true_index(9)
    reads = [np.frombuffer(bytes(r), np.uint8) for r in helpers.reads_from_text(text, 2000, (1, 100), 0.01, seed=2)]
    reads += [np.zeros(0, np.uint8)] * 3
    reads = [np.zeros(0, np.uint8)] + reads
    bases, off = helpers.concat_reads(reads)
    loc = lr.samples(text)
    one = pkg.ColPml.from_bytes(img)
    two = pkg.ColPml.from_bytes(img, devices=[0, 0])
    one.attach_locate(data=loc)
    two.attach_locate(data=loc)
    for min_len, cap in ((1, 0), (10, 5)):
        a = one.locate_all_batch(bases, off, min_len, cap)
        b = two.locate_all_batch(bases, off, min_len, cap)
        _check("replicas", b[:4], a[:4])
        assert b[4].n_reads == len(reads) and int(a[2][-1]) > len(reads)
    one.close()
    two.close()


def test_locate_all_pos_cap_too_small_then_a_second_call(pkg):
    img, text = tgl._true_index(3)
    ref = la.LocateAll(text)
    reads = tgl._reads(text, 7)
    bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
    n = len(reads)
    want = ref.batch(reads, 1, 0)
    total = int(want[2][-1])
    tbl = pkg.ColPml.from_bytes(img)
    tbl.attach_locate(data=lr.samples(text))
    L = pkg.lib()
    mlen, occ, pos_off = np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.full(n + 1, 7, np.uint64)
    pos = np.full(total + 8, 7, np.uint64)
    args = (tbl._h, bases.ctypes.data, off.ctypes.data, n, 1, 0, mlen.ctypes.data, occ.ctypes.data, pos_off.ctypes.data)
    for cap, p in ((0, None), (total - 1, pos.ctypes.data)):
        rc = L.colbwt_locate_all_batch(*args, p, cap, None)
        assert rc == -1 and L.colbwt_last_error().startswith(b"pos_cap too small"), (rc, L.colbwt_last_error())
        assert np.array_equal(pos_off, want[2]) and np.array_equal(mlen, want[0]) and np.array_equal(occ, want[1])
        assert (pos == 7).all()                                  # pos untouched
        pos_off[:] = 7
    st = pkg.Stats()
    assert L.colbwt_locate_all_batch(*args, pos.ctypes.data, total, C.byref(st)) == 0
    assert np.array_equal(pos[:total], want[3]) and (pos[total:] == 7).all() and st.n_reads == n and st.kernel_ms > 0
    with pytest.raises(pkg.ColbwtError) as ei:
        tbl.locate_all_batch(bases, off, 0)
    assert ei.value.code == -1 and "min_len" in str(ei.value)
    bare = pkg.ColPml.from_bytes(img)
    with pytest.raises(pkg.ColbwtError) as ei:
        bare.locate_all_batch(bases, off, 1)
    assert ei.value.code == -1 and "no locate samples attached" in str(ei.value)
    bare.close()
    tbl.close()


def test_col_bwt_build_locate_then_locate_all_equals_restatement(tmp_path):
    """`col-bwt build -r --locate` on three FASTA documents of two records, then `col-bwt locate --all -l 12`:
    every line equals the restatement's over the collection's text as oracle/rlbwt_oracle.py lays it out;
    `--all -k 3` caps the lists; plain `col-bwt locate -k 5` on the same reads stays as before."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import rlbwt_oracle as ro
    rng = np.random.default_rng(12)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    base = rng.choice(acgt, size=1500)
    docs, paths = [], []
    for k in range(3):
        recs = []
        for j in range(2):
            s = base[j * 300:j * 300 + 900].copy()
            mut = rng.random(s.size) < 0.02
            s[mut] = rng.choice(acgt, size=int(mut.sum()))
            recs.append(s)
        docs.append([r.tobytes() for r in recs])
        paths.append(str(tmp_path / f"g{k}.fa"))
        helpers.write_fasta(paths[-1], recs, [f"g{k}_{j}" for j in range(2)])
    launcher = [sys.executable, os.path.join(ROOT, "col-bwt_amd", "col-bwt")]
    outp = str(tmp_path / "coll")
    out = subprocess.run(launcher + ["build", "-r", "--locate", "-l", "20", "-o", outp] + paths, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    text, starts = ro.build_text(docs, revcomp=True)
    ref = la.LocateAll(text, starts)
    reads = [bytes(r) for r in helpers.reads_from_text(text, 200, (5, 150), 0.01, seed=13)]
    reads += [docs[0][0][:300], docs[1][1][-200:][::-1], b"NNNN", b"ACGTTGCAACGTG", b"CA"]
    names = [f"p{k}" for k in range(len(reads))]
    fa = str(tmp_path / "reads.fa")
    helpers.write_fasta(fa, [np.frombuffer(r, np.uint8) for r in reads], names)
    for extra, min_len, cap in ((["-l", "12"], 12, 0), (["-k", "3"], 16, 3), (["-l", "1"], 1, 0)):
        out = subprocess.run(launcher + ["locate", "--all", "-p", fa] + extra + [outp], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        want = ref.batch(reads, min_len, cap)
        assert open(fa + ".locate").read() == ref.file(names, reads, want), extra
    assert int(np.diff(want[2].astype(np.int64)).max()) > 100           # -l 1: the two-base read is everywhere
    out = subprocess.run(launcher + ["locate", "-p", fa, "-k", "5", outp], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = open(fa + ".locate").read().split("\n")
    assert lines[-1] == "" and len(lines) == len(reads) + 1
    for line, rd, nm in zip(lines, reads, names):
        mlen, occ, pos = ref.loc.locate(rd, 5)
        hits = ",".join("%d:%d" % lr.doc_offset(p, starts) for p in pos)
        assert line == f"{nm}\t{len(rd)}\t{mlen}\t{occ}\t{hits}", line
    bad = subprocess.run(launcher + ["locate", "-p", fa, "-l", "12", outp], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0            # -l belongs to --all


def test_locate_all_calls_do_not_leak_hbm(pkg):
    import torch
    img, text = tgl._true_index(11)
    loc = lr.samples(text)
    reads = [np.frombuffer(bytes(r), np.uint8) for r in helpers.reads_from_text(text, 500, (1, 100), 0.01, seed=3)]
    bases, off = helpers.concat_reads(reads)
    tbl = pkg.ColPml.from_bytes(img)
    tbl.attach_locate(data=loc)
    tbl.locate_all_batch(bases, off, 1)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        tbl.attach_locate(data=loc)
        tbl.locate_all_batch(bases, off, 1)
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] >= free0 - (64 << 20)
    tbl.close()
