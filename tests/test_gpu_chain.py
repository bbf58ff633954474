"""GPU tier of chain (include/colbwt.h colbwt_chain_*): chain_kernel on the MI355X against the plain-Python
restatement (tests/chain_restatement.py) in every instantiation of the kernel (chain_cases.SETTINGS), on every layout,
through every entry point, and the chain `col-bwt build` -> `col-bwt chain`."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_cases as cc
import chain_restatement as chr_
import helpers
import locate_restatement as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = (1, 2, 3, 4, 5, 6, 0)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reference():
    """The index, 260 reads and their records at every setting: computed once, shared and left unchanged."""
    img, text, starts, sa = cc.index5()
    reads = cc.mixed_reads(text, 260)
    ref = chr_.Chains(text, starts, sa)
    want = {s: ref.batch(reads, *s) for s in cc.SETTINGS}
    return img, lr.samples(text, sa, starts), starts, reads, want


def _table(pkg, layout=0, **kw):
    img, loc = _reference()[:2]
    tbl = pkg.ColPml.from_bytes(img, layout=layout, **kw)
    tbl.attach_locate(data=loc)
    return tbl


def _device_reads(torch, reads):
    dev = torch.device("cuda", 0)
    bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
    d_bases = torch.zeros(len(bases) + 128, dtype=torch.uint8, device=dev)
    d_bases[:len(bases)] = torch.from_numpy(bases)
    return bases, off, d_bases, torch.from_numpy(off.astype(np.int64)).to(dev)


def _garbage_records(torch, n):
    return torch.full((4 * n,), 0x5A5A5A5A5A5A, dtype=torch.int64, device=torch.device("cuda", 0))


def _records(d_chain):
    return d_chain.cpu().numpy().view(chr_.CHAIN)


def test_chain_equals_restatement_every_layout(pkg):
    _, _, _, reads, want = _reference()
    assert pkg.CHAIN == chr_.CHAIN and pkg.CHAIN.itemsize == 32
    bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
    for layout in LAYOUTS:
        tbl = _table(pkg, layout)
        for s in cc.SETTINGS:
            got, st = tbl.chain_batch(bases, off, *s)
            assert st.n_reads == len(reads)
            assert got.tobytes() == want[s].tobytes(), f"L{layout}/{s}"
        s = cc.SETTINGS[3]
        one = tbl.chain(reads[0], *s)
        assert one == {f: int(want[s][f][0]) for f in chr_.FIELDS}
        assert tbl.chain(b"NNNN", *s) is None
        tbl.close()


def test_chain_groups_that_straddle_a_wave_and_a_block(pkg):
    """Every setting as 1, 63, 64, 65 and 260 reads: a partial group of lanes, a partial wave, a partial block."""
    _, _, _, reads, want = _reference()
    tbl = _table(pkg)
    for n in (1, 63, 64, 65):
        bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads[:n]])
        for s in cc.SETTINGS:
            got, _ = tbl.chain_batch(bases, off, *s)
            assert got.tobytes() == want[s][:n].tobytes(), f"{n} reads/{s}"
    tbl.close()


def test_handcrafted_and_random_slots_through_chain_reduce_device(pkg):
    import torch
    dev = torch.device("cuda", 0)
    starts = _reference()[2]
    tbl = _table(pkg)
    hs, hl, hp, hand = cc.handcrafted(starts)
    sets = [("hand", hs, hl, hp, cc.BAND)]
    sets += [(f"rand{k}",) + cc.random_slots(100 + k, n, K, M, starts) + (band,) for k, (n, K, M, band) in enumerate(cc.RANDOM_SETS)]
    for name, s, ln, p, band in sets:
        n, K = s.shape
        M = p.shape[2]
        # arrays of exactly the slots' size, the records pre-filled with garbage
        d_s = torch.from_numpy(s.view(np.int32).reshape(-1)).to(dev)
        d_l = torch.from_numpy(ln.view(np.int32).reshape(-1)).to(dev)
        d_p = torch.from_numpy(p.view(np.int64).reshape(-1)).to(dev)
        d_chain = _garbage_records(torch, n)
        st = tbl.chain_reduce_device(d_s.data_ptr(), d_l.data_ptr(), d_p.data_ptr(), n, K, M, band, d_chain.data_ptr(), timed=True)
        assert st.n_reads == n
        got = _records(d_chain)
        assert got.tobytes() == chr_.reduce_slots(s, ln, p, band, starts).tobytes(), name
        if name == "hand":
            for k, (label, fields) in enumerate(hand):
                for field, value in fields.items():
                    assert int(got[field][k]) == value, (label, field)
    with pytest.raises(pkg.ColbwtError) as ei:
        tbl.chain_reduce_device(d_s.data_ptr(), d_l.data_ptr(), d_p.data_ptr(), 1, 257, 1, 8, d_chain.data_ptr())
    assert ei.value.code == -1 and "max_anchors * max_occ must be at most 256" in str(ei.value)
    tbl.close()


def test_chain_device_with_and_without_order_on_ragged_batches(pkg):
    """Reads of 0 .. 300 bases, empty reads and reads without an anchor among them: chain_device with and without
    d_order equals chain_batch and the restatement, and equals chain_reduce_device over anchors_device's own output."""
    import torch
    dev = torch.device("cuda", 0)
    img, _, starts, _, _ = _reference()
    _, text, _, sa = cc.index5()
    reads = [bytes(r) for r in helpers.reads_from_text(text, 300, (0, 300), 0.02, seed=6, extra=b"N")]
    reads += [b"", b"NNNNNNNN", b"", b"ACG"]
    ref = chr_.Chains(text, starts, sa)
    bases, off, d_bases, d_off = _device_reads(torch, reads)
    lens = np.diff(off.astype(np.int64))
    n = len(reads)
    assert (lens == 0).sum() >= 2
    order = torch.from_numpy(np.argsort(-lens, kind="stable").astype(np.int32)).to(dev)
    for layout in (1, 3, 5, 0):
        tbl = _table(pkg, layout)
        for min_len, K, M, band in (cc.SETTINGS[3], cc.SETTINGS[4], cc.SETTINGS[6]):
            want = ref.batch(reads, min_len, K, M, band)
            assert (want["text_begin"] == np.uint64(chr_.NONE)).sum() >= 4 and (want["n_chained"] >= 2).sum() >= 50
            host, _ = tbl.chain_batch(bases, off, min_len, K, M, band)
            assert host.tobytes() == want.tobytes(), f"L{layout} batch"
            d_work = torch.full((pkg.chain_work_bytes(n, K, M),), 0x5A, dtype=torch.uint8, device=dev)
            assert d_work.data_ptr() % 256 == 0
            for d_order in (None, order.data_ptr()):
                d_chain = _garbage_records(torch, n)
                st = tbl.chain_device(d_bases.data_ptr(), d_off.data_ptr(), n, len(bases), min_len, K, M, band, d_chain.data_ptr(),
                                      d_work.data_ptr(), d_order, timed=True)
                assert st.n_reads == n
                assert _records(d_chain).tobytes() == want.tobytes(), f"L{layout}/{(min_len, K, M, band)}/order {d_order is not None}"
            # the reduction alone over the arrays of an anchors call
            d_sum = torch.empty(n * 8, dtype=torch.int32, device=dev)
            d_start = torch.empty(n * K, dtype=torch.int32, device=dev)
            d_len = torch.empty(n * K, dtype=torch.int32, device=dev)
            d_occ = torch.empty(n * K, dtype=torch.int64, device=dev)
            d_pos = torch.empty(n * K * M, dtype=torch.int64, device=dev)
            tbl.anchors_device(d_bases.data_ptr(), d_off.data_ptr(), n, len(bases), min_len, K, M, d_sum.data_ptr(), d_start.data_ptr(),
                               d_len.data_ptr(), d_occ.data_ptr(), d_pos.data_ptr())
            d_chain = _garbage_records(torch, n)
            tbl.chain_reduce_device(d_start.data_ptr(), d_len.data_ptr(), d_pos.data_ptr(), n, K, M, band, d_chain.data_ptr(), timed=True)
            assert _records(d_chain).tobytes() == want.tobytes(), f"L{layout} reduce over anchors"
        tbl.close()


def test_chain_two_replicas_match_one(pkg):
    _, _, _, reads, want = _reference()
    many = reads * 8 + [b""] * 3
    bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in many])
    two = _table(pkg, devices=[0, 0])
    for s in (cc.SETTINGS[3], cc.SETTINGS[5]):
        got, st = two.chain_batch(bases, off, *s)
        assert st.n_reads == len(many)
        assert got[:len(reads) * 8].tobytes() == want[s].tobytes() * 8, f"replicas {s}"
        assert (got["text_begin"][-3:] == np.uint64(chr_.NONE)).all()
    two.close()


def test_chain_errors_through_python(pkg):
    img = _reference()[0]
    bases, off = helpers.concat_reads([np.frombuffer(b"ACGTACGTACGTACGTACGT", np.uint8)])
    bare = pkg.ColPml.from_bytes(img)
    with pytest.raises(pkg.ColbwtError) as ei:
        bare.chain_batch(bases, off)
    assert ei.value.code == -1 and "no locate samples attached" in str(ei.value)
    bare.close()
    tbl = _table(pkg)
    for args, msg in (((16, 0, 4, 8), "max_anchors must be at least 1"), ((16, 16, 0, 8), "max_occ must be at least 1"),
                      ((16, 257, 1, 8), "max_anchors * max_occ must be at most 256"), ((16, 65, 4, 8), "at most 256"),
                      ((0, 16, 4, 8), "min_len must be at least 1")):
        with pytest.raises(pkg.ColbwtError) as ei:
            tbl.chain_batch(bases, off, *args)
        assert ei.value.code == -1 and msg in str(ei.value), args
    tbl.close()


def test_col_bwt_build_then_chain_equals_restatement(tmp_path):
    """`col-bwt build -r --locate` on three FASTA documents of two records, then `col-bwt chain`: every line equals the
    restatement's over the collection's text; on the index built without --locate the command exits non-zero with
    locate's message and leaves no output."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import rlbwt_oracle as ro
    rng = np.random.default_rng(12)
    base = rng.choice(cc.ACGT, size=1500)
    docs, paths = [], []
    for k in range(3):
        recs = []
        for j in range(2):
            s = base[j * 300:j * 300 + 900].copy()
            mut = rng.random(s.size) < 0.02
            s[mut] = rng.choice(cc.ACGT, size=int(mut.sum()))
            recs.append(s)
        docs.append([r.tobytes() for r in recs])
        paths.append(str(tmp_path / f"g{k}.fa"))
        helpers.write_fasta(paths[-1], recs, [f"g{k}_{j}" for j in range(2)])
    launcher = [sys.executable, os.path.join(ROOT, "col-bwt_amd", "col-bwt")]
    outp, plain = str(tmp_path / "coll"), str(tmp_path / "plain")
    for cmd in (["build", "-r", "--locate", "-l", "20", "-o", outp], ["build", "-r", "-l", "20", "-o", plain]):
        out = subprocess.run(launcher + cmd + paths, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
    text, starts = ro.build_text(docs, revcomp=True)
    ref = chr_.Chains(text, starts)
    body = np.frombuffer(docs[1][0], np.uint8)
    reads = [cc.mutate(rng, body[at:at + 150], k % 3, k % 6) for k, at in enumerate(rng.integers(0, body.size - 150, 60))]
    reads += [docs[0][0][:300], docs[1][1][-200:][::-1], b"NNNN"]
    names = [f"p{k}" for k in range(len(reads))]
    fa = str(tmp_path / "reads.fa")
    helpers.write_fasta(fa, [np.frombuffer(r, np.uint8) for r in reads], names)
    out = subprocess.run(launcher + ["chain", "-p", fa, "-l", "10", "-k", "8", "-n", "6", "-b", "4", outp], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = ref.file(names, reads, 10, 8, 6, 4)
    assert open(fa + ".chains").read() == lines
    assert lines.rstrip("\n").split("\n")[-1].split("\t")[4:6] == ["*", "*"] and "\t*\t" not in lines.split("\n")[0]
    out = subprocess.run(launcher + ["chain", "-p", fa, outp], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(fa + ".chains").read() == ref.file(names, reads, 16, 16, 4, 16)
    os.remove(fa + ".chains")
    bad = subprocess.run(launcher + ["chain", "-p", fa, plain], capture_output=True, text=True, timeout=300)
    loc = subprocess.run(launcher + ["locate", "-p", fa, plain], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and loc.returncode != 0 and "col_loc" in bad.stderr
    assert bad.stderr.replace("col-bwt chain:", "") == loc.stderr.replace("col-bwt locate:", "")
    assert not os.path.exists(fa + ".chains")
    over = subprocess.run(launcher + ["chain", "-p", fa, "-k", "65", outp], capture_output=True, text=True, timeout=300)
    assert over.returncode != 0 and "256" in over.stderr


def test_chain_calls_do_not_leak_hbm(pkg):
    import torch
    _, _, _, reads, _ = _reference()
    bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
    tbl = _table(pkg)
    tbl.chain_batch(bases, off, *cc.SETTINGS[3])
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        tbl.chain_batch(bases, off, *cc.SETTINGS[3])
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] >= free0 - (64 << 20)
    tbl.close()
