"""GPU tier of the seeds reduction (csrc/seeds_reduce.h) at the batch sizes where its split of the
bases among waves changes: the chunk a wave owns grows from 2048 bases to 16384 with the batch
(helpers.seeds_chunk), and every batch the rest of the suite launches is small enough for 2048.  No
knob is set here: each case asserts, through the helper, the chunk the product picks for it.

A fault in the split writes wrong results for the few reads next to a wave boundary k * chunk and
nowhere else, so every case is checked twice (`_compare`):
  (a) every read of the batch against identities computed with torch cumulative sums and segment
      maxima over the input arrays, in slabs: n_seeds, max_len, cov and resets from the definitions
      (a run start is a non-zero base that is first in its read or follows a zero), zero summaries
      of empty reads, and exactly min(n_seeds, max_seeds) used slots, the others 0xFFFFFFFF / 0 / 0;
  (b) all eight summary words and all slots against the plain-Python restatement
      (tests/seeds_restatement.py) on a subset sliced and rebased on the host (`_subset`): the reads
      at the wave boundaries, the first and last reads, long reads, empty reads and a random sample.
"""

import numpy as np
import pytest

import helpers
import seeds_restatement as sr

pytestmark = pytest.mark.gpu

M32 = 0xFFFFFFFF
SLAB = 1 << 26                      # bases per step of the generators and of check (a)
EMPTY_RUNS = (1, 63, 64, 65, 200)   # planted runs of empty reads; above 64: a second round of the mark loop


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _lengths(rng, n):
    """Mostly 150, 5 % of 0..5, 1 % of 10 000 (mean about 241)."""
    u = rng.random(n)
    lens = np.full(n, 150, np.int64)
    tiny = u < 0.05
    lens[tiny] = rng.integers(0, 6, int(tiny.sum()))
    lens[(u >= 0.05) & (u < 0.06)] = 10_000
    return lens


def _synthetic(target_bases, wide, seed, n_planted=300):
    """A batch of about target_bases bases made on the device: read_off with n_planted read starts and
    n_planted runs of empty reads planted exactly on multiples of the batch's chunk; pml with about 5 %
    zeros (u16: 1..40; u32: up to 2^32 - 1), col ids about 5 % non-zero."""
    torch, dev = _torch()
    rng = np.random.default_rng(seed)
    cuts = np.concatenate(([0], np.cumsum(_lengths(rng, int(target_bases / 241.1))))).astype(np.uint64)
    nb = int(cuts[-1])
    c = helpers.seeds_chunk(nb)
    ks = rng.choice(np.arange(1, (nb - 1) // c + 1, dtype=np.uint64), size=2 * n_planted, replace=False)
    starts, runs = ks[:n_planted], ks[n_planted:]
    extra = [starts * np.uint64(c)]
    for t, k in enumerate(runs):
        extra.append(np.full(EMPTY_RUNS[t % len(EMPTY_RUNS)] + 1, int(k) * c, np.uint64))
    off = np.sort(np.concatenate([cuts] + extra))
    assert int(off[0]) == 0 and int(off[-1]) == nb
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    pml = torch.zeros(nb + 64, dtype=torch.int32 if wide else torch.int16, device=dev)
    cid = torch.zeros(nb + 64, dtype=torch.uint8, device=dev)
    for lo in range(0, nb, SLAB):
        n = min(SLAB, nb - lo)
        if wide:
            v = torch.randint(-(1 << 31), 1 << 31, (n,), generator=gen, device=dev, dtype=torch.int64)
            v = torch.where(v == 0, torch.ones_like(v), v).to(torch.int32)
        else:
            v = torch.randint(1, 41, (n,), generator=gen, device=dev, dtype=torch.int16)
        v[torch.rand(n, generator=gen, device=dev) < 0.05] = 0
        pml[lo:lo + n] = v
        ids = torch.randint(1, 256, (n,), generator=gen, device=dev, dtype=torch.int16).to(torch.uint8)
        ids[torch.rand(n, generator=gen, device=dev) >= 0.05] = 0
        cid[lo:lo + n] = ids
        del v, ids
    return {"pml": pml, "cid": cid, "off": torch.from_numpy(off.astype(np.int64)).to(dev), "off_h": off, "n_bases": nb,
            "n_reads": len(off) - 1, "wide": wide, "chunk": c, "planted": np.sort(ks), "true_query": False}


def _reduce(pkg, batch, min_len, max_seeds, slots=True):
    """One colbwt_seeds_reduce_device launch -> (summary, pos, len, cid) device tensors (the last three
    None without slots), pre-filled with patterns the pass must overwrite."""
    torch, dev = _torch()
    n = batch["n_reads"]
    d_sum = torch.full((n, 8), 0x2B2B2B2B, dtype=torch.int32, device=dev)
    d_pos = d_len = d_sc = None
    if slots:
        d_pos = torch.full((n, max_seeds), 7, dtype=torch.int32, device=dev)
        d_len = torch.full((n, max_seeds), 7, dtype=torch.int32, device=dev)
        d_sc = torch.full((n, max_seeds), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
    st = pkg.seeds_reduce_device(batch["pml"].data_ptr(), batch["cid"].data_ptr(), batch["off"].data_ptr(), n, batch["n_bases"],
                                 min_len, max_seeds, d_sum.data_ptr(), ptr(d_pos), ptr(d_len), ptr(d_sc),
                                 pml_bytes=4 if batch["wide"] else 2, timed=True)
    torch.cuda.synchronize()
    assert st.n_reads == n and st.n_bases == batch["n_bases"]
    return d_sum, d_pos, d_len, d_sc


def _subset(batch, seed=1):
    """The reads of check (b), by class -> sorted read numbers (numpy)."""
    rng = np.random.default_rng(seed)
    off, nb, c, n = batch["off_h"], batch["n_bases"], batch["chunk"], batch["n_reads"]
    lens = np.diff(off.astype(np.int64))
    n_k = (nb - 1) // c                                     # boundaries k c, k = 1 .. n_k, inside the batch
    if n_k <= 4096:
        ks = np.arange(1, n_k + 1)
    else:
        ks = np.unique(np.concatenate((np.arange(1, 65), np.arange(n_k - 63, n_k + 1), rng.integers(1, n_k + 1, 2000))))

    def around(positions):
        """Every read that starts at, ends at or contains one of the positions, and two on either side."""
        got = []
        for p in positions:
            first = int(np.searchsorted(off, np.uint64(p), "left"))          # first read starting at or after p
            last = int(np.searchsorted(off, np.uint64(p), "right")) - 1      # last read starting at or before p
            got.append(np.arange(max(first - 3, 0), min(last + 3, n)))
        return np.unique(np.concatenate(got)) if got else np.zeros(0, np.int64)

    cls = {"boundaries": around(int(k) * c for k in ks), "n_boundaries": len(ks),
           "planted": around(int(k) * c for k in batch.get("planted", ())),
           "ends": np.unique(np.concatenate((np.arange(min(64, n)), np.arange(max(n - 64, 0), n)))),
           "long": np.flatnonzero(lens > 4096)[:200],
           "empty": np.sort(rng.permutation(np.flatnonzero(lens == 0))[:500]),
           "random": np.unique(rng.integers(0, n, 20_000))}
    if nb > 1 << 32:
        cls["2^32"] = around([1 << 32])
    return cls


def _bad(label, name, got, want, r_lo, batch):
    torch, _ = _torch()
    bad = torch.nonzero(got != want)
    if bad.numel() == 0:
        return
    r = r_lo + int(bad[0, 0])
    o, e, c = int(batch["off_h"][r]), int(batch["off_h"][r + 1]), batch["chunk"]
    raise AssertionError(f"{label}: {name} of read {r} [{o}, {e}) is {int(got[tuple(bad[0])]) & M32}, not {int(want[tuple(bad[0])]) & M32}; "
                         f"{bad.shape[0]} differ in the slab; chunk {c}, start = {o // c} c + {o % c}, end = {e // c} c + {e % c}, "
                         f"start tile {o // 512}")


def _check_all(label, batch, got, min_len, max_seeds):
    """Check (a): every read, in slabs of whole reads."""
    torch, dev = _torch()
    off_h, off_d, n = batch["off_h"], batch["off"], batch["n_reads"]
    mask = M32 if batch["wide"] else 0xFFFF
    d_sum, d_pos, d_len, d_sc = got
    r_lo = 0
    while r_lo < n:
        r_hi = int(np.searchsorted(off_h, off_h[r_lo] + np.uint64(SLAB), "right")) - 1
        r_hi = min(max(r_hi, r_lo + 1), n)
        o, e = int(off_h[r_lo]), int(off_h[r_hi])
        L, nr = e - o, r_hi - r_lo
        v = batch["pml"][o:e].to(torch.int64) & mask
        z = v == 0
        rel = off_d[r_lo:r_hi + 1] - o
        lens = rel[1:] - rel[:-1]

        def seg(x):
            cs = torch.cat((torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(x.to(torch.int64), 0)))
            return cs[rel[1:]] - cs[rel[:-1]]

        start = torch.zeros(L + 1, dtype=torch.bool, device=dev)
        start[rel[:-1]] = True
        prev_zero = torch.cat((torch.ones(1, dtype=torch.bool, device=dev), z[:-1])) if L else z
        counts = ~z & (start[:L] | prev_zero) & (v >= min_len)           # the run starts whose seed counts
        read_of = torch.cumsum(torch.bincount(rel[1:-1], minlength=L + 1), 0)[:L]
        longest = torch.zeros(nr, dtype=torch.int64, device=dev).scatter_reduce_(0, read_of, v, "amax")
        S = d_sum[r_lo:r_hi].to(torch.int64) & M32
        _bad(label, "n_seeds", S[:, 0], seg(counts), r_lo, batch)
        _bad(label, "max_len", S[:, 1], longest, r_lo, batch)
        _bad(label, "cov", S[:, 2], seg(torch.where(counts, v, torch.zeros_like(v))) & M32, r_lo, batch)
        _bad(label, "resets", S[:, 3], seg(z), r_lo, batch)
        if batch["true_query"] and min_len == 1:
            _bad(label, "cov + resets", S[:, 2] + S[:, 3], lens, r_lo, batch)
        _bad(label, "summary of an empty read", S * (lens == 0)[:, None], torch.zeros_like(S), r_lo, batch)
        assert bool((S[:, 4] <= S[:, 0]).all()) and (batch["wide"] or bool((S[:, 5] <= S[:, 2]).all())), f"{label}: n_col, col_cov"   # u32 sums wrap
        assert bool((S[:, 6] + S[:, 7] <= torch.clamp(S[:, 4] - 1, min=0)).all()), f"{label}: asc + desc <= n_col - 1"
        if d_pos is not None:
            used = torch.arange(max_seeds, device=dev)[None, :] < torch.clamp(S[:, 0], max=max_seeds)[:, None]
            P, Ln, C = d_pos[r_lo:r_hi].to(torch.int64) & M32, d_len[r_lo:r_hi].to(torch.int64) & M32, d_sc[r_lo:r_hi]
            _bad(label, "used slots", (P != M32).to(torch.int64), used.to(torch.int64), r_lo, batch)
            _bad(label, "seed_len of an unused slot", Ln * ~used, torch.zeros_like(Ln), r_lo, batch)
            _bad(label, "seed_cid of an unused slot", C * ~used, torch.zeros_like(C), r_lo, batch)
            _bad(label, "seed_pos inside the read", (P < lens[:, None]) | ~used, torch.ones_like(used), r_lo, batch)
            _bad(label, "seed_len >= min_len", (Ln >= min_len) | ~used, torch.ones_like(used), r_lo, batch)
        r_lo = r_hi


def _gather(batch, ids):
    """The reads `ids` sliced out and rebased -> host (pml, cid, read_off)."""
    torch, dev = _torch()
    d_ids = torch.from_numpy(np.asarray(ids, np.int64)).to(dev)
    st = batch["off"][d_ids]
    ln = batch["off"][d_ids + 1] - st
    noff = torch.cat((torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(ln, 0)))
    at = torch.repeat_interleave(st - noff[:-1], ln) + torch.arange(int(noff[-1]), device=dev)
    pml = batch["pml"][at].cpu().numpy().view(np.uint32 if batch["wide"] else np.uint16)
    return pml, batch["cid"][at].cpu().numpy(), noff.cpu().numpy().astype(np.uint64)


def _check_subset(label, batch, got, min_len, max_seeds, ids, sliced):
    """Check (b): all eight words and all slots of the reads `ids` == the restatement."""
    torch, dev = _torch()
    pml, cid, off = sliced
    want = sr.seeds(pml, cid, off, min_len, max_seeds)
    d_ids = torch.from_numpy(np.asarray(ids, np.int64)).to(dev)
    names = ("summary", "seed_pos", "seed_len", "seed_cid")
    for name, g, w in zip(names, got, want):
        if g is None:
            continue
        g = g[d_ids].cpu().numpy()
        g = g.view(np.uint32) if g.dtype == np.int32 else g
        bad = np.argwhere(g != w)
        if bad.size:
            r = int(ids[bad[0][0]])
            o, e, c = int(batch["off_h"][r]), int(batch["off_h"][r + 1]), batch["chunk"]
            raise AssertionError(f"{label}: {name} of read {r} [{o}, {e}) differs at {bad[:5].tolist()}: {g[tuple(bad[0])]} != "
                                 f"{w[tuple(bad[0])]}; {len(np.unique(bad[:, 0]))} reads differ; chunk {c}, start = {o // c} c + {o % c}, "
                                 f"end = {e // c} c + {e % c}")
    return want


def _compare(batch, got, min_len, max_seeds, label="", ids=None, sliced=None):
    """(a) on every read, (b) on the subset.  `got`: (summary, pos, len, cid) device tensors, the last
    three None for a launch without slots."""
    _check_all(label, batch, got, min_len, max_seeds)
    if ids is None:
        ids = np.unique(np.concatenate([v for k, v in _subset(batch).items() if k != "n_boundaries"]))
    return _check_subset(label, batch, got, min_len, max_seeds, ids, sliced if sliced is not None else _gather(batch, ids))


def _subset_checked(batch, long_reads=True, empty_reads=True):
    """The subset with its class sizes asserted -> (ids, the sliced arrays)."""
    cls = _subset(batch)
    n_b = cls.pop("n_boundaries")
    n_k = (batch["n_bases"] - 1) // batch["chunk"]
    assert n_b == n_k or (n_k > 4096 and n_b >= 2000), (n_b, n_k)
    assert len(cls["boundaries"]) >= 5 * n_b * 3 // 4, (len(cls["boundaries"]), n_b)     # 5+ reads per boundary, some shared
    assert len(cls["ends"]) == 128 and len(cls["random"]) > min(19_000, batch["n_reads"] // 4)
    assert len(cls["long"]) == (200 if long_reads else 0) and len(cls["empty"]) == (500 if empty_reads else 0)
    if len(batch.get("planted", ())):
        off, c = batch["off_h"], batch["chunk"]
        at = np.searchsorted(off, batch["planted"] * np.uint64(c), "left")
        assert (off[at] == batch["planted"] * np.uint64(c)).all(), "a read starts on every planted boundary"
        n_at = np.searchsorted(off, batch["planted"] * np.uint64(c), "right") - at
        assert (n_at >= 201).sum() >= len(batch["planted"]) // 10 - 1 and (n_at == 1).sum() >= len(batch["planted"]) // 2 - 5
        assert len(cls["planted"]) >= 5 * len(batch["planted"])
    ids = np.unique(np.concatenate(list(cls.values())))
    return cls, ids, _gather(batch, ids)


def _free(*objs):
    torch, _ = _torch()
    for o in objs:
        if isinstance(o, dict):
            o.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("target,wide,chunk", [(1.4e8, False, 2560), (4e8, False, 6144), (1.1e9, False, 16384), (4e8, True, 6144)],
                         ids=["1.4e8-u16-c2560", "4e8-u16-c6144", "1.1e9-u16-c16384", "4e8-u32-c6144"])
def test_reduce_device_where_the_chunk_grows(pkg, target, wide, chunk):
    """seeds_reduce_device on synthetic arrays whose batch size selects chunk 2560, 6144 and 16384."""
    torch, _ = _torch()
    batch = _synthetic(target, wide, seed=int(target // 1e6) + wide)
    assert batch["chunk"] == chunk == helpers.seeds_chunk(batch["n_bases"])
    assert abs(batch["n_bases"] - target) < 0.02 * target
    cls, ids, sliced = _subset_checked(batch)
    big = (1 << 31) if wide else 20
    for min_len, max_seeds in ((1, 4), (big, 8)):
        got = _reduce(pkg, batch, min_len, max_seeds)
        want = _compare(batch, got, min_len, max_seeds, f"{batch['n_bases']} bases l{min_len} k{max_seeds}", ids, sliced)
        assert want[0][:, 0].any() and (want[0][:, 0] > max_seeds).any() and (want[0][:, 6] > 0).any() and (want[0][:, 7] > 0).any()
        del got
    got = _reduce(pkg, batch, big, 8, slots=False)
    _compare(batch, got, big, 8, f"{batch['n_bases']} bases, summaries only", ids, sliced)
    print(f"\n{batch['n_bases']} bases, {batch['n_reads']} reads, chunk {chunk}: subset {len(ids)} reads / {len(sliced[0])} bases "
          f"({ {k: len(v) for k, v in cls.items()} }), peak HBM {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")
    del got
    _free(batch)


def test_reduce_device_above_2_pow_32_bases(pkg):
    """4.4e9 bases in one launch: the 64-bit arithmetic of the tile loop, the marks and the wave split."""
    torch, _ = _torch()
    batch = _synthetic(4.4e9, False, seed=44)
    assert batch["n_bases"] > (1 << 32) + (1 << 26) and batch["chunk"] == 16384 == helpers.seeds_chunk(batch["n_bases"])
    cls, ids, sliced = _subset_checked(batch)
    off = batch["off_h"]
    at = int(np.searchsorted(off, np.uint64(1 << 32)))
    assert {at - 2, at - 1, at, at + 1} <= set(cls["2^32"].tolist()) and off[at - 2] < 1 << 32 < off[at + 1]
    assert set(range(batch["n_reads"] - 64, batch["n_reads"])) <= set(ids.tolist())
    assert (off[cls["boundaries"]] > np.uint64(1 << 32)).sum() > 300      # the last 64 boundaries alone: 5 reads each
    got = _reduce(pkg, batch, 16, 4)
    _compare(batch, got, 16, 4, f"{batch['n_bases']} bases l16 k4", ids, sliced)
    print(f"\n{batch['n_bases']} bases, {batch['n_reads']} reads: subset {len(ids)} reads / {len(sliced[0])} bases, "
          f"peak HBM {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")
    del got
    _free(batch)


def test_seeds_batch_c2_sample_one_and_two_replicas(pkg, c2_image):
    """seeds_batch on the C2 index (AUTO), 1.2 M x 150 bp reads from the device sampler: 1.8e8 bases,
    chunk 3072 on one replica; a devices=[0, 0] handle reduces two rebased shards of 9e7 bases each
    with chunk 2048 and must give the same bits.  AUTO sizes an index to the HBM that is free, so a
    second replica of its choice does not fit beside the first on the same device: the two-replica
    handle is opened in layout 2 (K-step rows, under 24 GB a replica), whose PML and col ids are the
    same bytes (test_full_scale_properties)."""
    torch, dev = _torch()
    n_reads, m, min_len, max_seeds = 1_200_000, 150, 20, 8
    nb = n_reads * m
    assert helpers.seeds_chunk(nb) == 3072 and helpers.seeds_chunk(nb // 2) == 2048
    one = pkg.ColPml.from_bytes(c2_image)
    d_bases = torch.zeros(nb + 128, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(n_reads + 1, dtype=torch.int64, device=dev)
    one.synth_reads_device(n_reads, m, 10, 78, d_bases.data_ptr(), d_off.data_ptr())
    torch.cuda.synchronize()
    bases, off = d_bases[:nb].cpu().numpy(), d_off.cpu().numpy().astype(np.uint64)
    del d_bases
    assert int(off[-1]) == nb and int(off[n_reads // 2]) == nb // 2
    pml, cid, _ = one.query_batch(bases, off)
    a = one.seeds_batch(bases, off, min_len, max_seeds)
    assert a[4].n_reads == n_reads and a[4].n_bases == nb
    batch = {"pml": torch.from_numpy(pml.view(np.int16)).to(dev), "cid": torch.from_numpy(cid).to(dev), "off": d_off, "off_h": off,
             "n_bases": nb, "n_reads": n_reads, "wide": False, "chunk": 3072, "true_query": True}
    cls, ids, sliced = _subset_checked(batch, long_reads=False, empty_reads=False)
    got = (torch.from_numpy(a[0].view(np.uint32).reshape(-1, 8).view(np.int32)).to(dev), torch.from_numpy(a[1].view(np.int32)).to(dev),
           torch.from_numpy(a[2].view(np.int32)).to(dev), torch.from_numpy(a[3]).to(dev))
    want = _compare(batch, got, min_len, max_seeds, "C2 sample, seeds_batch", ids, sliced)
    assert want[0][:, 0].sum() > len(ids) // 4, "the sample holds seeds"
    b1 = one.seeds_batch(bases, off, 1, 4)
    got1 = (torch.from_numpy(b1[0].view(np.uint32).reshape(-1, 8).view(np.int32)).to(dev), torch.from_numpy(b1[1].view(np.int32)).to(dev),
            torch.from_numpy(b1[2].view(np.int32)).to(dev), torch.from_numpy(b1[3]).to(dev))
    _compare(batch, got1, 1, 4, "C2 sample, seeds_batch l1 k4", ids, sliced)       # min_len 1: cov + resets == 150
    one.close()
    torch.cuda.empty_cache()
    two = pkg.ColPml.from_bytes(c2_image, layout=2, devices=[0, 0])
    assert two.info().n_devices == 2 and two.info().layout == 2
    b = two.seeds_batch(bases, off, min_len, max_seeds)
    two.close()
    assert b[4].n_reads == n_reads and b[4].n_bases == nb
    for name, x, y in zip(("summary", "seed_pos", "seed_len", "seed_cid"), a[:4], b[:4]):
        x, y = (x.view(np.uint32).reshape(-1, 8), y.view(np.uint32).reshape(-1, 8)) if name == "summary" else (x, y)
        bad = np.argwhere(x != y)
        assert bad.size == 0, f"two replicas: {name} differs at {bad[:5].tolist()} (shard cut at read {n_reads // 2})"
    print(f"\nC2 sample: subset {len(ids)} reads, peak HBM {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")
    _free(batch)
