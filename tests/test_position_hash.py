"""CPU tier: helpers.position_hash, the position-keyed hash the GPU tier and tools/ab_bench.py use
to compare result arrays too large to copy to the host.  A plain sum of all values (what the
comparison used to be) misses a permutation, a +1 / -1 pair and a shifted array; this hash must not,
and its total must not depend on how the array is sliced."""
import numpy as np
import torch

import helpers


def _pml(n, seed, dtype=torch.int16):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 1 << (16 if dtype == torch.int16 else 32), size=n, dtype=np.int64)
    v[rng.random(n) < 0.1] = 0
    v[:4] = (0, 1, 0xFFFF, 0x8000)                       # values with the int16 sign bit set
    return torch.from_numpy(v).to(torch.int32 if dtype == torch.int32 else torch.int64).to(dtype)


def test_hash_equals_its_python_definition():
    # int64 wrap-around and the logical shifts (torch's >> on int64 is arithmetic) against Python ints
    for dtype, mask in ((torch.int16, 0xFFFF), (torch.int32, 0xFFFFFFFF)):
        v = _pml(300, 1, dtype)
        c = torch.from_numpy(np.random.default_rng(2).integers(0, 256, size=300).astype(np.uint8))
        plain = [int(x) & mask for x in v.tolist()]
        assert helpers.position_hash(v) == helpers.position_hash_reference(plain)
        assert helpers.position_hash(v, start=12345) == helpers.position_hash_reference(plain, start=12345)
        assert helpers.position_hash(v, c) == helpers.position_hash_reference(plain, c.tolist())
    big = 3 << 40                                                     # positions past 2^32 (1e10-base batches)
    v = _pml(50, 3)
    assert helpers.position_hash(v, start=big) == helpers.position_hash_reference([x & 0xFFFF for x in v.tolist()], start=big)


def test_hash_sees_a_swap_a_cancelling_pair_and_a_shift():
    v = _pml(100_000, 4)
    c = torch.from_numpy(np.random.default_rng(5).integers(0, 256, size=v.numel()).astype(np.uint8))
    h = helpers.position_hash(v, c)
    i, j = 1000, 70_001
    assert int(v[i]) != int(v[j])

    w = v.clone()
    w[i], w[j] = v[j], v[i]                                          # permutation: the sum stays
    assert int(w.to(torch.int64).sum()) == int(v.to(torch.int64).sum())
    assert helpers.position_hash(w, c) != h

    k = int(torch.nonzero((v > 0) & (v < 0x7FFF))[5])
    w = v.clone()
    w[k] += 1
    w[k + 1 if int(v[k + 1]) > 0 else k + 2] -= 1                   # +1 / -1: the sum stays
    assert int(w.to(torch.int64).sum()) == int(v.to(torch.int64).sum())
    assert helpers.position_hash(w, c) != h

    cc = c.clone()
    cc[i], cc[j] = c[j], c[i]                                        # col ids are part of the hash
    assert c[i] == c[j] or helpers.position_hash(v, cc) != h

    assert helpers.position_hash(v, c, start=1) != h                 # the same values one position on
    w = torch.roll(v, 1)
    assert helpers.position_hash(w, torch.roll(c, 1)) != h


def test_hash_does_not_depend_on_the_slices():
    v = _pml(200_001, 6)
    c = torch.from_numpy(np.random.default_rng(7).integers(0, 256, size=v.numel()).astype(np.uint8))
    h = helpers.position_hash(v, c)
    for step in (1 << 10, 4099, 65_536, 199_999, 1 << 20):
        assert helpers.position_hash(v, c, slice_elems=step) == h, step
    cut = 77_777                                                     # pieces hashed at their own offsets add up
    assert (helpers.position_hash(v[:cut], c[:cut]) + helpers.position_hash(v[cut:], c[cut:], start=cut)) % (1 << 64) == h
    wide = _pml(50_000, 8, torch.int32)
    assert helpers.position_hash(wide, slice_elems=333) == helpers.position_hash(wide)
    as64 = v.to(torch.int64).bitwise_and(0xFFFF)                  # int64 input: same hash, left unchanged
    keep = as64.clone()
    assert helpers.position_hash(as64, c, slice_elems=4099) == h and torch.equal(as64, keep)
