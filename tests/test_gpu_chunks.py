"""GPU tier: the persistent-lane query kernels (layouts 3, 4, 5, 6) on a large RAGGED batch, every
base compared with the oracle, with the chunk plan of csrc/fat_cursor.h forced through
COLBWT_LINE_ROWS_CHUNK into multi-read chunks of 8, 3 and 2 reads (the last with single reads only:
the control) and left to the product's own choice.

On the chip a workgroup's share is thousands of reads, the claims of a workgroup's lanes race on
its LDS counter, and the rows arrive by LDS-DMA: what the emulated tier (tests/emu/chunk_emu.py)
cannot show.  The library reports neither `big` nor its grid and the test depends on neither: the
forced settings give the coverage whatever the grid is, the unset run is what users get.  Reads
cannot be placed on share boundaries without knowing the grid; the ragged lengths put boundaries
at all alignments.  Count and locate give one lane one read and do not use the chunk plan.

The mismatch-heavy reads are random over ACGT; bytes that occur nowhere in the text (N) and the
terminator are sprinkled over 40 000 bases only, because the oracle resolves each of them with a
scan over the whole table (3 ms each on this index: a third of the reads made of them as in the
emulated tier would keep 16 threads busy for hours).
"""
import os
import time

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

KNOB = "COLBWT_LINE_ROWS_CHUNK"
SETTINGS = (None, "8", "3,0", "2,1000")
N_READS = 3_000_000
GUARD = 4096                         # elements behind the last base that must keep their pattern
PAT16, PAT8 = 0x5AC3, 0xA5


@pytest.fixture(scope="module")
def ragged(oracle):
    """The C1 index (4 x 1 Mbp related sequences, true BWT: test_gpu_parity) and 3 M ragged reads
    with the oracle's answer, both on the device."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    base = rng.choice(acgt, size=1_000_000)
    seqs = [bytes(base)]
    for _ in range(3):
        s = base.copy()
        mut = rng.random(len(s)) < 0.01
        s[mut] = rng.choice(acgt, size=int(mut.sum()))
        seqs.append(bytes(s))
    t0 = time.time()
    image, text = helpers.true_bwt_index_large(seqs, seed=2, extra_splits=20_000)
    t1 = time.time()
    lens = helpers.ragged_lengths(rng, N_READS, n_long=3000)
    runs = rng.choice(N_READS - 10, size=300, replace=False)          # runs of 10 consecutive empty reads
    lens[(runs[:, None] + np.arange(10)[None, :]).reshape(-1)] = 0
    lens[[0, 1, N_READS - 2, N_READS - 1]] = 0                        # empty reads at both ends of the batch
    bases, off = helpers.ragged_reads(text, lens, rng, junk_alphabet=b"ACGT", sprinkle=b"N\x01", n_sprinkle=40_000)
    n = int(off[-1])
    assert 100_000_000 < n < 250_000_000
    t2 = time.time()
    print(f"index {t1 - t0:.1f} s, {N_READS} reads / {n} bases {t2 - t1:.1f} s", flush=True)
    epml, ecid = oracle.OracleIndex(image).query_batch(bases, off, threads=16)
    print(f"oracle {time.time() - t2:.1f} s", flush=True)
    assert 0.02 < float((epml == 0).mean()) < 0.6                     # extends and resets both
    d_bases = torch.zeros(n + 128, dtype=torch.uint8, device=dev)
    d_bases[:n] = torch.from_numpy(bases).to(dev)
    return dict(image=image, n=n, n_reads=N_READS, d_bases=d_bases,
                d_off=torch.from_numpy(off.astype(np.int64)).to(dev),
                e_pml=torch.from_numpy(epml.view(np.int16)).to(dev), e_cid=torch.from_numpy(ecid).to(dev))


def _run_settings(pkg, ragged, layout, settings, wide=False):
    import torch
    dev = torch.device("cuda", 0)
    n = ragged["n"]
    want_pml = ragged["e_pml"].to(torch.int32).bitwise_and_(0xFFFF) if wide else ragged["e_pml"]
    tbl = pkg.ColPml.from_bytes(ragged["image"], layout=layout)
    assert tbl.info().layout == layout
    d_pml = torch.empty(n + GUARD, dtype=torch.int32 if wide else torch.int16, device=dev)
    d_cid = torch.empty(n + GUARD, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    saved = os.environ.get(KNOB)
    try:
        for setting in settings:
            if setting is None:
                os.environ.pop(KNOB, None)
            else:
                os.environ[KNOB] = setting
            d_pml.fill_(PAT16)
            d_cid.fill_(PAT8)
            tbl.query_device(ragged["d_bases"].data_ptr(), ragged["d_off"].data_ptr(), ragged["n_reads"], n,
                             d_pml.data_ptr(), d_cid.data_ptr(), 4 if wide else 2, s)
            torch.cuda.synchronize()
            for name, got, want in (("PML", d_pml, want_pml), ("col ids", d_cid, ragged["e_cid"])):
                if not torch.equal(got[:n], want):
                    bad = torch.nonzero(got[:n] != want).flatten()
                    raise AssertionError(f"layout {layout}, {KNOB}={setting}: {name} differ from the oracle at {bad.numel()} of "
                                         f"{n} bases, first {bad[:8].tolist()}")
            assert bool((d_pml[n:] == PAT16).all()) and bool((d_cid[n:] == PAT8).all()), \
                f"layout {layout}, {KNOB}={setting}: wrote behind the last base"
    finally:
        if saved is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = saved
        tbl.close()


@pytest.mark.parametrize("layout", [3, 4, 5, 6])
def test_ragged_batch_matches_oracle_at_every_chunk_setting(pkg, ragged, layout):
    """u16 output, all three kernels and the deep entries: unset, 8, 3 and 2 reads per chunk with
    tail permille 100 / 0 / 1000, every base and col id equal to the oracle's."""
    _run_settings(pkg, ragged, layout, SETTINGS)


def test_ragged_batch_u32_output(pkg, ragged):
    """The u32 kernels store per base instead of through the wave collector: the default layout at
    three reads per chunk."""
    _run_settings(pkg, ragged, 6, ("3,0",), wide=True)
