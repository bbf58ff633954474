"""GPU tier (-m gpu): long and wide reads on a real BWT, where exact substrings really match.

The C1-shaped index (4 x 1 Mbp: one random sequence and three copies with 1 % SNPs, true BWT with
min-LCP thresholds and sub-run splits) is built once for the module.  On it a read cut from the
text keeps matching for thousands of bases, so PML values run into the thousands (u16 reads) and
past 65535 (u32 reads) -- unlike the synthetic move tables with 5 % substitutions, where matching
stretches stay short.  That is what the mismatch-line kernels' output path (lane_out.h: restart
masks plus the value above each 8-element piece, values rebuilt by the storing lane) must carry
across many flushes, and what the u32 instantiation stores element by element.

Checked against the oracle (PML / col ids) and against plain substring search over the text
(exact-match counts), on every HBM layout shape.
"""
import struct

import numpy as np
import pytest

import count_restatement
import helpers
from test_gpu_parity import LAYOUTS

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def c1(oracle):
    """(image, text, oracle index) of test_gpu_parity.py::test_c1_four_related_megabase_sequences."""
    rng = np.random.default_rng(1)
    base = rng.choice(ACGT, size=1_000_000)
    seqs = [bytes(base)]
    for _ in range(3):
        s = base.copy()
        mut = rng.random(len(s)) < 0.01
        s[mut] = rng.choice(ACGT, size=int(mut.sum()))
        seqs.append(bytes(s))
    image, text = helpers.true_bwt_index_large(seqs, seed=2, extra_splits=20_000)
    return image, text, oracle.OracleIndex(image)


def _reads(text, n, lens, sub, seed, extra=b""):
    return helpers.reads_from_text(text, n, lens, sub, seed=seed, extra=extra)


def _first_diff(got, want, off):
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return None
    k = int(np.searchsorted(off, bad[0], side="right") - 1)
    return (f"{bad.size} values differ; first at base {bad[0]} (read {k}, offset {bad[0] - int(off[k])} of "
            f"{int(off[k + 1] - off[k])}): got {got[bad[:6]].tolist()}, want {want[bad[:6]].tolist()}")


def _device_runs(torch, tbl, bases, off, pml_bytes):
    """query_device on the batch with a length-sorted d_order and without one; guard bytes past the
    batch must stay untouched.  -> [(pml, cid)] as numpy arrays."""
    dev = torch.device("cuda", 0)
    nb, n_reads = int(off[-1]), len(off) - 1
    d_bases = torch.zeros(nb + 128, dtype=torch.uint8, device=dev)
    d_bases[:nb] = torch.from_numpy(bases).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    lens = torch.from_numpy(np.diff(off.astype(np.int64)))
    d_order = torch.argsort(lens, descending=True, stable=True).to(torch.int32).to(dev)
    pdt = torch.int16 if pml_bytes == 2 else torch.int32
    out = []
    for order in (d_order, None):
        p = torch.full((nb + 64,), -1, dtype=pdt, device=dev)
        c = torch.full((nb + 64,), 0xEE, dtype=torch.uint8, device=dev)
        tbl.query_device(d_bases.data_ptr(), d_off.data_ptr(), n_reads, nb, p.data_ptr(), c.data_ptr(), pml_bytes, 0,
                         d_order=order.data_ptr() if order is not None else None)
        torch.cuda.synchronize()
        assert (p[nb:] == -1).all() and (c[nb:] == 0xEE).all(), "written past the batch"
        hp = p[:nb].cpu().numpy().view(np.uint16 if pml_bytes == 2 else np.uint32)
        out.append((hp, c[:nb].cpu().numpy()))
    return out


def test_long_reads_u16_every_layout(pkg, c1):
    """8-12 kbp reads (C4's length) on the real BWT, every layout shape, host and device entry
    points: PML stretches of thousands of bases pass through many flushes of lane_out.h."""
    import torch
    image, text, ref = c1
    reads = (_reads(text, 100, (8_000, 12_000), 0.0, 11) + _reads(text, 100, (8_000, 12_000), 0.001, 12)
             + _reads(text, 90, (8_000, 12_000), 0.01, 13) + _reads(text, 10, (8_000, 12_000), 0.001, 14, extra=b"Nacgt"))
    order = np.random.default_rng(15).permutation(len(reads))
    reads = [reads[k] for k in order]
    bases, off = helpers.concat_reads(reads)
    ep, ec = ref.query_batch(bases, off, threads=8)
    assert ep.max() >= 8000, ep.max()                        # long stretches really exercised
    assert (ep > 255).mean() > 0.5                           # most values need more than 8 bits
    for layout in LAYOUTS:
        tbl = pkg.ColPml.from_bytes(image, layout=layout)
        assert tbl.info().layout == layout & 0xFF
        pml, cid, _ = tbl.query_batch(bases, off)
        assert (msg := _first_diff(pml, ep, off)) is None, f"layout {layout:#x} host PML: {msg}"
        assert (msg := _first_diff(cid, ec, off)) is None, f"layout {layout:#x} host col ids: {msg}"
        for kind, (dp, dc) in zip(("ordered", "unordered"), _device_runs(torch, tbl, bases, off, 2)):
            assert (msg := _first_diff(dp, ep, off)) is None, f"layout {layout:#x} device {kind} PML: {msg}"
            assert (msg := _first_diff(dc, ec, off)) is None, f"layout {layout:#x} device {kind} col ids: {msg}"
        tbl.close()


def test_wide_reads_u32_every_layout(pkg, c1):
    """Exact and near-exact substrings of 66-150 kbp (PML values past 65535: the u32 kernels)
    mixed with a few hundred short reads, every layout shape; the short reads' values equal a u16
    run of the short reads alone; a u16 request on the batch is refused."""
    import torch
    image, text, ref = c1
    long_reads = _reads(text, 7, (66_000, 150_000), 0.0, 21) + _reads(text, 3, (66_000, 150_000), 0.00002, 22)
    short = _reads(text, 300, (1, 300), 0.01, 23, extra=b"Nn")
    reads, is_long = [], []
    for k in range(10):                                      # long reads spread through the batch
        reads += short[30 * k:30 * k + 30] + [long_reads[k]]
        is_long += [False] * 30 + [True]
    bases, off = helpers.concat_reads(reads)
    ep, ec = ref.query_batch(bases, off, wide=True, threads=8)
    assert ep.max() > 65535, ep.max()
    sb, so = helpers.concat_reads(short)
    short_at = np.concatenate([np.arange(int(off[k]), int(off[k + 1])) for k in range(len(reads)) if not is_long[k]])
    for layout in LAYOUTS:
        tbl = pkg.ColPml.from_bytes(image, layout=layout)
        pml, cid, _ = tbl.query_batch(bases, off, wide=True)
        assert pml.dtype == np.uint32
        assert (msg := _first_diff(pml, ep, off)) is None, f"layout {layout:#x} wide PML: {msg}"
        assert (msg := _first_diff(cid, ec, off)) is None, f"layout {layout:#x} wide col ids: {msg}"
        for kind, (dp, dc) in zip(("ordered", "unordered"), _device_runs(torch, tbl, bases, off, 4)):
            assert (msg := _first_diff(dp, ep, off)) is None, f"layout {layout:#x} device {kind} u32 PML: {msg}"
            assert (msg := _first_diff(dc, ec, off)) is None, f"layout {layout:#x} device {kind} u32 col ids: {msg}"
        sp, sc, _ = tbl.query_batch(sb, so)
        assert sp.dtype == np.uint16
        assert np.array_equal(sp, pml[short_at]) and np.array_equal(sc, cid[short_at]), f"layout {layout:#x}: u16 vs u32"
        with pytest.raises(pkg.ColbwtError):
            tbl.query_batch(bases, off, wide=False)
        tbl.close()


def _parse_bin(path, value_bytes):
    """The .pml.bin / .cid.bin container (bin_writer.h): per read u16 name length, name, u64 count,
    `count` values in computation order (the read's last base first)."""
    raw = open(path, "rb").read()
    out, at = [], 0
    while at < len(raw):
        (nl,) = struct.unpack_from("<H", raw, at)
        name = raw[at + 2:at + 2 + nl].decode()
        (m,) = struct.unpack_from("<Q", raw, at + 2 + nl)
        at += 10 + nl
        vals = np.frombuffer(raw, np.uint16 if value_bytes == 2 else np.uint8, m, at)
        out.append((name, vals[::-1]))
        at += m * value_bytes
    return out


def test_file_pipeline_batches_with_and_without_wide_reads(pkg, c1, tmp_path):
    """A FASTA whose query_file batches (small batch_bases) hold a read over 65535 bases in some and
    only short reads in others: the u32 / u16 choice is made per batch.  Text outputs byte-equal to
    the oracle's pml_query; the binary .pml.bin saturates at 65535 as bin_writer.h documents."""
    image, text, ref = c1
    short = _reads(text, 400, (500, 3_000), 0.001, 31, extra=b"Nacgt")
    wide = _reads(text, 4, (66_000, 120_000), 0.0, 32)
    reads = []
    for k in range(4):                                       # ~100 short reads (a few batches) between wide ones
        reads += short[100 * k:100 * k + 100] + [wide[k]]
    reads += _reads(text, 20, (8_000, 12_000), 0.0, 33)     # a tail of long u16 reads
    fa = str(tmp_path / "mixed.fa")
    helpers.write_fasta(fa, reads)
    tbl = pkg.ColPml.from_bytes(image)
    st = tbl.query_file(fa, batch_bases=60_000)
    assert st.n_reads == len(reads)
    ref.pml_query_files(fa, fa + ".opml", fa + ".ocid")
    for ext, oext in ((".pml", ".opml"), (".cid", ".ocid")):
        got, want = open(fa + ext, "rb").read(), open(fa + oext, "rb").read()
        assert got == want, f"{ext} differs from the oracle at byte {next(i for i, (a, b) in enumerate(zip(got, want)) if a != b) if len(got) == len(want) else 'length'}"
    tbl.query_file_binary(fa, batch_bases=60_000)
    bases, off = helpers.concat_reads(reads)
    ep, ec = ref.query_batch(bases, off, wide=True, threads=8)
    assert ep.max() > 65535
    pml_recs, cid_recs = _parse_bin(fa + ".pml.bin", 2), _parse_bin(fa + ".cid.bin", 1)
    assert [nm for nm, _ in pml_recs] == [f"r{k}" for k in range(len(reads))] == [nm for nm, _ in cid_recs]
    saturated = 0
    for k in range(len(reads)):
        lo, hi = int(off[k]), int(off[k + 1])
        want = np.minimum(ep[lo:hi], 65535)
        assert np.array_equal(pml_recs[k][1], want), f"read {k}: .pml.bin differs"
        assert np.array_equal(cid_recs[k][1], ec[lo:hi]), f"read {k}: .cid.bin differs"
        saturated += int((ep[lo:hi] > 65535).sum())
    assert saturated > 0
    tbl.close()


def _longest_suffix(text, read):
    """(mlen, occ): the longest suffix of `read` occurring in `text` (occurrence is monotone in the
    suffix length: binary search) and its overlapping occurrences."""
    m = len(read)
    lo, hi = 0, m
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if text.find(read[m - mid:]) >= 0:
            lo = mid
        else:
            hi = mid - 1
    if lo == 0:
        return 0, 0
    pat = read[m - lo:]
    occ, at = 0, text.find(pat)
    while at >= 0:
        occ += 1
        at = text.find(pat, at + 1)
    return lo, occ


def test_count_long_reads_every_layout(pkg, c1):
    """Exact-match counts of long reads: exact substrings give mlen == m and occ = their overlapping
    occurrences in the text; reads with substitutions give the longest occurring suffix; sp of a
    sample against the restatement (count_restatement.Table)."""
    import torch
    image, text, _ = c1
    exact = _reads(text, 60, (8_000, 12_000), 0.0, 41) + _reads(text, 2, (66_000, 100_000), 0.0, 42)
    subs = _reads(text, 60, (8_000, 12_000), 0.001, 43) + _reads(text, 40, (8_000, 12_000), 0.01, 44)
    reads = [bytes(r) for r in exact + subs]
    want = [_longest_suffix(text, r) for r in reads]
    for k in range(len(exact)):
        assert want[k][0] == len(reads[k])
    assert max(w[0] for w in want[len(exact):]) > 1000      # some substituted reads keep long exact suffixes
    wl = np.array([w[0] for w in want], np.uint32)
    wo = np.array([w[1] for w in want], np.uint64)
    sample = list(range(0, len(reads), len(reads) // 20))
    table = count_restatement.Table(image)
    wsp = {k: table.count(reads[k]) for k in sample}
    for k in sample:
        assert wsp[k][:2] == want[k], (k, wsp[k], want[k])
    bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
    for layout in (1, 2, 3, 4, 5, 6, 0):
        tbl = pkg.ColPml.from_bytes(image, layout=layout)
        mlen, occ, sp, _ = tbl.count_batch(bases, off, want_sp=True)
        for name, g, w in (("mlen", mlen, wl), ("occ", occ, wo)):
            bad = np.flatnonzero(g != w)
            assert bad.size == 0, f"layout {layout}: {name} differs at reads {bad[:5]}: {g[bad[:5]]} != {w[bad[:5]]}"
        assert [int(sp[k]) for k in sample] == [wsp[k][2] for k in sample], f"layout {layout}: sp"
        if layout == 0:                                      # the device entry point, reads in length order
            dev = torch.device("cuda", 0)
            nb, n = int(off[-1]), len(reads)
            d_bases = torch.zeros(nb + 128, dtype=torch.uint8, device=dev)
            d_bases[:nb] = torch.from_numpy(bases).to(dev)
            d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
            d_order = torch.argsort(torch.from_numpy(np.diff(off.astype(np.int64))), descending=True).to(torch.int32).to(dev)
            d_mlen = torch.zeros(n, dtype=torch.int32, device=dev)
            d_occ = torch.zeros(n, dtype=torch.int64, device=dev)
            d_sp = torch.zeros(n, dtype=torch.int64, device=dev)
            tbl.count_device(d_bases.data_ptr(), d_off.data_ptr(), n, nb, d_mlen.data_ptr(), d_occ.data_ptr(),
                             d_sp.data_ptr(), d_order.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(d_mlen.cpu().numpy().view(np.uint32), wl)
            assert np.array_equal(d_occ.cpu().numpy().view(np.uint64), wo)
            assert np.array_equal(d_sp.cpu().numpy().view(np.uint64), sp)
        tbl.close()
