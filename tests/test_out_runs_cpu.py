"""CPU tier of the output collector (csrc/lane_out.h, OutRuns: push_run, park_item, flush_wave), tested directly: the
probe (tests/emu/out_runs_probe.hip) compiled with g++ against the SIMT emulator into a stand-alone program under
ASan/UBSan (tests/emu/out_runs_probe.mk; nothing is preloaded) plays the scripts of tests/out_runs_cases.py -- every
case in one process -- and the two output arrays are compared, bit for bit, with the per-element formula of
tests/out_runs_restatement.py.  A failure names the lane, the chunk, the trip and the element of the push."""
import os
import subprocess

import numpy as np
import pytest

import out_runs_cases as oc
import out_runs_restatement as orr

HERE = os.path.dirname(os.path.abspath(__file__))
ALL = oc.ALL


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """The emulated probe over all cases, once -> the directory of its result files."""
    emu = os.path.join(HERE, "emu")
    subprocess.check_call(["make", "-C", emu, "-f", "out_runs_probe.mk", "out_runs_probe_emu"], stdout=subprocess.DEVNULL)
    directory = tmp_path_factory.mktemp("out_runs")
    out = oc.run_probe([os.path.join(emu, "out_runs_probe_emu")], directory, timeout=600)
    assert out.returncode == 0 and "OUT-RUNS-PROBE-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    return directory


def test_restatement_on_six_handwritten_pushes():
    """One chunk of 32 elements at address 10, reported from the top down by six pushes; every expected value a literal."""
    pushes = [
        (4, 4, ALL, ALL, 0xEEEEEEEE44434241, 0x1111111111111111),      # a read starts with four matches: 4 3 2 1
        (3, 7, ALL, ALL, 0xFFFFFFFFFF535251, 0x2222222222222222),      # three more: 7 6 5
        (4, 3, ALL, ALL, 0x9999999964636261, 0x3333333333333333),      # an absent character, then three matches: 3 2 1 0
        (2, 1, 0, ALL, 0x7777777777777271, 0x4444444444444444),        # an entry whose second base is a mismatch too: 0 0
        (3, 1, ALL, 0, 0x5555555555838281, 0x5555555555555555),        # a deep entry, mismatch - mismatch - match: 1 0 0
        (16, 17, ALL, ALL, 0x0807060504030201, 0x100F0E0D0C0B0A09),    # sixteen matches in one push: 17 .. 2
    ]
    pml, cid = orr.apply(48, [(10, 32, pushes)])
    fill = orr.PML_FILL
    assert pml.tolist() == [fill] * 10 + [17, 16, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2] + [1, 0, 0] + [0, 0] + [3, 2, 1, 0] + \
        [7, 6, 5] + [4, 3, 2, 1] + [fill] * 6
    fill = orr.CID_FILL
    assert cid.tolist() == [fill] * 10 + list(range(1, 17)) + [0x81, 0x82, 0x83] + [0x71, 0x72] + [0x61, 0x62, 0x63, 0x64] + \
        [0x51, 0x52, 0x53] + [0x41, 0x42, 0x43, 0x44] + [fill] * 6
    # the same through a bias, and the two kinds of entry that keep their first value
    assert (orr.apply(48, [((1 << 32) + 10, 32, pushes)], bias=1 << 32)[0] == pml).all()
    assert [orr.element((2, 1, ALL, ALL, 0xB2B1, 0), e) for e in range(2)] == [(1, 0xB1), (0, 0xB2)]
    assert [orr.element((3, 2, ALL, ALL, 0xC3C2C1, 0), e) for e in range(3)] == [(2, 0xC1), (1, 0xC2), (0, 0xC3)]
    assert orr.element((1, 0, ALL, ALL, 0xD1, 0), 0) == (0, 0xD1)


def test_cases_cover_what_they_are_built_for():
    """What the generator promises, read back from the scripts themselves: every kind of push in both instantiations,
    pushes of 15 and 16 only in push_run<true> cases, every chunk shape of the sweep, element addresses on both sides of
    2^32, the long read's values, the guard's limits (asserted where the guard case is built)."""
    cases = oc.all_cases()
    assert len(cases) == len(oc.CASE_NAMES)
    for up16 in (True, False):
        seen = set()
        for c in cases:
            if c["up16"] == up16:
                seen |= {p[:4] for ln in c["lanes"] for pushes in ln.pushes for p in pushes}
        sizes = {p[0] for p in seen}
        assert sizes == set(range(9)) | ({15, 16} if up16 else set()), sizes
        assert {(2, 1, 0, ALL), (2, 1, ALL, ALL), (3, 2, ALL, ALL), (3, 1, ALL, 0), (1, 0, ALL, ALL)} <= seen
        assert {(n, n - 1, ALL, ALL) for n in range(1, 9)} <= seen and {(n, n, ALL, ALL) for n in range(1, 9)} <= seen
    for name in ("alignment16", "alignment8"):
        shapes = {(a % 64, n) for ln in oc.case_named(name)["lanes"] for a, n in ln.chunks}
        assert shapes == {(r, n) for r in range(64) for n in oc.SWEEP_LENGTHS}
    spans = [(a, a + n) for ln in oc.case_named("high16_1")["lanes"] for a, n in ln.chunks]
    assert min(a for a, _ in spans) < 1 << 32 < max(e for _, e in spans)
    assert all(a >= (1 << 32) + 4096 for ln in oc.case_named("high16_0")["lanes"] for a, _ in ln.chunks)
    long = oc.case_named("long16")
    assert [len(ln.chunks) for ln in long["lanes"]].count(0) == 255
    want, _ = oc._expected("long16")
    base = long["lanes"][77].chunks[0][0]
    assert (want[base:base + 65535] == np.arange(65535, 0, -1)).all()
    random_lanes = [ln for seed in (1, 2, 3, 4, 5) for ln in oc.case_named(f"random16_{seed}")["lanes"]]
    assert len(random_lanes) == 5 * 256 and max(len(ln.chunks) for ln in random_lanes) == 6
    assert max(n for ln in random_lanes for _, n in ln.chunks) > 90


@pytest.mark.parametrize("name", oc.CASE_NAMES)
def test_emulated_collector_equals_restatement_under_asan(results, name):
    """Both arrays bit for bit -- the chunks and the guard elements around them -- and per lane and wave what the probe
    recorded: no push refused, the largest count the scheduler's, every lane finished with an empty collector, the
    canary words behind the flush's LDS area intact, the flush counts (emitting lanes per flush, whole blocks, ragged
    items) the scheduler's."""
    oc.check_case(oc.case_named(name), results)


def test_recorded_properties(results):
    """Taken from what the probe recorded on its side, not from the scheduler: the collector has been full (96 and
    never more), flushes with 0, 1, 31, 32, 33 and 64 emitting lanes, whole-block and ragged items, and both in one
    flush."""
    lanes, waves = {}, {}
    for name in oc.CASE_NAMES:
        lanes[name] = np.fromfile(f"{results}/{name}.lanes", np.uint32).reshape(-1, 4)
        waves[name] = np.fromfile(f"{results}/{name}.waves", np.uint32).reshape(-1, oc.WAVE_WORDS)
        assert (waves[name][:, oc.W_CANARY] == 1).all() and (lanes[name][:, 1:] == (0, 1, 0)).all(), name
    assert lanes["guard16"][:, 0].max() == 96 and (lanes["guard16"][:, 0] == 96).sum() >= 1
    assert max(l[:, 0].max() for l in lanes.values()) == 96
    assert max(lanes[n][:, 0].max() for n in oc.CASE_NAMES if n.startswith(("alignment8", "emitting8", "seams8", "random8"))) <= 95
    for name in ("emitting16", "emitting8"):
        w = waves[name]
        for k, emitters in enumerate((1, 31, 32, 33, 64)):
            assert w[k, emitters] == 3 and w[k, oc.W_MAX_EMIT] == emitters, (name, k)
        assert w[5, 0] >= 1 and w[6, 0] == w[6, oc.W_FLUSHES] > 0 and w[6, oc.W_MAX_EMIT] == 0
        assert w[8, 64] == 1 and w[8, oc.W_RAGGED] == 128 and w[10, 33] == 1 and w[10, oc.W_RAGGED] == 66
        assert w[9, oc.W_WHOLE] == 127 and w[9, oc.W_RAGGED] == 0
        assert w[7, oc.W_MIXED] >= 1 and w[11, oc.W_MIXED] >= 1
    for name in oc.CASE_NAMES:
        if not name.startswith(("emitting", "seams")):
            assert waves[name][:, oc.W_WHOLE].sum() > 0 and waves[name][:, oc.W_RAGGED].sum() > 0, name
    assert waves["long16"][1, oc.W_WHOLE] == 1023 and waves["long16"][0, 0] == waves["long16"][0, oc.W_FLUSHES]
