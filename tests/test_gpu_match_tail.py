"""GPU tier: the match tail of the K = 8 mismatch-line rows (csrc/fat_layout.h: a row carries the
steps 9 .. 16 of its leading positions; fat2_query.hip consumes 16 matching bases in one trip and
lane_out.h takes them in one push).  The cases of tests/match_tail_cases.py -- exact reads of every
length around one and two trips, benchmark-like reads, 2 000-base exact reads that keep the
collector at its guard, multi-read chunks, tables whose tails are partly invalid, and the shapes
that must not change -- each bit-equal to the oracle with COLBWT_MATCH_TAIL=1 and =0, on tables of
3 000 and 60 000 rows with layouts 5 and 6.  That the tail is really walked is shown by the trip
counters of the emulated tier (tests/emu/match_tail_emu.py); here every K = 8 table must report
rows with a tail."""
import pytest

import match_tail_cases as mt

pytestmark = pytest.mark.gpu

CASE_NAMES = (
    [f"{kind}/{t}" for t in ("synth3000_s0", "synth3000_s50", "synth60000_s0", "synth60000_s50") for kind in ("exact", "bench_like", "guard")]
    + [f"{kind}/{t}" for t in ("synth3000_s50", "synth60000_s0") for kind in ("chunk8", "chunk2_singles")]
    + [f"{kind}/{t}" for t in ("five_chars", "thr_mode1") for kind in ("exact", "bench_like")]
    + ["unchanged/synth3000_s50"])


@pytest.fixture(scope="module")
def world(pkg, oracle):
    tbls = mt.tables(pkg)
    cases = {c[0]: c for c in mt.cases(tbls)}
    assert sorted(cases) == sorted(CASE_NAMES)
    refs = {name: oracle.OracleIndex(img) for name, img in tbls.items()}
    return tbls, cases, refs, {}


@pytest.mark.parametrize("name", CASE_NAMES)
def test_match_tail_equals_oracle_on_and_off(pkg, world, name):
    tbls, cases, refs, expected = world
    _, t, reads, layouts, chunk = cases[name]
    key = (t, id(reads))
    if key not in expected:                                  # the chunk cases share the exact reads and their answer
        expected[key] = refs[t].query_batch(*reads)
    permille = mt.check_case(pkg, tbls[t], reads, layouts, chunk, expected[key], name)
    for layout, pm in permille.items():
        assert (pm > 0) == (layout in mt.TAIL_LAYOUTS), (name, hex(layout), pm)
