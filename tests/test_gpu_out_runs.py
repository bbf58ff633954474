"""GPU tier of the output collector (csrc/lane_out.h, OutRuns: push_run, park_item, flush_wave), tested directly: the
probe (tests/emu/out_runs_probe.hip) compiled by hipcc for gfx950 (tests/emu/out_runs_probe.mk) plays the scripts of
tests/out_runs_cases.py on the MI355X -- a child process of its own, every case in it -- and the two output arrays are
compared, bit for bit, with the per-element formula of tests/out_runs_restatement.py: the same cases and the same
comparisons as tests/test_out_runs_cpu.py makes on the emulator."""
import os
import subprocess

import numpy as np
import pytest

import out_runs_cases as oc

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """The probe over all cases on the GPU, once -> the directory of its result files.  Without hipcc the build fails,
    and so does every test here."""
    emu = os.path.join(HERE, "emu")
    subprocess.check_call(["make", "-C", emu, "-f", "out_runs_probe.mk", "out_runs_probe_gpu"], stdout=subprocess.DEVNULL)
    directory = tmp_path_factory.mktemp("out_runs_gpu")
    out = oc.run_probe(["timeout", "-k", "10", "120", os.path.join(emu, "out_runs_probe_gpu")], directory, timeout=150)
    assert out.returncode == 0 and "OUT-RUNS-PROBE-OK" in out.stdout, f"exit status {out.returncode}\n" + out.stdout[-3000:] + out.stderr[-3000:]
    return directory


@pytest.mark.parametrize("name", oc.CASE_NAMES)
def test_collector_equals_restatement(results, name):
    """Both arrays bit for bit -- the chunks and the guard elements around them -- and per lane and wave what the probe
    recorded: no push refused, the largest count the scheduler's, every lane finished with an empty collector, the
    canary words behind the flush's LDS area intact, the flush counts the scheduler's."""
    oc.check_case(oc.case_named(name), results)


def test_recorded_properties(results):
    """From the probe's own records: the collector has been full (96 and never more), 64 lanes of a wave have emitted in
    one flush and a wave has had a flush with nobody emitting, whole-block and ragged items have been stored."""
    lanes = {n: np.fromfile(f"{results}/{n}.lanes", np.uint32).reshape(-1, 4) for n in oc.CASE_NAMES}
    waves = {n: np.fromfile(f"{results}/{n}.waves", np.uint32).reshape(-1, oc.WAVE_WORDS) for n in oc.CASE_NAMES}
    for name in oc.CASE_NAMES:
        assert (waves[name][:, oc.W_CANARY] == 1).all() and (lanes[name][:, 1:] == (0, 1, 0)).all(), name
    assert max(l[:, 0].max() for l in lanes.values()) == 96 == lanes["guard16"][:, 0].max()
    for name in ("emitting16", "emitting8"):
        w = waves[name]
        for k, emitters in enumerate((1, 31, 32, 33, 64)):
            assert w[k, emitters] == 3 and w[k, oc.W_MAX_EMIT] == emitters, (name, k)
        assert w[5, 0] >= 1 and w[6, 0] == w[6, oc.W_FLUSHES] > 0
        assert w[9, oc.W_WHOLE] == 127 and w[9, oc.W_RAGGED] == 0 and w[7, oc.W_MIXED] >= 1 and w[11, oc.W_MIXED] >= 1
    assert waves["long16"][1, oc.W_WHOLE] == 1023
