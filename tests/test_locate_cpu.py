"""CPU tier of locate (include/colbwt.h colbwt_locate_*): the Python sample writer against the
suffix array it restates (phi from the samples == SA[ISA[x]-1] for every x), the brute-force locator
against count's restatement, and the kernel, attach and builder compiled against the SIMT emulator
against both, under ASan."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import count_restatement
import helpers
import locate_restatement as lr

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import rlbwt_oracle  # noqa: E402


def _parse(loc):
    n_docs = struct.unpack_from("<I", loc, 12)[0]
    n, r, s = struct.unpack_from("<QQQ", loc, 16)
    end_sa = np.frombuffer(loc, np.uint32, r, 40)
    pairs = np.frombuffer(loc, np.uint32, 2 * s, 40 + 4 * r).reshape(s, 2)
    docs = np.frombuffer(loc, np.uint32, n_docs, 40 + 4 * r + 8 * s)
    return n, end_sa, pairs, docs


@pytest.mark.parametrize("revcomp", [False, True])
def test_samples_restate_phi(revcomp):
    """phi(x) = val(a) + (x - a), a = largest sampled position <= x, equals SA[ISA[x]-1] for every x
    but SA[0] on a multi-document text whose separators make runs of 1s next to the final 0."""
    rng = np.random.default_rng(7)
    base = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=120)
    docs = [[base[: 80 + 10 * d].tobytes(), base[5:60].tobytes()] for d in range(3)]
    text, starts = rlbwt_oracle.build_text(docs, revcomp=revcomp)
    sa = lr.suffix_array(text)
    n, end_sa, pairs, dstart = _parse(lr.samples(text, sa, starts))
    assert n == len(text) and list(dstart) == starts
    assert pairs[0, 0] == 0 and (np.diff(pairs[:, 0].astype(np.int64)) > 0).all()
    isa = np.empty(n, np.int64)
    isa[sa] = np.arange(n)
    for x in range(n):
        if isa[x] == 0:
            continue
        a = int(np.searchsorted(pairs[:, 0], x, side="right")) - 1
        assert int(pairs[a, 1]) + (x - int(pairs[a, 0])) == sa[isa[x] - 1], x
    assert end_sa[-1] == sa[-1]


def test_locator_agrees_with_count_restatement():
    seqs = [b"ACGTTGCA" * 20, b"ACGTAC" * 7, b"TTTT"]
    img, text = helpers.true_bwt_index(seqs, seed=2)
    loc = lr.Locator(text)
    t = count_restatement.Table(img)
    for rd in helpers.reads_from_text(text, 60, (1, 40), 0.05, seed=3, extra=b"N"):
        mlen, occ, pos = loc.locate(bytes(rd), 1000)
        assert (mlen, occ) == t.count(bytes(rd))[:2]
        L = mlen
        assert sorted(pos) == sorted(p for p in range(len(text)) if text[p:p + L] == bytes(rd)[len(rd) - L:]) if L else pos == []


def test_emulated_locate_matches_brute_force_under_asan():
    """Layouts 1-3 and line rows on four true-BWT texts, max_occ 1 / 3 / 1000, reads with N, bytes <= 1,
    empty and whole-text reads; attach rejections; the builder's samples == the Python writer's bytes."""
    emu = os.path.join(HERE, "emu")
    subprocess.check_call(["make", "-C", emu, "libcolbwt_emu.so"], stdout=subprocess.DEVNULL)
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"]).decode().strip()
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([sys.executable, os.path.join(emu, "locate_emu.py")], env=env,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "LOCATE-EMU-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
