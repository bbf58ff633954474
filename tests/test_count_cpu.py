"""CPU tier of exact-match counting (include/colbwt.h colbwt_count_*): the plain-Python
restatement against brute-force substring counting on real BWT indexes, and the kernel + host
plumbing compiled against the SIMT emulator against the restatement."""
import os
import subprocess
import sys

import numpy as np
import pytest

import count_restatement
import helpers

HERE = os.path.dirname(os.path.abspath(__file__))


def _texts():
    rng = np.random.default_rng(21)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    a = rng.choice(acgt, size=400).tobytes()
    yield "acgt+repeats", [a, a[100:250], rng.choice(acgt, size=200).tobytes(), b"ACGTACGTACGT" * 5], b"ACGT"
    yield "sigma2", [rng.choice(np.frombuffer(b"ab", np.uint8), size=300).tobytes()], b"ab"
    yield "homopolymer", [b"A" * 120, b"C" * 3, b"A" * 40], b"AC"
    prot = b"ACDEFGHIKLMNPQRSTVWY"
    yield "protein", [rng.choice(np.frombuffer(prot, np.uint8), size=300).tobytes()], prot


@pytest.mark.parametrize("label,seqs,alpha", list(_texts()), ids=[t[0] for t in _texts()])
def test_restatement_equals_brute_force(label, seqs, alpha):
    img, text = helpers.true_bwt_index(seqs, seed=len(label))
    reads = helpers.reads_from_text(text, 60, (1, 80), 0.02, seed=3, alphabet=alpha, extra=b"Nz")
    reads = [bytes(r) for r in reads]
    reads += [text[:-1], b"", b"N", b"NNN" + seqs[0][:5], seqs[0][-7:] + b"Q", seqs[0][:30]]
    t = count_restatement.Table(img)
    for rd in reads:
        assert t.count(rd) == count_restatement.brute_force(text, rd), (label, rd)
    assert t.count(text[:-1])[:2] == (len(text) - 1, 1)     # the whole text occurs once


def test_restatement_decodes_what_unpack_col_pml_decodes():
    img = helpers.random_table(np.random.default_rng(2), 500, max_len=30, split_prob=0.2)
    ref = helpers.unpack_col_pml(img)
    t = count_restatement.Table(img)
    assert t.n == ref["n"] and t.r == ref["r"]
    for j in range(0, 500, 7):
        assert (t.char(j), t.idx(j), t.interval(j), t.offset(j)) == \
            (int(ref["char"][j]), int(ref["idx"][j]), int(ref["interval"][j]), int(ref["offset"][j]))


def test_emulated_count_kernel_matches_restatement_under_asan():
    """Layouts 1-3 and line rows, true-BWT and synthetic tables (long rows, sub-run splits), ragged
    batches, count_file on FASTA / FASTQ / .gz -- kernel and host code under ASan."""
    emu = os.path.join(HERE, "emu")
    subprocess.check_call(["make", "-C", emu, "libcolbwt_emu.so"], stdout=subprocess.DEVNULL)
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"]).decode().strip()
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([sys.executable, os.path.join(emu, "count_emu.py")], env=env,
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "COUNT-EMU-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
