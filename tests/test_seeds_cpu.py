"""CPU tier of the seeds reduction (include/colbwt.h colbwt_seeds_*): the plain-Python restatement
against the invariants of a true query output and against a second, vectorised formulation, and the
kernel + host plumbing compiled against the SIMT emulator against the restatement."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import seeds_restatement as sr
from __graft_entry__ import load_oracle, load_package

HERE = os.path.dirname(os.path.abspath(__file__))
PARAMS = ((1, 1000), (1, 2), (3, 3), (8, 1), (20, 16))


def _cases():
    rng = np.random.default_rng(31)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    seqs = [rng.choice(acgt, size=400).tobytes() for _ in range(3)] + [b"ACGTACGTACGT" * 6]
    seqs.append(seqs[0][100:300])
    for extra in (0, 20, 150):
        img, text = helpers.true_bwt_index(seqs, seed=7 + extra, extra_splits=extra)
        reads = helpers.reads_from_text(text, 150, (1, 300), 0.03, seed=5, extra=b"Nn")
        reads += [np.frombuffer(text[:-1], np.uint8), np.zeros(0, np.uint8), np.frombuffer(b"N", np.uint8)]
        yield f"true-bwt splits {extra}", img, reads
    for seed, alpha, max_len, split in ((1, b"ACGT", 9, 0.1), (2, b"AC", 5, 0.3), (3, b"ACGTNX", 30, 0.05)):
        trng = np.random.default_rng(seed)
        img = helpers.random_table(trng, 3000, alphabet=alpha, max_len=max_len, split_prob=split)
        reads = helpers.backward_walk_reads(img, 80, 150, 0.02, seed)
        reads += [trng.choice(np.frombuffer(alpha + b"Z", np.uint8), size=int(m)) for m in trng.integers(0, 90, 60)]
        yield f"random table sigma {len(alpha)}", img, reads


CASES = list(_cases())


@pytest.mark.parametrize("label,img,reads", CASES, ids=[c[0] for c in CASES])
def test_restatement_on_oracle_output(label, img, reads):
    """The three invariants of include/colbwt.h hold, and the loop equals the vectorised formulation."""
    bases, off = helpers.concat_reads(reads)
    pml, cid = load_oracle().OracleIndex(bytes(img)).query_batch(bases, off)
    assert pml.any() and (label.startswith("random") or cid.any())
    for min_len, max_seeds in PARAMS:
        got = sr.seeds(pml, cid, off, min_len, max_seeds)
        sr.check_invariants(got[0], got[1], got[2], off, min_len, max_seeds)
        want = sr.seeds_vectorised(pml, cid, off, min_len, max_seeds)
        for name, g, w in zip(("summary", "seed_pos", "seed_len", "seed_cid"), got, want):
            assert np.array_equal(g, w), (label, min_len, max_seeds, name)
        # unused slots, and the run property the definition does not rely on
        n = np.minimum(got[0][:, 0], max_seeds)
        for r in range(len(reads)):
            assert (got[1][r, n[r]:] == sr.SEED_NONE).all() and not got[2][r, n[r]:].any() and not got[3][r, n[r]:].any()
            assert (np.diff(got[1][r, :n[r]].astype(np.int64)) < 0).all(), "largest pos first"


def test_restatement_equals_vectorised_on_arbitrary_arrays():
    rng = np.random.default_rng(9)
    for trial in range(40):
        lens = rng.integers(0, 40, rng.integers(1, 60))
        off = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
        n = int(off[-1])
        top = (3, 30, 2 ** 32)[trial % 3]
        pml = np.where(rng.random(n) < 0.25, 0, rng.integers(1, top, n)).astype(np.uint32)
        cid = np.where(rng.random(n) < 0.7, 0, rng.integers(1, 256, n)).astype(np.uint8)
        for min_len, max_seeds in ((1, 3), (2, 1000), (8, 1)):
            got = sr.seeds(pml, cid, off, min_len, max_seeds)
            want = sr.seeds_vectorised(pml, cid, off, min_len, max_seeds)
            for g, w in zip(got, want):
                assert np.array_equal(g, w), (trial, min_len, max_seeds)


def test_restatement_by_hand():
    #            read 0: runs [0,3) id 7, [4,6) id 0 | read 1: run [0,2) id 9 wraps from 250
    pml = np.array([3, 2, 1, 0, 2, 1, 2, 1, 0, 1], np.uint16)
    cid = np.array([0, 7, 5, 9, 0, 0, 0, 9, 3, 250], np.uint8)
    off = np.array([0, 6, 10], np.uint64)
    s, pos, ln, sc = sr.seeds(pml, cid, off, 1, 2)
    assert s[0].tolist() == [2, 3, 5, 1, 1, 3, 0, 0] and pos[0].tolist() == [4, 0] and ln[0].tolist() == [2, 3]
    assert sc[0].tolist() == [0, 7]
    # read 1: seeds (0, 2, 9) and (3, 1, 250); a = 9 at the smaller pos, b = 250: d = 241 -> desc
    assert s[1].tolist() == [2, 2, 3, 1, 2, 3, 0, 1] and pos[1].tolist() == [3, 0] and sc[1].tolist() == [250, 9]
    s, pos, ln, sc = sr.seeds(pml, cid, off, 3, 2)
    assert s[0].tolist() == [1, 3, 3, 1, 1, 3, 0, 0] and pos[0].tolist() == [0, sr.SEED_NONE]


def test_exports_and_header_declare_seeds():
    pkg = load_package()
    header = open(pkg.HEADER_PATH).read()
    for name in ("colbwt_seeds_reduce_device", "colbwt_seeds_batch", "colbwt_seeds_file"):
        assert name in pkg.EXPORTS and name + "(" in header


def test_seeds_chunk_restatement_is_pinned():
    """helpers.seeds_chunk, the tests' restatement of seeds_chunk() in csrc/seeds_reduce.h, at values
    derived by hand from ceil(n_bases / 65536 / 512) * 512 clamped to 2048..16384, and the knob's
    rule: a multiple of 512 in 512..16384, anything else ignored."""
    for n_bases, chunk in ((0, 2048), (18_000_000, 2048), (90_000_000, 2048), (134_283_263, 2048), (134_283_264, 2560),
                           (140_000_000, 2560), (180_000_000, 3072), (400_000_000, 6144), (15873 * 65536 - 1, 15872),
                           (15873 * 65536, 16384), (1_100_000_000, 16384), (1_500_000_000, 16384), (4_400_000_000, 16384)):
        assert helpers.seeds_chunk(n_bases) == chunk, n_bases
        assert helpers.seeds_chunk(n_bases, {}) == chunk and helpers.seeds_chunk(n_bases, {"OTHER": "512"}) == chunk
    for text in ("512", "1024", "1536", "2048", "2560", "16384"):
        assert helpers.seeds_chunk(400_000_000, {helpers.SEEDS_KNOB: text}) == int(text)
    for text in ("", "0", "256", "513", "2049", "16896", "32768", "-512", "+512", " 512", "512 ", "0x200", "5e2", "2048,1"):
        assert helpers.seeds_chunk(400_000_000, {helpers.SEEDS_KNOB: text}) == 6144, text
    assert [helpers.seeds_waves(n, 2048) for n in (0, 1, 2048, 2049, 4096)] == [1, 1, 1, 2, 2]


def test_emulated_seeds_kernel_matches_restatement_under_asan():
    """Layouts 1-3 and line rows, empty / 1-base / ragged / long reads, the u32 path, crafted arrays
    and alignment sweeps through seeds_reduce_device, seeds_file on FASTA / FASTQ / .gz, two
    replicas; then read starts, runs of empty reads, a read over several chunks and batches of exactly
    k chunks at the wave boundaries of COLBWT_SEEDS_CHUNK = 512, 1024, 2048, 2560 and 16384, and
    seeds_batch with one and two replicas at 512 and 16384 -- kernel and host code under ASan."""
    emu = os.path.join(HERE, "emu")
    subprocess.check_call(["make", "-C", emu, "libcolbwt_emu.so"], stdout=subprocess.DEVNULL)
    asan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"]).decode().strip()
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0")
    env.pop(helpers.SEEDS_KNOB, None)
    out = subprocess.run([sys.executable, os.path.join(emu, "seeds_emu.py")], env=env,
                         capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and "SEEDS-EMU-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
