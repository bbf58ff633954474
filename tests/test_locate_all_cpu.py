"""CPU tier of locate-all (include/colbwt.h colbwt_locate_all_*): the restatement
(tests/locate_all_restatement.py) against a plain scan of the text, and the entry points compiled with
the product sources against the SIMT emulator into a stand-alone program under ASan/UBSan
(tests/emu/locate_all_emu_main.cpp, built by tests/emu/locate_all_emu.mk with a tile of 4 positions and
with the product's tile), whose outputs are compared with the restatement byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import locate_all_restatement as la
import locate_restatement as lr

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import rlbwt_oracle  # noqa: E402

LINE_ROWS_4 = 4 | (4 << 8)          # include/colbwt.h COLBWT_LAYOUT_LINE_ROWS_STEPS(4)


def _scan(text, pattern):
    """Every p with text[p:p+len(pattern)] == pattern, by scanning the text."""
    found = []
    p = text.find(pattern)
    while p >= 0:
        found.append(p)
        p = text.find(pattern, p + 1)
    return found


@pytest.mark.parametrize("revcomp", [False, True])
def test_restatement_equals_scan_on_a_multi_document_text(revcomp):
    rng = np.random.default_rng(31)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    base = rng.choice(acgt, size=160)
    docs = []
    for d in range(4):
        recs = []
        for j in range(2):
            s = base[j * 30:j * 30 + 90 + 10 * d].copy()
            mut = rng.random(s.size) < 0.03
            s[mut] = rng.choice(acgt, size=int(mut.sum()))
            recs.append(s.tobytes())
        docs.append(recs)
    text, starts = rlbwt_oracle.build_text(docs, revcomp=revcomp)
    reads = [bytes(r) for r in helpers.reads_from_text(text, 80, (1, 50), 0.02, seed=8, extra=b"N")]
    reads += [docs[1][0], b"", b"N", docs[2][1][:20] + b"\x01" + docs[2][1][20:30], b"A", b"AC"]
    ref = la.LocateAll(text, starts)
    brute = lr.Locator(text)
    names = [f"r{k}" for k in range(len(reads))]
    for min_len in (1, 12):
        for cap in (0, 3):
            mlen, occ, pos_off, pos = ref.batch(reads, min_len, cap)
            assert pos_off[0] == 0 and pos_off.size == len(reads) + 1 and pos.size == int(pos_off[-1]) and pos.dtype == np.uint64
            lines = ref.file(names, reads, (mlen, occ, pos_off, pos)).split("\n")
            assert lines[-1] == "" and len(lines) == len(reads) + 1
            for k, rd in enumerate(reads):
                L = int(mlen[k])
                hits = _scan(text, rd[len(rd) - L:]) if L else []
                assert int(occ[k]) == len(hits)
                got = [int(x) for x in pos[int(pos_off[k]):int(pos_off[k + 1])]]
                w = len(hits) if L >= min_len else 0
                w = min(w, cap) if cap else w
                assert len(got) == w and set(got) <= set(hits) and len(set(got)) == w
                # locate's order: the same list the brute-force locator gives at max_occ = w
                bm, bo, bp = brute.locate(rd, max(w, 1))
                assert (bm, bo) == (L, len(hits)) and got == bp[:w]
                want_hits = ",".join("%d:%d" % lr.doc_offset(p, starts) for p in got)
                assert lines[k] == f"r{k}\t{len(rd)}\t{L}\t{len(hits)}\t{want_hits}"
            if min_len == 1 and cap == 0:
                assert int(occ.max()) >= 40 and (np.diff(pos_off.astype(np.int64)) == occ.astype(np.int64)).all()
            if min_len == 12:
                assert ((mlen < 12) & (occ > 0)).any() and (np.diff(pos_off.astype(np.int64))[mlen < 12] == 0).all()


def _emu_inputs(tmp):
    """Index image, sample file, FASTA files and raw read dumps of the emulator cases -> the case list."""
    rng = np.random.default_rng(2)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    a = rng.choice(acgt, size=260).tobytes()
    seqs = [a, a[60:200], rng.choice(acgt, size=150).tobytes(), b"ACGT" * 25, a[:70]]
    img, text = helpers.true_bwt_index(seqs, seed=6, extra_splits=40)
    body = text[:-1]
    starts = [int(x) for x in np.cumsum([0] + [len(s) for s in seqs[:-1]])]
    sa = lr.suffix_array(text)
    stem = os.path.join(tmp, "d5")
    open(stem + ".col_pml", "wb").write(bytes(img))
    open(stem + ".col_loc", "wb").write(lr.samples(text, sa, starts))
    ref = la.LocateAll(text, starts, sa)
    special = [body,                                       # the whole text
               b"",                                        # empty
               b"N" + body[:6], body[10:30] + b"N",        # N at either end
               body[:5] + b"\x01" + body[5:25],            # a byte <= 1 ends the search
               body[3:9] + b"\x00",                        # ... also as the last byte
               b"ACGT" * 26, body[-8:], b"A"]
    sampled = [bytes(r) for r in helpers.reads_from_text(text, 248, (1, 60), 0.02, seed=4, extra=b"N")]
    more = [b"A", b"AC", b"ACGT" * 3]                      # tens of tiles of 4, runs longer than a tile
    read_sets = {260: sampled + special + more, 66: special + sampled[:54] + more, 4: [body[100:140]] + more}
    fasta_sets = {}
    for n, reads in read_sets.items():
        assert len(reads) == n
        bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
        with open(os.path.join(tmp, f"reads{n}.bin"), "wb") as f:
            f.write(np.uint64(n).tobytes() + off.tobytes() + bases.tobytes())
        fasta_sets[n] = [(f"r{k}", r) for k, r in enumerate(reads) if all(b >= 32 for b in r)]   # what a FASTA line can hold
        helpers.write_fasta(os.path.join(tmp, f"reads{n}.fa"), [np.frombuffer(r, np.uint8) for _, r in fasta_sets[n]],
                            [nm for nm, _ in fasta_sets[n]])
    cases = []
    for layout in (2, LINE_ROWS_4):
        for min_len, cap in ((1, 0), (12, 0), (1, 3)):
            cases.append((layout, min_len, cap, 260))
        for n in (4, 66):
            cases.append((layout, 1, 0, n))
    with open(os.path.join(tmp, "cases.txt"), "w") as f:
        for k, (layout, min_len, cap, n) in enumerate(cases):
            f.write(f"c{k} d5 {layout} {min_len} {cap} reads{n}\n")
    return cases, ref, read_sets, fasta_sets, text, sa


@pytest.mark.parametrize("tile", [4, 0])
def test_emulated_locate_all_equals_restatement_under_asan(tmp_path, tile):
    """Plan + fill (whole, in two read ranges, with pos_cap below the need), colbwt_locate_all_batch and
    colbwt_locate_all_file per case in a stand-alone sanitized program built with a tile of 4 positions and
    with the product's tile: layouts 2 and line rows K = 4, (min_len, max_per_read) (1, 0) / (12, 0) / (1, 3),
    reads with N, a byte <= 1, an empty read, the whole text, A, AC and ACGT x 3, as 4 / 66 / 260 reads;
    then the argument errors."""
    tmp = str(tmp_path)
    out_name = "locate_all_emu_t4" if tile else "locate_all_emu"
    exe = os.path.join(HERE, "emu", out_name)
    make = ["make", "-C", os.path.join(HERE, "emu"), "-f", "locate_all_emu.mk", "OUT=" + out_name]
    subprocess.check_call(make + ([f"TILE=-DCOLBWT_LOCATE_ALL_TILE={tile}"] if tile else []), stdout=subprocess.DEVNULL)
    cases, ref, read_sets, fasta_sets, text, sa = _emu_inputs(tmp)
    # what the small tile is for: reads of tens of tiles, and folded runs longer than a tile inside their ranges
    _, sp, ep = ref.range(b"A")
    assert ep - sp + 1 >= 40 * 4
    t = np.frombuffer(text, np.uint8)
    bwt = np.maximum(t[(sa - 1) % len(t)], 1)[sp:ep + 1]
    ends = np.flatnonzero(np.append(bwt[1:] != bwt[:-1], True))
    assert int(np.diff(ends).max()) > 4, "no run longer than a tile of 4 inside the range of A"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe, tmp], env=env, capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and "LOCATE-ALL-EMU-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.startswith(f"tile {tile or 256}\n")
    assert "ok argument errors" in out.stdout
    for k, (layout, min_len, cap, n) in enumerate(cases):
        label = f"c{k} {(layout, min_len, cap, n)}"
        mlen, occ, pos_off, pos = ref.batch(read_sets[n], min_len, cap)
        want = mlen.tobytes() + occ.tobytes() + pos_off.tobytes() + pos.tobytes()
        assert open(os.path.join(tmp, f"c{k}.out"), "rb").read() == want, label
        names, reads = [nm for nm, _ in fasta_sets[n]], [r for _, r in fasta_sets[n]]
        assert open(os.path.join(tmp, f"c{k}.locate")).read() == ref.file(names, reads, ref.batch(reads, min_len, cap)), label
