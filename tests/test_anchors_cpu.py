"""CPU tier of anchors (include/colbwt.h colbwt_anchors_*): the restatement (tests/anchors_restatement.py)
against a plain scan of the text, and the entry points compiled with the product sources against the SIMT
emulator into a stand-alone program under ASan/UBSan (tests/emu/anchors_emu_main.cpp, built by
tests/emu/anchors_emu.mk), whose outputs are compared with the restatement byte for byte -- on true BWT
indexes with positions, and on a synthetic table (no text, max_occ = 0) for the progress rule."""
import os
import subprocess
import sys

import numpy as np
import pytest

import anchors_restatement as ar
import count_restatement as cr
import helpers
import locate_restatement as lr
from __graft_entry__ import load_package

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import rlbwt_oracle  # noqa: E402

LINE_ROWS_4 = 4 | (4 << 8)          # include/colbwt.h COLBWT_LAYOUT_LINE_ROWS_STEPS(4)
SETTINGS = ((1, 16, 4), (12, 2, 1), (1, 16, 0))     # (min_len, max_anchors, max_occ)


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
    planted = ar.planted_reads(text, 120, seed=8)
    special = [b"", b"N", docs[2][1][:20] + b"\x01" + docs[2][1][20:30], text, b"N" + docs[1][0][:30] + b"NN" + docs[3][1][5:40] + b"N",
               rng.choice(acgt, size=200).tobytes()]             # unrelated to the text: tens of short factors
    reads = [r for r, _ in planted] + special
    subs = [d for _, d in planted] + [None] * len(special)
    ref = ar.Anchors(text, starts)
    brute = lr.Locator(text)
    seen = set()
    for rd, d in zip(reads, subs):
        factors, skipped = ref.factors(rd)
        m = len(rd)
        assert sum(f[1] for f in factors) + skipped == m
        covered = np.zeros(m, bool)
        for start, L, occ, pos in factors:
            hits = _scan(text, rd[start:start + L])
            assert L >= 1 and occ == len(hits) and len(pos) == occ and set(pos) == set(hits)
            assert all(b > 1 for b in rd[start:start + L]) and not covered[start:start + L].any()
            covered[start:start + L] = True
        for k, (start, L, occ, pos) in enumerate(factors):
            # left-maximal: the read starts here, or the base in front is skipped, or the extension occurs nowhere
            assert start == 0 or not covered[start - 1] or text.find(rd[start - 1:start + L]) < 0 or rd[start - 1] <= 1
            if k:
                assert start + L <= factors[k - 1][0], "largest start first"
        assert int((~covered).sum()) == skipped
        for k in np.flatnonzero(~covered):          # a skipped base occurs nowhere as a character of the text (or is <= 1)
            assert rd[k] <= 1 or text.find(rd[k:k + 1]) < 0
        if d is not None:
            assert len(factors) + skipped <= 2 * d + 1, (rd, d)
        mlen, occ, pos = brute.locate(rd, 1 << 20)
        if mlen:
            assert factors[0] == (m - mlen, mlen, occ, pos)
        else:
            assert not factors or factors[0][0] + factors[0][1] < m
        # coverage of the cases
        if len(factors) >= 3:
            seen.add("three factors")
        if m and not covered[0]:
            seen.add("skipped at the start")
        if m and not covered[-1]:
            seen.add("skipped at the end")
        if (~covered[1:-1]).any():
            seen.add("skipped inside")
        kept12 = [f for f in factors if f[1] >= 12]
        if len(kept12) > 2:
            seen.add("more anchors than max_anchors 2")
        if len(factors) > 16:
            seen.add("more anchors than max_anchors 16")
        if any(a[1] < 12 <= b[1] or b[1] < 12 <= a[1] for a, b in zip(factors, factors[1:])):
            seen.add("short factor next to a long one")
        if any(f[2] > 1 for f in kept12) and any(f[2] > 4 for f in factors):
            seen.add("occ above max_occ")
    assert seen == {"three factors", "skipped at the start", "skipped at the end", "skipped inside", "more anchors than max_anchors 2",
                    "more anchors than max_anchors 16", "short factor next to a long one", "occ above max_occ"}, seen
    # the packed arrays and the file lines say the same as the factor lists
    names = [f"r{k}" for k in range(len(reads))]
    for min_len, K, W in SETTINGS + ((12, 16, 2),):
        summary, start, ln, occ, pos = ref.batch(reads, min_len, K, W)
        lines = ref.file(names, reads, min_len, K, W).split("\n")
        assert lines[-1] == "" and len(lines) == len(reads) + 1
        for k, rd in enumerate(reads):
            factors, skipped = ref.factors(rd)
            kept = [f for f in factors if f[1] >= min_len]
            s = dict(zip(ar.SUMMARY, (int(x) for x in summary[k])))
            assert s["n_factors"] == len(factors) and s["skipped"] == skipped and s["n_kept"] == len(kept)
            assert s["max_len"] == max((f[1] for f in factors), default=0) and s["cov"] == sum(f[1] for f in kept)
            assert s["n_unique"] == sum(1 for f in kept if f[2] == 1) and s["cov_unique"] == sum(f[1] for f in kept if f[2] == 1)
            assert s["n_stored"] == min(len(kept), K)
            if min_len == 1:
                assert s["cov"] + s["skipped"] == len(rd)
            ns = s["n_stored"]
            assert (start[k, ns:] == ar.ANCHOR_NONE).all() and not ln[k, ns:].any() and not occ[k, ns:].any()
            items = []
            for t, f in enumerate(kept[:K]):
                assert (int(start[k, t]), int(ln[k, t]), int(occ[k, t])) == f[:3]
                w = min(f[2], W)
                if W:
                    assert [int(x) for x in pos[k, t, :w]] == f[3][:w] and (pos[k, t, w:] == lr.NONE).all()
                items.append(f"{f[0]}:{f[1]}:{f[2]}" + "".join("@%d:%d" % lr.doc_offset(p, starts) for p in f[3][:w]))
            if W:
                assert (pos[k, ns:] == lr.NONE).all()
            else:
                assert pos is None
            assert lines[k] == (f"r{k}\t{len(rd)}\t{s['n_factors']}\t{s['n_kept']}\t{s['cov']}\t{s['max_len']}\t{s['skipped']}"
                                f"\t{s['n_unique']}\t{s['cov_unique']}\t" + ",".join(items))


def _emu_inputs(tmp):
    """Index images, the sample file, FASTA files and raw read dumps of the emulator cases -> the case list."""
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
    ref = ar.Anchors(text, starts, sa)
    special = [body,                                       # the whole text
               b"",                                        # empty
               b"N" + body[:6], body[10:30] + b"N",        # N at either end
               body[:5] + b"\x01" + body[5:25],            # a byte <= 1 is skipped, the search goes on behind it
               body[3:9] + b"\x00",                        # ... also as the last byte
               b"N", b"NNN", body[40:70] + b"NN" + body[300:340] + b"N" + body[5:9],
               b"ACGT" * 26, body[-8:], rng.choice(acgt, size=180).tobytes()]     # the last: more than 16 factors
    sampled = [r for r, _ in ar.planted_reads(text, 245, seed=4)]
    more = [b"A", b"AC", b"ACGT" * 3]
    read_sets = {260: sampled + special + more, 66: special + sampled[:51] + more, 4: [body[100:140]] + more}
    # the synthetic table: reads walked out of it with substitutions, and junk
    synth = load_package().synth_index(3000, mean_len=5, split_permille=100, seed=9).tobytes()
    open(os.path.join(tmp, "synth.col_pml"), "wb").write(synth)
    trng = np.random.default_rng(12)
    sreads = [bytes(r) for r in helpers.backward_walk_reads(synth, 40, 120, 0.03, 3)]
    sreads += [trng.choice(np.frombuffer(b"ACGTN\x01", np.uint8), size=int(m)).tobytes() for m in trng.integers(0, 90, 26)]
    read_sets["s66"] = sreads
    fasta_sets = {}
    for n, reads in read_sets.items():
        assert len(reads) == (66 if n == "s66" else n)
        bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in reads])
        with open(os.path.join(tmp, f"reads{n}.bin"), "wb") as f:
            f.write(np.uint64(len(reads)).tobytes() + off.tobytes() + bases.tobytes())
        fasta_sets[n] = [(f"r{k}", r) for k, r in enumerate(reads) if all(b >= 32 for b in r)]   # what a FASTA line can hold
        helpers.write_fasta(os.path.join(tmp, f"reads{n}.fa"), [np.frombuffer(r, np.uint8) for _, r in fasta_sets[n]],
                            [nm for nm, _ in fasta_sets[n]])
    cases = []
    for layout in (2, LINE_ROWS_4):
        for setting in SETTINGS:
            cases.append(("d5", layout, setting, 260))
        for n in (4, 66):
            cases.append(("d5", layout, SETTINGS[0], n))
        cases.append(("synth", layout, (1, 16, 0), "s66"))
        cases.append(("synth", layout, (12, 2, 0), "s66"))
    with open(os.path.join(tmp, "cases.txt"), "w") as f:
        for k, (index, layout, (min_len, K, W), n) in enumerate(cases):
            f.write(f"c{k} {index} {layout} {min_len} {K} {W} reads{n}\n")
    return cases, ref, read_sets, fasta_sets, synth


def test_emulated_anchors_equal_restatement_under_asan(tmp_path):
    """colbwt_anchors_device (with and without an order array, with NULL slots), colbwt_anchors_batch and
    colbwt_anchors_file per case in a stand-alone sanitized program: layouts 2 and line rows K = 4, the settings
    (1, 16, 4) / (12, 2, 1) / (1, 16, 0) -- the last without samples attached -- as 4 / 66 / 260 reads (a partial
    wave, a partial block), then a synthetic table at max_occ = 0 against the table-level restatement (every read
    terminates and sum(len) + skipped == m), then the argument errors."""
    tmp = str(tmp_path)
    exe = os.path.join(HERE, "emu", "anchors_emu")
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu"), "-f", "anchors_emu.mk"], stdout=subprocess.DEVNULL)
    cases, ref, read_sets, fasta_sets, synth = _emu_inputs(tmp)
    table = cr.Table(synth)
    search = ar.table_search(table)
    synth_parsed = {}
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe, tmp], env=env, capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and "ANCHORS-EMU-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert "ok argument errors" in out.stdout
    for k, (index, layout, (min_len, K, W), n) in enumerate(cases):
        label = f"c{k} {(index, layout, min_len, K, W, n)}"
        reads = read_sets[n]
        got = open(os.path.join(tmp, f"c{k}.out"), "rb").read()
        names, freads = [nm for nm, _ in fasta_sets[n]], [r for _, r in fasta_sets[n]]
        text_out = open(os.path.join(tmp, f"c{k}.anchors")).read()
        if index == "d5":
            assert got == ar.raw(ref.batch(reads, min_len, K, W)), label
            assert text_out == ref.file(names, freads, min_len, K, W), label
            continue
        for rd in reads:
            if rd not in synth_parsed:
                synth_parsed[rd] = ar.parse(search, rd)
                factors, skipped = synth_parsed[rd]
                assert sum(f[1] for f in factors) + skipped == len(rd)
        want = ar.pack([synth_parsed[rd] for rd in reads], min_len, K, 0)
        assert got == ar.raw(want), label
        summary = np.frombuffer(got[:32 * len(reads)], np.uint32).reshape(-1, 8)
        lens = np.array([len(r) for r in reads])
        assert (summary[:, 0] <= lens).all() and summary[:, 0].max() >= 3
