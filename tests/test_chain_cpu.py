"""CPU tier of chain (include/colbwt.h colbwt_chain_*): the restatement (tests/chain_restatement.py) against a
brute force over every chain of a few hits and against reads planted in a text, and the entry points compiled
with the product sources against the SIMT emulator into a stand-alone program under ASan/UBSan
(tests/emu/chain_emu_main.cpp, built by tests/emu/chain_emu.mk), whose records are compared with the restatement
byte for byte."""
import bisect
import itertools
import os
import subprocess
import sys

import numpy as np

import chain_cases as cc
import chain_restatement as chr_
import helpers
import locate_restatement as lr

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import rlbwt_oracle  # noqa: E402

ACGT = cc.ACGT
EMU_SETTINGS = cc.SETTINGS
EMU_SIZES = (1, 63, 64, 65, 260)


def _drift(hj, hi, band, doc_start):
    """The transition rule of include/colbwt.h written out for small coordinates, independently of the restatement:
    the drift of j -> i, or None when hit j may not precede hit i."""
    (aj, sj, _, tj), (ai, si, li, ti) = hj, hi
    if aj >= ai:
        return None
    gr = sj - (si + li)                      # the read stretch between the two hits
    gt = tj - (ti + li)                      # the text stretch between them
    if gr < 0 or gt < 0:
        return None
    if bisect.bisect_right(doc_start, ti) != bisect.bisect_right(doc_start, tj):     # documents: the last start <= t
        return None
    return abs(gt - gr) if abs(gt - gr) <= band else None


def _brute(hits, band, doc_start):
    """Every chain as an ascending tuple of hit numbers whose neighbours satisfy the transition rule -> {chain: value},
    value = sum of l minus the drifts."""
    out = {}
    for size in range(1, len(hits) + 1):
        for sub in itertools.combinations(range(len(hits)), size):
            value = sum(hits[i][2] for i in sub)
            for j, i in zip(sub, sub[1:]):
                d = _drift(hits[j], hits[i], band, doc_start)
                if d is None:
                    break
                value -= d
            else:
                out[sub] = value
    return out


def test_restatement_equals_brute_force_on_few_hits():
    rng = np.random.default_rng(17)
    doc_start = [0, 60]
    band = 3
    seen = set()
    for trial in range(400):
        K, M = int(rng.integers(1, 5)), int(rng.integers(1, 3))
        start, ln, pos = cc.random_slots(int(rng.integers(1 << 30)), 1, K, M, doc_start)
        if trial % 4 == 0:
            ln[start != cc.AN] = np.where(rng.random(K) < 0.5, 0, ln)[start != cc.AN]    # empty anchors: same-slot pairs with gr = 0
        hits = chr_.hits_of(start[0], ln[0], pos[0])
        assert len(hits) <= 8
        rec, path, text_end = chr_.best_chain(hits, band, doc_start)
        r = dict(zip(chr_.FIELDS, rec))
        if not hits:
            assert rec == chr_.NO_CHAIN
            seen.add("no hits")
            continue
        chains = _brute(hits, band, doc_start)
        best_at = [max(v for c, v in chains.items() if c[-1] == i) for i in range(len(hits))]     # f(i) by enumeration
        assert r["score"] == max(chains.values()) == max(best_at) and r["n_hits"] == len(hits)
        chain = tuple(reversed(path))                                                              # ascending hit numbers
        assert chains[chain] == r["score"] and r["n_chained"] == len(chain)
        e, b = chain[-1], chain[0]
        assert e == best_at.index(max(best_at)), "the smallest end among equals"
        for j, i in zip(chain, chain[1:]):                   # each predecessor: the smallest j among the best candidates
            cands = {x: best_at[x] - d for x in range(i) if (d := _drift(hits[x], hits[i], band, doc_start)) is not None}
            top = max(cands.values())
            assert top > 0 and j == min(x for x, v in cands.items() if v == top)
        # a chain starts where no predecessor adds anything
        d0 = [best_at[x] - d for x in range(b) if (d := _drift(hits[x], hits[b], band, doc_start)) is not None]
        assert not d0 or max(d0) <= 0
        assert (r["text_begin"], r["read_begin"]) == (hits[e][3], hits[e][1])
        assert r["read_end"] == hits[b][1] + hits[b][2] and r["text_len"] == hits[b][3] + hits[b][2] - hits[e][3] == text_end - hits[e][3]
        outside = [h for h in hits if h[3] + h[2] <= r["text_begin"] or h[3] >= text_end]
        assert r["score2"] == max(_brute(outside, band, doc_start).values(), default=0)
        assert r["score2"] <= r["score"]
        if len(chain) >= 3:
            seen.add("three hits chained")
        if r["score2"] > 0:
            seen.add("a runner-up")
        if outside == [] and len(hits) > len(chain):
            seen.add("swallowed")
        if sum(1 for v in best_at if v == max(best_at)) > 1:
            seen.add("tied ends")
        if r["score"] < sum(hits[i][2] for i in chain):
            seen.add("a drift paid")
        # two hits of one slot that the other clauses would let chain: only a_j < a_i keeps them apart
        same = [(x, y) for x in range(len(hits)) for y in range(x + 1, len(hits)) if hits[x][0] == hits[y][0]
                and _drift((hits[x][0] - 1,) + hits[x][1:], hits[y], band, doc_start) is not None]
        if same:
            seen.add("a same-slot pair within the band")
    assert seen == {"no hits", "three hits chained", "a runner-up", "swallowed", "tied ends", "a drift paid",
                    "a same-slot pair within the band"}, seen


def test_handcrafted_records_are_what_the_header_says():
    doc_start = [0, 700, 1500]
    start, ln, pos, want = cc.handcrafted(doc_start)
    got = chr_.reduce_slots(start, ln, pos, cc.BAND, doc_start)
    for k, (label, fields) in enumerate(want):
        for name, value in fields.items():
            assert int(got[name][k]) == value, (label, name, int(got[name][k]), value)


def _planted(rng, text, docs_bytes, doc_start, n, read_len=150, max_subs=7):
    """-> [(read, planted text position, kind)]: substrings of the documents' forward records, mutated."""
    out = []
    for k in range(n):
        d = int(rng.integers(len(docs_bytes)))
        rec = docs_bytes[d]
        at = int(rng.integers(0, len(rec) - read_len))
        src = np.frombuffer(rec[at:at + read_len], np.uint8)
        kind = k % 3
        out.append((cc.mutate(rng, src, kind, int(rng.integers(0, max_subs + 1))), doc_start[d] + at, kind))
        assert text[doc_start[d] + at:doc_start[d] + at + read_len] == rec[at:at + read_len]
    return out


def test_planted_reads_on_unrelated_documents_map_to_their_origin():
    """4 unrelated 3-kbp documents with reverse complements, 141 planted 150-bp reads with 0 .. 7 substitutions, a third
    with one inserted and a third with one deleted base; min_len 10, 16 x 4 slots, band 8.  Every read has a chain on
    its own diagonal (+-1 on the reads with an indel); no read is left out."""
    rng = np.random.default_rng(5)
    recs = [rng.choice(ACGT, size=3000).tobytes() for _ in range(4)]
    text, doc_start = rlbwt_oracle.build_text([[r] for r in recs], revcomp=True)
    planted = _planted(rng, text, recs, doc_start, 141)
    ref = chr_.Chains(text, doc_start)
    got = ref.batch([rd for rd, _, _ in planted], 10, 16, 4, 8)
    joined = 0
    for (rd, origin, kind), c in zip(planted, got):
        assert int(c["text_begin"]) != chr_.NONE, (rd, origin)
        diagonal = int(c["text_begin"]) - int(c["read_begin"])
        assert abs(diagonal - origin) <= (1 if kind else 0), (rd, origin, kind, c)
        assert 1 <= c["n_chained"] <= c["n_hits"] and c["score2"] <= c["score"] and c["read_begin"] < c["read_end"] <= len(rd)
        joined += int(c["n_chained"] >= 2)
    assert joined >= 100, joined


def test_planted_reads_on_related_documents_have_a_runner_up():
    rng = np.random.default_rng(6)
    base = rng.choice(ACGT, size=1500)
    recs = []
    for d in range(4):
        s = base.copy()
        mut = rng.random(s.size) < 0.01
        s[mut] = rng.choice(ACGT, size=int(mut.sum()))
        recs.append(s.tobytes())
    text, doc_start = rlbwt_oracle.build_text([[r] for r in recs], revcomp=True)
    planted = _planted(rng, text, recs, doc_start, 60)
    got = chr_.Chains(text, doc_start).batch([rd for rd, _, _ in planted], 10, 16, 4, 8)
    assert (got["text_begin"] != np.uint64(chr_.NONE)).all()
    assert (got["score2"] <= got["score"]).all() and (got["score2"] > 0).any()
    assert (got["score2"] > got["score"] // 2).sum() >= 30         # the other documents hold nearly the same locus


def test_emulated_chain_equals_restatement_under_asan(tmp_path):
    """colbwt_chain_device (with and without an order array), colbwt_chain_batch, colbwt_chain_file and
    colbwt_anchors_device + colbwt_chain_reduce_device per case in a stand-alone sanitized program: every instantiation
    of the kernel -- (max_anchors, max_occ, band) = (2, 1, 0), (8, 1, 8), (3, 3, 8), (16, 4, 8), (13, 5, 8), (64, 4, 16),
    and (8, 4, 8) and (48, 4, 16) for G = 32 and R = 3 -- as 1, 63, 64, 65 and 260 reads, so that groups straddle a wave
    and a block; then the handcrafted and random slot arrays through colbwt_chain_reduce_device, then the argument
    errors, those of an index with 4097 documents included."""
    tmp = str(tmp_path)
    exe = os.path.join(HERE, "emu", "chain_emu")
    subprocess.check_call(["make", "-C", os.path.join(HERE, "emu"), "-f", "chain_emu.mk"], stdout=subprocess.DEVNULL)
    img, text, starts, sa = cc.index5()
    stem = os.path.join(tmp, "d5")
    open(stem + ".col_pml", "wb").write(bytes(img))
    open(stem + ".col_loc", "wb").write(lr.samples(text, sa, starts))
    ref = chr_.Chains(text, starts, sa)
    reads = cc.mixed_reads(text, max(EMU_SIZES))
    fasta = {}
    for n in EMU_SIZES:
        part = reads[:n]
        bases, off = helpers.concat_reads([np.frombuffer(r, np.uint8) for r in part])
        with open(os.path.join(tmp, f"reads{n}.bin"), "wb") as f:
            f.write(np.uint64(n).tobytes() + off.tobytes() + bases.tobytes())
        fasta[n] = [(f"r{k}", r) for k, r in enumerate(part) if r]          # a FASTA record needs a base
        helpers.write_fasta(os.path.join(tmp, f"reads{n}.fa"), [np.frombuffer(r, np.uint8) for _, r in fasta[n]], [nm for nm, _ in fasta[n]])
    cases = [(setting, n) for setting in EMU_SETTINGS for n in EMU_SIZES]
    with open(os.path.join(tmp, "cases.txt"), "w") as f:
        for k, ((min_len, K, M, band), n) in enumerate(cases):
            f.write(f"c{k} d5 {2 if k % 2 else 4 | (4 << 8)} {min_len} {K} {M} {band} reads{n}\n")
    hs, hl, hp, hand = cc.handcrafted(starts)
    slot_sets = {"hand": (hs, hl, hp, cc.BAND)}
    for k, (n, K, M, band) in enumerate(cc.RANDOM_SETS):
        slot_sets[f"rand{k}"] = cc.random_slots(100 + k, n, K, M, starts) + (band,)
    with open(os.path.join(tmp, "slots.txt"), "w") as f:
        for name, (s, ln, p, band) in slot_sets.items():
            f.write(f"{name} {s.shape[0]} {s.shape[1]} {p.shape[2]} {band}\n")
            open(os.path.join(tmp, name + ".slots"), "wb").write(s.tobytes() + ln.tobytes() + p.tobytes())

    # more than 4096 documents: an argument error (the driver looks for DIR/many)
    mrng = np.random.default_rng(8)
    img_m, text_m = helpers.true_bwt_index_large([mrng.choice(ACGT, size=4200).tobytes()], seed=2)
    open(os.path.join(tmp, "many.col_pml"), "wb").write(bytes(img_m))
    open(os.path.join(tmp, "many.col_loc"), "wb").write(lr.samples(text_m, doc_start=list(range(4097))))

    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe, tmp], env=env, capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and "CHAIN-EMU-OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert "ok argument errors" in out.stdout and "ok more than 4096 documents are refused" in out.stdout

    want = {s: ref.batch(reads, *s) for s in EMU_SETTINGS}
    for s in EMU_SETTINGS[2:]:
        assert (want[s]["n_chained"] >= 2).sum() >= 100 and (want[s]["score2"] > 0).sum() >= 20, s
    assert int(want[EMU_SETTINGS[4]]["n_hits"].max()) > 32 and int(want[EMU_SETTINGS[5]]["n_hits"].max()) > 64
    for k, (setting, n) in enumerate(cases):
        got = open(os.path.join(tmp, f"c{k}.out"), "rb").read()
        assert got == want[setting][:n].tobytes(), f"c{k} {setting} {n}"
        lines = "".join(chr_.line(nm, len(rd), want[setting][int(nm[1:])], starts) + "\n" for nm, rd in fasta[n])
        assert open(os.path.join(tmp, f"c{k}.chains")).read() == lines, f"c{k} {setting} {n}"
    for name, (s, ln, p, band) in slot_sets.items():
        got = np.frombuffer(open(os.path.join(tmp, name + ".out"), "rb").read(), chr_.CHAIN)
        ref_recs = chr_.reduce_slots(s, ln, p, band, starts)
        assert got.tobytes() == ref_recs.tobytes(), name
        if s.shape[1] >= 8:
            assert (ref_recs["n_chained"] >= 3).sum() >= s.shape[0] // 4, name
    got = np.frombuffer(open(os.path.join(tmp, "hand.out"), "rb").read(), chr_.CHAIN)
    for k, (label, fields) in enumerate(hand):
        for field, value in fields.items():
            assert int(got[field][k]) == value, (label, field)
