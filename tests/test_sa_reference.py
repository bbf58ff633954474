"""CPU tier: the fast numpy reference (tests/sa_reference.py) that the pangenome-scale GPU test
trusts equals the slow one it restates -- oracle/rlbwt_oracle.build (sa, lcp, heads, lens, thr,
mums) and tests/locate_restatement (samples, Locator) -- on the texts tests/test_rlbwt.py builds."""
import os
import sys

import numpy as np
import pytest

import helpers
import locate_restatement as lr
import sa_reference as sr
from test_rlbwt import ACGT, related_docs

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import rlbwt_oracle as ro  # noqa: E402


def _cases():
    rng = np.random.default_rng(21)
    yield "survey", [[b"GATTACA"], [b"GATTACCGATAACA"]], 3, False
    yield "tiny", [[b"A"], [b"A"]], 1, False
    yield "one_doc", [[b"ACGTTGCAACGT", b"ACGT"]], 2, True
    yield "repeats", [[b"ACACACAC" * 40], [b"ACACACAC" * 40 + b"G"]], 5, False
    yield "homopolymer", [[b"A" * 300 + b"CGT"], [b"GT" + b"A" * 200], [b"A" * 250]], 4, True
    for k in range(6):
        nd = int(rng.integers(1, 5))
        docs = related_docs(rng, nd, int(rng.integers(40, 700)), 0.04, records=int(rng.integers(1, 3)), with_n=k % 3 == 2)
        yield f"random{k}", docs, int(rng.integers(1, 12)), bool(k & 1)
    yield "blocks", related_docs(rng, 2, 5200, 0.02, with_n=True), 8, False
    # more than 32 documents: windows longer than one 32-bit word of document flags
    for rc in (False, True):
        base = rng.choice(ACGT, size=70)
        docs = []
        for _ in range(37):
            s = base.copy()
            at = rng.integers(0, 35, size=2)
            s[at] = rng.choice(ACGT, size=2)
            docs.append([bytes(s)])
        yield f"many_docs_rc{int(rc)}", docs, 6, rc
    yield "identical_pair", [[b"ACGTTAGCAT" * 30], [b"ACGTTAGCAT" * 30], [b"ACGTTAGGAT" * 30]], 5, True


CASES = list(_cases())


@pytest.mark.parametrize("label,docs,min_len,revcomp", CASES, ids=[c[0] for c in CASES])
def test_fast_reference_equals_the_slow_oracle(label, docs, min_len, revcomp):
    slow = ro.build(docs, min_len=min_len, revcomp=revcomp)
    fast = sr.build(slow["text"], slow["doc_start"], min_len)
    assert fast["sa"].tolist() == slow["sa"]
    assert fast["lcp"].tolist() == slow["lcp"]
    assert fast["cap"].tolist() == ro.capped_lcp(slow["text"], slow["sa"])
    assert fast["bwt"].tobytes() == slow["bwt"]
    assert fast["heads"].tolist() == slow["heads"]
    assert fast["lens"].tolist() == slow["lens"]
    assert fast["thr"].tolist() == slow["thr"]
    assert fast["mums"] == slow["mums"]
    # round count: the last rank array is the first without ties
    assert 8 << (fast["rounds"] - 1) > max(slow["lcp"])
    assert fast["rounds"] == 1 or 8 << (fast["rounds"] - 2) <= max(slow["lcp"])
    if label.startswith("many_docs"):
        assert len(slow["mums"]) >= 1
    # the file bytes the GPU test compares with
    nd = len(docs)
    assert ro.file_bytes(fast, nd) == ro.file_bytes(slow, nd)
    # locate: the sample writer over the numpy suffix array, and the locator
    assert sr.samples(slow["text"], fast["sa"], slow["doc_start"]) == lr.samples(slow["text"], doc_start=slow["doc_start"])
    slow_loc, fast_loc = lr.Locator(slow["text"], slow["sa"]), sr.Locator(slow["text"], fast["sa"])
    text = slow["text"]
    reads = [bytes(r) for r in helpers.reads_from_text(text, 60, (1, 60), 0.03, seed=len(text), extra=b"N")]
    reads += [text[:-1], text[3:40], b"", b"N", b"\x01", text[:9] + b"\x01" + text[9:30], text[-12:], b"A" * 400]
    for rd in reads:
        for k in (1, 3, 1000):
            assert fast_loc.locate(rd, k) == slow_loc.locate(rd, k), (rd[:40], k)
        mlen, occ, sp = fast_loc.count(rd)
        if mlen:
            assert [int(p) for p in fast["sa"][sp:sp + occ]] == sorted(slow_loc.locate(rd, occ)[2], key=lambda p: text[p:])
