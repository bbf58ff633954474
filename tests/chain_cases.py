"""Slot arrays for colbwt_chain_reduce_device that no anchors call would produce: the handcrafted reads of the
chain tests, each with the record worked out by hand from include/colbwt.h, and random arrays dense in
transitions, ties and NONE entries.  Shared by tests/test_chain_cpu.py and tests/test_gpu_chain.py.  Test
instrument only."""
import numpy as np

import chain_restatement as chr_
import helpers
import locate_restatement as lr

AN = chr_.ANCHOR_NONE
PN = chr_.NONE
U32 = (1 << 32) - 1
K, M, BAND = 4, 2, 8          # the shape and the band of the handcrafted set
ACGT = np.frombuffer(b"ACGT", np.uint8)
# (min_len, max_anchors, max_occ, band): the group sizes G = 8, 8, 16, 64, 64, 64, 32, 64 of the kernel with
# R = 1, 1, 1, 1, 2, 4, 1, 3 hits per lane: every instantiation of chain_kernel
SETTINGS = ((12, 2, 1, 0), (8, 8, 1, 8), (8, 3, 3, 8), (6, 16, 4, 8), (4, 13, 5, 8), (1, 64, 4, 16), (8, 8, 4, 8), (1, 48, 4, 16))
# the random slot sets of the reduction: (n_reads, max_anchors, max_occ, band)
RANDOM_SETS = ((70, 2, 1, 0), (70, 8, 1, 8), (70, 3, 3, 8), (70, 16, 4, 8), (70, 13, 5, 8), (70, 48, 4, 3), (40, 64, 4, 16),
               (70, 6, 5, 8), (70, 17, 1, 8))


def handcrafted(doc_start):
    """-> (start [n, K], len [n, K], pos [n, K, M], [(label, expected fields as a dict)]).  doc_start needs a second
    document that starts at 100 or later; the text positions used lie in document 0 except where a case says so."""
    D = int(doc_start[1])
    assert len(doc_start) >= 2 and D >= 100
    last = int(doc_start[-1])
    far = last + 5000                      # positions in the last document, far from every boundary
    cases = []

    def add(label, slots, **want):
        cases.append((label, slots, want))

    none = dict(text_begin=PN, text_len=0, read_begin=0, read_end=0, score=0, score2=0, n_chained=0, n_hits=0)
    add("no used slot", [], **none)
    add("one hit", [(100, 20, [far])], text_begin=far, text_len=20, read_begin=100, read_end=120, score=20, score2=0, n_chained=1, n_hits=1)
    add("all positions NONE in a used slot", [(100, 20, [])], **none)
    add("the second position only", [(100, 20, [PN, far])], text_begin=far, text_len=20, score=20, n_chained=1, n_hits=1)
    # hit 1 (slot 1, far+94) follows hit 0 with drift 6: f = 14.  Hit 2 (slot 1, far+88) is 12 off hit 0's diagonal: f = 0.
    # Hit 3 could take hit 2 at drift 3, but f(2) - 3 < 0, and hit 1 is 9 off: f = 20, alone.  Were hit 1 -> hit 2 allowed
    # (gr = 0, gt = 6), f(2) would be 8, f(3) 25 and the chain 0 -> 1 -> 2 -> 3.
    add("two hits of one anchor that would chain if allowed", [(200, 20, [far + 200]), (100, 0, [far + 94, far + 88]), (50, 20, [far + 35])],
        score=20, score2=20, n_chained=1, n_hits=4, text_begin=far + 200, text_len=20, read_begin=200, read_end=220)
    add("two occurrences of one anchor", [(100, 20, [far + 500, far])], score=20, score2=20, n_chained=1, n_hits=2, text_begin=far + 500)
    add("drift exactly band", [(100, 20, [far + 100]), (60, 20, [far + 60 - BAND])], score=40 - BAND, score2=0, n_chained=2, n_hits=2,
        text_begin=far + 60 - BAND, text_len=60 + BAND, read_begin=60, read_end=120)
    add("drift band + 1", [(100, 20, [far + 100]), (60, 20, [far + 60 - BAND - 1])], score=20, score2=20, n_chained=1, n_hits=2,
        text_begin=far + 100, text_len=20, read_begin=100, read_end=120)
    add("gt = 0", [(100, 20, [far + 100]), (80, 20, [far + 80])], score=40, n_chained=2, text_begin=far + 80, text_len=40)
    add("gt = -1", [(100, 20, [far + 100]), (80, 20, [far + 81])], score=20, score2=0, n_chained=1, text_begin=far + 100)
    add("gr < 0", [(100, 20, [far + 100]), (90, 20, [far + 80])], score=20, n_chained=1, text_begin=far + 100)
    add("two neighbouring documents", [(100, 20, [D + 2]), (70, 20, [D - 28])], score=20, score2=20, n_chained=1, n_hits=2, text_begin=D + 2)
    add("the same pair inside one document", [(100, 20, [far + 2]), (70, 20, [far - 28])], score=40, score2=0, n_chained=2, text_begin=far - 28)
    add("equal-score predecessors", [(200, 20, [far + 204, far + 196]), (100, 20, [far + 100])], score=36, n_chained=2, n_hits=3,
        text_begin=far + 100, text_len=124, read_end=220)
    add("equal-score chain ends", [(100, 20, [far + 100]), (50, 20, [far + 3000])], score=20, score2=20, text_begin=far + 100, n_chained=1)
    add("f(j) - drift == 0", [(100, BAND, [far + 100 + BAND]), (60, 20, [far + 60])], score=20, n_chained=1, read_begin=60, read_end=80,
        text_begin=far + 60, score2=BAND)
    add("the interval swallows every other hit", [(100, 20, [far + 100]), (70, 10, [far + 90]), (40, 20, [far + 40])], score=40, score2=0,
        n_chained=2, n_hits=3, text_begin=far + 40, text_len=80)
    add("an unused slot between used ones", [(100, 20, [far + 100]), None, (40, 20, [far + 40])], score=40, n_chained=2, n_hits=2)
    add("lengths near 2^31", [(1 << 31, (1 << 31) - 1, [1 << 33]), (1, (1 << 31) - 1, [(1 << 33) - (1 << 31) + 1])], score=U32 - 1,
        n_chained=2, text_len=U32 - 1, read_begin=1, read_end=U32, text_begin=(1 << 33) - (1 << 31) + 1)
    add("f saturates", [(U32 - 1, U32 - 5, [1 << 40]), ((1 << 31) - 2, 1 << 31, [(1 << 40) - (1 << 31)])], score=U32, n_chained=2,
        text_len=U32, read_begin=(1 << 31) - 2, read_end=U32 - 7, text_begin=(1 << 40) - (1 << 31))
    n = len(cases)
    start = np.full((n, K), AN, np.uint32)
    ln = np.full((n, K), 0x5A5A5A5A, np.uint32)                 # whatever: an unused slot's len and pos are not looked at
    pos = np.full((n, K, M), PN, np.uint64)
    for k, (_, slots, _) in enumerate(cases):
        for a, slot in enumerate(slots):
            if slot is None:
                pos[k, a] = 12345                                # garbage under an unused slot
                continue
            start[k, a], ln[k, a] = slot[0], slot[1]
            pos[k, a, :len(slot[2])] = slot[2]
    return start, ln, pos, [(label, want) for label, _, want in cases]


def random_slots(seed, n, max_anchors, max_occ, doc_start):
    """Arrays of the anchors' shape with many transitions per read: slots mostly descending in s with small gaps and
    overlaps, positions on one or two diagonals with a jitter of a few bases, near a document boundary for some
    reads, NONE entries and unused slots anywhere."""
    rng = np.random.default_rng(seed)
    start = np.full((n, max_anchors), AN, np.uint32)
    ln = rng.integers(0, 1 << 32, (n, max_anchors), dtype=np.uint32)
    pos = np.full((n, max_anchors, max_occ), PN, np.uint64)
    bounds = [int(x) for x in doc_start]
    for k in range(n):
        used = rng.random(max_anchors) < rng.choice([0.0, 0.5, 0.9, 1.0], p=[0.05, 0.25, 0.4, 0.3])
        s = int(rng.integers(0, 20)) + 14 * max_anchors
        base = bounds[int(rng.integers(0, len(bounds)))] + int(rng.integers(-40, 400)) - 7 * max_anchors
        diag = [base, base + int(rng.integers(-6, 7)), base + int(rng.integers(500, 900))]
        for a in range(max_anchors):
            L = int(rng.integers(1, 13))
            s -= L + int(rng.integers(-2, 6))
            if s < 0:
                break
            if not used[a]:
                pos[k, a] = rng.integers(0, 1 << 20, max_occ)
                continue
            start[k, a], ln[k, a] = s, L
            for q in range(max_occ):
                if rng.random() < 0.75:
                    pos[k, a, q] = max(diag[int(rng.choice(3, p=[0.6, 0.25, 0.15]))] + s + int(rng.integers(-3, 4)), 0)
    return start, ln, pos


def mutate(rng, src, kind, n_subs):
    """A read out of text bytes `src`: n_subs substitutions, then one inserted (kind 1) or deleted (kind 2) base."""
    rd = src.copy()
    at = rng.choice(rd.size, size=n_subs, replace=False)
    rd[at] = (np.searchsorted(ACGT, rd[at]) + rng.integers(1, 4, n_subs)) % 4          # always another base
    rd[at] = ACGT[rd[at]]
    if kind == 1:
        rd = np.insert(rd, int(rng.integers(30, rd.size - 30)), rng.choice(ACGT))
    elif kind == 2:
        rd = np.delete(rd, int(rng.integers(30, rd.size - 30)))
    return rd.tobytes()


def index5():
    """The index of the emulator and GPU comparisons: five documents, the second a diverged copy of the first, as an
    image with its samples -> (image, text, doc_start, suffix array)."""
    rng = np.random.default_rng(21)
    a = rng.choice(ACGT, size=420)
    b = a.copy()
    mut = rng.random(b.size) < 0.02
    b[mut] = rng.choice(ACGT, size=int(mut.sum()))
    seqs = [a.tobytes(), b.tobytes(), rng.choice(ACGT, size=380).tobytes(), b"ACGT" * 25, a[:90].tobytes()]
    img, text = helpers.true_bwt_index(seqs, seed=3, extra_splits=40)
    starts = [int(x) for x in np.cumsum([0] + [len(s) for s in seqs[:-1]])]
    return img, text, starts, lr.suffix_array(text)


def mixed_reads(text, n):
    """n reads: mutated substrings of the text with and without an indel, then reads that straddle two documents, junk,
    N runs and the empty read."""
    rng = np.random.default_rng(33)
    body = np.frombuffer(text[:-1], np.uint8)
    special = [b"", b"N", text[:-1][400:440] + b"NN" + text[:-1][445:500], rng.choice(ACGT, size=200).tobytes(), b"ACGT" * 30,
               text[:-1][380:470], text[:-1][:5]]
    reads = []
    while len(reads) < n - len(special):
        m = int(rng.integers(70, 150))
        at = int(rng.integers(0, body.size - m))
        reads.append(mutate(rng, body[at:at + m], len(reads) % 3, int(rng.integers(0, 6))))
    reads = reads[:1] + special + reads[1:]
    return reads[:n]
