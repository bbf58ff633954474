"""Plain-Python restatement of anchors (include/colbwt.h colbwt_anchors_*), written from the header text: the
greedy right-to-left factorisation of a read as a loop around the brute-force locator of
tests/locate_restatement.py on prefixes of the read, the per-read summary, the slot arrays and the lines of a
.anchors file.  A second loop of the same shape runs over the rows of a .col_pml image
(tests/count_restatement.py Table) for synthetic tables, which have no text.  Test instrument only."""
import numpy as np

import locate_restatement as lr

ANCHOR_NONE = 0xFFFFFFFF
SUMMARY = ("n_factors", "max_len", "skipped", "n_kept", "cov", "n_unique", "cov_unique", "n_stored")
_ALL = 1 << 20          # the largest max_occ: the cache keeps that many positions per factor


def parse(search, read):
    """The loop of the header over any `search(prefix) -> (L, occ, positions)`:
    -> ([(start, len, occ, positions), ..] in computation order, skipped)."""
    read = bytes(read)
    factors, skipped = [], 0
    e = len(read) - 1
    while e >= 0:
        L, occ, pos = search(read[:e + 1])
        if L == 0:
            skipped += 1
            e -= 1
        else:
            factors.append((e - L + 1, L, occ, pos))
            e -= L
    return factors, skipped


def table_search(table):
    """locate's search over the rows of a count_restatement.Table: its count, with the byte <= 1 rule added
    (the search ends at such a byte).  No positions."""
    def search(prefix):
        cut = max((k for k, c in enumerate(prefix) if c <= 1), default=-1)
        L, occ, _ = table.count(prefix[cut + 1:])
        return L, occ, []
    return search


def summarise(factors, skipped, min_len, max_anchors):
    kept = [f for f in factors if f[1] >= min_len]
    uniq = [f for f in kept if f[2] == 1]
    return (len(factors), max((f[1] for f in factors), default=0), skipped, len(kept), sum(f[1] for f in kept), len(uniq),
            sum(f[1] for f in uniq), min(len(kept), max_anchors)), kept[:max_anchors]


def pack(parsed, min_len, max_anchors, max_occ):
    """[(factors, skipped)] per read -> summary u32 [n, 8], start u32 [n, K], len u32 [n, K], occ u64 [n, K],
    pos u64 [n, K, max_occ] (None when max_occ == 0)."""
    n, K = len(parsed), max_anchors
    summary = np.zeros((n, 8), np.uint32)
    start = np.full((n, K), ANCHOR_NONE, np.uint32)
    ln = np.zeros((n, K), np.uint32)
    occ = np.zeros((n, K), np.uint64)
    pos = np.full((n, K, max_occ), lr.NONE, np.uint64) if max_occ else None
    for k, (factors, skipped) in enumerate(parsed):
        summary[k], stored = summarise(factors, skipped, min_len, K)
        for t, (s, L, o, p) in enumerate(stored):
            start[k, t], ln[k, t], occ[k, t] = s, L, o
            if max_occ:
                w = min(o, max_occ)
                pos[k, t, :w] = p[:w]
    return summary, start, ln, occ, pos


def raw(result):
    """The bytes the emulator driver writes for a pack() result: summary, start, len, occ, pos."""
    return b"".join(a.tobytes() for a in result if a is not None)


class Anchors:
    def __init__(self, text, doc_start=(0,), sa=None, locator=None):
        self.loc = locator if locator is not None else lr.Locator(text, sa)
        self.doc_start = [int(x) for x in doc_start]
        self._parsed = {}

    def factors(self, read):
        """-> ([(start, len, occ, [SA[ep], SA[ep-1], ..]), ..] largest start first, skipped)"""
        read = bytes(read)
        if read not in self._parsed:
            self._parsed[read] = parse(lambda prefix: self.loc.locate(prefix, _ALL), read)
        return self._parsed[read]

    def batch(self, reads, min_len, max_anchors, max_occ):
        return pack([self.factors(r) for r in reads], min_len, max_anchors, max_occ)

    def line(self, name, read, min_len, max_anchors, max_occ):
        """One line of a .anchors file, without the newline."""
        factors, skipped = self.factors(read)
        (nf, mx, sk, nk, cov, nu, cu, _), stored = summarise(factors, skipped, min_len, max_anchors)
        items = []
        for s, L, o, p in stored:
            hits = "".join("@%d:%d" % lr.doc_offset(x, self.doc_start) for x in p[:min(o, max_occ)])
            items.append(f"{s}:{L}:{o}{hits}")
        return f"{name}\t{len(read)}\t{nf}\t{nk}\t{cov}\t{mx}\t{sk}\t{nu}\t{cu}\t" + ",".join(items)

    def file(self, names, reads, min_len, max_anchors, max_occ):
        return "".join(self.line(nm, rd, min_len, max_anchors, max_occ) + "\n" for nm, rd in zip(names, reads))


def planted_reads(text, n_reads, seed, max_len=150, max_subs=5, alphabet=b"ACGTN"):
    """-> [(read, d)]: substrings of `text` of 1 .. max_len bytes that hold no byte <= 1, with d = 0 .. max_subs
    positions overwritten by bytes drawn from `alphabet`: each read is within d substitutions of a text substring."""
    rng = np.random.default_rng(seed)
    t = np.frombuffer(bytes(text), np.uint8)
    alpha = np.frombuffer(alphabet, np.uint8)
    out = []
    while len(out) < n_reads:
        m = int(rng.integers(1, min(max_len, len(t) - 1) + 1))
        s = int(rng.integers(0, len(t) - m))
        rd = t[s:s + m].copy()
        if (rd <= 1).any():
            continue
        d = int(rng.integers(0, min(max_subs, m) + 1))
        at = rng.choice(m, size=d, replace=False)
        rd[at] = rng.choice(alpha, size=d)
        out.append((rd.tobytes(), d))
    return out
