"""Plain-Python restatement of locate (include/colbwt.h colbwt_locate_*): the .col_loc sample file
written from a suffix array, and a brute-force locator over sorted suffixes.  Test instrument only."""
import bisect
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import rlbwt_oracle  # noqa: E402

NONE = (1 << 64) - 1


def suffix_array(text):
    return np.asarray(rlbwt_oracle.suffix_array(bytes(text)), np.int64)


def samples(text, sa=None, doc_start=(0,)):
    """-> the .col_loc bytes of `text`: header, end_sa of every folded run (bytes <= 1 one character),
    phi pairs (SA[j], SA[j-1]) at every unfolded byte change, sorted by SA[j], doc_start."""
    text = bytes(text)
    sa = suffix_array(text) if sa is None else np.asarray(sa, np.int64)
    t = np.frombuffer(text, np.uint8)
    n = len(t)
    bwt = t[(sa - 1) % n]
    folded = np.maximum(bwt, 1)
    ends = np.flatnonzero(np.append(folded[1:] != folded[:-1], True))
    end_sa = sa[ends].astype(np.uint32)
    j = np.flatnonzero(bwt[1:] != bwt[:-1]) + 1
    pairs = np.stack([sa[j], sa[j - 1]], axis=1).astype(np.uint32)
    pairs = pairs[np.argsort(pairs[:, 0], kind="stable")]
    docs = np.asarray(doc_start, np.uint32)
    head = b"COLBWTLC" + struct.pack("<IIQQQ", 1, len(docs), n, len(end_sa), len(pairs))
    return head + end_sa.tobytes() + pairs.tobytes() + docs.tobytes()


class Locator:
    """Brute force over the sorted suffixes of a text: for L = 1, 2, .. the suffixes that start with
    the read's last L bytes form the range [sp, ep] (two bisections over SA); the search ends at a byte <= 1 or
    an empty range.  -> (mlen, occ, [SA[ep], SA[ep-1], .. at most max_occ])."""

    def __init__(self, text, sa=None):
        self.text = bytes(text)
        self.sa = [int(p) for p in (suffix_array(self.text) if sa is None else sa)]

    def locate(self, read, max_occ):
        read = bytes(read)
        m = len(read)
        best = (0, 0, [])
        for L in range(1, m + 1):
            suf = read[m - L:]
            if suf[0] <= 1:
                break
            key = lambda p: self.text[p:p + L]  # noqa: E731  (sorted suffixes: their L-prefixes ascend)
            lo = bisect.bisect_left(self.sa, suf, key=key)
            hi = bisect.bisect_right(self.sa, suf, lo, key=key)
            if hi <= lo:
                break
            best = (L, hi - lo, [int(self.sa[hi - 1 - i]) for i in range(min(hi - lo, max_occ))])
        return best


def doc_offset(pos, doc_start):
    d = int(np.searchsorted(np.asarray(doc_start, np.int64), pos, side="right")) - 1
    return d, int(pos) - int(doc_start[d])
