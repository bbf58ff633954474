"""Plain-Python restatement of locate-all (include/colbwt.h colbwt_locate_all_*) on top of the brute-force
locator of tests/locate_restatement.py: the search is Locator's, a read gets w = occ positions (capped by
max_per_read when that is not 0) when mlen >= min_len and none otherwise, packed as compressed sparse
rows.  Test instrument only."""
import bisect

import numpy as np

import locate_restatement as lr


class LocateAll:
    def __init__(self, text, doc_start=(0,), sa=None, locator=None):
        self.loc = locator if locator is not None else lr.Locator(text, sa)
        self.sa = np.asarray(self.loc.sa, np.uint64)
        self.doc_start = [int(x) for x in doc_start]
        self._found = {}

    def range(self, read):
        """Locator.locate's search without its position list: -> (mlen, sp, ep), the suffix-array range
        [sp, ep] of the read's longest matching suffix (sp > ep when mlen == 0)."""
        read = bytes(read)
        if read not in self._found:
            text, sa, m = self.loc.text, self.loc.sa, len(read)
            best = (0, 0, -1)
            for L in range(1, m + 1):
                suf = read[m - L:]
                if suf[0] <= 1:
                    break
                key = lambda p: text[p:p + L]  # noqa: E731
                lo = bisect.bisect_left(sa, suf, key=key)
                hi = bisect.bisect_right(sa, suf, lo, key=key)
                if hi <= lo:
                    break
                best = (L, lo, hi - 1)
            self._found[read] = best
        return self._found[read]

    def positions(self, read, min_len, max_per_read):
        """-> (mlen, occ, uint64 array SA[ep], SA[ep-1], .. of the read's w positions)"""
        mlen, sp, ep = self.range(read)
        occ = ep - sp + 1 if mlen else 0
        w = occ if mlen >= min_len else 0
        if max_per_read:
            w = min(w, max_per_read)
        return mlen, occ, self.sa[ep - w + 1:ep + 1][::-1] if w else np.zeros(0, np.uint64)

    def batch(self, reads, min_len, max_per_read=0):
        """-> mlen u32[n], occ u64[n], pos_off u64[n + 1], pos u64[pos_off[n]]"""
        n = len(reads)
        mlen = np.zeros(n, np.uint32)
        occ = np.zeros(n, np.uint64)
        pos_off = np.zeros(n + 1, np.uint64)
        parts = []
        for k, rd in enumerate(reads):
            mlen[k], occ[k], p = self.positions(rd, min_len, max_per_read)
            pos_off[k + 1] = pos_off[k] + np.uint64(len(p))
            parts.append(p)
        pos = np.concatenate(parts) if parts else np.zeros(0, np.uint64)
        return mlen, occ, pos_off, pos.astype(np.uint64)

    def line(self, name, read, mlen, occ, positions):
        """One line of a .locate file, without the newline."""
        hits = ",".join("%d:%d" % lr.doc_offset(int(p), self.doc_start) for p in positions)
        return f"{name}\t{len(read)}\t{int(mlen)}\t{int(occ)}\t{hits}"

    def file(self, names, reads, result):
        """The .locate bytes of a batch() result."""
        mlen, occ, pos_off, pos = result
        return "".join(self.line(nm, rd, mlen[k], occ[k], pos[int(pos_off[k]):int(pos_off[k + 1])]) + "\n"
                       for k, (nm, rd) in enumerate(zip(names, reads)))
