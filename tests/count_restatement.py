"""Plain-Python restatement of exact-match counting (backward search) over the rows of a
`.col_pml` image -- the checker of colbwt_count_* on synthetic tables.  Written from the
semantics in include/colbwt.h, not from the kernel:

  [sp, ep] = [0, n-1]; for i = m-1 .. 0, c = P[i]:
    s = first position >= sp whose row character is c, e = last position <= ep holding c;
    c absent from the table, or s > e: stop;
    sp, ep = LF(s), LF(e)  (landing row + offset, then fast-forward); sp > ep: stop (base not consumed)
  mlen = bases consumed, occ = ep - sp + 1 (0 when mlen == 0), sp (0 when mlen == 0).

Rows are decoded one at a time from the image (the fields helpers.unpack_col_pml decodes), so
the restatement also runs over tables of hundreds of millions of rows.
"""
import bisect
import struct

HDR = 32
ROW = 18


class Table:
    def __init__(self, image):
        self.buf = memoryview(image).cast("B")   # bytes or a uint8 array, not copied
        _, self.n, self.r, _ = struct.unpack_from("<4Q", self.buf, 0)
        # characters present (small tables; on huge ones an absent character fails the scans instead)
        self._present = {self.buf[HDR + ROW * j] for j in range(self.r)} if self.r <= 1 << 20 else None

    def char(self, j):
        return self.buf[HDR + ROW * j]

    def idx(self, j):
        if j >= self.r:
            return self.n
        return int.from_bytes(self.buf[HDR + ROW * j + 1:HDR + ROW * j + 6], "little")

    def interval(self, j):
        return int.from_bytes(self.buf[HDR + ROW * j + 6:HDR + ROW * j + 10], "little")

    def offset(self, j):
        return int.from_bytes(self.buf[HDR + ROW * j + 10:HDR + ROW * j + 12], "little")

    def length(self, j):
        return self.idx(j + 1) - self.idx(j)

    def present(self, c):
        if self._present is not None:
            return c in self._present
        return True   # huge tables: an absent character shows up as a failed scan

    def row_of(self, p):
        """Row holding position p (idx[row] <= p < idx[row + 1])."""
        return bisect.bisect_right(_IdxSeq(self), p) - 1

    def lf(self, p):
        """LF_table::LF (LF_table.hpp:251-262) of position p, as a position."""
        j = self.row_of(p)
        o = p - self.idx(j)
        k = self.interval(j)
        t = self.offset(j) + o
        while t >= self.length(k) and k < self.r - 1:   # fast-forward
            t -= self.length(k)
            k += 1
        return self.idx(k) + t

    def succ_pos(self, p, c):
        """First position >= p whose row character is c, or None."""
        j = self.row_of(p)
        if self.char(j) == c:
            return p
        for k in range(j + 1, self.r):
            if self.char(k) == c:
                return self.idx(k)
        return None

    def pred_pos(self, p, c):
        """Last position <= p whose row character is c, or None."""
        j = self.row_of(p)
        if self.char(j) == c:
            return p
        for k in range(j - 1, -1, -1):
            if self.char(k) == c:
                return self.idx(k + 1) - 1
        return None

    def count(self, read):
        """-> (mlen, occ, sp) of one read (bytes-like)."""
        read = bytes(read)
        sp, ep = 0, self.n - 1
        k = 0
        for c in reversed(read):
            if not self.present(c):
                break
            s, e = self.succ_pos(sp, c), self.pred_pos(ep, c)
            if s is None or e is None or s > e:
                break
            ns, ne = self.lf(s), self.lf(e)
            if ns > ne:
                break
            sp, ep = ns, ne
            k += 1
        if k == 0:
            return 0, 0, 0
        return k, ep - sp + 1, sp


class _IdxSeq:
    """idx[0 .. r) as a sequence for bisect."""

    def __init__(self, t):
        self.t = t

    def __len__(self):
        return self.t.r

    def __getitem__(self, j):
        return self.t.idx(j)


def count_reads(image, reads):
    """[(mlen, occ, sp)] for every read."""
    t = Table(image)
    return [t.count(rd) for rd in reads]


def brute_force(text, read, with_sp=True):
    """(mlen, occ, sp) by substring counting over `text` (a true-BWT index's text: unique smallest
    terminator): the longest suffix of the read that occurs, its overlapping occurrences and the
    number of the text's suffixes that sort below it (quadratic; None unless with_sp)."""
    text, read = bytes(text), bytes(read)
    m = len(read)
    best = 0
    for L in range(1, m + 1):
        if text.find(read[m - L:]) < 0:
            break
        best = L
    if best == 0:
        return 0, 0, 0
    pat = read[m - best:]
    occ = sum(1 for i in range(len(text) - best + 1) if text[i:i + best] == pat)
    sp = sum(1 for i in range(len(text)) if text[i:] < pat) if with_sp else None
    return best, occ, sp
