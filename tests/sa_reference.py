"""Fast numpy restatement of oracle/rlbwt_oracle.py (suffix array, LCP, RLBWT, thresholds,
multi-MUMs) and of tests/locate_restatement.Locator, for texts of tens of Mchar: the pure-Python
loops of the slow oracle (Kasai, capped LCP, thresholds, multi-MUMs) stop at a few Mchar.

TEST INFRASTRUCTURE ONLY.  The definitions are the slow oracle's, stated again over whole arrays:

  suffix array   prefix doubling seeded with the first 8 bytes of every suffix packed in a u64
                 (zero past the end; the final 0 is unique); each round re-sorts only the suffixes
                 still in a group of size > 1 by (rank, rank h further on).  Ranks are group-head
                 positions, so equal rank after round j <=> equal first 8 * 2^j bytes, and every
                 round's rank array is kept (int32) for the LCP.
  LCP            binary lifting over those rank arrays, then at most 7 byte comparisons.
  capped LCP     min(LCP, distance from SA[k] to the first separator at or after it).
  RLBWT          runs of the folded BWT (bytes <= 1 are one class).
  thresholds     per character, the first minimum of (capped LCP << 32 | position) over
                 (end of the previous run of c, head of this run]: one np.minimum.reduceat.
  multi-MUMs     the window tests of rlbwt_oracle.multi_mums over a sliding minimum of width
                 n_docs - 1; the one-per-document and left-maximal tests only on the candidates.

tests/test_sa_reference.py pins every output to the slow oracle on the texts tests/test_rlbwt.py uses.
"""
import bisect

import numpy as np

import locate_restatement

_MAX_U64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _group_heads(sorted_keys):
    head = np.empty(sorted_keys.size, bool)
    head[:1] = True
    head[1:] = sorted_keys[1:] != sorted_keys[:-1]
    return head


def _tied(head):
    """Mask of the entries whose group (a head and the non-heads after it) holds more than one."""
    starts = np.flatnonzero(head)
    sizes = np.diff(np.append(starts, head.size))
    return np.repeat(sizes > 1, sizes)


def suffix_array(text):
    """-> (sa int64, levels): levels[j] (int32) is the rank array after round j; the last is unique."""
    t = np.frombuffer(bytes(text), np.uint8)
    n = t.size
    assert n >= 1 and t[-1] == 0 and (t[:-1] > 0).all(), "the text ends with its only 0"
    padded = np.zeros(n + 8, np.uint64)
    padded[:n] = t
    key = np.zeros(n, np.uint64)
    for b in range(8):
        key = (key << np.uint64(8)) | padded[b:b + n]
    del padded
    sa = np.argsort(key).astype(np.int64)
    key = key[sa]
    head = _group_heads(key)
    del key
    rank = np.empty(n, np.int32)
    rank[sa] = np.maximum.accumulate(np.where(head, np.arange(n, dtype=np.int64), 0))
    levels = [rank.copy()]
    act = np.flatnonzero(_tied(head))          # suffix-array slots still tied, ascending
    h = 8
    while act.size:
        s = sa[act]
        nxt = s + h
        second = np.where(nxt < n, rank[np.minimum(nxt, n - 1)].astype(np.int64) + 1, 0)
        k = (rank[s].astype(np.uint64) << np.uint64(32)) | second.astype(np.uint64)
        o = np.argsort(k)
        k, s = k[o], s[o]
        sa[act] = s                            # groups keep their slots: they are ordered by head position
        head = _group_heads(k)
        rank[s] = np.maximum.accumulate(np.where(head, act, 0))
        levels.append(rank.copy())
        act = act[_tied(head)]
        h *= 2
    return sa, levels


def lcp_array(text, sa, levels):
    """lcp[k] = common prefix of suffixes sa[k-1], sa[k]; lcp[0] = 0 (int64)."""
    t = np.frombuffer(bytes(text), np.uint8)
    n = t.size
    a, b = sa[:-1], sa[1:]
    l = np.zeros(n - 1, np.int64)

    def equal_at(arr):
        pa, pb = a + l, b + l
        ok = (pa < n) & (pb < n)
        return ok & (arr[np.minimum(pa, n - 1)] == arr[np.minimum(pb, n - 1)])
    for j in range(len(levels) - 2, -1, -1):
        l += (8 << j) * equal_at(levels[j])
    for _ in range(7):
        l += equal_at(t)
    return np.concatenate(([0], l))


def capped_lcp(text, sa, lcp):
    """The LCP cut at the first separator (byte <= 1) of SA[k]: what a pattern can tell apart."""
    t = np.frombuffer(bytes(text), np.uint8)
    seps = np.flatnonzero(t <= 1)
    nxt = seps[np.searchsorted(seps, sa)]
    return np.minimum(lcp, nxt - sa)


def rlbwt(text, sa):
    """-> (bwt uint8, heads uint8, lens int64, starts int64): runs of the folded characters."""
    t = np.frombuffer(bytes(text), np.uint8)
    bwt = t[sa - 1]                                  # sa == 0: t[-1], the final 0
    folded = np.maximum(bwt, 1)
    starts = np.flatnonzero(_group_heads(folded))
    return bwt, folded[starts], np.diff(np.append(starts, t.size)), starts


def thresholds(heads, lens, starts, cap):
    """First position of the minimum capped LCP in (end of the previous run of c, head of the run]."""
    n = int(np.sum(lens))
    ends = starts + lens - 1
    key = np.empty(n + 1, np.uint64)
    key[:n] = (cap.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    key[n] = _MAX_U64
    thr = np.zeros(heads.size, np.int64)
    for c in np.unique(heads):
        runs = np.flatnonzero(heads == c)
        if runs.size < 2:
            continue
        idx = np.empty(2 * (runs.size - 1), np.int64)
        idx[0::2] = ends[runs[:-1]] + 1              # segment k: [end of run k-1 + 1, head of run k]
        idx[1::2] = starts[runs[1:]] + 1             # the gap to the next segment (ignored)
        thr[runs[1:]] = (np.minimum.reduceat(key, idx)[0::2] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return thr


def _window_min(x, w):
    """out[i] = min(x[i:i + w]) for i in 0 .. x.size - w (blocks of w: suffix and prefix minima)."""
    m = x.size
    nb = -(-m // w)
    X = np.full(nb * w, np.iinfo(x.dtype).max, x.dtype)
    X[:m] = x
    X = X.reshape(nb, w)
    pre = np.minimum.accumulate(X, axis=1).ravel()
    suf = np.minimum.accumulate(X[:, ::-1], axis=1)[:, ::-1].ravel()
    return np.minimum(suf[:m - w + 1], pre[w - 1:m])


def multi_mums(text, sa, doc_start, cap, min_len, chunk=1 << 16):
    """[(length, suffix-array rank of the first suffix)], ascending by rank."""
    t = np.frombuffer(bytes(text), np.uint8)
    n, nd = t.size, len(doc_start)
    if nd < 2 or n < nd:
        return []
    inner = _window_min(cap[1:], nd - 1)             # inner[i] = min(cap[i + 1 .. i + nd - 1]), i <= n - nd
    i = np.arange(n - nd + 1)
    after = np.full(i.size, -1, np.int64)
    after[:-1] = cap[nd:]                            # cap[i + nd]; none past the end
    ok = (inner >= max(1, min_len)) & (cap[:n - nd + 1] < inner) & (after < inner)
    cand = np.flatnonzero(ok)
    docs = np.asarray(doc_start, np.int64)
    out = []
    for c0 in range(0, cand.size, chunk):
        c = cand[c0:c0 + chunk]
        pos = sa[c[:, None] + np.arange(nd)]
        d = np.sort(np.searchsorted(docs, pos, side="right") - 1, axis=1)
        one_each = (np.diff(d, axis=1) > 0).all(axis=1)
        before = t[pos - 1]
        same = (before == before[:, :1]).all(axis=1) & (before[:, 0] > 1)
        keep = c[one_each & ~same]
        out += list(zip(inner[keep].tolist(), keep.tolist()))
    return out


def build(text, doc_start, min_len=20):
    """Everything rlbwt_oracle.build gives for a prepared text, as numpy arrays (mums: list of tuples)."""
    sa, levels = suffix_array(text)
    lcp = lcp_array(text, sa, levels)
    rounds = len(levels)
    del levels
    cap = capped_lcp(text, sa, lcp)
    bwt, heads, lens, starts = rlbwt(text, sa)
    return dict(text=bytes(text), doc_start=list(doc_start), sa=sa, lcp=lcp, cap=cap, rounds=rounds, bwt=bwt, heads=heads,
                lens=lens, starts=starts, thr=thresholds(heads, lens, starts, cap),
                mums=multi_mums(text, sa, doc_start, cap, min_len))


def samples(text, sa, doc_start=(0,)):
    """The .col_loc bytes (locate_restatement.samples takes a numpy suffix array as it is)."""
    return locate_restatement.samples(text, sa, doc_start)


class Locator:
    """locate_restatement.Locator's search over a numpy suffix array: the range [sp, ep] of the
    suffixes starting with the read's last L bytes by two bisections of SA with a slice key.  A
    suffix of the read that occurs has shorter suffixes that occur, so the longest L (read bytes
    <= 1 end it) is found by bisecting L as well.  -> (mlen, occ, [SA[ep], SA[ep-1], .. at most max_occ])."""

    def __init__(self, text, sa):
        self.text = bytes(text)
        self.sa = np.asarray(sa, np.int64)

    def _range(self, suf):
        L = len(suf)
        key = lambda p: self.text[p:p + L]  # noqa: E731  (sorted suffixes: their L-prefixes ascend)
        lo = bisect.bisect_left(self.sa, suf, key=key)
        return lo, bisect.bisect_right(self.sa, suf, lo, key=key)

    def search(self, read):
        """-> (mlen, sp, ep + 1); (0, 0, 0) when not even the last byte occurs."""
        read = bytes(read)
        m = len(read)
        top = next((m - 1 - i for i in range(m - 1, -1, -1) if read[i] <= 1), m)
        lo_l, hi_l, best = 0, top, (0, 0)
        while lo_l < hi_l:
            mid = (lo_l + hi_l + 1) // 2
            sp, ep1 = self._range(read[m - mid:])
            if ep1 > sp:
                lo_l, best = mid, (sp, ep1)
            else:
                hi_l = mid - 1
        return (lo_l,) + best if lo_l else (0, 0, 0)

    def count(self, read):
        """-> (mlen, occ, sp) as colbwt_count_* reports them."""
        mlen, sp, ep1 = self.search(read)
        return mlen, ep1 - sp, sp

    def locate(self, read, max_occ):
        mlen, sp, ep1 = self.search(read)
        return mlen, ep1 - sp, self.sa[max(sp, ep1 - max_occ):ep1][::-1].tolist()
