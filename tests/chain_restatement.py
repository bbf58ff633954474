"""Plain-Python restatement of chain (include/colbwt.h colbwt_chain_*), written from the header text: the hits
of a read's slot arrays, the dynamic program, the best chain, the runner-up, the packed 32-byte records and the
lines of a .chains file.  The slot arrays come from tests/anchors_restatement.py, documents and offsets from
tests/locate_restatement.py.  Test instrument only."""
import numpy as np

import anchors_restatement as ar
import locate_restatement as lr

ANCHOR_NONE = ar.ANCHOR_NONE
NONE = lr.NONE
U32 = (1 << 32) - 1
M64 = (1 << 64) - 1
CHAIN = np.dtype([("text_begin", np.uint64), ("text_len", np.uint32), ("read_begin", np.uint32), ("read_end", np.uint32),
                  ("score", np.uint32), ("score2", np.uint32), ("n_chained", np.uint16), ("n_hits", np.uint16)])
FIELDS = CHAIN.names
NO_CHAIN = (NONE, 0, 0, 0, 0, 0, 0, 0)


def _signed(x):
    """A value taken modulo 2^64, read as signed 64-bit."""
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def doc_of(t, doc_start):
    """The last d with doc_start[d] <= t (0 at the least: doc_start[0] is 0)."""
    d = 0
    for k, x in enumerate(doc_start):
        if x <= t:
            d = k
    return d


def hits_of(start, ln, pos):
    """Slot arrays of one read (start[K], len[K], pos[K][M]) -> [(a, s, l, t)] numbered by (a, q) ascending."""
    out = []
    for a in range(len(start)):
        if int(start[a]) == ANCHOR_NONE:
            continue
        for q in range(len(pos[a])):
            if int(pos[a][q]) != NONE:
                out.append((a, int(start[a]), int(ln[a]), int(pos[a][q])))
    return out


def drift_of(hj, hi, band, same_doc):
    """The drift of the transition j -> i (j < i is the caller's), or None when j may not precede i."""
    aj, sj, _, tj = hj
    ai, si, li, ti = hi
    if not aj < ai:
        return None
    gr = sj - (si + li)
    gt = _signed(tj - ((ti + li) & M64))
    if gr < 0 or gt < 0 or not same_doc:
        return None
    drift = abs(gt - gr)
    return drift if drift <= band else None


def program(hits, band, doc_start):
    """-> (f, pred) of every hit: f(i) = l_i + max(0, max_j (f(j) - drift)), stored saturated to u32."""
    docs = [doc_of(h[3], doc_start) for h in hits]
    f, pred = [], []
    for i, hi in enumerate(hits):
        best, frm = 0, None
        for j in range(i):
            d = drift_of(hits[j], hi, band, docs[i] == docs[j])
            if d is not None and f[j] - d > best:       # strictly larger: the smallest j among equals stays
                best, frm = f[j] - d, j
        f.append(min(hi[2] + best, U32))
        pred.append(frm)
    return f, pred


def best_chain(hits, band, doc_start):
    """-> (record tuple in FIELDS order, the path [e, .., b] as hit numbers, text_end)."""
    if not hits:
        return NO_CHAIN, [], None
    f, pred = program(hits, band, doc_start)
    e = max(range(len(hits)), key=lambda i: (f[i], -i))
    path = [e]
    while pred[path[-1]] is not None:
        path.append(pred[path[-1]])
    b = path[-1]
    _, se, _, te = hits[e]
    _, sb, lb, tb = hits[b]
    text_end = (tb + lb) & M64
    outside = [h for h in hits if ((h[3] + h[2]) & M64) <= te or h[3] >= text_end]
    score2 = max(program(outside, band, doc_start)[0], default=0)
    rec = (te, min((text_end - te) & M64, U32), se, (sb + lb) & U32, f[e], score2, len(path), len(hits))
    return rec, path, text_end


def chain_of(start, ln, pos, band, doc_start):
    return best_chain(hits_of(start, ln, pos), band, doc_start)[0]


def pack(records):
    out = np.zeros(len(records), CHAIN)
    for k, rec in enumerate(records):
        out[k] = rec
    return out


def reduce_slots(start, ln, pos, band, doc_start):
    """start / len [n, K], pos [n, K, M] -> CHAIN records [n]: what colbwt_chain_reduce_device computes."""
    return pack([chain_of(start[k], ln[k], pos[k], band, doc_start) for k in range(len(start))])


def line(name, m, rec, doc_start):
    """One line of a .chains file, without the newline."""
    r = dict(zip(FIELDS, (int(x) for x in rec)))
    where = "*\t*" if r["text_begin"] == NONE else "%d\t%d" % lr.doc_offset(r["text_begin"], doc_start)
    return (f"{name}\t{m}\t{r['read_begin']}\t{r['read_end']}\t{where}\t{r['text_len']}\t{r['score']}\t{r['score2']}"
            f"\t{r['n_chained']}\t{r['n_hits']}")


class Chains:
    """Chains of reads against a text: anchors by tests/anchors_restatement.py, then the reduction."""

    def __init__(self, text, doc_start=(0,), sa=None, anchors=None):
        self.anchors = anchors if anchors is not None else ar.Anchors(text, doc_start, sa)
        self.doc_start = [int(x) for x in doc_start]

    def batch(self, reads, min_len, max_anchors, max_occ, band):
        _, start, ln, _, pos = self.anchors.batch(reads, min_len, max_anchors, max_occ)
        return reduce_slots(start, ln, pos, band, self.doc_start)

    def file(self, names, reads, min_len, max_anchors, max_occ, band):
        recs = self.batch(reads, min_len, max_anchors, max_occ, band)
        return "".join(line(nm, len(rd), rec, self.doc_start) + "\n" for nm, rd, rec in zip(names, reads, recs))
