"""Plain-Python restatement of docs (include/colbwt.h colbwt_docs_*) on top of the brute-force locator
of tests/locate_restatement.py: the walked positions are locate's first min(occ, max_walk) when
mlen >= min_len, each mapped to its document.  Test instrument only."""
import numpy as np

import locate_restatement as lr


def mask_words(n_docs):
    return (n_docs + 63) // 64


class Docs:
    def __init__(self, text, doc_start, sa=None, locator=None):
        self.loc = locator if locator is not None else lr.Locator(text, sa)
        self.doc_start = [int(x) for x in doc_start]
        self.n_docs = len(self.doc_start)
        self.words = mask_words(self.n_docs)
        self._located = {}

    def locate(self, read, max_walk):
        """Locator.locate(read, max_walk); the search is done once per read (its positions do not
        depend on the cap, which only cuts the list)."""
        key = bytes(read)
        if key not in self._located:
            self._located[key] = self.loc.locate(key, 1 << 62)
        mlen, occ, pos = self._located[key]
        return mlen, occ, pos[:max_walk]

    def docs(self, read, min_len, max_walk):
        """-> (mlen, occ, [document numbers, ascending])"""
        mlen, occ, pos = self.locate(read, max_walk)
        if mlen < min_len:
            pos = []
        return mlen, occ, sorted({lr.doc_offset(p, self.doc_start)[0] for p in pos})

    def batch(self, reads, min_len, max_walk):
        """-> mlen u32[n], occ u64[n], n_hit u32[n], mask u64[n, W], doc_reads u64[n_docs], doc_only u64[n_docs]"""
        n = len(reads)
        mlen = np.zeros(n, np.uint32)
        occ = np.zeros(n, np.uint64)
        n_hit = np.zeros(n, np.uint32)
        mask = np.zeros((n, self.words), np.uint64)
        doc_reads = np.zeros(self.n_docs, np.uint64)
        doc_only = np.zeros(self.n_docs, np.uint64)
        for k, rd in enumerate(reads):
            mlen[k], occ[k], ds = self.docs(bytes(rd), min_len, max_walk)
            n_hit[k] = len(ds)
            for d in ds:
                mask[k, d >> 6] |= np.uint64(1 << (d & 63))
                doc_reads[d] += np.uint64(1)
                if len(ds) == 1:
                    doc_only[d] += np.uint64(1)
        return mlen, occ, n_hit, mask, doc_reads, doc_only


def mask_docs(row):
    return [64 * w + b for w, x in enumerate(np.asarray(row, np.uint64).tolist()) for b in range(64) if (x >> b) & 1]


def docs_line(name, m, mlen, occ, docs):
    """One line of a .docs file, without the newline."""
    return f"{name}\t{m}\t{mlen}\t{occ}\t{len(docs)}\t{','.join(str(d) for d in docs)}"


def docs_file(names, reads, result):
    """The .docs bytes of a batch() result."""
    mlen, occ, _, mask, _, _ = result
    return "".join(docs_line(nm, len(rd), int(mlen[k]), int(occ[k]), mask_docs(mask[k])) + "\n"
                   for k, (nm, rd) in enumerate(zip(names, reads)))


def tally_file(doc_reads, doc_only):
    """The .tally bytes."""
    return "".join(f"{d}\t{int(a)}\t{int(b)}\n" for d, (a, b) in enumerate(zip(doc_reads, doc_only)))


def invented_cuts(n, n_docs, seed):
    """n_docs document starts over a text of n characters: 0 and n_docs-1 distinct cuts, some of them neighbours."""
    rng = np.random.default_rng(seed)
    assert n_docs <= n
    cuts = set([0])
    if n_docs > 2:
        cuts.update((1, 2))                      # documents of one character
    while len(cuts) < n_docs:
        cuts.add(int(rng.integers(1, n)))
    return sorted(cuts)
