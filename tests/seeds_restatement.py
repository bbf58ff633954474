"""Plain-Python restatement of the seeds reduction (include/colbwt.h colbwt_seeds_*): a per-read
loop over (pml, cid, read_off, min_len, max_seeds), written from the definitions and nothing else.
`seeds_vectorised` is a second, independent formulation (numpy over the diff of the zero mask) the
CPU tier holds the loop against; `format_lines` is the line format of colbwt_seeds_file."""
import numpy as np

FIELDS = ("n_seeds", "max_len", "cov", "resets", "n_col", "col_cov", "asc", "desc")
SEED_NONE = 0xFFFFFFFF
M32 = 0xFFFFFFFF


def seeds(pml, cid, read_off, min_len, max_seeds):
    """-> (summary (n_reads, 8) uint32 in FIELDS order, seed_pos, seed_len (n_reads, max_seeds) uint32,
    seed_cid (n_reads, max_seeds) uint8)."""
    n_reads = len(read_off) - 1
    summary = np.zeros((n_reads, 8), np.uint32)
    pos = np.full((n_reads, max_seeds), SEED_NONE, np.uint32)
    ln = np.zeros((n_reads, max_seeds), np.uint32)
    sc = np.zeros((n_reads, max_seeds), np.uint8)
    for r in range(n_reads):
        lo, hi = int(read_off[r]), int(read_off[r + 1])
        p = np.asarray(pml[lo:hi]).tolist()         # Python ints
        c = np.asarray(cid[lo:hi]).tolist()
        m = hi - lo
        found = []                                  # every seed of the read, smallest pos first
        k = 0
        while k < m:
            if p[k] == 0:
                k += 1
                continue
            e = k
            while e < m and p[e] >= 1:
                e += 1
            ident = next((c[j] for j in range(k, e) if c[j] != 0), 0)
            found.append((k, p[k], ident))
            k = e
        counting = [s for s in found if s[1] >= min_len]
        with_col = [s for s in counting if s[2] != 0]
        asc = desc = 0
        for (_, _, a), (_, _, b) in zip(with_col, with_col[1:]):
            d = (b - a + 255) % 255
            asc += 1 <= d <= 127
            desc += 128 <= d <= 254
        summary[r] = (len(counting), max(p, default=0), sum(s[1] for s in counting) & M32, sum(v == 0 for v in p),
                      len(with_col), sum(s[1] for s in with_col) & M32, asc, desc)
        for t, (k, length, ident) in enumerate(reversed(counting)):    # computation order: largest pos first
            if t == max_seeds:
                break
            pos[r, t], ln[r, t], sc[r, t] = k, length, ident
    return summary, pos, ln, sc


def seeds_vectorised(pml, cid, read_off, min_len, max_seeds):
    """The same results from whole-array operations: run starts and ends from the diff of the
    "pml >= 1" mask (read boundaries forced to 0), ids from a minimum over the positions of
    non-zero col ids, sums with reduceat-free bincounts."""
    pml = np.asarray(pml).astype(np.int64)
    cid = np.asarray(cid).astype(np.int64)
    off = np.asarray(read_off).astype(np.int64)
    n_reads, n = len(off) - 1, len(pml)
    lens = np.diff(off)
    read_of = np.repeat(np.arange(n_reads), lens)
    start = np.zeros(n, bool)
    start[off[:-1][lens > 0]] = True
    last = np.zeros(n, bool)
    last[off[1:][lens > 0] - 1] = True
    nz = pml >= 1
    prev_nz = np.concatenate(([False], nz[:-1])) & ~start
    next_nz = np.concatenate((nz[1:], [False])) & ~last
    k = np.flatnonzero(nz & ~prev_nz)                 # run starts
    e = np.flatnonzero(nz & ~next_nz) + 1             # run ends, same order
    # id: the first non-zero col id at or after k, when it lies before e
    has = np.flatnonzero((cid != 0) & nz)
    at = np.searchsorted(has, k)
    ident = np.zeros(len(k), np.int64)
    ok = at < len(has)
    cand = has[np.minimum(at, max(len(has) - 1, 0))] if len(has) else np.zeros(len(k), np.int64)
    ok &= cand < e if len(has) else False
    ident[ok] = cid[cand[ok]]
    length = pml[k]
    rd = read_of[k]
    counts = length >= min_len
    col = counts & (ident != 0)
    summary = np.zeros((n_reads, 8), np.uint32)
    summary[:, 0] = np.bincount(rd[counts], minlength=n_reads)
    mx = np.zeros(n_reads, np.int64)
    np.maximum.at(mx, read_of, pml)
    summary[:, 1] = mx
    cov = np.zeros(n_reads, np.int64)
    np.add.at(cov, rd[counts], length[counts])
    summary[:, 2] = cov & M32
    summary[:, 3] = np.bincount(read_of[~nz], minlength=n_reads)
    summary[:, 4] = np.bincount(rd[col], minlength=n_reads)
    ccov = np.zeros(n_reads, np.int64)
    np.add.at(ccov, rd[col], length[col])
    summary[:, 5] = ccov & M32
    ci, cr = ident[col], rd[col]
    same = cr[1:] == cr[:-1]
    d = (ci[1:] - ci[:-1] + 255) % 255
    summary[:, 6] = np.bincount(cr[1:][same & (d >= 1) & (d <= 127)], minlength=n_reads)
    summary[:, 7] = np.bincount(cr[1:][same & (d >= 128)], minlength=n_reads)
    pos = np.full((n_reads, max_seeds), SEED_NONE, np.uint32)
    ln = np.zeros((n_reads, max_seeds), np.uint32)
    sc = np.zeros((n_reads, max_seeds), np.uint8)
    ck, cl, cc, crd = k[counts], length[counts], ident[counts], rd[counts]
    n_of = np.bincount(crd, minlength=n_reads)
    first = np.concatenate(([0], np.cumsum(n_of)[:-1]))
    slot = n_of[crd] - 1 - (np.arange(len(ck)) - first[crd])      # rank from the read's end
    keep = slot < max_seeds
    pos[crd[keep], slot[keep]] = ck[keep] - off[crd[keep]]
    ln[crd[keep], slot[keep]] = cl[keep]
    sc[crd[keep], slot[keep]] = cc[keep]
    return summary, pos, ln, sc


def check_invariants(summary, pos, ln, read_off, min_len, max_seeds):
    """The three invariants include/colbwt.h states for a true query output."""
    m = np.diff(np.asarray(read_off).astype(np.int64))
    s = summary.astype(np.int64)
    assert np.all(s[:, 0] <= s[:, 3] + 1), "n_seeds <= resets + 1"
    if min_len == 1:
        assert np.array_equal(s[:, 2] + s[:, 3], m), "cov + resets == m"
        full = s[:, 0] <= max_seeds
        assert np.array_equal(ln.max(axis=1, initial=0).astype(np.int64)[full], s[full, 1]), "max_len == largest stored len"


def format_lines(names, read_off, summary, pos, ln, sc, max_seeds):
    out = []
    for r, name in enumerate(names):
        q = [int(v) for v in summary[r]]
        k = min(q[0], max_seeds)
        seeds_txt = ",".join(f"{int(pos[r, t])}:{int(ln[r, t])}:{int(sc[r, t])}" for t in range(k))
        m = int(read_off[r + 1]) - int(read_off[r])
        out.append(f"{name}\t{m}\t{q[0]}\t{q[2]}\t{q[1]}\t{q[3]}\t{q[4]}\t{q[5]}\t{q[6]}\t{q[7]}\t{seeds_txt}\n")
    return "".join(out).encode()
