"""What the output collector of the line-fetching kernels (csrc/lane_out.h, OutRuns) has to write, restated from the
wide branch of csrc/fat2_query.hip ("report the run") and from nothing else: no masks, no blocks, no flush schedule.

A lane reports its chunk -- `length` elements from element address `addr` on -- from the top down, one push per trip.
A push (n, l_new, keep, keep1, ids, ids2) made when `rem` elements of the chunk are still to come covers the addresses
addr + rem - n .. addr + rem - 1, i.e. element e of the push goes to  g - n + 1 + e  with  g = addr + rem - 1:

    PML value   (keep if e < 2 else keep1 if e < 4 else True) ? l_new - e : 0
    col id      byte e of  ids | ids2 << 64

The collector supports only the pushes the kernels make, and the cases (tests/out_runs_cases.py) generate only these.
L is the value of the lane's current element 0 (the element reported last); it is 0 at the start of a chunk and of a
read:

    continuation             n in 0..8, with push_run<true> also 15 and 16;  l_new = L + n, both keeps set
    absent character         n in 1..8;  l_new = n - 1 (the oldest element is 0)
    scan or one-base entry   n = 1, l_new = 0
    entry, two bases         n = 2, l_new = 1, keep all-ones (1, 0) or 0 (0, 0)
    deep entry, three bases  n = 3, l_new = 2 (2, 1, 0)  or  l_new = 1 with keep1 = 0 (1, 0, 0)
    new read inside a chunk  L = 0 before the read's first push

The bytes of ids / ids2 from byte n on are arbitrary (the collector masks them).  A 15- or 16-element push is made only
in a trip with  cnt + 16 + 8 (3 - (trip & 3)) <= 96,  cnt the collector's count before the push.  The wave flushes every
fourth trip with gl = addr + rem, final = (rem == 0); a lane enters its next chunk only in a trip that finds cnt == 0.
"""
import numpy as np

PML_FILL = 0xA5A5          # what the probe pre-fills the two arrays with
CID_FILL = 0xA5


def element(push, e):
    """-> (PML value, col id) of element e of a push."""
    n, l_new, keep, keep1, ids, ids2 = push
    assert 0 <= e < n
    kept = keep if e < 2 else keep1 if e < 4 else True
    value = l_new - e if kept else 0
    assert 0 <= value <= 0xFFFF, push
    return value, ((ids | (ids2 << 64)) >> (8 * e)) & 0xFF


def apply(n_out, chunks, bias=0):
    """chunks: (addr, length, pushes) of every chunk of every lane, addresses raised by `bias` -> the two arrays of
    n_out elements: the fill pattern, and under every chunk what its pushes say."""
    pml = np.full(n_out, PML_FILL, np.uint16)
    cid = np.full(n_out, CID_FILL, np.uint8)
    written = np.zeros(n_out, bool)
    for addr, length, pushes in chunks:
        rem = length
        for push in pushes:
            n = push[0]
            assert n <= rem
            for e in range(n):
                at = addr - bias + rem - n + e
                assert not written[at], "two chunks overlap"
                written[at] = True
                pml[at], cid[at] = element(push, e)
            rem -= n
        assert rem == 0, "a chunk is reported completely"
    return pml, cid
