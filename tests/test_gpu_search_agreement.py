"""One backward search behind count, locate, locate-all, docs and anchors (csrc/count_query.h search_step and
longest_suffix): on the MI355X the five modes give the same longest matching suffix for the same reads, on
every layout, in read order (the device entry points without d_order) and through the ragged-batch path (the
host entry points, which order the lanes by read length), and that answer is the restatements'.

Anchors restart where locate stops, so slot 0 of a read is its longest matching suffix exactly when that factor
ends at the read's end; a read whose last base matches nothing has mlen 0 in the other modes and an earlier
factor, or none, in slot 0.  Count walks through bytes <= 1, where the others stop: it is compared with them
on the reads without such a byte and with its own restatement on all reads."""
import numpy as np
import pytest

import anchors_restatement as ar
import count_restatement as cr
import docs_restatement as dr
import helpers
import locate_all_restatement as lar
import locate_restatement as lr
import test_gpu_anchors as tga

LAYOUTS = (1, 2, 3, 4, 5, 6, 0)
INDEX_SEED, READ_SEED = 2, 10
N_PLANTED = 249          # + 11 edge reads = 260: a second block of 256 lanes whose one wave holds 4 reads
MAX_WALK = 256

pytestmark = pytest.mark.gpu


def _reads(text, seed):
    body = text[:-1]
    reads = [r for r, _ in ar.planted_reads(text, N_PLANTED, seed=seed)]
    reads += [body[300:300 + m] for m in (0, 1, 63, 64, 65, 128, 129)]      # either side of the 64-byte window refill
    reads += [body, b"N", body[7:40] + b"\x01" + body[40:75], body[30:60] + b"\x00"]
    return reads


def _want(img, text, reads):
    """The restatements' answers, in the shape _batch_answers and _device_answers return."""
    loc = lr.Locator(text)
    table = cr.Table(img)
    n = len(reads)
    located = [loc.locate(r, 1) for r in reads]
    pos = np.full((n, 1), lr.NONE, np.uint64)
    for k, (_, _, p) in enumerate(located):
        pos[k, :len(p)] = p
    counted = [table.count(r) for r in reads]
    return {
        "count": (np.array([c[0] for c in counted], np.uint32), np.array([c[1] for c in counted], np.uint64)),
        "locate": (np.array([x[0] for x in located], np.uint32), np.array([x[1] for x in located], np.uint64), pos),
        "all": lar.LocateAll(text, locator=loc).batch(reads, 1, 0),
        "docs": dr.Docs(text, (0,), locator=loc).batch(reads, 1, MAX_WALK)[:4],
        "anchors": ar.Anchors(text, locator=loc).batch(reads, 1, 1, 1)[1:],
    }


def _batch_answers(tbl, bases, off):
    return {
        "count": tbl.count_batch(bases, off)[:2],
        "locate": tbl.locate_batch(bases, off, 1)[:3],
        "all": tbl.locate_all_batch(bases, off, 1, 0)[:4],
        "docs": tbl.docs_batch(bases, off, 1, MAX_WALK, want_tally=False)[:4],
        "anchors": tbl.anchors_batch(bases, off, 1, 1, 1)[1:5],
    }


def _device_answers(pkg, torch, tbl, bases, off):
    dev = torch.device("cuda", 0)
    n, nb, words = len(off) - 1, len(bases), tbl.docs_mask_words()
    d_bases = torch.zeros(nb + 128, dtype=torch.uint8, device=dev)
    d_bases[:nb] = torch.from_numpy(bases)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)

    def i32(count):
        return torch.full((count,), 0x5A5A5A5A, dtype=torch.int32, device=dev)

    def i64(count):
        return torch.full((count,), 0x5A5A5A5A5A5A, dtype=torch.int64, device=dev)

    def u32(t):
        return t.cpu().numpy().view(np.uint32)

    def u64(t):
        return t.cpu().numpy().view(np.uint64)

    head = (d_bases.data_ptr(), d_off.data_ptr(), n, nb)
    out = {}
    m, o = i32(n), i64(n)
    tbl.count_device(*head, m.data_ptr(), o.data_ptr(), timed=True)
    out["count"] = (u32(m), u64(o))
    m, o, p = i32(n), i64(n), i64(n)
    tbl.locate_device(*head, 1, m.data_ptr(), o.data_ptr(), p.data_ptr(), timed=True)
    out["locate"] = (u32(m), u64(o), u64(p).reshape(n, 1))
    m, o, po = i32(n), i64(n), i64(n + 1)
    work = torch.zeros(pkg.locate_all_work_bytes(n), dtype=torch.uint8, device=dev)
    total, _ = tbl.locate_all_plan_device(*head, 1, 0, m.data_ptr(), o.data_ptr(), po.data_ptr(), work.data_ptr())
    p = i64(total)
    tbl.locate_all_fill_device(n, 0, n, po.data_ptr(), p.data_ptr(), total, work.data_ptr(), timed=True)
    out["all"] = (u32(m), u64(o), u64(po), u64(p))
    m, o, hit, mask = i32(n), i64(n), i32(n), i64(n * words)
    work = torch.zeros(pkg.docs_work_bytes(n), dtype=torch.uint8, device=dev)
    tbl.docs_device(*head, 1, MAX_WALK, m.data_ptr(), o.data_ptr(), hit.data_ptr(), mask.data_ptr(), work.data_ptr(), timed=True)
    out["docs"] = (u32(m), u64(o), u32(hit), u64(mask).reshape(n, words))
    summary, s, ln, o, p = i32(8 * n), i32(n), i32(n), i64(n), i64(n)
    tbl.anchors_device(*head, 1, 1, 1, summary.data_ptr(), s.data_ptr(), ln.data_ptr(), o.data_ptr(), p.data_ptr(), timed=True)
    out["anchors"] = (u32(s).reshape(n, 1), u32(ln).reshape(n, 1), u64(o).reshape(n, 1), u64(p).reshape(n, 1, 1))
    return out


def _check(label, got, want, lens, low):
    mlen, occ, pos0 = got["locate"][0], got["locate"][1], got["locate"][2][:, 0]
    for mode in ("all", "docs"):
        assert np.array_equal(got[mode][0], mlen) and np.array_equal(got[mode][1], occ), (label, mode)
    start, ln, a_occ, a_pos = (a[:, 0] for a in got["anchors"])
    ends = (start != ar.ANCHOR_NONE) & (start.astype(np.int64) + ln == lens)       # slot 0 is the read's suffix
    assert np.array_equal(np.where(ends, ln, 0), mlen) and np.array_equal(np.where(ends, a_occ, 0), occ), (label, "anchors")
    has = mlen > 0
    assert np.array_equal(pos0[has], a_pos[has, 0]) and (pos0[~has] == lr.NONE).all(), (label, "pos[0]")
    pos_off, pos = got["all"][2], got["all"][3]
    assert np.array_equal(np.diff(pos_off), occ), (label, "widths")
    for k in np.flatnonzero(has):
        assert pos0[k] in pos[int(pos_off[k]):int(pos_off[k + 1])], (label, "pos[0] among all", k)
    assert np.array_equal(got["count"][0][~low], mlen[~low]) and np.array_equal(got["count"][1][~low], occ[~low]), (label, "count")
    for mode, arrays in want.items():                      # agreement cannot hide a shared error
        for j, (g, w) in enumerate(zip(got[mode], arrays)):
            assert np.array_equal(g.reshape(w.shape), w), (label, mode, j)


def test_every_mode_finds_the_same_longest_suffix(pkg):
    import torch
    img, text = tga._true_index(INDEX_SEED)
    reads = _reads(text, READ_SEED)
    arrs = [np.frombuffer(r, np.uint8) for r in reads]
    bases, off = helpers.concat_reads(arrs)
    lens = np.diff(off.astype(np.int64))
    low = np.array([bool((a <= 1).any()) for a in arrs])
    want = _want(img, text, reads)
    # what the reads must exercise, by the restatement
    mlen, occ = want["locate"][:2]
    assert len(reads) > 256 and len(reads) % 64 != 0
    assert 2 * int((mlen >= 16).sum()) >= len(reads) and (occ > 4).any()
    assert any(0 < mlen[k] < lens[k] and arrs[k][lens[k] - 1 - int(mlen[k])] <= 1 for k in np.flatnonzero(low))   # stops on a byte <= 1
    samples = lr.samples(text)
    for layout in LAYOUTS:
        tbl = pkg.ColPml.from_bytes(img, layout=layout)
        tbl.attach_locate(data=samples)
        _check(f"L{layout}/read order", _device_answers(pkg, torch, tbl, bases, off), want, lens, low)
        _check(f"L{layout}/ragged batch", _batch_answers(tbl, bases, off), want, lens, low)
        tbl.close()
