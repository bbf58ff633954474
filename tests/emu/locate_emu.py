#!/usr/bin/env python3
"""CPU-tier check of locate (csrc/locate_query.h, the attach in capi.hip, the builder's samples in
rlbwt_build.hip) compiled against the SIMT emulator, against tests/locate_restatement.py.  Run by
tests/test_locate_cpu.py in a subprocess with libasan preloaded.  Prints LOCATE-EMU-OK at the end."""
import os
import struct
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

from __graft_entry__ import load_package  # noqa: E402
import helpers  # noqa: E402
import locate_restatement as lr  # noqa: E402
import rlbwt_oracle  # noqa: E402

pkg = load_package()
pkg.LIB_PATH = os.path.join(HERE, "libcolbwt_emu.so")   # emulated build instead of the HIP one

LINE_ROWS_4 = 4 | (4 << 8)          # include/colbwt.h COLBWT_LAYOUT_LINE_ROWS_STEPS(4)
LAYOUTS = (1, 2, 3, LINE_ROWS_4)


def texts():
    rng = np.random.default_rng(21)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    a = rng.choice(acgt, size=400).tobytes()
    yield "acgt+repeats", [a, a[100:250], rng.choice(acgt, size=200).tobytes(), b"ACGTACGTACGT" * 5], b"ACGT"
    yield "sigma2", [rng.choice(np.frombuffer(b"ab", np.uint8), size=300).tobytes()], b"ab"
    yield "homopolymer", [b"A" * 120, b"C" * 3, b"A" * 40], b"AC"
    prot = b"ACDEFGHIKLMNPQRSTVWY"
    yield "protein", [rng.choice(np.frombuffer(prot, np.uint8), size=300).tobytes()], prot


def check(image, text, reads, label, layouts=LAYOUTS, max_occs=(1, 3, 1000)):
    loc = lr.samples(text)
    ref = lr.Locator(text)
    bases, off = helpers.concat_reads(reads)
    for layout in layouts:
        tbl = pkg.ColPml.from_bytes(bytes(image), layout=layout)
        tbl.attach_locate(data=loc)
        cm, co, _, _ = tbl.count_batch(bases, off)
        for k in max_occs:
            want = [ref.locate(r, k) for r in reads]
            mlen, occ, pos, st = tbl.locate_batch(bases, off, k)
            assert st.n_reads == len(reads)
            for i, (wm, wo, wp) in enumerate(want):
                got = (int(mlen[i]), int(occ[i]), [int(x) for x in pos[i, :min(int(occ[i]), k)]])
                assert got == (wm, wo, wp), f"{label}/L{layout}/k{k}: read {i} {bytes(reads[i])[:40]!r}: {got} != {(wm, wo, wp)}"
                assert (pos[i, len(wp):] == pkg.LOCATE_NONE).all(), f"{label}/L{layout}/k{k}: read {i}: slots past k"
            clean = np.array([np.all(np.asarray(r) > 1) for r in reads])
            assert np.array_equal(mlen[clean], cm[clean]) and np.array_equal(occ[clean], co[clean]), f"{label}/L{layout}: != count"
        tbl.close()
    print(f"ok {label}: {len(reads)} reads, layouts {layouts}, max_occ {max_occs}")


def read_set(text, alpha, seed):
    reads = [np.frombuffer(bytes(r), np.uint8) for r in helpers.reads_from_text(text, 40, (1, 60), 0.02, seed=seed, alphabet=alpha,
                                                                                 extra=b"N")]
    body = text[:-1]
    reads += [np.frombuffer(body, np.uint8),                              # the whole text
              np.zeros(0, np.uint8),                                      # empty
              np.frombuffer(b"N" + body[:6], np.uint8),
              np.frombuffer(body[:5] + b"\x01" + body[5:12], np.uint8),   # a separator byte ends the search
              np.frombuffer(body[3:9] + b"\x00", np.uint8),               # ... also as the last byte
              np.frombuffer(body[-8:], np.uint8)]
    return reads


def check_rejects(image, text):
    """Attach refuses a .col_loc with a wrong n, a wrong r or unsorted phi positions; the index still counts."""
    good = lr.samples(text)
    n, r, s = struct.unpack_from("<QQQ", good, 16)
    bad_n = good[:16] + struct.pack("<Q", n + 1) + good[24:]
    bad_r = bytearray(good[:24] + struct.pack("<Q", r - 1) + good[32:40] + good[40 + 4:])   # one end_sa fewer: length still fits
    phi = 40 + 4 * r
    unsorted = bytearray(good)
    a, b = phi + 8, phi + 16                                                # swap samples 1 and 2
    unsorted[a:a + 8], unsorted[b:b + 8] = good[b:b + 8], good[a:a + 8]
    tbl = pkg.ColPml.from_bytes(bytes(image), layout=2)
    for name, data, code in (("n", bad_n, -3), ("r", bytes(bad_r), -3), ("phi order", bytes(unsorted), -3)):
        try:
            tbl.attach_locate(data=data)
        except pkg.ColbwtError as e:
            assert e.code == code, (name, e)
        else:
            raise AssertionError(f"attach accepted a .col_loc with a bad {name}")
        try:
            tbl.locate(b"ACG")
        except pkg.ColbwtError as e:
            assert e.code == -1, e
        else:
            raise AssertionError("locate ran without samples")
    assert tbl.count(text[:10])[0] == 10            # still usable
    tbl.attach_locate(data=good)
    assert tbl.locate(text[:10])[:2] == (10, 1)
    tbl.close()
    print("ok attach rejects a wrong n, a wrong r, unsorted phi positions")


def check_builder():
    """The emulated builder's samples == the Python writer's bytes (multi-document text, reverse complements)."""
    rng = np.random.default_rng(4)
    base = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=150)
    docs = []
    for d in range(3):
        recs = []
        for _ in range(2):
            s = base.copy()
            mut = rng.random(s.size) < 0.05
            s[mut] = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(mut.sum()))
            recs.append(s[: 90 + 20 * d].tobytes())
        docs.append(recs)
    text, starts = rlbwt_oracle.build_text(docs, revcomp=True)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "t.col_loc")
        pkg.rlbwt_from_text(text, starts, min_mum=10, locate_path=path)
        got = open(path, "rb").read()
    want = lr.samples(text, doc_start=starts)
    assert got == want, f"builder samples differ: {len(got)} vs {len(want)} bytes"
    print(f"ok builder samples: n = {len(text)}, {len(docs)} documents, {len(got)} bytes")


def main():
    for label, seqs, alpha in texts():
        img, text = helpers.true_bwt_index(seqs, seed=len(label))
        check(img, text, read_set(text, alpha, 5), label)
    img, text = helpers.true_bwt_index(next(texts())[1], seed=3)
    check_rejects(img, text)
    check_builder()
    print("LOCATE-EMU-OK")


if __name__ == "__main__":
    main()
