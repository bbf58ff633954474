"""colbwt_amd -- host-side Python mirror of the reference's query interface
(`col_pml`, include/col_bwt.hpp:386-575; `pml_query`, src/pml_query.cpp) over
the MI355X-native C-ABI library `libcolbwt.so` (include/colbwt.h).

This module is plumbing: ctypes over the C-ABI.  All computation happens in
the hand-written HIP kernels of `csrc/`.  There is no CPU fallback: if the
library is missing or no HIP device is usable, calls raise `ColbwtError`.

The directory is named `col-bwt_amd` (not importable by that name); load it
with `__graft_entry__.load_package()` which registers it as `colbwt_amd`.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcolbwt.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "colbwt.h")

# every symbol include/colbwt.h declares (checked by tests/test_capi_symbols.py)
EXPORTS = (
    "colbwt_version", "colbwt_last_error", "colbwt_index_open", "colbwt_index_open_memory",
    "colbwt_index_open_layout", "colbwt_index_open_memory_layout",
    "colbwt_index_open_devices", "colbwt_index_open_memory_devices",
    "colbwt_index_close", "colbwt_index_info", "colbwt_query_batch", "colbwt_query_batch_u32",
    "colbwt_query_device", "colbwt_query_device_ordered", "colbwt_query_file", "colbwt_query_file_binary",
    "colbwt_binary_to_text", "colbwt_synth_index_bytes", "colbwt_synth_index", "colbwt_synth_index_thr", "colbwt_pml_pack_device", "colbwt_read_end_mask_device", "colbwt_pml_unpack_device",
    "colbwt_index_cid_dictionary", "colbwt_cid_code_bits", "colbwt_cid_pack_device", "colbwt_cid_unpack_device",
    "colbwt_synth_reads_device", "colbwt_build_col_pml", "colbwt_build_col_pml_arrays",
    "colbwt_col_split", "colbwt_col_split_arrays", "colbwt_col_split_error",
    "colbwt_rlbwt_build_text", "colbwt_rlbwt_build_files", "colbwt_rlbwt_get", "colbwt_rlbwt_free", "colbwt_rlbwt_error",
    "colbwt_count_batch", "colbwt_count_device", "colbwt_count_file",
    "colbwt_index_attach_locate", "colbwt_index_attach_locate_memory", "colbwt_locate_docs", "colbwt_locate_batch",
    "colbwt_locate_device", "colbwt_locate_file",
    "colbwt_rlbwt_build_text_locate", "colbwt_rlbwt_build_files_locate", "colbwt_rlbwt_write_locate",
    "colbwt_seeds_reduce_device", "colbwt_seeds_batch", "colbwt_seeds_file",
    "colbwt_docs_mask_words", "colbwt_docs_work_bytes", "colbwt_docs_batch", "colbwt_docs_device", "colbwt_docs_file",
    "colbwt_locate_all_tile", "colbwt_locate_all_work_bytes", "colbwt_locate_all_plan_device", "colbwt_locate_all_fill_device",
    "colbwt_locate_all_batch", "colbwt_locate_all_file",
    "colbwt_anchors_device", "colbwt_anchors_batch", "colbwt_anchors_file",
    "colbwt_chain_work_bytes", "colbwt_chain_reduce_device", "colbwt_chain_device", "colbwt_chain_batch", "colbwt_chain_file",
)

SEED_NONE = 0xFFFFFFFF          # include/colbwt.h COLBWT_SEED_NONE: seed_pos of a slot past the read's min(n_seeds, max_seeds)
# colbwt_seed_summary as a numpy record: one per read
SEED_SUMMARY = np.dtype([(k, np.uint32) for k in ("n_seeds", "max_len", "cov", "resets", "n_col", "col_cov", "asc", "desc")])
LOCATE_NONE = (1 << 64) - 1     # include/colbwt.h COLBWT_LOCATE_NONE: a position slot past the read's min(occ, max_occ)
ANCHOR_NONE = 0xFFFFFFFF        # include/colbwt.h COLBWT_ANCHOR_NONE: anchor_start of a slot past the read's n_stored
# colbwt_anchor_summary as a numpy record: one per read
AnchorSummary = np.dtype([(k, np.uint32) for k in ("n_factors", "max_len", "skipped", "n_kept", "cov", "n_unique", "cov_unique",
                                                   "n_stored")])
# colbwt_chain as a numpy record: one per read, 32 bytes; text_begin is LOCATE_NONE (and the rest 0) for a read without hits
CHAIN = np.dtype([("text_begin", np.uint64), ("text_len", np.uint32), ("read_begin", np.uint32), ("read_end", np.uint32),
                  ("score", np.uint32), ("score2", np.uint32), ("n_chained", np.uint16), ("n_hits", np.uint16)])


class ColbwtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"colbwt error {code}: {msg}")
        self.code = code


class Info(C.Structure):
    _fields_ = [("bwt_r", C.c_uint64), ("n", C.c_uint64), ("r", C.c_uint64), ("sigma", C.c_uint32),
                ("device", C.c_uint32), ("device_bytes", C.c_uint64), ("layout", C.c_uint32),
                ("layout_shape", C.c_uint32), ("table_rows", C.c_uint64), ("n_devices", C.c_uint32),
                ("tail_permille", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_bases", C.c_uint64), ("h2d_ms", C.c_double),
                ("kernel_ms", C.c_double), ("d2h_ms", C.c_double), ("algorithmic_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib = None


def lib():
    """Loads libcolbwt.so; raises loudly when the HIP extension is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ColbwtError(-100, f"{LIB_PATH} not built: run __graft_entry__.build() "
                                "(the query path has no CPU fallback)")
    # One HIP runtime per process: PyTorch bundles its own libamdhip64 (same
    # soname as /opt/rocm's).  Importing torch first makes libcolbwt.so bind to
    # that copy; loading ours first would leave torch with a second runtime
    # that sees no GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
    L.colbwt_version.restype = C.c_char_p
    L.colbwt_last_error.restype = C.c_char_p
    L.colbwt_index_open.argtypes = [C.c_char_p, vp, i32, C.POINTER(vp)]
    L.colbwt_index_open_memory.argtypes = [vp, u64, vp, i32, C.POINTER(vp)]
    L.colbwt_index_open_layout.argtypes = [C.c_char_p, vp, i32, i32, C.POINTER(vp)]
    L.colbwt_index_open_memory_layout.argtypes = [vp, u64, vp, i32, i32, C.POINTER(vp)]
    L.colbwt_index_open_devices.argtypes = [C.c_char_p, vp, C.POINTER(i32), i32, i32, C.POINTER(vp)]
    L.colbwt_index_open_memory_devices.argtypes = [vp, u64, vp, C.POINTER(i32), i32, i32, C.POINTER(vp)]
    L.colbwt_index_close.argtypes = [vp]
    L.colbwt_index_close.restype = None
    L.colbwt_index_info.argtypes = [vp, C.POINTER(Info)]
    L.colbwt_query_batch.argtypes = [vp, vp, vp, u64, vp, vp, C.POINTER(Stats)]
    L.colbwt_query_batch_u32.argtypes = [vp, vp, vp, u64, vp, vp, C.POINTER(Stats)]
    L.colbwt_query_device.argtypes = [vp, vp, vp, u64, u64, vp, i32, vp, vp, C.POINTER(Stats)]
    L.colbwt_query_device_ordered.argtypes = [vp, vp, vp, u64, u64, vp, i32, vp, vp, vp, C.POINTER(Stats)]
    L.colbwt_query_file.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, u64, C.POINTER(Stats)]
    L.colbwt_query_file_binary.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, u64, C.POINTER(Stats)]
    L.colbwt_binary_to_text.argtypes = [C.c_char_p, i32, C.c_char_p]
    L.colbwt_synth_index_bytes.argtypes = [u64]
    L.colbwt_synth_index_bytes.restype = u64
    L.colbwt_synth_index.argtypes = [u64, C.c_uint32, C.c_uint32, u64, vp, u64]
    L.colbwt_synth_index_thr.argtypes = [u64, C.c_uint32, C.c_uint32, u64, C.c_int, vp, u64]
    L.colbwt_pml_pack_device.argtypes = [vp, u64, vp, vp]
    L.colbwt_read_end_mask_device.argtypes = [vp, u64, vp, vp]
    L.colbwt_pml_unpack_device.argtypes = [vp, vp, u64, u64, u64, vp, vp]
    L.colbwt_index_cid_dictionary.argtypes = [vp, vp, C.POINTER(C.c_uint32)]
    L.colbwt_cid_code_bits.argtypes = [C.c_uint32]
    L.colbwt_cid_code_bits.restype = C.c_uint32
    L.colbwt_cid_pack_device.argtypes = [vp, u64, vp, C.c_uint32, vp, vp]
    L.colbwt_cid_unpack_device.argtypes = [vp, u64, u64, vp, C.c_uint32, vp, vp]
    L.colbwt_synth_reads_device.argtypes = [vp, u64, C.c_uint32, C.c_uint32, u64, vp, vp, vp]
    L.colbwt_build_col_pml.argtypes = [C.c_char_p, C.c_char_p]
    L.colbwt_build_col_pml_arrays.argtypes = [vp, u64, vp, vp, u64, vp, u64, vp, u64, vp, u64, C.POINTER(u64)]
    L.colbwt_count_batch.argtypes = [vp, vp, vp, u64, vp, vp, vp, C.POINTER(Stats)]
    L.colbwt_count_device.argtypes = [vp, vp, vp, u64, u64, vp, vp, vp, vp, vp, C.POINTER(Stats)]
    L.colbwt_count_file.argtypes = [vp, C.c_char_p, C.c_char_p, u64, C.POINTER(Stats)]
    u32 = C.c_uint32
    L.colbwt_index_attach_locate.argtypes = [vp, C.c_char_p]
    L.colbwt_index_attach_locate_memory.argtypes = [vp, vp, u64]
    L.colbwt_locate_docs.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.colbwt_locate_batch.argtypes = [vp, vp, vp, u64, u32, vp, vp, vp, C.POINTER(Stats)]
    L.colbwt_locate_device.argtypes = [vp, vp, vp, u64, u64, u32, vp, vp, vp, vp, vp, C.POINTER(Stats)]
    L.colbwt_locate_file.argtypes = [vp, C.c_char_p, C.c_char_p, u32, u64, C.POINTER(Stats)]
    L.colbwt_rlbwt_build_text_locate.argtypes = [vp, u64, vp, u32, u64, C.c_int, C.POINTER(vp)]
    L.colbwt_rlbwt_build_files_locate.argtypes = [C.POINTER(C.c_char_p), u32, C.c_int, u64, C.c_int, C.c_char_p, C.POINTER(vp)]
    L.colbwt_rlbwt_write_locate.argtypes = [vp, C.c_char_p]
    L.colbwt_seeds_reduce_device.argtypes = [vp, i32, vp, vp, u64, u64, u32, u32, vp, vp, vp, vp, vp, C.POINTER(Stats)]
    L.colbwt_seeds_batch.argtypes = [vp, vp, vp, u64, u32, u32, vp, vp, vp, vp, C.POINTER(Stats)]
    L.colbwt_seeds_file.argtypes = [vp, C.c_char_p, C.c_char_p, u32, u32, u64, C.POINTER(Stats)]
    L.colbwt_docs_mask_words.argtypes = [vp]
    L.colbwt_docs_mask_words.restype = u32
    L.colbwt_docs_work_bytes.argtypes = [u64]
    L.colbwt_docs_work_bytes.restype = u64
    L.colbwt_docs_batch.argtypes = [vp, vp, vp, u64, u32, u32, vp, vp, vp, vp, vp, vp, C.POINTER(Stats)]
    L.colbwt_docs_device.argtypes = [vp, vp, vp, u64, u64, u32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(Stats)]
    L.colbwt_docs_file.argtypes = [vp, C.c_char_p, C.c_char_p, u32, u32, u64, C.POINTER(Stats)]
    L.colbwt_locate_all_tile.argtypes = []
    L.colbwt_locate_all_tile.restype = u32
    L.colbwt_locate_all_work_bytes.argtypes = [u64]
    L.colbwt_locate_all_work_bytes.restype = u64
    L.colbwt_locate_all_plan_device.argtypes = [vp, vp, vp, u64, u64, u32, u64, vp, vp, vp, vp, vp, vp, C.POINTER(u64), C.POINTER(Stats)]
    L.colbwt_locate_all_fill_device.argtypes = [vp, u64, u64, u64, vp, vp, u64, vp, vp, C.POINTER(Stats)]
    L.colbwt_locate_all_batch.argtypes = [vp, vp, vp, u64, u32, u64, vp, vp, vp, vp, u64, C.POINTER(Stats)]
    L.colbwt_locate_all_file.argtypes = [vp, C.c_char_p, C.c_char_p, u32, u64, u64, C.POINTER(Stats)]
    L.colbwt_anchors_device.argtypes = [vp, vp, vp, u64, u64, u32, u32, u32, vp, vp, vp, vp, vp, vp, vp, C.POINTER(Stats)]
    L.colbwt_anchors_batch.argtypes = [vp, vp, vp, u64, u32, u32, u32, vp, vp, vp, vp, vp, C.POINTER(Stats)]
    L.colbwt_anchors_file.argtypes = [vp, C.c_char_p, C.c_char_p, u32, u32, u32, u64, C.POINTER(Stats)]
    L.colbwt_chain_work_bytes.argtypes = [u64, u32, u32]
    L.colbwt_chain_work_bytes.restype = u64
    L.colbwt_chain_reduce_device.argtypes = [vp, vp, vp, vp, u64, u32, u32, u32, vp, vp, C.POINTER(Stats)]
    L.colbwt_chain_device.argtypes = [vp, vp, vp, u64, u64, u32, u32, u32, u32, vp, vp, vp, vp, C.POINTER(Stats)]
    L.colbwt_chain_batch.argtypes = [vp, vp, vp, u64, u32, u32, u32, u32, vp, C.POINTER(Stats)]
    L.colbwt_chain_file.argtypes = [vp, C.c_char_p, C.c_char_p, u32, u32, u32, u32, u64, C.POINTER(Stats)]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise ColbwtError(rc, lib().colbwt_last_error().decode("utf-8", "replace"))


def __getattr__(name):
    if name == "LOCATE_ALL_TILE":   # colbwt_locate_all_tile: positions per tile of a locate-all walk, as the library was built
        return int(lib().colbwt_locate_all_tile())
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def version():
    return lib().colbwt_version().decode()


class ColPml:
    """The reference's `col_pml` (col_bwt.hpp:386): load an index, query reads.

    `ColPml.load(prefix)` <-> `col_pml tbl; tbl.load(ifstream(prefix + ".col_pml"))`
    (pml_query.cpp:109-112); `query_pml(pattern)` <-> col_bwt.hpp:403-412.
    """

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def load(cls, prefix_or_file, device=0, layout=0, devices=None):
        """layout: 0 = engine default, 1 = one-step rows, 2 / 3 = K-step rows, 4 = line rows, 5 = line rows with
        mismatch lines (same results)."""
        h = C.c_void_p()
        if devices is not None:
            dv = (C.c_int * len(devices))(*[int(d) for d in devices])
            _check(lib().colbwt_index_open_devices(os.fsencode(prefix_or_file), None, dv, len(devices), int(layout),
                                                   C.byref(h)))
        else:
            _check(lib().colbwt_index_open_layout(os.fsencode(prefix_or_file), None, int(device), int(layout),
                                                  C.byref(h)))
        return cls(h)

    @classmethod
    def from_bytes(cls, image, device=0, layout=0, devices=None):
        """devices: a list of device ordinals (one replica each; a device may repeat) instead of `device`."""
        arr = np.ascontiguousarray(np.frombuffer(image, dtype=np.uint8))
        h = C.c_void_p()
        if devices is not None:
            dv = (C.c_int * len(devices))(*[int(d) for d in devices])
            _check(lib().colbwt_index_open_memory_devices(arr.ctypes.data, arr.size, None, dv, len(devices), int(layout),
                                                          C.byref(h)))
        else:
            _check(lib().colbwt_index_open_memory_layout(arr.ctypes.data, arr.size, None, int(device), int(layout),
                                                         C.byref(h)))
        return cls(h)

    def info(self):
        out = Info()
        _check(lib().colbwt_index_info(self._h, C.byref(out)))
        return out

    # -- col_pml::query_pml(const char*, size_t), col_bwt.hpp:409-412 ---------
    def query_pml(self, pattern):
        """One read -> (pml, cid) uint64 arrays, index k <-> pattern[k]."""
        p = np.frombuffer(bytes(pattern), dtype=np.uint8)
        off = np.array([0, p.size], dtype=np.uint64)
        pml, cid, _ = self.query_batch(p, off, wide=p.size > 65535)
        return pml.astype(np.uint64), cid.astype(np.uint64)

    def query_batch(self, bases, read_off, wide=False):
        """Many reads at once (host buffers in, host buffers out)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        n_reads = read_off.size - 1
        total = int(read_off[-1]) if n_reads >= 0 and read_off.size else 0
        pml = np.zeros(total, np.uint32 if wide else np.uint16)
        cid = np.zeros(total, np.uint8)
        st = Stats()
        fn = lib().colbwt_query_batch_u32 if wide else lib().colbwt_query_batch
        _check(fn(self._h, bases.ctypes.data, read_off.ctypes.data, max(n_reads, 0),
                  pml.ctypes.data, cid.ctypes.data, C.byref(st)))
        return pml, cid, st

    def query_device(self, d_bases, d_read_off, n_reads, n_bases, d_pml, d_cid, pml_bytes=2,
                     stream=0, timed=False, d_order=None):
        """Device-resident entry point: arguments are raw device pointers (ints).
        d_order: optional device array of read indices by decreasing length."""
        st = Stats()
        _check(lib().colbwt_query_device_ordered(self._h, d_bases, d_read_off, n_reads, n_bases, d_pml,
                                                 pml_bytes, d_cid, d_order, stream,
                                                 C.byref(st) if timed else None))
        return st

    # -- pml_query main, vec mode (pml_query.cpp:92-143) ----------------------
    def query_file(self, pattern_path, pml_path=None, cid_path=None, batch_bases=0):
        st = Stats()
        _check(lib().colbwt_query_file(self._h, os.fsencode(pattern_path),
                                       os.fsencode(pml_path) if pml_path else None,
                                       os.fsencode(cid_path) if cid_path else None,
                                       batch_bases, C.byref(st)))
        return st

    def query_file_binary(self, pattern_path, pml_bin_path=None, cid_bin_path=None, batch_bases=0):
        """`col-bwt query`'s binary outputs (<pattern>.pml.bin / .cid.bin; Movi-like container, unverified)."""
        st = Stats()
        _check(lib().colbwt_query_file_binary(self._h, os.fsencode(pattern_path),
                                              os.fsencode(pml_bin_path) if pml_bin_path else None,
                                              os.fsencode(cid_bin_path) if cid_bin_path else None,
                                              batch_bases, C.byref(st)))
        return st

    # -- exact-match counting (backward search; include/colbwt.h colbwt_count_batch) --
    def count_batch(self, bases, read_off, want_sp=False):
        """Many reads -> (mlen uint32, occ uint64, sp uint64 or None, Stats), one entry per read:
        mlen = length of the longest suffix of the read that occurs in the text, occ = its occurrences,
        sp = its rank among the text's suffixes (want_sp)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        n_reads = max(read_off.size - 1, 0)
        mlen = np.zeros(n_reads, np.uint32)
        occ = np.zeros(n_reads, np.uint64)
        sp = np.zeros(n_reads, np.uint64) if want_sp else None
        st = Stats()
        _check(lib().colbwt_count_batch(self._h, bases.ctypes.data, read_off.ctypes.data, n_reads, mlen.ctypes.data,
                                        occ.ctypes.data, sp.ctypes.data if want_sp else None, C.byref(st)))
        return mlen, occ, sp, st

    def count(self, pattern):
        """One read -> (mlen, occ, sp) as ints."""
        p = np.frombuffer(bytes(pattern), dtype=np.uint8)
        mlen, occ, sp, _ = self.count_batch(p, np.array([0, p.size], np.uint64), want_sp=True)
        return int(mlen[0]), int(occ[0]), int(sp[0])

    def count_device(self, d_bases, d_read_off, n_reads, n_bases, d_mlen, d_occ, d_sp=None, d_order=None, stream=0,
                     timed=False):
        """Device-resident count entry point: raw device pointers (ints); d_sp / d_order may be None."""
        st = Stats()
        _check(lib().colbwt_count_device(self._h, d_bases, d_read_off, n_reads, n_bases, d_mlen, d_occ, d_sp, d_order,
                                         stream, C.byref(st) if timed else None))
        return st

    def count_file(self, pattern_path, out_path=None, batch_bases=0):
        """FASTA/FASTQ(.gz) -> text lines "name\tm\tmlen\tocc" (default <pattern>.count)."""
        st = Stats()
        _check(lib().colbwt_count_file(self._h, os.fsencode(pattern_path), os.fsencode(out_path) if out_path else None,
                                       batch_bases, C.byref(st)))
        return st

    # -- seeds: per-read PML peaks and chain summaries (include/colbwt.h colbwt_seeds_*) ------------
    def seeds_batch(self, bases, read_off, min_len=16, max_seeds=16, want_seeds=True):
        """Many reads -> (summary, seed_pos, seed_len, seed_cid, Stats): summary a SEED_SUMMARY record per
        read; the slot arrays (n_reads, max_seeds), largest pos first, unused slots SEED_NONE / 0 / 0
        (None each when not want_seeds).  Query and reduction run on the device."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        n_reads = max(read_off.size - 1, 0)
        summary = np.zeros(n_reads, SEED_SUMMARY)
        k = int(max_seeds)
        pos = np.zeros((n_reads, max(k, 0)), np.uint32) if want_seeds else None
        ln = np.zeros((n_reads, max(k, 0)), np.uint32) if want_seeds else None
        sc = np.zeros((n_reads, max(k, 0)), np.uint8) if want_seeds else None
        st = Stats()
        _check(lib().colbwt_seeds_batch(self._h, bases.ctypes.data, read_off.ctypes.data, n_reads, int(min_len), k,
                                        summary.ctypes.data, *((a.ctypes.data if want_seeds else None) for a in (pos, ln, sc)),
                                        C.byref(st)))
        return summary, pos, ln, sc, st

    def seeds(self, pattern, min_len=16, max_seeds=16):
        """One read -> (summary dict, [(pos, len, id), ..] largest pos first)."""
        p = np.frombuffer(bytes(pattern), dtype=np.uint8)
        summary, pos, ln, sc, _ = self.seeds_batch(p, np.array([0, p.size], np.uint64), min_len, max_seeds)
        k = min(int(summary["n_seeds"][0]), int(max_seeds))
        return ({f: int(summary[f][0]) for f in SEED_SUMMARY.names},
                [(int(pos[0, t]), int(ln[0, t]), int(sc[0, t])) for t in range(k)])

    @staticmethod
    def seeds_reduce_device(d_pml, d_cid, d_read_off, n_reads, n_bases, min_len, max_seeds, d_summary, d_seed_pos=None,
                            d_seed_len=None, d_seed_cid=None, pml_bytes=2, stream=0, timed=False):
        """The reduction alone over device buffers a query_device call filled (raw device pointers, ints);
        needs no index.  The three slot arrays may all be None."""
        return seeds_reduce_device(d_pml, d_cid, d_read_off, n_reads, n_bases, min_len, max_seeds, d_summary, d_seed_pos,
                                   d_seed_len, d_seed_cid, pml_bytes, stream, timed)

    def seeds_file(self, pattern_path, out_path=None, min_len=16, max_seeds=16, batch_bases=0):
        """FASTA/FASTQ(.gz) -> text lines "name\tm\tn_seeds\tcov\tmax_len\tresets\tn_col\tcol_cov\tasc\tdesc\tpos:len:id,.."
        (default <pattern>.seeds)."""
        st = Stats()
        _check(lib().colbwt_seeds_file(self._h, os.fsencode(pattern_path), os.fsencode(out_path) if out_path else None,
                                       int(min_len), int(max_seeds), batch_bases, C.byref(st)))
        return st

    # -- locate (include/colbwt.h colbwt_locate_*) -------------------------------------------------
    def attach_locate(self, prefix_or_file=None, data=None):
        """Loads the locate samples onto every replica: <prefix>.col_loc (or the path itself), or a
        .col_loc image in memory (`data`, bytes-like)."""
        if data is not None:
            arr = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8))
            _check(lib().colbwt_index_attach_locate_memory(self._h, arr.ctypes.data, arr.size))
        else:
            _check(lib().colbwt_index_attach_locate(self._h, os.fsencode(prefix_or_file)))

    def locate_docs(self):
        """doc_start of the attached samples (uint64 array): first text position of every document."""
        n = C.c_uint32(0)
        L = lib()
        L.colbwt_locate_docs(self._h, None, 0, C.byref(n))     # their number (the call itself fails for want of room)
        out = np.zeros(n.value, np.uint64)
        _check(L.colbwt_locate_docs(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def locate_batch(self, bases, read_off, max_occ=16):
        """Many reads -> (mlen uint32, occ uint64, pos uint64 [n_reads, max_occ], Stats): pos[k, :min(occ, max_occ)]
        are the text positions SA[ep], SA[ep-1], .. of read k's longest matching suffix, the rest LOCATE_NONE."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        n_reads = max(read_off.size - 1, 0)
        mlen = np.zeros(n_reads, np.uint32)
        occ = np.zeros(n_reads, np.uint64)
        pos = np.zeros((n_reads, max(int(max_occ), 0)), np.uint64)
        st = Stats()
        _check(lib().colbwt_locate_batch(self._h, bases.ctypes.data, read_off.ctypes.data, n_reads, int(max_occ),
                                         mlen.ctypes.data, occ.ctypes.data, pos.ctypes.data, C.byref(st)))
        return mlen, occ, pos, st

    def locate(self, pattern, max_occ=16):
        """One read -> (mlen, occ, [positions]) as ints (at most max_occ positions)."""
        p = np.frombuffer(bytes(pattern), dtype=np.uint8)
        mlen, occ, pos, _ = self.locate_batch(p, np.array([0, p.size], np.uint64), max_occ)
        k = min(int(occ[0]), int(max_occ))
        return int(mlen[0]), int(occ[0]), [int(x) for x in pos[0, :k]]

    def locate_device(self, d_bases, d_read_off, n_reads, n_bases, max_occ, d_mlen, d_occ, d_pos, d_order=None, stream=0,
                      timed=False):
        """Device-resident locate entry point: raw device pointers (ints); d_pos holds n_reads * max_occ u64."""
        st = Stats()
        _check(lib().colbwt_locate_device(self._h, d_bases, d_read_off, n_reads, n_bases, int(max_occ), d_mlen, d_occ, d_pos,
                                          d_order, stream, C.byref(st) if timed else None))
        return st

    def locate_file(self, pattern_path, out_path=None, max_occ=16, batch_bases=0):
        """FASTA/FASTQ(.gz) -> text lines "name\tm\tmlen\tocc\tdoc:offset,.." (default <pattern>.locate)."""
        st = Stats()
        _check(lib().colbwt_locate_file(self._h, os.fsencode(pattern_path), os.fsencode(out_path) if out_path else None,
                                        int(max_occ), batch_bases, C.byref(st)))
        return st

    # -- locate-all: every occurrence, as compressed sparse rows (include/colbwt.h colbwt_locate_all_*) --
    def locate_all_batch(self, bases, read_off, min_len=16, max_per_read=0):
        """Many reads -> (mlen uint32, occ uint64, pos_off uint64 [n_reads + 1], pos uint64 [pos_off[-1]], Stats):
        pos[pos_off[k]:pos_off[k+1]] are ALL text positions SA[ep], SA[ep-1], .. of read k's longest matching suffix
        when it has at least min_len bases (at most max_per_read of them when that is not 0), none otherwise.
        A first call sizes pos, a second fills it."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        n_reads = max(read_off.size - 1, 0)
        mlen = np.zeros(n_reads, np.uint32)
        occ = np.zeros(n_reads, np.uint64)
        pos_off = np.zeros(n_reads + 1, np.uint64)
        st = Stats()
        head = (self._h, bases.ctypes.data, read_off.ctypes.data, n_reads, int(min_len), int(max_per_read), mlen.ctypes.data,
                occ.ctypes.data, pos_off.ctypes.data)
        rc = lib().colbwt_locate_all_batch(*head, None, 0, C.byref(st))
        if rc != 0 and not (rc == -1 and lib().colbwt_last_error().startswith(b"pos_cap too small")):
            _check(rc)
        pos = np.zeros(int(pos_off[-1]), np.uint64)
        if rc != 0:
            _check(lib().colbwt_locate_all_batch(*head, pos.ctypes.data, pos.size, C.byref(st)))
        return mlen, occ, pos_off, pos, st

    def locate_all(self, pattern, min_len=1, max_per_read=0):
        """One read -> (mlen, occ, [positions]) as ints."""
        p = np.frombuffer(bytes(pattern), dtype=np.uint8)
        mlen, occ, _, pos, _ = self.locate_all_batch(p, np.array([0, p.size], np.uint64), min_len, max_per_read)
        return int(mlen[0]), int(occ[0]), [int(x) for x in pos]

    def locate_all_plan_device(self, d_bases, d_read_off, n_reads, n_bases, min_len, max_per_read, d_mlen, d_occ, d_pos_off, d_work,
                               d_order=None, stream=0, want_total=True, timed=False):
        """Search + plan on device buffers (raw device pointers, ints): fills d_mlen, d_occ, d_pos_off (n_reads + 1 u64)
        and d_work (locate_all_work_bytes(n_reads) bytes, 256-byte aligned) -> (pos_off[n_reads] or None, Stats).
        Asynchronous unless want_total or timed."""
        st = Stats()
        total = C.c_uint64(0)
        _check(lib().colbwt_locate_all_plan_device(self._h, d_bases, d_read_off, n_reads, n_bases, int(min_len), int(max_per_read),
                                                   d_mlen, d_occ, d_pos_off, d_work, d_order, stream,
                                                   C.byref(total) if want_total else None, C.byref(st) if timed else None))
        return (int(total.value) if want_total else None), st

    def locate_all_fill_device(self, n_reads, read_lo, read_hi, d_pos_off, d_pos, pos_cap, d_work, stream=0, timed=False):
        """The walk of the reads [read_lo, read_hi) of a planned batch into d_pos[0 .. pos_cap) (raw device pointers):
        slot 0 is pos[pos_off[read_lo]]; nothing at or past pos_cap is written."""
        st = Stats()
        _check(lib().colbwt_locate_all_fill_device(self._h, n_reads, read_lo, read_hi, d_pos_off, d_pos, int(pos_cap), d_work, stream,
                                                   C.byref(st) if timed else None))
        return st

    def locate_all_file(self, pattern_path, out_path=None, min_len=16, max_per_read=0, batch_bases=0):
        """FASTA/FASTQ(.gz) -> text lines "name\tm\tmlen\tocc\tdoc:offset,.." with every position (default <pattern>.locate)."""
        st = Stats()
        _check(lib().colbwt_locate_all_file(self._h, os.fsencode(pattern_path), os.fsencode(out_path) if out_path else None,
                                            int(min_len), int(max_per_read), batch_bases, C.byref(st)))
        return st

    # -- anchors: left-maximal exact matches along the whole read (include/colbwt.h colbwt_anchors_*) --
    def anchors_batch(self, bases, read_off, min_len=16, max_anchors=16, max_occ=1, want_slots=True):
        """Many reads -> (summary, start, len, occ, pos, Stats): summary an AnchorSummary record per read; start / len
        (uint32) and occ (uint64) are (n_reads, max_anchors), largest start first, unused slots ANCHOR_NONE / 0 / 0; pos
        (uint64) is (n_reads, max_anchors, max_occ) with LOCATE_NONE past min(occ, max_occ), or None when max_occ == 0
        (which needs no locate samples).  Not want_slots: summaries only, the four arrays None."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        n_reads = max(read_off.size - 1, 0)
        k, w = max(int(max_anchors), 0), max(int(max_occ), 0)
        summary = np.zeros(n_reads, AnchorSummary)
        start = np.zeros((n_reads, k), np.uint32) if want_slots else None
        ln = np.zeros((n_reads, k), np.uint32) if want_slots else None
        occ = np.zeros((n_reads, k), np.uint64) if want_slots else None
        pos = np.zeros((n_reads, k, w), np.uint64) if want_slots and w else None
        st = Stats()
        _check(lib().colbwt_anchors_batch(self._h, bases.ctypes.data, read_off.ctypes.data, n_reads, int(min_len), int(max_anchors),
                                          int(max_occ), summary.ctypes.data,
                                          *((a.ctypes.data if a is not None else None) for a in (start, ln, occ, pos)), C.byref(st)))
        return summary, start, ln, occ, pos, st

    def anchors(self, pattern, min_len=16, max_anchors=16, max_occ=1):
        """One read -> (summary dict, [(start, len, occ, [positions]), ..] largest start first)."""
        p = np.frombuffer(bytes(pattern), dtype=np.uint8)
        summary, start, ln, occ, pos, _ = self.anchors_batch(p, np.array([0, p.size], np.uint64), min_len, max_anchors, max_occ)
        out = []
        for t in range(int(summary["n_stored"][0])):
            k = min(int(occ[0, t]), int(max_occ))
            out.append((int(start[0, t]), int(ln[0, t]), int(occ[0, t]), [int(x) for x in pos[0, t, :k]] if k else []))
        return {f: int(summary[f][0]) for f in AnchorSummary.names}, out

    def anchors_device(self, d_bases, d_read_off, n_reads, n_bases, min_len, max_anchors, max_occ, d_summary, d_start=None,
                       d_len=None, d_occ=None, d_pos=None, d_order=None, stream=0, timed=False):
        """Device-resident anchors entry point: raw device pointers (ints).  d_start / d_len / d_occ all or none; d_pos
        (n_reads * max_anchors * max_occ u64) exactly when they are given and max_occ > 0."""
        st = Stats()
        _check(lib().colbwt_anchors_device(self._h, d_bases, d_read_off, n_reads, n_bases, int(min_len), int(max_anchors),
                                           int(max_occ), d_summary, d_start, d_len, d_occ, d_pos, d_order, stream,
                                           C.byref(st) if timed else None))
        return st

    def anchors_file(self, pattern_path, out_path=None, min_len=16, max_anchors=16, max_occ=1, batch_bases=0):
        """FASTA/FASTQ(.gz) -> text lines "name\tm\tn_factors\tn_kept\tcov\tmax_len\tskipped\tn_unique\tcov_unique\tA,A,..",
        A = start:len:occ@doc:offset@.. (default <pattern>.anchors)."""
        st = Stats()
        _check(lib().colbwt_anchors_file(self._h, os.fsencode(pattern_path), os.fsencode(out_path) if out_path else None,
                                         int(min_len), int(max_anchors), int(max_occ), batch_bases, C.byref(st)))
        return st

    # -- chain: the best colinear chain of each read's anchors (include/colbwt.h colbwt_chain_*) --
    def chain_batch(self, bases, read_off, min_len=16, max_anchors=16, max_occ=4, band=16):
        """Many reads -> (chain, Stats): a CHAIN record per read; the anchors stay on the device."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        n_reads = max(read_off.size - 1, 0)
        chain = np.zeros(n_reads, CHAIN)
        st = Stats()
        _check(lib().colbwt_chain_batch(self._h, bases.ctypes.data, read_off.ctypes.data, n_reads, int(min_len), int(max_anchors),
                                        int(max_occ), int(band), chain.ctypes.data, C.byref(st)))
        return chain, st

    def chain(self, pattern, min_len=16, max_anchors=16, max_occ=4, band=16):
        """One read -> its chain as a dict of the CHAIN fields, or None when no anchor has a position."""
        p = np.frombuffer(bytes(pattern), dtype=np.uint8)
        chain, _ = self.chain_batch(p, np.array([0, p.size], np.uint64), min_len, max_anchors, max_occ, band)
        if int(chain["text_begin"][0]) == LOCATE_NONE:
            return None
        return {f: int(chain[f][0]) for f in CHAIN.names}

    def chain_reduce_device(self, d_start, d_len, d_pos, n_reads, max_anchors, max_occ, band, d_chain, stream=0, timed=False):
        """The reduction alone over device arrays of the shape anchors_device fills: raw device pointers (ints);
        d_chain n_reads CHAIN records, 16-byte aligned."""
        st = Stats()
        _check(lib().colbwt_chain_reduce_device(self._h, d_start, d_len, d_pos, n_reads, int(max_anchors), int(max_occ), int(band),
                                                d_chain, stream, C.byref(st) if timed else None))
        return st

    def chain_device(self, d_bases, d_read_off, n_reads, n_bases, min_len, max_anchors, max_occ, band, d_chain, d_work, d_order=None,
                     stream=0, timed=False):
        """Device-resident chain entry point: anchors into d_work (chain_work_bytes(n_reads, max_anchors, max_occ) bytes,
        256-byte aligned), then the reduction into d_chain."""
        st = Stats()
        _check(lib().colbwt_chain_device(self._h, d_bases, d_read_off, n_reads, n_bases, int(min_len), int(max_anchors), int(max_occ),
                                         int(band), d_chain, d_work, d_order, stream, C.byref(st) if timed else None))
        return st

    def chain_file(self, pattern_path, out_path=None, min_len=16, max_anchors=16, max_occ=4, band=16, batch_bases=0):
        """FASTA/FASTQ(.gz) -> text lines "name\tm\tread_begin\tread_end\tdoc\toffset\ttext_len\tscore\tscore2\tn_chained\tn_hits"
        (default <pattern>.chains); doc and offset are "*" for a read without a chain."""
        st = Stats()
        _check(lib().colbwt_chain_file(self._h, os.fsencode(pattern_path), os.fsencode(out_path) if out_path else None,
                                       int(min_len), int(max_anchors), int(max_occ), int(band), batch_bases, C.byref(st)))
        return st

    # -- docs: the documents holding each read's longest exact match (include/colbwt.h colbwt_docs_*) --
    def docs_mask_words(self):
        """W = ceil(n_docs / 64): u64 mask words per read (0 when no locate samples are attached)."""
        return int(lib().colbwt_docs_mask_words(self._h))

    def docs_batch(self, bases, read_off, min_len=16, max_walk=256, want_tally=True):
        """Many reads -> (mlen uint32, occ uint64, n_hit uint32, mask uint64 [n_reads, W], doc_reads, doc_only, Stats):
        bit d & 63 of mask[k, d >> 6] is set iff one of the first min(occ, max_walk) occurrences of read k's longest
        matching suffix (of at least min_len bases) starts in document d; doc_reads[d] / doc_only[d] (uint64 [n_docs],
        None each when not want_tally) count the reads hitting d / hitting d alone.  Everything runs on the device."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.uint64)
        n_reads = max(read_off.size - 1, 0)
        words = self.docs_mask_words()
        mlen = np.zeros(n_reads, np.uint32)
        occ = np.zeros(n_reads, np.uint64)
        n_hit = np.zeros(n_reads, np.uint32)
        mask = np.zeros((n_reads, words), np.uint64)
        n_docs = self.locate_docs().size if want_tally and words else 0
        doc_reads = np.zeros(n_docs, np.uint64) if want_tally else None
        doc_only = np.zeros(n_docs, np.uint64) if want_tally else None
        st = Stats()
        _check(lib().colbwt_docs_batch(self._h, bases.ctypes.data, read_off.ctypes.data, n_reads, int(min_len), int(max_walk),
                                       mlen.ctypes.data, occ.ctypes.data, n_hit.ctypes.data, mask.ctypes.data,
                                       doc_reads.ctypes.data if want_tally else None, doc_only.ctypes.data if want_tally else None,
                                       C.byref(st)))
        return mlen, occ, n_hit, mask, doc_reads, doc_only, st

    def docs(self, pattern, min_len=16, max_walk=256):
        """One read -> (mlen, occ, [document numbers, ascending]) as ints."""
        p = np.frombuffer(bytes(pattern), dtype=np.uint8)
        mlen, occ, _, mask, _, _, _ = self.docs_batch(p, np.array([0, p.size], np.uint64), min_len, max_walk, want_tally=False)
        return int(mlen[0]), int(occ[0]), _mask_docs(mask[0])

    def docs_device(self, d_bases, d_read_off, n_reads, n_bases, min_len, max_walk, d_mlen, d_occ, d_n_hit, d_mask, d_work,
                    d_doc_reads=None, d_doc_only=None, d_order=None, stream=0, timed=False):
        """Device-resident docs entry point: raw device pointers (ints).  d_mask holds n_reads * docs_mask_words() u64,
        d_work docs_work_bytes(n_reads) bytes (256-byte aligned); the tallies (n_docs u64 each, or None) are ADDED to."""
        st = Stats()
        _check(lib().colbwt_docs_device(self._h, d_bases, d_read_off, n_reads, n_bases, int(min_len), int(max_walk), d_mlen, d_occ,
                                        d_n_hit, d_mask, d_doc_reads, d_doc_only, d_work, d_order, stream,
                                        C.byref(st) if timed else None))
        return st

    def docs_file(self, pattern_path, out_path=None, min_len=16, max_walk=256, batch_bases=0):
        """FASTA/FASTQ(.gz) -> text lines "name\tm\tmlen\tocc\tn_hit\td,d,.." (default <pattern>.docs) and
        <out>.tally, one line "d\tdoc_reads\tdoc_only" per document."""
        st = Stats()
        _check(lib().colbwt_docs_file(self._h, os.fsencode(pattern_path), os.fsencode(out_path) if out_path else None,
                                      int(min_len), int(max_walk), batch_bases, C.byref(st)))
        return st

    def cid_dictionary(self):
        """The distinct col ids the table's rows hold, ascending (uint8 array): the dictionary of the gather codec."""
        ids = np.zeros(256, np.uint8)
        n = C.c_uint32(0)
        _check(lib().colbwt_index_cid_dictionary(self._h, ids.ctypes.data, C.byref(n)))
        return ids[:n.value].copy()

    def synth_reads_device(self, n_reads, read_len, sub_permille, seed, d_bases, d_read_off, stream=0):
        _check(lib().colbwt_synth_reads_device(self._h, n_reads, read_len, sub_permille, seed,
                                               d_bases, d_read_off, stream))

    def close(self):
        if self._h:
            lib().colbwt_index_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def doc_offsets(positions, doc_start):
    """Text positions -> (document number, offset inside the document) arrays (LOCATE_NONE entries are
    left out by the caller; doc_start from ColPml.locate_docs)."""
    positions = np.asarray(positions, np.uint64)
    doc_start = np.asarray(doc_start, np.uint64)
    doc = np.searchsorted(doc_start, positions, side="right").astype(np.int64) - 1
    return doc, positions - doc_start[doc]


def docs_work_bytes(n_reads):
    """colbwt_docs_work_bytes: size of the device workspace a docs_device call over n_reads reads needs."""
    return int(lib().colbwt_docs_work_bytes(int(n_reads)))


def locate_all_work_bytes(n_reads):
    """colbwt_locate_all_work_bytes: size of the device workspace a locate-all plan over n_reads reads needs."""
    return int(lib().colbwt_locate_all_work_bytes(int(n_reads)))


def chain_work_bytes(n_reads, max_anchors, max_occ):
    """colbwt_chain_work_bytes: size of the device scratch a chain_device call keeps its anchors in."""
    return int(lib().colbwt_chain_work_bytes(int(n_reads), int(max_anchors), int(max_occ)))


def _mask_docs(mask_row):
    """One read's mask words (ColPml.docs_batch) -> its document numbers, ascending."""
    return [64 * w + b for w, x in enumerate(np.asarray(mask_row, np.uint64).tolist()) for b in range(64) if (x >> b) & 1]


def binary_to_text(bin_path, value_bytes, text_path):
    """Container -> reference text (`col-bwt view`); value_bytes 2 = .pml.bin, 1 = .cid.bin."""
    _check(lib().colbwt_binary_to_text(os.fsencode(bin_path), int(value_bytes), os.fsencode(text_path)))


def read_binary(bin_path, value_bytes):
    """Parses a container: [(name, values in pattern order as a numpy array)]."""
    raw = np.fromfile(bin_path, dtype=np.uint8)
    out, at = [], 0
    dt = np.uint16 if value_bytes == 2 else np.uint8
    while at < raw.size:
        nl = int(raw[at:at + 2].view(np.uint16)[0])
        name = raw[at + 2:at + 2 + nl].tobytes().decode()
        m = int(raw[at + 2 + nl:at + 10 + nl].view(np.uint64)[0])
        at += 10 + nl
        out.append((name, raw[at:at + m * value_bytes].view(dt)[::-1].copy()))
        at += m * value_bytes
    return out


def seeds_reduce_device(d_pml, d_cid, d_read_off, n_reads, n_bases, min_len, max_seeds, d_summary, d_seed_pos=None,
                        d_seed_len=None, d_seed_cid=None, pml_bytes=2, stream=0, timed=False):
    """colbwt_seeds_reduce_device: pml / cid / read_off device arrays -> summaries and seed slots (device pointers, ints)."""
    st = Stats()
    _check(lib().colbwt_seeds_reduce_device(d_pml, pml_bytes, d_cid, d_read_off, n_reads, n_bases, int(min_len), int(max_seeds),
                                            d_summary, d_seed_pos, d_seed_len, d_seed_cid, stream,
                                            C.byref(st) if timed else None))
    return st


def pml_pack_device(d_pml, n_bases, d_mask, stream=0):
    """Gather codec (include/colbwt.h): one bit per base, set where the PML value is 0."""
    _check(lib().colbwt_pml_pack_device(d_pml, n_bases, d_mask, stream))


def read_end_mask_device(d_read_off, n_reads, d_mask, stream=0):
    """Bit set at the last base of every non-empty read (d_mask zeroed by the caller)."""
    _check(lib().colbwt_read_end_mask_device(d_read_off, n_reads, d_mask, stream))


def cid_code_bits(n_ids):
    """Bits per base of the col-id codes of a dictionary of n_ids ids."""
    return int(lib().colbwt_cid_code_bits(int(n_ids)))


def cid_pack_device(d_cid, n_bases, ids, d_planes, stream=0):
    """Gather codec: col ids -> codes of the dictionary `ids` (uint8 array), cid_code_bits(len(ids)) bit planes per 32 bases."""
    ids = np.ascontiguousarray(ids, np.uint8)
    _check(lib().colbwt_cid_pack_device(d_cid, n_bases, ids.ctypes.data, ids.size, d_planes, stream))


def cid_unpack_device(d_planes, first_word, n_words, ids, d_cid, stream=0):
    """Rebuilds the col ids of 32-base words [first_word, first_word + n_words) from their bit planes."""
    ids = np.ascontiguousarray(ids, np.uint8)
    _check(lib().colbwt_cid_unpack_device(d_planes, first_word, n_words, ids.ctypes.data, ids.size, d_cid, stream))


def pml_unpack_device(d_zero_mask, d_end_mask, first_word, n_words, total_words, d_pml, stream=0):
    """Rebuilds the u16 PML values of 32-base words [first_word, first_word + n_words)."""
    _check(lib().colbwt_pml_unpack_device(d_zero_mask, d_end_mask, first_word, n_words, total_words, d_pml, stream))


def synth_index(rows, mean_len=8, split_permille=0, seed=42, thr_mode=0):
    """Synthetic `.col_pml` image (SURVEY.md 8(d) recipe) as a uint8 numpy array.
    thr_mode 0: thresholds uniform in [0, n); 1: between consecutive runs of a character."""
    nbytes = lib().colbwt_synth_index_bytes(rows)
    out = np.empty(nbytes, np.uint8)
    _check(lib().colbwt_synth_index_thr(rows, mean_len, split_permille, seed, thr_mode, out.ctypes.data, nbytes))
    return out


def build_col_pml(prefix, out_path=None):
    """`build_col_bwt <prefix>` (src/build_col_bwt.cpp:38-52): writes <prefix>.col_pml."""
    _check_build(lib().colbwt_build_col_pml(os.fsencode(prefix), os.fsencode(out_path) if out_path else None))


def build_col_pml_arrays(heads, lens, col_ids, split_pos, thr_pos):
    """col_pml(heads, lengths, col_ids, thresholds, splits) + serialize -> image bytes (uint8 array)."""
    heads = np.ascontiguousarray(heads, np.uint8)
    lens = np.ascontiguousarray(lens, np.uint64)
    col_ids = np.ascontiguousarray(col_ids, np.uint8)
    split_pos = np.ascontiguousarray(split_pos, np.uint64)
    thr_pos = np.ascontiguousarray(thr_pos, np.uint64)
    need = C.c_uint64(0)
    args = [heads.ctypes.data, heads.size, lens.ctypes.data, col_ids.ctypes.data, col_ids.size,
            split_pos.ctypes.data, split_pos.size, thr_pos.ctypes.data, thr_pos.size]
    lib().colbwt_build_col_pml_arrays(*args, None, 0, C.byref(need))
    out = np.zeros(need.value, np.uint8)
    _check_build(lib().colbwt_build_col_pml_arrays(*args, out.ctypes.data, out.size, C.byref(need)))
    return out


def col_split(prefix, mode="tunnels", split_rate=1, device=0):
    """`col_split <prefix> -m mode -s rate` (src/col_split.cpp:62-140, with build_FL folded in): writes
    <prefix>.col_runs and <prefix>.col_ids."""
    L = lib()
    L.colbwt_col_split_error.restype = C.c_char_p
    rc = L.colbwt_col_split(os.fsencode(prefix), 1 if mode == "all" else 0, int(split_rate), int(device))
    if rc != 0:
        raise ColbwtError(rc, L.colbwt_col_split_error().decode())


def col_split_arrays(heads, lens, mum_len, mum_pos, num_docs, mode="tunnels", split_rate=1, device=0):
    """-> (split positions uint64 ascending, col ids uint8, n): what .col_runs / .col_ids would hold."""
    L = lib()
    L.colbwt_col_split_error.restype = C.c_char_p
    L.colbwt_col_split_arrays.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                          C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p,
                                          C.POINTER(C.c_uint64)]
    heads = np.ascontiguousarray(heads, np.uint8)
    lens = np.ascontiguousarray(lens, np.uint64)
    mum_len = np.ascontiguousarray(mum_len, np.uint64)
    mum_pos = np.ascontiguousarray(mum_pos, np.uint64)
    cap = int(lens.sum()) + 8
    pos = np.zeros(cap, np.uint64)
    ids = np.zeros(cap, np.uint8)
    k, n = C.c_uint64(0), C.c_uint64(0)
    rc = L.colbwt_col_split_arrays(heads.ctypes.data, heads.size, lens.ctypes.data, mum_len.ctypes.data, mum_pos.ctypes.data,
                                   mum_len.size, int(num_docs), 1 if mode == "all" else 0, int(split_rate), int(device),
                                   pos.ctypes.data, cap, C.byref(k), ids.ctypes.data, C.byref(n))
    if rc != 0:
        raise ColbwtError(rc, L.colbwt_col_split_error().decode())
    return pos[:k.value].copy(), ids[:k.value].copy(), int(n.value)


class _RlbwtView(C.Structure):
    _fields_ = [("n", C.c_uint64), ("n_runs", C.c_uint64), ("n_mums", C.c_uint64), ("n_docs", C.c_uint32), ("rounds", C.c_int32),
                ("heads", C.POINTER(C.c_uint8)), ("lens", C.POINTER(C.c_uint64)), ("thr_pos", C.POINTER(C.c_uint64)),
                ("mum_len", C.POINTER(C.c_uint64)), ("mum_pos", C.POINTER(C.c_uint64))]


def _rlbwt_result(L, handle):
    v = _RlbwtView()
    L.colbwt_rlbwt_get.argtypes = [C.c_void_p, C.POINTER(_RlbwtView)]
    L.colbwt_rlbwt_free.argtypes = [C.c_void_p]
    L.colbwt_rlbwt_get(handle, C.byref(v))

    def arr(ptr, count, dtype):
        return np.ctypeslib.as_array(ptr, shape=(count,)).astype(dtype, copy=True) if count else np.zeros(0, dtype)
    out = dict(n=int(v.n), n_docs=int(v.n_docs), rounds=int(v.rounds), heads=arr(v.heads, v.n_runs, np.uint8),
               lens=arr(v.lens, v.n_runs, np.uint64), thr=arr(v.thr_pos, v.n_runs, np.uint64),
               mum_len=arr(v.mum_len, v.n_mums, np.uint64), mum_pos=arr(v.mum_pos, v.n_mums, np.uint64))
    L.colbwt_rlbwt_free(handle)
    return out


def rlbwt_from_text(text, doc_start, min_mum=20, device=0, locate_path=None):
    """RLBWT, thresholds and multi-MUMs of a prepared text (separators 1, final 0) on the device:
    -> dict(n, n_docs, rounds, heads, lens, thr, mum_len, mum_pos).  locate_path: also gathers the
    locate samples and writes them there as a .col_loc."""
    L = lib()
    L.colbwt_rlbwt_error.restype = C.c_char_p
    L.colbwt_rlbwt_build_text.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]
    t = np.frombuffer(bytes(text), np.uint8)
    ds = np.ascontiguousarray(doc_start, np.uint64)
    h = C.c_void_p()
    fn = L.colbwt_rlbwt_build_text_locate if locate_path else L.colbwt_rlbwt_build_text
    rc = fn(t.ctypes.data, t.size, ds.ctypes.data, ds.size, int(min_mum), int(device), C.byref(h))
    if rc == 0 and locate_path:
        rc = L.colbwt_rlbwt_write_locate(h, os.fsencode(locate_path))
        if rc != 0:
            msg = L.colbwt_rlbwt_error().decode()
            L.colbwt_rlbwt_free.argtypes = [C.c_void_p]
            L.colbwt_rlbwt_free(h)
            raise ColbwtError(rc, msg)
    if rc != 0:
        raise ColbwtError(rc, L.colbwt_rlbwt_error().decode())
    return _rlbwt_result(L, h)


def rlbwt_from_fastas(paths, out_prefix=None, min_mum=20, revcomp=False, device=0, locate=False):
    """`mumemto mum -K -R -T` of the reference's driver (col-bwt.py:121-145): one document per file;
    writes <out_prefix>.bwt.heads / .bwt.len / .thr_pos / .col_mums (and with `locate` <out_prefix>.col_loc)
    when given; returns the arrays."""
    L = lib()
    L.colbwt_rlbwt_error.restype = C.c_char_p
    L.colbwt_rlbwt_build_files.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.c_int, C.c_uint64, C.c_int, C.c_char_p,
                                           C.POINTER(C.c_void_p)]
    arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
    h = C.c_void_p()
    fn = L.colbwt_rlbwt_build_files_locate if locate else L.colbwt_rlbwt_build_files
    rc = fn(arr, len(paths), int(bool(revcomp)), int(min_mum), int(device), os.fsencode(out_prefix) if out_prefix else None,
            C.byref(h))
    if rc != 0:
        raise ColbwtError(rc, L.colbwt_rlbwt_error().decode())
    return _rlbwt_result(L, h)


def _check_build(rc):
    if rc != 0:
        raise ColbwtError(rc, "index construction failed (missing/short input file or bad argument)")
