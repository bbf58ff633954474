/*
 * colbwt.h -- C-ABI of the MI355X-native col-bwt PML / chain-statistic query
 * engine (libcolbwt.so, hand-written HIP for gfx950).
 *
 * The reference (drnatebrown/col-bwt) has no FFI layer; the entry points below
 * are the ones a binding of its query path would need.  Each cites the
 * reference interface (file:line under /root/reference) it replaces.
 *
 *   col_pml tbl; tbl.load(ifstream)            col_bwt.hpp:375-380, LF_table.hpp:347-357
 *        -> colbwt_index_open / colbwt_index_open_memory
 *   tbl.query_pml(const char*, size_t)         col_bwt.hpp:409-412 (one read)
 *        -> colbwt_query_batch (many reads per call; read k of the batch is
 *           what one query_pml call returns: pml[k'], cid[k'] <-> pattern[k'])
 *   pml_to_vec / main of pml_query             pml_query.cpp:65-90, 92-143
 *        -> colbwt_query_file (FASTA/FASTQ[.gz] in, text .pml/.cid out)
 *   ~col_pml                                   (implicit)
 *        -> colbwt_index_close
 *
 * Conventions: plain pointers and sizes, caller-owned buffers, int return
 * codes (0 = ok, <0 = error; message via colbwt_last_error(), thread-local),
 * no exceptions cross the ABI.  An index may be queried from several host
 * threads at once on distinct batches (each call uses its own stream).
 * There is NO CPU fallback: every query entry point fails with
 * COLBWT_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef COLBWT_H
#define COLBWT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COLBWT_OK 0
#define COLBWT_ERR_ARG (-1)        /* bad argument (null, misaligned, sizes)  */
#define COLBWT_ERR_IO (-2)         /* file missing / short read               */
#define COLBWT_ERR_FORMAT (-3)     /* .col_pml fails validation               */
#define COLBWT_ERR_NO_DEVICE (-4)  /* no usable HIP device                    */
#define COLBWT_ERR_HIP (-5)        /* a HIP call failed                       */
#define COLBWT_ERR_NOMEM (-6)

typedef struct colbwt_index colbwt_index; /* opaque: table resident in HBM */

/* On-disk widths of the reference build (common.hpp:46-54).  Only the shipped
 * values are accepted; the struct exists so a binding can assert them. */
typedef struct colbwt_widths {
    uint32_t bwt_bytes; /* BWT_BYTES 5 */
    uint32_t run_bytes; /* RUN_BYTES 4 */
    uint32_t len_bytes; /* LEN_BYTES 2 */
    uint32_t id_bits;   /* ID_BITS   8 */
} colbwt_widths;

typedef struct colbwt_info {
    uint64_t bwt_r;        /* maximal BWT runs      (col_bwt.hpp:383)  */
    uint64_t n;            /* BWT length            (LF_table.hpp:360) */
    uint64_t r;            /* rows (sub-runs)       (LF_table.hpp:361) */
    uint32_t sigma;        /* distinct characters present in the table */
    uint32_t device;       /* HIP device ordinal                       */
    uint64_t device_bytes; /* HBM held by the index (locate samples included) */
    uint32_t layout;       /* COLBWT_LAYOUT_ONE_STEP / _TWO_ / _THREE_ / _LINE_ROWS / _MISMATCH_LINES[_DEEP] */
    uint32_t layout_shape; /* line rows: own steps << 8 | steps per mismatch slot; else 0 */
    uint64_t table_rows;   /* rows of the HBM table actually queried   */
    uint32_t n_devices;    /* replicas of the table (colbwt_index_open_devices); the fields above describe the first */
    uint32_t tail_permille; /* K = 8 rows of a mismatch-line layout that carry a match tail, per mille (rounded up); else 0 */
} colbwt_info;

typedef struct colbwt_stats {
    uint64_t n_reads;
    uint64_t n_bases;
    double h2d_ms;     /* reads host->HBM (0 for the device entry point)    */
    double kernel_ms;  /* HIP-event time of the query kernel(s), on-stream  */
    double d2h_ms;     /* results HBM->host (0 for the device entry point)  */
    uint64_t algorithmic_bytes; /* 27 B/base, SURVEY.md section 8(d)         */
} colbwt_stats;

const char *colbwt_version(void);
const char *colbwt_last_error(void);

/* col_pml::load (col_bwt.hpp:375-380).  `prefix_or_file`: either the index
 * prefix (".col_pml" is appended, pml_query.cpp:110-111; extension from
 * col_bwt.hpp:434-437) or the path of the .col_pml file itself.  `widths` may
 * be NULL (shipped widths).  Unlike the reference (UB on a bad file) the
 * loader validates: size == r, file length == 32 + 18*size, idx strictly
 * increasing from 0 and < n, interval < r. */
int colbwt_index_open(const char *prefix_or_file, const colbwt_widths *widths, int device,
                      colbwt_index **out);
/* Same over an in-memory image of the .col_pml file. */
int colbwt_index_open_memory(const void *col_pml_bytes, uint64_t len, const colbwt_widths *widths,
                             int device, colbwt_index **out);
/* HBM table layouts (results are identical).  ONE_STEP:
 * 16-byte rows, one LF step per row load.  TWO_STEP / THREE_STEP: rows split at
 * the pre-images of row boundaries (allowed: the query is a function of BWT
 * positions) so that a row also knows the characters / col ids of the next one /
 * two steps and the landings of LF^2 / LF^3 -- one 128-byte line fill serves up
 * to K bases while the read keeps matching; about 4x / 7x the HBM footprint.
 * AUTO = the engine's choice: line rows when they can be built (fewer than 2^32-1
 * refined rows at every level, enough HBM), else the deepest K-step layout that can. */
#define COLBWT_LAYOUT_AUTO 0
#define COLBWT_LAYOUT_ONE_STEP 1
#define COLBWT_LAYOUT_TWO_STEP 2
#define COLBWT_LAYOUT_THREE_STEP 3
/* LINE_ROWS: one whole 128-byte line per row, fetched lane-cooperatively (8 lanes x 16 bytes per
 * row, one instruction): up to 8 look-ahead steps and, for the three most frequent other
 * characters, where a mismatch re-orients to and what the next step meets from there -- a
 * mismatch costs no line fill of its own.  About 4x the footprint of THREE_STEP.  The depth
 * (number of look-ahead steps K, 4..8) may be given; 0 = the engine's default. */
#define COLBWT_LAYOUT_LINE_ROWS 4
#define COLBWT_LAYOUT_LINE_ROWS_STEPS(K) (COLBWT_LAYOUT_LINE_ROWS | ((K) << 8))
/* MISMATCH_LINES: line rows whose mismatch information lives in a table of its own, one 64-byte
 * entry per (row of the file cut at its thresholds, character): an entry resolves the mismatching
 * base and the base after it whatever that base is, and a stretch of mismatching bases goes from
 * entry to entry -- a line fill per two bases instead of one per base.  LINE_ROWS + ~190 bytes per
 * row of the file. */
#define COLBWT_LAYOUT_MISMATCH_LINES 5
#define COLBWT_LAYOUT_MISMATCH_LINES_STEPS(K) (COLBWT_LAYOUT_MISMATCH_LINES | ((K) << 8))
/* MISMATCH_LINES_DEEP: the same with 128-byte entries that also resolve the base after those two when
 * it matches -- between two mismatches of a stretch there is often exactly one matching base, and
 * with it resolved in the entry the lane goes from entry to entry.  MISMATCH_LINES + ~190 bytes per
 * row of the file.  Measured on C2: 37.1 line fetches per read instead of 40.7, 10.6-11.0 ms per
 * launch instead of 11.5-11.6.  AUTO takes the deep entries when the table with
 * them still leaves 32 GB of what the open could allocate (HBM, COLBWT_HBM_BUDGET_MB) for batches
 * and their results, the 64-byte entries otherwise; asking for MISMATCH_LINES gets the 64-byte ones. */
#define COLBWT_LAYOUT_MISMATCH_LINES_DEEP 6
#define COLBWT_LAYOUT_MISMATCH_LINES_DEEP_STEPS(K) (COLBWT_LAYOUT_MISMATCH_LINES_DEEP | ((K) << 8))
int colbwt_index_open_layout(const char *prefix_or_file, const colbwt_widths *widths, int device, int layout,
                             colbwt_index **out);
int colbwt_index_open_memory_layout(const void *col_pml_bytes, uint64_t len, const colbwt_widths *widths,
                                    int device, int layout, colbwt_index **out);
/* The table replicated on several devices -- the `device_mask` of SURVEY.md 8(b) as a list, so a
 * device may appear twice (two replicas in one HBM).  The reference processes its reads one
 * after the other in one process (pml_query.cpp:74-86); here the host entry points
 * (colbwt_query_batch[_u32], colbwt_query_file) cut every batch into contiguous shards of equal
 * base count, one per replica, queried side by side and copied straight into the caller's arrays:
 * no exchange between devices.  Every replica gets the layout the first one ended up with.  The
 * device-resident entry points address the replica on the buffers' device. */
int colbwt_index_open_devices(const char *prefix_or_file, const colbwt_widths *widths, const int *devices,
                              int n_devices, int layout, colbwt_index **out);
int colbwt_index_open_memory_devices(const void *col_pml_bytes, uint64_t len, const colbwt_widths *widths,
                                     const int *devices, int n_devices, int layout, colbwt_index **out);
void colbwt_index_close(colbwt_index *idx);
int colbwt_index_info(const colbwt_index *idx, colbwt_info *out);

/* col_pml::query_pml for a batch of reads held in HOST memory
 * (col_bwt.hpp:409-412 -> :460-472 -> :498-529).  Read k is
 * bases[read_off[k] .. read_off[k+1]); read_off has n_reads+1 entries,
 * read_off[0] == 0.  Outputs are indexed like `bases`.  PML is u16; a batch
 * containing a read longer than 65535 must use the _u32 form (ERR_ARG
 * otherwise).  `stats` may be NULL. */
int colbwt_query_batch(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off,
                       uint64_t n_reads, uint16_t *pml, uint8_t *cid, colbwt_stats *stats);
int colbwt_query_batch_u32(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off,
                           uint64_t n_reads, uint32_t *pml, uint8_t *cid, colbwt_stats *stats);

/* Same computation with every buffer already resident in HBM on the index's
 * device (the benchmark / multi-GPU path).  Requirements: d_bases has at least
 * 64 readable bytes past read_off[n_reads] (the kernel reads whole 64-byte
 * blocks); d_bases and d_cid are 16-byte aligned, d_pml 32-byte aligned;
 * pml_bytes is 2 or 4 (2 needs every read <= 65535 bases).  `hip_stream` is a
 * hipStream_t (NULL = default stream); the call is asynchronous unless
 * `stats` is non-NULL, in which case it records HIP events on the stream,
 * synchronises it and fills kernel_ms.
 * Concurrency contract: a launch keeps no state outside its arguments (the
 * kernels' work counters live in LDS), so ANY number of calls may be in flight
 * on one index at once -- from any host threads, on any streams -- as long as
 * their output buffers are distinct; there is no bound to respect and nothing
 * to serialise (tests/test_gpu_parity.py queues 48 launches on 24 streams). */
int colbwt_query_device(colbwt_index *idx, const uint8_t *d_bases, const uint64_t *d_read_off,
                        uint64_t n_reads, uint64_t n_bases, void *d_pml, int pml_bytes,
                        uint8_t *d_cid, void *hip_stream, colbwt_stats *stats);

/* Same with an explicit lane assignment for ragged batches: d_order (device,
 * n_reads entries, nullable) lists the read indices by decreasing length, so the
 * 64 lanes of a wave walk reads of similar length.  Results are identical with
 * or without it (each read's values only depend on that read); the host entry
 * points build the order themselves when a batch is ragged and the layout uses
 * it.  d_order is ADVISORY: the one- and two-step layouts assign lanes by it,
 * the three-step and line-row layouts ignore it -- their persistent lanes claim
 * chunks of consecutive reads and balance ragged batches themselves. */
int colbwt_query_device_ordered(colbwt_index *idx, const uint8_t *d_bases, const uint64_t *d_read_off,
                                uint64_t n_reads, uint64_t n_bases, void *d_pml, int pml_bytes,
                                uint8_t *d_cid, const uint32_t *d_order, void *hip_stream,
                                colbwt_stats *stats);

/* pml_query in vec mode (pml_query.cpp:92-143): reads FASTA/FASTQ (optionally
 * gzip) from pattern_path, writes text pml_path / cid_path (NULL => pattern +
 * ".pml" / ".cid", pml_query.cpp:124-125) in the byte format of pml_to_vec
 * (pml_query.cpp:78-85).  `batch_bases` bounds the bases per GPU batch
 * (0 = default). */
int colbwt_query_file(colbwt_index *idx, const char *pattern_path, const char *pml_path,
                      const char *cid_path, uint64_t batch_bases, colbwt_stats *stats);

/* The same program writing the results as binary containers -- what `col-bwt query` produces
 * (scripts/col-bwt.py:194-198: PATTERN.split.pml.bin / .split.cid.bin, written there by the
 * un-vendored Movi fork).  Record shape as SURVEY.md 8(c) recalls it of upstream Movi -- "Movi-like,
 * UNVERIFIED", parity unpinned: per read  u16 name_len | name | u64 count | count values,
 * values in computation order (the read's last base first); u16 lengths (saturated at 65535) in
 * pml_bin_path (NULL => pattern + ".pml.bin"), u8 col ids in cid_bin_path (".cid.bin").  The text
 * files stay the bit-exact contract; this exists because formatting ~4 text bytes per base
 * bounds pml_query end to end. */
int colbwt_query_file_binary(colbwt_index *idx, const char *pattern_path, const char *pml_bin_path,
                             const char *cid_bin_path, uint64_t batch_bases, colbwt_stats *stats);
/* Container -> the reference's text (pml_query.cpp:78-85): `col-bwt view`.  value_bytes: 2 for
 * .pml.bin, 1 for .cid.bin.  Host code. */
int colbwt_binary_to_text(const char *bin_path, int value_bytes, const char *text_path);

/* ---- exact-match counting (backward search) ----------------------------------------------
 * How often does a read occur in the text, and how much of it?  Backward search over the same
 * table: for read P[0..m), start with the whole BWT range [sp, ep] = [0, n-1] and for
 * i = m-1 .. 0, c = P[i]: s = first position >= sp whose BWT character is c, e = last position
 * <= ep holding c; c absent from the table or s > e ends the search; else sp = LF(s), ep = LF(e)
 * (the move-structure step of the query above), and sp > ep afterwards (synthetic tables only)
 * ends it too without consuming the base.  Read bytes are compared exactly as the query compares
 * them.  Per read (not per base):
 *   mlen  bases consumed = the length of the longest suffix of the read that occurs in the text
 *         (mlen == m: the whole read occurs)
 *   occ   ep - sp + 1 of the last non-empty range = the occurrences of that suffix; 0 when mlen == 0
 *         (empty reads included)
 *   sp    (nullable) the first position of that range = the suffix's rank among the text's
 *         suffixes; 0 when mlen == 0
 * Works on every layout; needs nothing beyond what the open put in HBM.  Arguments, error codes,
 * stream and concurrency contract as colbwt_query_batch / colbwt_query_device_ordered: read k is
 * bases[read_off[k] .. read_off[k+1]), reads up to 2^32-1 bases; the host form shards the reads
 * over the replicas of a colbwt_index_open_devices handle.  Device form: d_bases 16-byte aligned
 * with 64 readable bytes past read_off[n_reads], d_mlen 4-byte and d_occ / d_sp 8-byte aligned,
 * d_order (nullable) assigns lanes as in colbwt_query_device_ordered (results identical). */
int colbwt_count_batch(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads,
                       uint32_t *mlen, uint64_t *occ, uint64_t *sp, colbwt_stats *stats);
int colbwt_count_device(colbwt_index *idx, const uint8_t *d_bases, const uint64_t *d_read_off, uint64_t n_reads,
                        uint64_t n_bases, uint32_t *d_mlen, uint64_t *d_occ, uint64_t *d_sp, const uint32_t *d_order,
                        void *hip_stream, colbwt_stats *stats);
/* FASTA/FASTQ(.gz) in (the reader and batch pipeline of colbwt_query_file), one text line per read
 * out: "name\tm\tmlen\tocc\n", name as colbwt_query_file prints it after '>'.  out_path NULL =>
 * pattern + ".count". */
int colbwt_count_file(colbwt_index *idx, const char *pattern_path, const char *out_path, uint64_t batch_bases,
                      colbwt_stats *stats);

/* ---- locate: text positions of each read's longest exact match ----------------------------
 * The backward search of colbwt_count_* with one exception: a read byte <= 1 ends the search (the
 * folded separator / terminator class, where the table's LF is not the text's).  On reads without
 * such a byte mlen and occ equal count's.  With k = min(occ, max_occ), the read's max_occ result
 * slots hold SA[ep], SA[ep-1], .., SA[ep-k+1]: the start positions in the indexed text of
 * occurrences of P[m-mlen..m), in suffix-array order from the range's last suffix down; the slots
 * past k hold COLBWT_LOCATE_NONE.  Every occurrence: colbwt_locate_all_* below.
 *
 * Samples: <prefix>.col_loc, written by the builder (colbwt_rlbwt_build_files_locate, build_rlbwt -L,
 * col-bwt build --locate); they cannot be rebuilt from a .col_pml.  Little-endian:
 *   header   u8 magic[8] "COLBWTLC" | u32 version = 1 | u32 n_docs | u64 n | u64 r | u64 s  (40 bytes)
 *   end_sa   u32[r]    SA at the last position of every folded run (bytes <= 1 one character, as in
 *                      .bwt.heads), in BWT order: r = the .col_pml's bwt_r
 *   phi      u32[2s]   pairs (SA[j], SA[j-1]) for every j >= 1 where the UNFOLDED BWT byte changes
 *                      (0 and 1 distinct), sorted by SA[j]; SA[j] = 0 is always among them
 *   docs     u32[n_docs]  doc_start: first text position of every document
 * phi(x) = SA[ISA[x]-1] = val(a) + (x - a) for a = the largest sampled position <= x.
 *
 * colbwt_index_attach_locate(_memory) loads the samples onto every replica of an open index (prefix +
 * ".col_loc", else the path itself).  It checks n and r against the table, that the table has exactly
 * r rows ending a run (the next row holds another character, or it is the last row), every value
 * < n and ascending phi positions.  HBM: 4 bytes per row of the layout in HBM + 12 to 16 bytes per
 * phi sample.  On failure no replica keeps samples; the index still answers query and count.
 * colbwt_locate_docs copies doc_start (cap entries of room; *n_docs receives their number).
 *
 * Entry points as colbwt_count_batch / colbwt_count_device (sharding over replicas, d_order,
 * alignment: d_pos 8-byte aligned), with max_occ in 1 .. 2^20 and pos / d_pos holding
 * n_reads * max_occ u64 slots (read k: [k * max_occ, (k+1) * max_occ)).
 * colbwt_locate_file: one text line per read "name\tm\tmlen\tocc\tdoc:offset,doc:offset,..\n"
 * (doc = 0-based document number in build order, offset = position - doc_start[doc]; the last field
 * is empty when occ == 0), out_path NULL => pattern + ".locate". */
#define COLBWT_LOCATE_NONE (~(uint64_t)0)
int colbwt_index_attach_locate(colbwt_index *idx, const char *prefix_or_file);
int colbwt_index_attach_locate_memory(colbwt_index *idx, const void *col_loc_bytes, uint64_t len);
int colbwt_locate_docs(const colbwt_index *idx, uint64_t *doc_start, uint32_t cap, uint32_t *n_docs);
int colbwt_locate_batch(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, uint32_t max_occ,
                        uint32_t *mlen, uint64_t *occ, uint64_t *pos, colbwt_stats *stats);
int colbwt_locate_device(colbwt_index *idx, const uint8_t *d_bases, const uint64_t *d_read_off, uint64_t n_reads,
                         uint64_t n_bases, uint32_t max_occ, uint32_t *d_mlen, uint64_t *d_occ, uint64_t *d_pos,
                         const uint32_t *d_order, void *hip_stream, colbwt_stats *stats);
int colbwt_locate_file(colbwt_index *idx, const char *pattern_path, const char *out_path, uint32_t max_occ,
                       uint64_t batch_bases, colbwt_stats *stats);

/* ---- locate-all: every occurrence of each read's longest exact match, as compressed sparse rows ----
 * colbwt_locate_* reports at most max_occ positions per read in n_reads * max_occ slots; here a read
 * gets exactly as many slots as it has positions: one offset array, one packed position array.  The
 * search is exactly colbwt_locate_*'s (a read byte <= 1 ends it); mlen and occ are reported for every
 * read.  Parameters min_len >= 1 and max_per_read, where 0 means no cap; locate samples must be attached.
 *   walked   w = occ (min(occ, max_per_read) when max_per_read != 0) when mlen >= min_len, else w = 0.
 *   pos_off  n_reads + 1 u64 entries: pos_off[0] = 0, pos_off[k+1] = pos_off[k] + w_k.
 *   pos      read k owns pos[pos_off[k] .. pos_off[k+1]): SA[ep], SA[ep-1], .., SA[ep-w+1] as u64 --
 *            locate's order, so the first min(w, K) entries equal what colbwt_locate_batch returns at
 *            max_occ = K.  No slot holds COLBWT_LOCATE_NONE.
 * The output is deterministic: every slot has one writer and no atomics are involved.
 *
 * On the device the work is split in two.  colbwt_locate_all_plan_device runs the search and two scans:
 * it fills d_mlen, d_occ (n_reads entries) and d_pos_off (n_reads + 1), and leaves per-read state (the
 * BWT position of ep, SA[ep], tile offsets) in d_work: 256-byte aligned,
 * colbwt_locate_all_work_bytes(n_reads) bytes, a function of n_reads alone.  It is asynchronous on
 * `hip_stream` unless `total` or `stats` is given; with `total` (host, nullable) it synchronises the
 * stream and stores pos_off[n_reads], the size the position array needs.  colbwt_locate_all_fill_device
 * then walks the positions of the reads [read_lo, read_hi) of that batch into d_pos[0 ..): slot 0 is
 * pos[pos_off[read_lo]], so a caller with little memory fills in pieces.  It must find d_work and
 * d_pos_off as the plan left them, allocates nothing, reads its bounds from device memory (no host
 * read-back) and runs a grid of fixed size whose lanes stride over the range's tiles: a read's range
 * is cut into tiles of colbwt_locate_all_tile() positions (256 unless the library was built otherwise),
 * each restarted from the SA sample at the nearest end of a BWT run at or below its start and walked
 * by one lane, so one read of a million occurrences is thousands of short walks and not one long one.
 * Nothing at or past d_pos[pos_cap] is ever written: the kernel guards every store, and a range that
 * needs more than pos_cap slots is cut off there without an error (size d_pos from pos_off).  Several
 * fills of one plan may be in flight at once.  Arguments, alignment (d_pos_off / d_pos 8-byte), error
 * codes and d_order (search only) as colbwt_locate_device / colbwt_docs_device; "no locate samples
 * attached" is COLBWT_ERR_ARG; the fill addresses the replica on d_work's device.  kernel_ms of the plan
 * covers the search and the scans, kernel_ms of the fill the walk.  Fewer than 2^32-1 reads per call.
 *
 * colbwt_locate_all_batch: reads in host memory, sharded over the replicas as colbwt_locate_batch
 * shards them; the shards' offsets are rebased on the host.  mlen, occ and pos_off are filled whenever
 * the search ran.  When pos_off[n_reads] > pos_cap the call returns COLBWT_ERR_ARG ("pos_cap too
 * small") with those three filled and pos untouched (pos may be NULL with pos_cap 0): the sizing
 * convention of colbwt_build_col_pml_arrays.  kernel_ms is the sum of plan and fill.
 * colbwt_locate_all_file: FASTA/FASTQ(.gz) in, the lines of colbwt_locate_file out
 * ("name\tm\tmlen\tocc\tdoc:offset,..\n") with all w positions of every read (the last field is empty
 * when w == 0); out_path NULL => pattern + ".locate".  It plans a batch of batch_bases bases (0: 64 M) on
 * the handle's first replica, then fills, copies and writes it in read ranges, so that it never holds
 * more than COLBWT_LOCATE_ALL_FILE_POSITIONS positions at once; a single read with more fails with
 * COLBWT_ERR_NOMEM and a message that names max_per_read. */
#define COLBWT_LOCATE_ALL_FILE_POSITIONS ((uint64_t)1 << 24)
uint32_t colbwt_locate_all_tile(void);
uint64_t colbwt_locate_all_work_bytes(uint64_t n_reads);
int colbwt_locate_all_plan_device(colbwt_index *idx, const uint8_t *d_bases, const uint64_t *d_read_off, uint64_t n_reads,
                                  uint64_t n_bases, uint32_t min_len, uint64_t max_per_read, uint32_t *d_mlen, uint64_t *d_occ,
                                  uint64_t *d_pos_off, void *d_work, const uint32_t *d_order, void *hip_stream, uint64_t *total,
                                  colbwt_stats *stats);
int colbwt_locate_all_fill_device(colbwt_index *idx, uint64_t n_reads, uint64_t read_lo, uint64_t read_hi, const uint64_t *d_pos_off,
                                  uint64_t *d_pos, uint64_t pos_cap, const void *d_work, void *hip_stream, colbwt_stats *stats);
int colbwt_locate_all_batch(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, uint32_t min_len,
                            uint64_t max_per_read, uint32_t *mlen, uint64_t *occ, uint64_t *pos_off, uint64_t *pos, uint64_t pos_cap,
                            colbwt_stats *stats);
int colbwt_locate_all_file(colbwt_index *idx, const char *pattern_path, const char *out_path, uint32_t min_len, uint64_t max_per_read,
                           uint64_t batch_bases, colbwt_stats *stats);

/* ---- anchors: left-maximal exact matches along the whole read --------------------------------
 * colbwt_count_* / colbwt_locate_* answer for one stretch of the read, its longest matching suffix.
 * Here the search restarts instead of ending: the anchors of read P[0..m) are the greedy right-to-left
 * factorisation of the read against the text, defined through the search colbwt_locate_* specifies.
 * Parameters min_len >= 1, max_anchors in 1 .. 2^16, max_occ in 0 .. 2^20.
 *   e = m - 1
 *   while e >= 0:
 *     (L, occ, [sp, ep]) = locate's search on the prefix P[0..e]: the longest suffix of P[0..e] that
 *                          occurs; a byte <= 1 or a character absent from the table ends it
 *     if L == 0:  skipped += 1; e -= 1                    (this base lies in no match)
 *     else:       factor (start = e - L + 1, len = L, occ, positions SA[ep], SA[ep-1], ..); e -= L
 *   left-maximal  a factor cannot be extended to the left: the base in front of it is the one that
 *            failed, or the read starts there.  The base that failed is the last base of the next
 *            factor: it is retried from the full range, not dropped.
 *   progress on a synthetic table the full-range retry of a present character may still come back empty
 *            (sp > ep after LF): that is L == 0 and the base is skipped, so the loop advances on every
 *            validated table.
 *   factor 0 when colbwt_locate_* reports mlen > 0 for the read, factor 0 is locate's answer:
 *            start = m - mlen, and len, occ and the first min(occ, max_occ) positions in the same order.
 *   bound    the greedy parse is the partition of the non-skipped bases into the FEWEST substrings of
 *            the text (each greedy factor reaches at least as far left as any other parse's factor
 *            that ends at or right of the same base).  A read within d substitutions of a text substring
 *            splits into at most d + 1 substrings of the text and d single bases, each of which is a
 *            factor or skipped, so n_factors + skipped <= 2d + 1: n_factors is a lower bound on mismatches.
 *   summary  colbwt_anchor_summary, eight u32, written for every read:
 *     n_factors   all factors (len >= 1)
 *     max_len     longest factor, whatever min_len is
 *     skipped     bases in no factor; sum(len over all factors) + skipped == m
 *     n_kept      factors with len >= min_len: the anchors
 *     cov         sum of len over anchors; with min_len == 1, cov + skipped == m
 *     n_unique    anchors with occ == 1
 *     cov_unique  sum of len over anchors with occ == 1
 *     n_stored    min(n_kept, max_anchors)
 *   slots    a read's anchors in computation order -- largest start first, the order of the binary
 *            containers and of seeds; the first n_stored fill the read's max_anchors slots: read k owns
 *            [k * max_anchors, (k+1) * max_anchors) of anchor_start (u32), anchor_len (u32), anchor_occ
 *            (u64), and slot s owns anchor_pos[s * max_occ, (s+1) * max_occ) (u64): SA[ep], SA[ep-1], ..,
 *            the first min(occ, max_occ) in locate's order.  Unused slots hold COLBWT_ANCHOR_NONE, 0 and
 *            0; every position entry past min(occ, max_occ), in used and unused slots alike, holds
 *            COLBWT_LOCATE_NONE.  Factors shorter than min_len are counted in the summary and never walked.
 *   max_occ == 0  no positions are produced, anchor_pos is NULL and the mode needs NO locate samples;
 *            every other output is identical with and without samples.  With max_occ >= 1 samples must
 *            be attached ("no locate samples attached" is COLBWT_ERR_ARG, as for locate).
 * The output is deterministic: every slot has one writer and no atomics are involved.  There are no
 * per-base arrays: the per-base restart-at-zero matching length is a function of the factors (e - k + 1
 * at base k of a factor whose last base is e, 0 on a skipped base).  Interior factors are left-maximal but
 * not necessarily right-maximal, so these are NOT super-maximal exact matches.
 *
 * colbwt_anchors_device: arguments, stream, stats, d_order and the concurrency contract as
 * colbwt_locate_device; it allocates nothing and initialises every slot itself.  d_bases 16-byte aligned
 * with 64 readable bytes past read_off[n_reads], d_summary 16-byte, d_start / d_len 4-byte, d_occ / d_pos
 * 8-byte aligned.  d_start, d_len and d_occ may all be NULL together (summaries only; d_pos NULL too);
 * d_pos must be non-NULL exactly when the slots are given and max_occ > 0.  Fewer than 2^32-1 reads per
 * call, reads up to 2^32-1 bases.
 * colbwt_anchors_batch: reads in host memory, sharded over the replicas as colbwt_locate_batch shards
 * them; the same rule for the slot pointers.
 * colbwt_anchors_file: FASTA/FASTQ(.gz) in (the reader and batch pipeline of colbwt_locate_file), one
 * line per read "name\tm\tn_factors\tn_kept\tcov\tmax_len\tskipped\tn_unique\tcov_unique\tA,A,..\n", A =
 * "start:len:occ" followed by "@doc:offset" for each stored position (doc and offset as
 * colbwt_locate_file prints them), e.g. "120:30:2@0:1543@3:88,95:24:1@1:7"; the last field is empty when
 * nothing is stored; out_path NULL => pattern + ".anchors"; batch_bases 0 is colbwt_query_file's default,
 * cut by the slot bytes per read as colbwt_locate_file cuts it by max_occ. */
#define COLBWT_ANCHOR_NONE 0xFFFFFFFFu
typedef struct colbwt_anchor_summary {
    uint32_t n_factors, max_len, skipped, n_kept, cov, n_unique, cov_unique, n_stored;
} colbwt_anchor_summary;
int colbwt_anchors_device(colbwt_index *idx, const uint8_t *d_bases, const uint64_t *d_read_off, uint64_t n_reads, uint64_t n_bases,
                          uint32_t min_len, uint32_t max_anchors, uint32_t max_occ, colbwt_anchor_summary *d_summary,
                          uint32_t *d_start, uint32_t *d_len, uint64_t *d_occ, uint64_t *d_pos, const uint32_t *d_order,
                          void *hip_stream, colbwt_stats *stats);
int colbwt_anchors_batch(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, uint32_t min_len,
                         uint32_t max_anchors, uint32_t max_occ, colbwt_anchor_summary *summary, uint32_t *anchor_start,
                         uint32_t *anchor_len, uint64_t *anchor_occ, uint64_t *anchor_pos, colbwt_stats *stats);
int colbwt_anchors_file(colbwt_index *idx, const char *pattern_path, const char *out_path, uint32_t min_len, uint32_t max_anchors,
                        uint32_t max_occ, uint64_t batch_bases, colbwt_stats *stats);

/* ---- chain: the best colinear chain of each read's anchors, reduced on the device ------------
 * colbwt_anchors_* says which stretches of a read occur and where; this joins them: one locus per
 * read with a score and a runner-up, 32 bytes per read instead of the slot arrays.
 *   inputs   the slot arrays of colbwt_anchors_* for one read: anchor_start[K], anchor_len[K],
 *            anchor_pos[K * M], K = max_anchors, M = max_occ >= 1, and a u32 parameter band.  The arrays
 *            are taken as given: any arrays of that shape do, positions are not validated.
 *   hits     slot a is USED iff anchor_start[a] != COLBWT_ANCHOR_NONE.  A hit is (a, s = anchor_start[a],
 *            l = anchor_len[a], t = anchor_pos[a * M + q]) for a used slot and every q < M with
 *            anchor_pos[a * M + q] != COLBWT_LOCATE_NONE.  Hits are numbered 0 .. H-1 by (a, q) ascending;
 *            on the output of anchors that is right to left in the read.  doc(t) is the document of t
 *            under the attached samples' doc_start: the last d with doc_start[d] <= t, the rule of docs.
 *   transition  hit j may precede hit i iff  j < i and a_j < a_i;  gr = s_j - (s_i + l_i) >= 0;
 *            gt = t_j - (t_i + l_i) >= 0;  doc(t_i) == doc(t_j);  drift = |gt - gr| <= band.
 *            gr and gt are signed 64-bit (t_i + l_i and the difference are taken modulo 2^64, then read
 *            as signed; s_i + l_i does not wrap).
 *   score    f(i) = l_i + max(0, max over j of (f(j) - drift(j, i))): a predecessor is taken only when
 *            f(j) - drift > 0, and among equal candidates the smallest j wins.  f is computed in signed
 *            64-bit and stored saturated to u32 (2^32-1); later hits see the stored value.
 *   best chain  ends at the hit e with the largest f, the smallest e among equals; following the
 *            predecessors back leads to its first hit b, the rightmost in the read.
 *              read_begin = s_e            read_end = s_b + l_b (modulo 2^32)
 *              text_begin = t_e            text_end = t_b + l_b (modulo 2^64)
 *              text_len   = text_end - text_begin, saturated to u32
 *              score = f(e)    n_chained = hits on the path    n_hits = H
 *   runner-up  score2 is the largest f of the same dynamic program run again over the hits that lie
 *            outside the best chain's text interval -- t + l <= text_begin or t >= text_end -- in their
 *            order; 0 when there are none.  It is the best alternative locus: score - score2 is what a
 *            caller turns into a mapping quality.
 *   no hits  text_begin = COLBWT_LOCATE_NONE and every other field is 0.
 *   limits   1 <= max_anchors, 1 <= max_occ, max_anchors * max_occ <= 256; anything else is
 *            COLBWT_ERR_ARG with a message.  Locate samples must be attached ("no locate samples attached"
 *            is COLBWT_ERR_ARG, as for locate), with at most 4096 documents, as for docs.
 *   out of scope  a chain never joins two documents.  Records, and the reverse-complement half, inside one
 *            document are not told apart, because .col_loc holds no record table: the position is a text
 *            position, printed as doc:offset the way locate prints it.  No base-level alignment, no
 *            SAM/PAF, no strand field.
 * The output is deterministic: every word has one writer and no atomics are involved.
 *
 * colbwt_chain_reduce_device: the reduction alone, over device arrays that a colbwt_anchors_device call
 * filled (or any arrays of that shape): d_start / d_len n_reads * max_anchors u32 (4-byte aligned), d_pos
 * n_reads * max_anchors * max_occ u64 (8-byte aligned), d_chain n_reads records (16-byte aligned).  Stream,
 * stats and the concurrency contract as colbwt_anchors_device; the replica is the one on d_pos's device.
 * It allocates nothing.  Fewer than 2^32-1 reads per call.
 * colbwt_chain_device: anchors (min_len, max_anchors, max_occ; d_bases, d_read_off, d_order as
 * colbwt_anchors_device) into the caller's scratch d_work -- colbwt_chain_work_bytes(n_reads, max_anchors,
 * max_occ) bytes, 256-byte aligned -- then the reduction, on one stream.  The scratch holds the anchors'
 * summary, start, len, occ and pos arrays, each starting at a multiple of 256 bytes, in that order.
 * colbwt_chain_batch: reads in host memory, sharded over the replicas as colbwt_anchors_batch shards
 * them; only the records come back.
 * colbwt_chain_file: FASTA/FASTQ(.gz) in, one line per read
 * "name\tm\tread_begin\tread_end\tdoc\toffset\ttext_len\tscore\tscore2\tn_chained\tn_hits\n" (doc and offset of
 * text_begin as colbwt_locate_file prints them; both "*" when there is no chain); out_path NULL =>
 * pattern + ".chains"; batch_bases 0 is colbwt_anchors_file's default. */
typedef struct colbwt_chain {
    uint64_t text_begin;
    uint32_t text_len, read_begin, read_end, score, score2;
    uint16_t n_chained, n_hits;
} __attribute__((aligned(16))) colbwt_chain;
uint64_t colbwt_chain_work_bytes(uint64_t n_reads, uint32_t max_anchors, uint32_t max_occ);
int colbwt_chain_reduce_device(colbwt_index *idx, const uint32_t *d_start, const uint32_t *d_len, const uint64_t *d_pos,
                               uint64_t n_reads, uint32_t max_anchors, uint32_t max_occ, uint32_t band, colbwt_chain *d_chain,
                               void *hip_stream, colbwt_stats *stats);
int colbwt_chain_device(colbwt_index *idx, const uint8_t *d_bases, const uint64_t *d_read_off, uint64_t n_reads, uint64_t n_bases,
                        uint32_t min_len, uint32_t max_anchors, uint32_t max_occ, uint32_t band, colbwt_chain *d_chain, void *d_work,
                        const uint32_t *d_order, void *hip_stream, colbwt_stats *stats);
int colbwt_chain_batch(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, uint32_t min_len,
                       uint32_t max_anchors, uint32_t max_occ, uint32_t band, colbwt_chain *chain, colbwt_stats *stats);
int colbwt_chain_file(colbwt_index *idx, const char *pattern_path, const char *out_path, uint32_t min_len, uint32_t max_anchors,
                      uint32_t max_occ, uint32_t band, uint64_t batch_bases, colbwt_stats *stats);

/* ---- seeds: per-read PML peaks and chain summaries, reduced on the device -----------------
 * What read classification consumes of a query's output, so that tens of bytes per read leave the
 * device instead of 3 bytes per base.  The reference has no such mode; these semantics are this
 * project's own.  Read P[0..m) has values pml[k] and cid[k] as colbwt_query_* produces them;
 * parameters min_len >= 1 and max_seeds in 1 .. 2^16.
 *   run      a maximal stretch [k, e) of consecutive bases of ONE read with pml >= 1 (runs never
 *            cross a read boundary).  On a query's output e - k == pml[k]: PML counts up by one
 *            towards smaller k and restarts at 0; the definition does not assume it.
 *   seed     of a run: (pos = k, len = pml[k], id), id = cid[j] for the smallest j in [k, e) with
 *            cid[j] != 0, else 0 -- the col id met closest to the peak, i.e. last in the order the
 *            query computes.  A seed COUNTS when len >= min_len.
 *   summary  per read, over ALL counting seeds (not only the stored ones):
 *     n_seeds  number of counting seeds
 *     max_len  largest pml value of the read, whatever min_len is
 *     cov      sum of len over counting seeds
 *     resets   number of bases with pml == 0
 *     n_col    number of counting seeds with id != 0
 *     col_cov  sum of len over counting seeds with id != 0
 *     asc, desc  over pairs of counting seeds with id != 0 that are neighbours in read order: with a
 *              the id at the smaller pos, b at the larger and d = (b - a + 255) % 255, d in 1..127
 *              counts in asc, 128..254 in desc, 0 in neither.  Col ids are binned cyclically into
 *              1..255 (col_split.hip: bin_id), so a wrap-around step still counts as ascending.
 *            Sums are taken modulo 2^32; on a query's output cov <= m, so nothing wraps.
 *   slots    a read's counting seeds in computation order -- largest pos first, the order of the
 *            binary containers; the first min(n_seeds, max_seeds) of them fill the read's max_seeds
 *            slots of seed_pos (u32), seed_len (u32), seed_cid (u8): read k owns
 *            [k * max_seeds, (k+1) * max_seeds).  Unused slots hold COLBWT_SEED_NONE, 0 and 0.
 * On a query's output: with min_len == 1, cov + resets == m; n_seeds <= resets + 1; max_len equals
 * the largest stored len when min_len == 1 (and max_seeds >= n_seeds).
 *
 * colbwt_seeds_reduce_device is the reduction alone, over device buffers a colbwt_query_device call
 * filled (d_pml of pml_bytes 2 or 4, d_cid, d_read_off; any arrays of that shape do); it needs no
 * index and runs on the current device, which must hold the buffers.  d_pml and d_summary 16-byte
 * aligned, d_cid 8-byte, d_seed_pos / d_seed_len 4-byte; the three slot arrays may all be NULL when
 * only summaries are wanted.  Fewer than 2^32-1 reads per call, reads up to 2^32-1 bases.
 * Asynchronous on `hip_stream` unless `stats` is given (then kernel_ms is its time).  The output is
 * deterministic: no atomics are involved.
 * colbwt_seeds_batch: reads in host memory as colbwt_query_batch takes them; the query (u16 PML, or
 * u32 when a read is longer than 65535) and the reduction run on the device and only summaries and
 * slots come back (seed_pos / seed_len / seed_cid all NULL: summaries only).  Sharded over the
 * replicas of a colbwt_index_open_devices handle.  kernel_ms covers query + reduction.
 * colbwt_seeds_file: FASTA/FASTQ(.gz) in (the reader and batch pipeline of colbwt_count_file), one
 * line per read "name\tm\tn_seeds\tcov\tmax_len\tresets\tn_col\tcol_cov\tasc\tdesc\tpos:len:id,..\n"
 * (the stored seeds; the last field is empty when there are none); out_path NULL => pattern + ".seeds". */
#define COLBWT_SEED_NONE 0xFFFFFFFFu
typedef struct colbwt_seed_summary {
    uint32_t n_seeds, max_len, cov, resets, n_col, col_cov, asc, desc;
} colbwt_seed_summary;
int colbwt_seeds_reduce_device(const void *d_pml, int pml_bytes, const uint8_t *d_cid, const uint64_t *d_read_off, uint64_t n_reads,
                               uint64_t n_bases, uint32_t min_len, uint32_t max_seeds, colbwt_seed_summary *d_summary,
                               uint32_t *d_seed_pos, uint32_t *d_seed_len, uint8_t *d_seed_cid, void *hip_stream,
                               colbwt_stats *stats);
int colbwt_seeds_batch(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, uint32_t min_len,
                       uint32_t max_seeds, colbwt_seed_summary *summary, uint32_t *seed_pos, uint32_t *seed_len, uint8_t *seed_cid,
                       colbwt_stats *stats);
int colbwt_seeds_file(colbwt_index *idx, const char *pattern_path, const char *out_path, uint32_t min_len, uint32_t max_seeds,
                      uint64_t batch_bases, colbwt_stats *stats);

/* ---- docs: the documents holding each read's longest exact match ---------------------------
 * "Which genomes contain this read?", answered on the device: locate's search, then a walk over the
 * occurrences that keeps only the DOCUMENT of each, so that a bit mask per read and a tally per batch
 * leave the device instead of max_occ positions per read.  The reference has no such mode; these
 * semantics are this project's own.  Parameters min_len >= 1 and max_walk in 1 .. 2^20; locate samples
 * must be attached (colbwt_index_attach_locate); n_docs and doc_start are the attached .col_loc's
 * (colbwt_locate_docs), at most 4096 documents (more are an argument error of the three entry
 * points, checked right after the samples), W = ceil(n_docs / 64) = colbwt_docs_mask_words (0 when no samples are attached).
 *   search   exactly colbwt_locate_*'s: a read byte <= 1 ends it.  mlen and occ are as locate defines
 *            them and are reported for every read, whatever min_len is.
 *   walked   w = min(occ, max_walk) when mlen >= min_len, otherwise w = 0.  The walked positions are
 *            locate's first w: SA[ep], SA[ep-1], .., SA[ep-w+1].
 *   mask     read k owns the u64 words [k * W, (k+1) * W).  Bit d & 63 of word d >> 6 is set iff a walked
 *            position p has doc_start[d] <= p and (d == n_docs-1 or p < doc_start[d+1]): an occurrence
 *            belongs to the document its first character lies in.  Bits at or above n_docs are 0.
 *   n_hit    (u32) the number of set bits.  A read's set is complete iff occ <= max_walk or
 *            n_hit == n_docs (the walk may stop once n_hit == n_docs: that cannot change an output).
 *   tally    doc_reads[d] counts the reads whose mask has bit d, doc_only[d] the reads with n_hit == 1
 *            and bit d (both nullable, u64[n_docs]).  The device entry point ADDS to what the arrays
 *            hold, so a caller accumulates over batches; the host entry point writes the totals of its
 *            call.  Integer adds: the result does not depend on their order.
 *
 * Arguments, error codes, sharding over replicas, stream and stats as colbwt_locate_batch / _device /
 * _file ("no locate samples attached" is an argument error); kernel_ms covers every stage (search,
 * order, walk, tally).  Device form: allocates nothing; d_work must be 256-byte aligned and hold
 * colbwt_docs_work_bytes(n_reads) bytes, and calls in flight at once need distinct work buffers.
 * d_mask and the tallies 8-byte aligned, d_n_hit 4-byte; fewer than 2^32-1 reads per call; d_order
 * (nullable) is advisory and goes to the search stage only -- the walk runs over the reads sorted by w.
 * The host form takes its scratch as colbwt_locate_batch does and sums the shards' tallies on the host.
 * colbwt_docs_file: FASTA/FASTQ(.gz) in (the reader and batch pipeline of colbwt_locate_file), one
 * line per read "name\tm\tmlen\tocc\tn_hit\td,d,..\n" (document numbers ascending; the last field is
 * empty when n_hit == 0), out_path NULL => pattern + ".docs"; after the last batch <out>.tally, one
 * line "d\tdoc_reads\tdoc_only\n" per document; batch_bases 0 is colbwt_query_file's default, cut by
 * W / 16 when W > 16 as colbwt_locate_file cuts it by max_occ.  A failing colbwt_docs_batch leaves
 * doc_reads / doc_only as they were. */
uint32_t colbwt_docs_mask_words(const colbwt_index *idx);
uint64_t colbwt_docs_work_bytes(uint64_t n_reads);
int colbwt_docs_batch(colbwt_index *idx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, uint32_t min_len,
                      uint32_t max_walk, uint32_t *mlen, uint64_t *occ, uint32_t *n_hit, uint64_t *mask, uint64_t *doc_reads,
                      uint64_t *doc_only, colbwt_stats *stats);
int colbwt_docs_device(colbwt_index *idx, const uint8_t *d_bases, const uint64_t *d_read_off, uint64_t n_reads, uint64_t n_bases,
                       uint32_t min_len, uint32_t max_walk, uint32_t *d_mlen, uint64_t *d_occ, uint32_t *d_n_hit, uint64_t *d_mask,
                       uint64_t *d_doc_reads, uint64_t *d_doc_only, void *d_work, const uint32_t *d_order, void *hip_stream,
                       colbwt_stats *stats);
int colbwt_docs_file(colbwt_index *idx, const char *pattern_path, const char *out_path, uint32_t min_len, uint32_t max_walk,
                     uint64_t batch_bases, colbwt_stats *stats);

/* ---- index construction (SURVEY.md 8(f) "next" #1) ------------------------ */

/* build_col_bwt <prefix> (src/build_col_bwt.cpp:14-52): reads <prefix>.bwt.heads,
 * .bwt.len, .col_ids, .col_runs (plain sdsl::bit_vector as col_split writes it,
 * col_split.hpp:384-386), .thr_pos and writes <prefix>.col_pml (or out_path)
 * exactly as col_pml(heads, lengths, col_ids, thresholds, splits) + serialize
 * would (col_bwt.hpp:124-230, 391-395, 440-457, 360-370).  Host code. */
int colbwt_build_col_pml(const char *prefix, const char *out_path);
/* Same over decoded arrays: split_pos = ascending positions of the set bits of
 * .col_runs; lens / thr_pos already widened from 5 bytes.  *out_len receives
 * the image size (also when out is NULL / too small, then ERR_ARG). */
int colbwt_build_col_pml_arrays(const uint8_t *heads, uint64_t n_heads, const uint64_t *lens,
                                const uint8_t *col_ids, uint64_t n_ids, const uint64_t *split_pos,
                                uint64_t n_splits, const uint64_t *thr_pos, uint64_t n_thr, void *out,
                                uint64_t out_cap, uint64_t *out_len);

/* ---- sub-run splitting (SURVEY.md 8(f) "next" #2) -------------------------- */

/* build_FL + col_split (src/build_FL.cpp:27-74, src/col_split.cpp:62-140; include/ds/FL_table.hpp,
 * include/col_split.hpp): multi-MUMs -> where sub-runs start and their chain statistic.
 * `col_split <prefix> -m tunnels|all -s <rate>`: reads <prefix>.bwt.heads, .bwt.len and .col_mums
 * (5-byte num_docs, then 5-byte (length, position) pairs; position = rank in F / suffix-array
 * order of the first of num_docs consecutive suffixes, ascending), writes <prefix>.col_runs (a plain
 * sdsl::bit_vector: u64 length in bits + words) and <prefix>.col_ids (one byte per set bit) --
 * the inputs of colbwt_build_col_pml.  The FL table is rebuilt from the RLBWT instead of read from
 * the reference's .FL_table file (which embeds an sdsl sd_vector).  Every multi-MUM is FL-stepped on
 * the device (the reference steps them one after the other, twice); the overlap sweep
 * (find_col_runs, col_split.hpp:258-342) runs on the host.  The reference's -o overlap option is
 * parsed there but never used (col_split.hpp:215), so it has no counterpart.  `all` mode: up to
 * 1024 documents.  Needs 4 (tunnels) or 8 (all) bytes of HBM per BWT position. */
#define COLBWT_SPLIT_TUNNELS 0
#define COLBWT_SPLIT_ALL 1
int colbwt_col_split(const char *prefix, int mode, int split_rate, int device);
/* Same over decoded arrays; results as colbwt_build_col_pml_arrays takes them: split_pos = the
 * ascending positions of the set bits of .col_runs (room for `cap`), col_ids one byte each,
 * *n_split their number (also when the arrays are too small, then ERR_ARG), *bwt_len = n. */
int colbwt_col_split_arrays(const uint8_t *heads, uint64_t n_heads, const uint64_t *lens, const uint64_t *mum_len,
                            const uint64_t *mum_pos, uint64_t n_mums, uint32_t num_docs, int mode, int split_rate,
                            int device, uint64_t *split_pos, uint64_t cap, uint64_t *n_split, uint8_t *col_ids,
                            uint64_t *bwt_len);
const char *colbwt_col_split_error(void);

/* ---- RLBWT, thresholds and multi-MUMs from FASTA (SURVEY.md 8(f) "next" #4) ---- */

/* What the reference's driver takes from `mumemto mum -K -R -T -l <min> [-r]` (scripts/col-bwt.py:
 * 121-145): <prefix>.bwt.heads (one character per BWT run), .bwt.len (5-byte run lengths),
 * .thr_pos (5-byte threshold position per run, col_bwt.hpp:446-448) and .col_mums (5-byte num_docs,
 * then 5-byte (length, position) pairs, col_split.cpp:90-106) -- the inputs of colbwt_col_split and
 * colbwt_build_col_pml.  mumemto itself is an un-vendored dependency, so its conventions are
 * restated here and UNVERIFIED against it ("parity unpinned"):
 *   text        every record of every file as it is + separator 1 (+ its reverse complement + 1 when
 *               `revcomp`; one document per file), then one final 0; suffixes compare byte-wise
 *   runs        maximal stretches of equal characters with every byte <= 1 (the final 0, the
 *               separators) taken as ONE character, head 1 -- the class the reference folds them to
 *               when it reads .bwt.heads (col_bwt.hpp:167-171) and groups thresholds by
 *               (col_bwt.hpp:446-451): entry k of .thr_pos belongs to group k of the builder
 *   threshold   first position of the minimum LCP in (end of the previous run of the character,
 *               head of this run]; 0 for a character's first run.  LCPs are cut at the first
 *               separator: what lies behind one can never be matched by a pattern
 *   multi-MUM   num_docs consecutive suffixes, one from every document, that share >= min_mum
 *               characters (never across a separator), more than with either neighbouring suffix,
 *               and are not all preceded by the same character; position = suffix-array rank of
 *               the first, length = the shared prefix
 * The suffix array (prefix doubling over rocPRIM radix sorts), the LCP array, the runs, the
 * thresholds and the multi-MUM scan all run on the device.  Text < 2^32-1 characters, <= 4096
 * documents; HBM 29 bytes per character + 4 per doubling round. */
typedef struct colbwt_rlbwt colbwt_rlbwt;
typedef struct colbwt_rlbwt_view {
    uint64_t n;        /* BWT length */
    uint64_t n_runs;
    uint64_t n_mums;
    uint32_t n_docs;
    int32_t rounds;    /* prefix-doubling rounds the suffix sort took */
    const uint8_t *heads;      /* n_runs */
    const uint64_t *lens;      /* n_runs */
    const uint64_t *thr_pos;   /* n_runs */
    const uint64_t *mum_len;   /* n_mums */
    const uint64_t *mum_pos;   /* n_mums, ascending */
} colbwt_rlbwt_view;
/* text[0..n): separators 1 in place, text[n-1] its only 0; doc_start[d] = first character of
 * document d, ascending from 0. */
int colbwt_rlbwt_build_text(const uint8_t *text, uint64_t n, const uint64_t *doc_start, uint32_t n_docs,
                            uint64_t min_mum, int device, colbwt_rlbwt **out);
/* FASTA/FASTQ(.gz) files, one document each; writes the four files when out_prefix is not NULL,
 * hands the result back when `out` is not NULL. */
int colbwt_rlbwt_build_files(const char *const *fastas, uint32_t n_files, int revcomp, uint64_t min_mum, int device,
                             const char *out_prefix, colbwt_rlbwt **out);
/* The same builds that also gather the locate samples (colbwt_locate_*) on the device: end_sa at the
 * run ends and the phi pairs, sorted by position.  _files writes <out_prefix>.col_loc beside the
 * four files; colbwt_rlbwt_write_locate writes the .col_loc of a handle built by either (ERR_ARG for
 * a handle built without samples). */
int colbwt_rlbwt_build_text_locate(const uint8_t *text, uint64_t n, const uint64_t *doc_start, uint32_t n_docs,
                                   uint64_t min_mum, int device, colbwt_rlbwt **out);
int colbwt_rlbwt_build_files_locate(const char *const *fastas, uint32_t n_files, int revcomp, uint64_t min_mum, int device,
                                    const char *out_prefix, colbwt_rlbwt **out);
int colbwt_rlbwt_write_locate(const colbwt_rlbwt *h, const char *path);
void colbwt_rlbwt_get(const colbwt_rlbwt *h, colbwt_rlbwt_view *view);   /* pointers live until _free */
void colbwt_rlbwt_free(colbwt_rlbwt *h);
const char *colbwt_rlbwt_error(void);

/* ---- multi-GPU gather codec (the path's one exchange step) -----------------
 * The reference has no counterpart: its reads are processed by one process
 * (pml_query.cpp:74).  With the reads sharded over N GPUs the per-base results
 * are gathered on rank 0; the PML values of a read are determined by where
 * they are zero (length + 1 per match, 0 at a mismatch: col_bwt.hpp:516-521),
 * so a rank sends one bit per base and rank 0 rebuilds the 16-bit values
 * (the col ids: see colbwt_cid_pack_device below).
 * Device pointers; masks are uint32 words, bit b of word w = base 32w + b of
 * the rank's concatenated reads; all calls are asynchronous on `hip_stream`.
 *   pack     d_mask[(n_bases+31)/32] <- (d_pml[k] == 0); d_pml 32-byte aligned
 *   end mask bit (read_off[r+1]-1) set for every non-empty read; d_mask must be
 *            zeroed by the caller, (n_bases+31)/32 words
 *   unpack   rebuilds d_pml[32*first_word .. 32*(first_word+n_words)) from the
 *            zero mask and the end mask (both total_words long; the range must
 *            end at a read end or at total_words); d_pml needs room for whole
 *            32-value blocks and 64-byte alignment */
int colbwt_pml_pack_device(const uint16_t *d_pml, uint64_t n_bases, uint32_t *d_mask, void *hip_stream);
/* The col ids of the results are ids that rows of the table hold (col_bwt.hpp:513), and every rank
 * holds the same table: they travel as codes of that dictionary, colbwt_cid_code_bits(n_ids) =
 * max(1, ceil(log2(n_ids))) bits per base -- the same on every rank, so the gathers keep equal,
 * known sizes -- laid out as bit planes: `bits` words per 32 bases, word p = bit p of the 32 codes.
 * 7 distinct ids (the C2 index): 3 bits, so results travel at 0.5 bytes per base instead of 3.
 *   dictionary  ids[0 .. *n_ids) <- the distinct col ids of the table's rows, ascending (ids: 256 bytes)
 *   pack        d_planes[bits * (n_bases+31)/32] <- codes of d_cid[0 .. n_bases) (16-byte aligned);
 *               `ids` is a HOST array (the dictionary), an id outside it packs as code 0
 *   unpack      d_cid[32*first_word .. 32*(first_word+n_words)) <- ids of the codes in the planes of
 *               those words (d_planes is the whole array: word w's planes at d_planes[bits * w]);
 *               d_cid 32-byte aligned with room for whole 32-id blocks */
int colbwt_index_cid_dictionary(const colbwt_index *idx, uint8_t *ids, uint32_t *n_ids);
uint32_t colbwt_cid_code_bits(uint32_t n_ids);
int colbwt_cid_pack_device(const uint8_t *d_cid, uint64_t n_bases, const uint8_t *ids, uint32_t n_ids, uint32_t *d_planes,
                           void *hip_stream);
int colbwt_cid_unpack_device(const uint32_t *d_planes, uint64_t first_word, uint64_t n_words, const uint8_t *ids, uint32_t n_ids,
                             uint8_t *d_cid, void *hip_stream);
int colbwt_read_end_mask_device(const uint64_t *d_read_off, uint64_t n_reads, uint32_t *d_mask, void *hip_stream);
int colbwt_pml_unpack_device(const uint32_t *d_zero_mask, const uint32_t *d_end_mask, uint64_t first_word,
                             uint64_t n_words, uint64_t total_words, uint16_t *d_pml, void *hip_stream);

/* ---- synthetic inputs (benchmark / test generators) ------ */

/* Bytes needed for a synthetic .col_pml image of `rows` rows. */
uint64_t colbwt_synth_index_bytes(uint64_t rows);
/* Direct move-table synthesis: adjacent-distinct ACGT heads (+ one 0x01 run of
 * length 1 at row rows/2), Geometric(mean_len) lengths, (interval, offset)
 * from the stable char-sorted F order, col ids from {0,0,0,1,2,3,17,200,255},
 * thresholds uniform in [0,n).  `split_permille`: per-mille probability that a
 * row repeats the previous row's character (a sub-run split; 0 => bwt_r == r).
 * Writes the file image into `out` (colbwt_synth_index_bytes(rows) bytes). */
int colbwt_synth_index(uint64_t rows, uint32_t mean_len, uint32_t split_permille, uint64_t seed,
                       void *out, uint64_t out_len);
/* As above with a choice of where the thresholds fall: UNIFORM in [0, n) (the
 * SURVEY.md 8(d) recipe), or BETWEEN_RUNS: between the previous run of the same
 * character and the run's head, as in a real index (mumemto's .thr_pos). */
#define COLBWT_SYNTH_THR_UNIFORM 0
#define COLBWT_SYNTH_THR_BETWEEN_RUNS 1
int colbwt_synth_index_thr(uint64_t rows, uint32_t mean_len, uint32_t split_permille, uint64_t seed,
                           int thr_mode, void *out, uint64_t out_len);
/* Backward-walk reads sampled ON THE DEVICE from the loaded index:
 * read[m-1-k] = char at LF^k(p0), p0 uniform; 0x01 -> 'A'; substitutions at
 * `sub_permille`/1000.  Writes n_reads*read_len bytes (+64 pad bytes zeroed)
 * to d_bases and n_reads+1 offsets to d_read_off (both device pointers). */
int colbwt_synth_reads_device(colbwt_index *idx, uint64_t n_reads, uint32_t read_len,
                              uint32_t sub_permille, uint64_t seed, uint8_t *d_bases,
                              uint64_t *d_read_off, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* COLBWT_H */
