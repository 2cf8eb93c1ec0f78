/*
 * biodemux_hip.h — C-ABI of libbiodemux_hip.so, the MI355X (gfx950) drop-in for the
 * per-read classification hot path of I-Mihara/BioDemuX.jl v1.6.0.
 *
 * The reference has NO FFI seam (it is 100 % Julia).  The seam this library creates replaces
 * the body of worker_task's per-read loop (src/core.jl:243-267): instead of one
 * determine_filename(seq, config, ws) (src/classification.jl:871) per read, the Julia host
 * packs a chunk into one byte vector + offsets and makes ONE ccall per chunk.  Each entry
 * point below names the reference code it replaces.  INTEGRATION.md shows the Julia binding.
 *
 * Conventions
 *   - plain C types only; no exceptions cross the ABI; every function returns 0 on success or
 *     a negative BDX_E_* code, with a message retrievable by bdx_last_error().
 *   - all sequence positions are 1-based inclusive, as in Julia.
 *   - the caller owns every buffer it passes, for the duration of the call only (device
 *     entry points: until bdx_sync() returns).  The library owns its tables, stream and
 *     staging buffers.  Nothing returned needs freeing except the context.
 *   - one context per OS thread / per GPU; a single context is not re-entrant
 *     (the reference runs nthreads() independent workers, core.jl:454-466).
 */
#ifndef BIODEMUX_HIP_H
#define BIODEMUX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BDX_ABI_VERSION 1

/* error codes */
#define BDX_OK 0
#define BDX_E_INVALID (-1)   /* bad argument / config outside the supported domain */
#define BDX_E_DEVICE (-2)    /* HIP runtime error (no GPU, OOM, launch failure) */
#define BDX_E_STATE (-3)     /* call sequence error */
#define BDX_E_COMM (-4)      /* RCCL not available / a collective failed */
#define BDX_E_SPACE (-5)     /* an output buffer is too small; the needed size is reported */

/* DemuxConfig.matching_algorithm (classification.jl:57): :semiglobal / :hamming / :exact */
#define BDX_ALG_SEMIGLOBAL 0
#define BDX_ALG_HAMMING 1
#define BDX_ALG_EXACT 2

/* bdx_pass_t.explicit_window (0 = normal operation) */
#define BDX_WINDOW_FIND_BEST 1
#define BDX_WINDOW_ALIGN_ONE 2

/* bdx_config_t.filter: candidate pre-filter in front of the exact per-barcode evaluation.
 * Every filter is lossless (it can only drop barcodes whose alignment would return Inf),
 * so results are identical for every value; OFF forces the unfiltered path. */
#define BDX_FILTER_AUTO 0
#define BDX_FILTER_OFF 1
#define BDX_FILTER_QGRAM 2     /* pigeonhole exact-piece seeds */
#define BDX_FILTER_BITPAR 3    /* Myers bit-parallel lower bound (m <= 32) */

/* DynamicRange, classification.jl:9-14 (already parsed by the host; resolve() of :96-100
 * runs per read on the device). */
typedef struct {
    int64_t start_offset;
    int64_t end_offset;
    int32_t start_from_end;
    int32_t end_from_end;
} bdx_range_t;

/* The per-pass slice of DemuxConfig selected in match_barcode_pass (classification.jl:778-792). */
typedef struct {
    bdx_range_t ref_search_range;
    bdx_range_t barcode_start_range;
    bdx_range_t barcode_end_range;
    int32_t trim_side;            /* 0 = nothing, 3, 5 (core.jl:308-313 validation is repeated) */
    int32_t n_barcodes;
    const uint8_t *bc_bytes;      /* config.bc_seqs concatenated (already preprocessed, fileio.jl:44-67) */
    const uint32_t *bc_off;       /* n_barcodes + 1 offsets into bc_bytes */
    const int32_t *bc_len_no_N;   /* config.bc_lengths_no_N (fileio.jl:69) */
    /* Unit-level override used to expose the reference's exported functions through the same
     * kernel.  explicit_window == BDX_WINDOW_FIND_BEST: the four values below replace
     * (first:last of final_search_range, max_start_pos, min_end_pos) of classification.jl
     * :799-809 verbatim for every read and the :805 sanity check is skipped — the pass then
     * equals one call of find_best_matching_bc (:722).  explicit_window ==
     * BDX_WINDOW_ALIGN_ONE: additionally the reducer is bypassed and the pass outputs are the
     * direct return of ONE alignment call on barcode 1 with max_error = max_error_rate
     * (semiglobal_alignment :447 / semiglobal_alignment_N :463 / hamming_align :557 /
     * exact_align :485). */
    int32_t explicit_window;
    int32_t _pad;
    int64_t win_first, win_last, win_max_start_pos, win_min_end_pos;
} bdx_pass_t;

typedef struct {
    uint32_t abi_version;         /* = BDX_ABI_VERSION */
    uint32_t struct_size;         /* = sizeof(bdx_config_t) */
    int32_t algorithm;            /* BDX_ALG_* */
    int32_t is_dual;              /* config.is_dual */
    double max_error_rate;        /* Float64, compared exactly as in classification.jl:658,696 */
    double min_delta;             /* Float64; == 0.0 selects the no_delta reducer (:723) */
    int32_t match, mismatch, indel;
    int32_t has_nindel;           /* nindel !== nothing -> NScoring (:644-648) */
    int32_t nindel;
    int32_t need_traceback;       /* config.summary (stats !== nothing, :812) */
    int32_t filter;               /* BDX_FILTER_* */
    int32_t device;               /* HIP device ordinal */
    bdx_pass_t pass[2];
} bdx_config_t;

/* Per-read outputs.  Any pointer may be NULL (that output is skipped).  For the host entry
 * point these are host pointers, for the device entry point device pointers.
 *   bc1        int32[n]  >0 = config.ids index (1-based, as Julia), 0 = "unknown",
 *                        -1 = "ambiguous_classification"  (classification.jl:879-883, :890-894, :897-899)
 *   bc2        int32[n]  config.ids2 index when dual and matched, else 0
 *   keep_start, keep_end int32[n]  determine_filename's 2nd/3rd return (:907-937):
 *                        (-1,-1) unknown/ambiguous, (1,0) empty keep range, else 1-based inclusive
 * Per-pass outputs, pass 1 at [2i] and pass 2 at [2i+1]: the return tuple of
 * find_best_matching_bc (classification.jl:722) for that pass —
 *   pass_bc    int32[2n] min_score_bc (1-based; 0 = no barcode accepted, pass not run, or the
 *                        range sanity check :805 failed)
 *   pass_score double[2n] min_score (Float64 raw / normalisation; +Inf when pass_bc == 0)
 *   pass_delta double[2n] delta (+Inf from the no_delta reducer :666; sub_min - min :711 otherwise)
 *   pass_start, pass_end int32[2n]  best_start, best_end (-1 for ScoreOnly / none)
 *   pass_raw   int32[2n] integer numerator of min_score (cost or mismatches), -1 if none
 * match_barcode_pass's status follows as: pass_bc == 0 -> :unknown; pass_delta < min_delta ->
 * :ambiguous (:822); else :match. */
typedef struct {
    int32_t *bc1;
    int32_t *bc2;
    int32_t *keep_start;
    int32_t *keep_end;
    int32_t *pass_start;
    int32_t *pass_end;
    int32_t *pass_raw;
    double *pass_score;
    int32_t *pass_bc;
    double *pass_delta;
} bdx_outputs_t;

typedef struct bdx_ctx bdx_ctx;

/* Library / ABI version (BDX_ABI_VERSION). */
int32_t bdx_abi_version(void);

/* Replaces: build_config's validation (core.jl:308-313) + per-worker workspace creation
 * SemiGlobalWorkspace(max_m, need_origin) (core.jl:229-233).  Copies the config, uploads the
 * barcode tables, creates a stream.  On failure *out is NULL and bdx_last_error(NULL) holds
 * the message. */
int32_t bdx_create(const bdx_config_t *config, bdx_ctx **out);

/* Releases everything bdx_create made. */
void bdx_destroy(bdx_ctx *ctx);

/* Message of the last failing call on ctx (or of the last failing bdx_create when ctx is
 * NULL).  The Julia shim turns a non-zero return into error(msg), matching the reference's
 * throw-from-worker behaviour (core.jl:593-597). */
const char *bdx_last_error(const bdx_ctx *ctx);

/* Replaces: worker_task's per-read loop (core.jl:243-267), i.e. n_reads calls of
 * determine_filename / determine_filename_and_stats (classification.jl:871, :940).
 * seq_bytes = the chunk's read sequences concatenated (code units, not upper-cased — the
 * reference compares raw bytes, classification.jl:185,597); seq_off[i]..seq_off[i+1] bounds
 * read i (n_reads+1 entries, seq_off[0] may be non-zero).  Blocks until the outputs are
 * filled.  Also accumulates the DemuxStats scalar counters (see bdx_get_counts). */
int32_t bdx_classify_host(bdx_ctx *ctx, const uint8_t *seq_bytes, const int64_t *seq_off,
                          int64_t n_reads, const bdx_outputs_t *out);

/* Same, with every pointer (seq_bytes, seq_off, outputs) already resident in HBM on
 * ctx's device.  Asynchronous on the context's stream; call bdx_sync() before reading.
 * This is the entry the multi-GPU driver and bench.py use.
 * Calls may be enqueued one after another with nothing in between.  A call waits for the
 * stream before it returns in three cases only: config.need_traceback (summary = true: the
 * batch's longest read is measured, the statistics tables may grow), no read-length hint
 * (bdx_set_read_length_hint: the batch is measured), and a batch larger than any before
 * (a hand-over buffer grows: the old one is released with hipFree, which synchronises the
 * device).  Inputs and outputs must stay valid until the stream has passed the call.
 * Offsets: d_seq_off[0] may be non-zero and the offsets may lie beyond 2^31 and 2^32; every
 * address is formed as d_seq_bytes + d_seq_off[i] in 64 bits (d_seq_bytes itself need not
 * point into the allocation that holds the batch, only the sums must).
 * Bytes outside [d_seq_off[0], d_seq_off[n_reads]): the kernels fetch read bytes in 16-byte
 * granules at 16-byte aligned addresses (a tile's or workgroup's contiguous span, a read's
 * slot or column window), or byte by byte inside a read.  A granule is fetched only when it
 * holds an address of the closed range d_seq_bytes + [d_seq_off[0], d_seq_off[n_reads]]: up
 * to 15 bytes in front of the first read and up to 15 behind the last may be LOADED, so
 * they must be readable — they are whenever the batch lies in a hipMalloc allocation,
 * whose pages are whole multiples of 16 bytes; for a batch of empty reads the granule of
 * d_seq_bytes + d_seq_off[0] itself may be loaded, so that must be such an address.  Those bytes
 * are never INTERPRETED: every position that reaches a seed probe, a sweep or a DP cell is
 * masked or bounded by its read's own offsets, so what lies around a batch (other reads,
 * barcode bases, garbage) never changes a result.  Established by reading every fetch site
 * (geometry / load_bytes, load_scat / scat_geo in bdx_wave_kernel.h; the dense, list and
 * window-upload forms in bdx_bitpar.hip; the staged span and the unstaged reads in
 * bdx_device.hip) and held by tests/test_offset_base_gpu.py (hostile surroundings, bases
 * that cross 2^31 and 2^32).  The same holds for bdx_classify_host's seq_bytes / seq_off,
 * which uploads only [seq_off[0], seq_off[n_reads]) (or each read's window). */
int32_t bdx_classify_device(bdx_ctx *ctx, const uint8_t *d_seq_bytes, const int64_t *d_seq_off,
                            int64_t n_reads, const bdx_outputs_t *d_out);

/* Optional: the typical (maximum) read length of the batches to come.  The fused kernels size
 * their LDS staging for it; without a hint every device batch is measured first (one tiny
 * kernel + a 4-byte copy, which synchronises the stream).  Reads longer than planned are
 * still classified exactly, by a slower path.  0 clears the hint. */
int32_t bdx_set_read_length_hint(bdx_ctx *ctx, int32_t typical_read_length);

/* Waits for the context's stream. */
int32_t bdx_sync(bdx_ctx *ctx);

/* Use an existing hipStream_t (e.g. PyTorch's current stream) for all work of this context.
 * NULL restores the context's own stream.  The library does not order the new stream after
 * the old one: a caller that switches while work of this context may still be running makes
 * the new stream wait for it first (an event recorded on the old stream, or bdx_sync()).  The
 * counter vector (bdx_set_counts_buffer) and the statistics tables are untouched by a switch. */
int32_t bdx_set_stream(bdx_ctx *ctx, void *hip_stream);

/* DemuxStats scalar part (classification.jl:736-744, updated at :942,:950,:953,:963,:966,
 * :976-978): counts[0..3] = total, matched, unmatched, ambiguous reads; counts[4 + (bc1-1)*S +
 * (bc2 ? bc2-1 : 0)] = sample_counts[(bc1,bc2)], S = max(1, n_barcodes of pass 2 when dual).
 * bdx_counts_len returns 4 + B1*S. */
int64_t bdx_counts_len(const bdx_ctx *ctx);

/* Copies the accumulated counters to the host (synchronises the stream). */
int32_t bdx_get_counts(bdx_ctx *ctx, int64_t *out, int64_t n);

/* Zeroes the counters. */
int32_t bdx_reset_counts(bdx_ctx *ctx);

/* DemuxStats histograms (classification.jl:746-757, filled at :827-865 for every pass that returns :match;
 * merged like reporting.jl:10-56).  Collected on the device when config.need_traceback (summary = true), as three
 * int64 tables per pass, each [rows][n_barcodes(pass)] row-major by key:
 *   BDX_STATS_POS  key = best_start (row r holds key r + key0, key0 = 1 - longest barcode: origins may precede the read)
 *   BDX_STATS_LEN  key = best_end - best_start + 1
 *   BDX_STATS_RAW  key = integer numerator of min_score; the host derives round(raw / normalisation, digits = 2) (:835)
 * Summing a row over the barcodes gives bc{1,2}_{pos,len,score}_counts, a column bc{1,2}_per_bc_*.  The pos table
 * grows with the longest read seen; len has 2 * (longest barcode) + 2 rows when no start / end range binds (an
 * alignment spans its barcode's bases plus at most as many insertions) and grows with the reads otherwise; raw has
 * floor(max_error_rate * normalisation) + 1 rows; bdx_stats_shape reports the current shape.  reduced != 0 reads the tables
 * summed over the ranks by bdx_allreduce_counts* (which all-reduces them together with the counter vector). */
#define BDX_STATS_POS 0
#define BDX_STATS_LEN 1
#define BDX_STATS_RAW 2
int32_t bdx_stats_shape(const bdx_ctx *ctx, int32_t pass, int32_t which, int64_t *rows, int64_t *key0, int64_t *n_barcodes);
int32_t bdx_get_stats(bdx_ctx *ctx, int32_t pass, int32_t which, int32_t reduced, int64_t *out, int64_t n_words);

/* Device address of the int64 counter vector — the buffer a multi-GPU host all-reduces
 * (sum) over RCCL, the analogue of merge_stats (reporting.jl:1-9).  bdx_set_counts_buffer
 * lets the host supply its own device buffer (e.g. a torch tensor) of bdx_counts_len()
 * int64 so the collective can run on it directly; NULL restores the internal one. */
void *bdx_counts_device_ptr(bdx_ctx *ctx);
int32_t bdx_set_counts_buffer(bdx_ctx *ctx, void *d_counts);

/* ---- merge_stats across GPUs (reporting.jl:1-9; called at core.jl:495 and :628) ----------------------
 * The reference sums the per-worker DemuxStats in one process.  With one context per GPU the scalar part of
 * that merge is ONE all-reduce (sum, int64, bdx_counts_len() words) over RCCL / xGMI, reachable from any host
 * language through the calls below (RCCL itself is opened lazily, on the first communicator call).
 *
 * One process, several devices (the Julia host: one HipWorker per GPU):
 *     bdx_comm_init_all(ctxs, n)        ncclCommInitAll over the contexts' (distinct) devices; rank i = ctxs[i]
 *     bdx_allreduce_counts_all(ctxs, n) the grouped collective, driven by the calling thread
 * One process per GPU (torchrun / mpirun):
 *     bdx_comm_get_unique_id(id)        on rank 0; the host ships the BDX_COMM_ID_BYTES bytes to every rank
 *     bdx_comm_init_rank(ctx, id, rank, n_ranks)
 *     bdx_allreduce_counts(ctx)         also valid for one context per OS thread in the first shape
 * The collective is enqueued on the context's stream and writes the SUM into a second, library-owned vector
 * (bdx_reduced_counts_device_ptr / bdx_get_reduced_counts, which synchronises); the per-rank counters stay as
 * they are, so accumulation can go on.  Without a communicator the "sum" is a copy (a 1-GPU host runs the same
 * sequence).  All contexts of a communicator must be built from the same config. */
#define BDX_COMM_ID_BYTES 128
int32_t bdx_comm_get_unique_id(void *id_out);
int32_t bdx_comm_init_rank(bdx_ctx *ctx, const void *id, int32_t rank, int32_t n_ranks);
int32_t bdx_comm_init_all(bdx_ctx *const *ctxs, int32_t n);
int32_t bdx_comm_destroy(bdx_ctx *ctx);          /* also done by bdx_destroy */
int32_t bdx_comm_rank(const bdx_ctx *ctx);       /* 0 without a communicator */
int32_t bdx_comm_size(const bdx_ctx *ctx);       /* 1 without a communicator */
int32_t bdx_allreduce_counts(bdx_ctx *ctx);
int32_t bdx_allreduce_counts_all(bdx_ctx *const *ctxs, int32_t n);
void *bdx_reduced_counts_device_ptr(bdx_ctx *ctx);
int32_t bdx_get_reduced_counts(bdx_ctx *ctx, int64_t *out, int64_t n);

/* Optional: page-locked host memory for the buffers given to bdx_classify_host (the reference's reader task
 * would fill its chunk buffers here, core.jl:43-110).  With pinned buffers the host <-> device copies are
 * asynchronous DMA at PCIe speed; ordinary (pageable) memory works too, just slower.  NULL on failure. */
void *bdx_host_alloc(size_t bytes);
void bdx_host_free(void *p);

/* Device FASTQ pipeline: FASTQ text already in device memory becomes per-output-file FASTQ blocks without a host
 * round trip (the reference's reader_task / writer_task, core.jl:43-110, :118-224, on the device).  Each step has the
 * contract of a host function of the project's FASTQ library (csrc/bdx_io.cpp), which the tests hold it to.  All three
 * run on the context's stream and device and synchronise it before they return.  Line offsets are byte offsets
 * relative to d_text; a record is 4 lines (header, sequence, plus, quality).
 *
 * bdx_fq_index_device: line table of d_text[0, text_len) for up to max_reads records (4 * max_reads entries of
 * d_line_off / d_line_len).  A line's length excludes "\n" and a "\r" before it.  final == 0 (more text follows):
 * only complete records.  final != 0: an unterminated last line counts, and a truncated last record is padded with
 * (off = text_len, len = 0) lines.  *n_records: records indexed; *next: the offset after the last line consumed. */
int32_t bdx_fq_index_device(bdx_ctx *ctx, const uint8_t *d_text, int64_t text_len, int32_t final, int64_t max_reads,
                            int64_t *d_line_off, int32_t *d_line_len, int64_t *n_records, int64_t *next);

/* The index by byte spans: a text cut at ANY byte offsets is indexed span by span, in any order and on any contexts.
 * The reference frames records by line count alone (four readline calls a record, core.jl:65-75, :96-101), so the
 * record a line belongs to follows from the number of newlines in front of it, modulo 4; newline counts of disjoint
 * byte ranges are independent and chain with one addition per range.  Both entries run on the context's stream and
 * device and synchronise it before they return.
 *
 * bdx_fq_count_lines_device: *n_newlines = the number of '\n' bytes in d_text[0, len).  Any pointer alignment.
 *
 * bdx_fq_index_span_device: d_text[0, text_len) holds the file's bytes from the span's first byte on: the span
 * (span_len <= text_len bytes) and a tail behind it.  phase = (newlines in the file in front of the span) mod 4.
 * starts_line != 0: the span's byte 0 begins a line (it is the file's first byte, or the byte in front of it is
 * '\n').  final != 0: d_text reaches the end of the file.
 *   A line that starts inside the window has the global number phase + (newlines in front of its first byte),
 * whether or not starts_line is set; starts_line only says whether offset 0 is itself a line start — if it is not,
 * the bytes in front of the window's first newline belong to a line of an earlier span and are no line start here.
 * A line begins a record when its global number is 0 mod 4.  The output is the line table (4 lines a record,
 * offsets relative to d_text, lengths without "\n" and without a "\r" in front of it: 4 * max_reads entries of room)
 * of exactly the records whose first line starts at an offset < span_len; their lines are taken as far into the
 * tail as they reach.  *n_records: those records.
 *   *complete = 0, with BDX_OK, when final == 0 and the last such record's fourth line is not terminated inside
 * text_len: the caller offers a longer tail and calls again (the line table is unspecified then).  With final != 0
 * the rules of bdx_fq_index_device hold for the last record: an unterminated last line counts, a truncated record is
 * padded with (off = text_len, len = 0) lines.  When more than max_reads records start in the span the call returns
 * BDX_E_SPACE with the needed count in *n_records.  BDX_E_INVALID: a negative length, span_len > text_len, phase
 * outside 0 .. 3, a NULL pointer.
 *   The partition property: over any text and any span size S >= 1, with span k = bytes [kS, (k + 1)S), the tail
 * long enough (or the rest of the text with final = 1), phase and starts_line as defined above, the spans' tables,
 * shifted by kS and concatenated in span order, are the line table bdx_fq_index_device gives for the whole text with
 * final = 1 — every record once, none lost. */
int32_t bdx_fq_count_lines_device(bdx_ctx *ctx, const uint8_t *d_text, int64_t len, int64_t *n_newlines);
int32_t bdx_fq_index_span_device(bdx_ctx *ctx, const uint8_t *d_text, int64_t text_len, int64_t span_len, int32_t phase,
                                 int32_t starts_line, int32_t final, int64_t max_reads, int64_t *d_line_off,
                                 int32_t *d_line_len, int64_t *n_records, int32_t *complete);

/* bdx_fq_pack_device: the sequence lines of records [0, n) packed as the chunk bdx_classify_device takes:
 * d_seq_off[0] = 0, d_seq_off[i + 1] = d_seq_off[i] + length of read i (n + 1 entries).  d_seq holds seq_cap bytes
 * (the sum of the lengths is at most text_len); *seq_bytes (optional) receives that sum. */
int32_t bdx_fq_pack_device(bdx_ctx *ctx, const uint8_t *d_text, int64_t text_len, const int64_t *d_line_off,
                           const int32_t *d_line_len, int64_t n, uint8_t *d_seq, int64_t seq_cap, int64_t *d_seq_off,
                           int64_t *seq_bytes);

/* bdx_fq_gather_device: the output of one stream of a batch (R1 or R2).  Record i goes to class 0 (bc1 == 0,
 * unknown), 1 (bc1 < 0, ambiguous) or 2 + (bc1 - 1) * stride + (max(bc2, 1) - 1); d_out receives the records
 * class by class, in input order inside a class, each as header "\n" seq[a..b] "\n" plus "\n" qual[a..b'] "\n"
 * ("\r" is never written).  trim != 0 and keep_start != -1: a = max(keep_start, 1), b = min(keep_end, seq length),
 * b' = min(b, quality length), empty when a > b (core.jl:162-173); otherwise the lines are written whole.
 * class_bytes (HOST memory, n_classes entries) receives the bytes of every class's block: the blocks follow each
 * other in class order from d_out[0].  Fails with BDX_E_INVALID (class_bytes still filled) when they need more
 * than out_cap bytes; text_len + 4 is always enough. */
int32_t bdx_fq_gather_device(bdx_ctx *ctx, const uint8_t *d_text, int64_t text_len, const int64_t *d_line_off,
                             const int32_t *d_line_len, int64_t n, const int32_t *d_bc1, const int32_t *d_bc2,
                             int32_t stride, int32_t n_classes, const int32_t *d_keep_start, const int32_t *d_keep_end,
                             int32_t trim, uint8_t *d_out, int64_t out_cap, int64_t *class_bytes);

/* Opt-in record and pair checks over a line table (csrc/bdx_fastq.hip; the reference frames records by line count alone
 * and checks nothing, core.jl:65-75, :175-190).  Three record rules, selected by a bit mask:
 *   BDX_FQ_CHECK_HEADER  a record breaks it when line 1 is empty or its first byte is not '@'
 *   BDX_FQ_CHECK_PLUS    ... when line 3 is empty or its first byte is not '+'
 *   BDX_FQ_CHECK_LENGTH  ... when len(line 2) != len(line 4)
 * Lengths are those of the line table: without "\n" and without a "\r" in front of it.  The padded lines of a truncated
 * last record (off = text_len, len = 0) are ordinary empty lines to these rules, so a record cut after line 1 or 2 breaks
 * the plus rule, one cut after line 3 the length rule unless its sequence line is empty: only a cut after an empty
 * sequence line passes, and that is the same text as a whole record with an empty sequence and an empty quality line.
 *
 * One pair rule.  The NAME of a header line is its bytes after the first one (whatever that is: '@' is the header rule's
 * business), up to but not including the first ' ' or '\t', or to the end of the line, with ONE trailing "/1" or "/2"
 * dropped if that token ends in one.  An empty line has the empty name.  Two records pair when their names have the
 * same length and the same bytes.
 *
 * Not checked: the sequence alphabet, the quality range, anything of a header behind the first blank.
 *
 * Both entries run on the context's stream and device and synchronise before they return.
 * bdx_fq_check_device: *first_bad = the lowest index in [0, n) of a record that breaks a rule selected in `rules`, or
 * -1 if there is none; *broken = the selected rules that record breaks, or 0.
 * bdx_fq_check_pair_device: *first_bad = the lowest index in [0, n) at which record i of the first table and record i of
 * the second do not pair, or -1.  Only header lines are read.
 * n == 0 is BDX_OK with -1.  BDX_E_INVALID (with -1 / 0 stored when the result pointers are there): a NULL pointer, a
 * negative length or count, `rules` with bits outside 7 or 0, more than 2^32 - 1 records, a line (of the lines the call
 * reads: all four / the headers) that lies outside its text ("a line of the line table lies outside the text").  No byte
 * outside [d_text, d_text + text_len) is read, whatever the alignment of d_text.  A correct call on the same context
 * works after every refusal.
 * The host counterparts, with the same contract over bdx_fq_file texts and host tables, are bdx_fq_check and
 * bdx_fq_check_pair of csrc/bdx_io.cpp (libbdx_io.so); the device entries are tested against them. */
#define BDX_FQ_CHECK_HEADER 1
#define BDX_FQ_CHECK_PLUS 2
#define BDX_FQ_CHECK_LENGTH 4
int32_t bdx_fq_check_device(bdx_ctx *ctx, const uint8_t *d_text, int64_t text_len, const int64_t *d_line_off,
                            const int32_t *d_line_len, int64_t n, int32_t rules, int64_t *first_bad, int32_t *broken);
int32_t bdx_fq_check_pair_device(bdx_ctx *ctx, const uint8_t *d_text1, int64_t text_len1, const int64_t *d_line_off1,
                                 const int32_t *d_line_len1, const uint8_t *d_text2, int64_t text_len2,
                                 const int64_t *d_line_off2, const int32_t *d_line_len2, int64_t n, int64_t *first_bad);

/* Device DEFLATE for the pipeline's gzip output (csrc/bdx_deflate.hip).  The input is what bdx_fq_gather_device
 * leaves: per-class blocks back to back in device memory (any byte offsets), their sizes in the host array class_bytes.
 * Every non-empty block is cut into chunks of at most bdx_fq_deflate_chunk() bytes and every chunk becomes one
 * complete gzip member written by the device: FEXTRA header with OS = 255 and the 'D','X' subfield (4 bytes LE: the
 * member's total size, the tag the project's reader walks and inflates in parallel), one dynamic-Huffman block (or one
 * stored block when that is not smaller), CRC-32, ISIZE.  A block's members concatenated are a valid .gz for any
 * reader.  The same input bytes give the same output bytes on every run and in every context.
 *
 * bdx_fq_deflate_bound: the most bytes the members of these blocks can take (len + 33 per chunk); needs no context
 * and no device.  0 when every class is empty, negative for a negative entry.
 *
 * bdx_fq_deflate_device: runs on the context's stream and device and synchronises before it returns.  class_cbytes
 * (HOST memory, n_classes entries) receives the bytes of class c's members, which follow one another in class order
 * from d_out[0]; an empty class has no member and 0 bytes.  Fails with BDX_E_INVALID, writing nothing, when
 * out_cap < bdx_fq_deflate_bound(class_bytes, n_classes).
 *
 * Levels.  bdx_fq_deflate_levels: how many compression levels the encoder has (2); needs no context and no device.
 * bdx_fq_deflate_level_device: bdx_fq_deflate_device's contract at the given level.  Level 1 writes exactly
 * bdx_fq_deflate_device's bytes (that entry is level 1).  Level 2 is the stronger and slower one: matches may start
 * inside the 256-position sub-block being parsed, every hash keeps its 8 most recent positions, a match gives way to a
 * literal when the next position's is longer, and the block header is run-length coded; chunk size, member framing, one
 * block per member, the stored fallback (so bdx_fq_deflate_bound serves both levels), CRC and determinism are level 1's.
 * A level outside 1 .. bdx_fq_deflate_levels() fails with BDX_E_INVALID and a message: nothing is launched and
 * class_cbytes is zeroed. */
int32_t bdx_fq_deflate_chunk(void);
int64_t bdx_fq_deflate_bound(const int64_t *class_bytes, int32_t n_classes);
int32_t bdx_fq_deflate_device(bdx_ctx *ctx, const uint8_t *d_in, const int64_t *class_bytes, int32_t n_classes,
                              uint8_t *d_out, int64_t out_cap, int64_t *class_cbytes);
int32_t bdx_fq_deflate_levels(void);
int32_t bdx_fq_deflate_level_device(bdx_ctx *ctx, int32_t level, const uint8_t *d_in, const int64_t *class_bytes,
                                    int32_t n_classes, uint8_t *d_out, int64_t out_cap, int64_t *class_cbytes);

/* Device inflate for the pipeline's .gz input (csrc/bdx_inflate.hip): size-tagged gzip members (BGZF, or the 'D','X'
 * members above) already in device memory are decoded, each into a slot of its own in d_out, and every member's CRC-32
 * and ISIZE are checked on the device.  The decoder is a complete RFC 1951 / RFC 1952 one (stored, fixed and dynamic
 * blocks, any number of them; FEXTRA, FNAME, FCOMMENT, FHCRC) and accepts a member exactly when zlib does.  The four
 * tables are HOST arrays of n_members entries: member m is d_comp[comp_off[m], +comp_len[m]) and inflates to
 * d_out[plain_off[m], +plain_len[m]), plain_len being the ISIZE its trailer states.  No byte outside a member is read
 * and none outside its slot is written, whatever the member holds.
 *
 * bdx_fq_inflate_member_max: the largest plain_len a member may have (65536, BGZF's); needs no context and no device.
 *
 * bdx_fq_inflate_device: runs on the context's stream and device and synchronises before it returns.  The tables are
 * checked first (lengths >= 0, plain_len <= bdx_fq_inflate_member_max(), every slot inside out_cap): BDX_E_INVALID
 * before anything is launched.  n_members == 0 is BDX_OK.  status (HOST memory, n_members entries, may be NULL)
 * receives per member 0 or why it was refused: 1 bad header, 2 bad block type, 3 bad stored lengths, 4 bad code set,
 * 5 bad symbol, 6 distance too far, 7 output overrun, 8 output short, 9 input exhausted, 10 CRC mismatch, 11 ISIZE
 * mismatch.  When any member is refused the call returns BDX_E_INVALID and bdx_last_error names the first one and its
 * reason; status is filled for all members and the slots of the good ones are valid. */
int32_t bdx_fq_inflate_member_max(void);
int32_t bdx_fq_inflate_device(bdx_ctx *ctx, const uint8_t *d_comp, const int64_t *comp_off, const int32_t *comp_len,
                              const int64_t *plain_off, const int32_t *plain_len, int32_t n_members, uint8_t *d_out,
                              int64_t out_cap, int32_t *status);

/* Stream inflate for an ORDINARY .gz input (csrc/bdx_inflate_stream.hip): d_comp[0, comp_len) is a whole .gz file in
 * device memory, one or more gzip members of any size back to back, tagged or not (tags are ignored).  The file is cut
 * at multiples of chunk_bytes; every chunk guesses a block start (a dynamic block's header is redundant enough to be
 * recognised) and decodes from there, the guesses a confirmed decoder arrives at are chained, and what a match copies
 * from the unknown 32 KiB in front of a guess is resolved afterwards.  Exactness never rests on a guess: a wrong or
 * missing one costs speed only.  Accepts a file exactly when zlib accepts every member; what follows the last member
 * and does not begin with 1f 8b is ignored, as zlib's gzread ignores it.
 *
 * bdx_fq_inflate_stream_chunk: the default chunk_bytes; needs no context and no device.
 *
 * bdx_fq_inflate_stream_device: chunk_bytes is 0 (the default) or 64 .. 2^24.  The arguments are checked before
 * anything is launched (BDX_E_INVALID).  Runs on the context's stream and synchronises before it returns.
 *   BDX_OK         d_out[0, *plain_len) holds the plain bytes of all members, every CRC-32 and ISIZE verified
 *   BDX_E_SPACE    out_cap is too small: *plain_len is the size needed (known before any output byte exists: d_out is
 *                  untouched)
 *   BDX_E_INVALID  a member is refused: bdx_last_error names the member, the compressed byte offset and one of the
 *                  eleven reasons of bdx_fq_inflate_device; d_out[0, out_cap) is unspecified
 * info (HOST memory, 8 entries, may be NULL) receives: members, chunks, segments confirmed at a guessed start,
 * candidates discarded, chunks without a candidate, the compressed bytes of the longest segment, 0, 0.
 * Device memory taken for the call: 2 * *plain_len bytes (released before it returns) and 32 bytes per chunk. */
int32_t bdx_fq_inflate_stream_chunk(void);
int32_t bdx_fq_inflate_stream_device(bdx_ctx *ctx, const uint8_t *d_comp, int64_t comp_len, int32_t chunk_bytes,
                                     uint8_t *d_out, int64_t out_cap, int64_t *plain_len, int64_t *info);

/* The stream inflate in WINDOWS (csrc/bdx_inflate_window_core.h): the same file, of any size, goes through the device
 * a bounded window at a time.  A window object carries what the next window needs: where the position is (a block
 * start at a bit of the next byte, a member's trailer, between members, trailing bytes), the member's index, CRC-32 and
 * size so far, and the last 32 KiB of plain text (about 64 KiB of device memory).  Several objects may share a context;
 * the scratch of a call is the context's and is not kept between calls.
 *
 * bdx_fq_inflate_window_open: chunk_bytes as for bdx_fq_inflate_stream_device.  The object stands at byte 0 of a file.
 * Its state is initialised when open returns (it synchronises): the object may be fed on any stream the context is given later.
 * bdx_fq_inflate_window_feed: d_comp[0, comp_len) are the file's bytes from the absolute offset the object stands at,
 * the sum of every *consumed so far; comp_len <= 2^28; last != 0 says that they end with the file.  Runs on the
 * context's stream and synchronises (after the chain, after the verdict) before it returns.
 *   BDX_OK         d_out[0, *plain_len) is the text of everything consumed; *consumed whole bytes are done with (the
 *                  byte that holds the next block's first bit is not among them); every member that ended in the
 *                  window has had its CRC-32 and ISIZE checked.  The window stops at the last block end, trailer or
 *                  member boundary up to which every bit it needed lay in the buffer.  *consumed == 0 and
 *                  *plain_len == 0 with last == 0: the buffer holds no complete block — feed a longer one from the same
 *                  offset.  With last != 0 everything is consumed, or ignored as trailing bytes, or refused.
 *   BDX_E_SPACE    out_cap is too small: *plain_len is the room needed; nothing is consumed, the object is unchanged
 *                  and d_out is untouched: the same call with that room succeeds
 *   BDX_E_INVALID  a member is refused: bdx_last_error names its index in the file, the absolute compressed byte and
 *                  one of the eleven reasons.  The object is dead: every later feed returns BDX_E_STATE.
 * info as for bdx_fq_inflate_stream_device, per call; its first entry counts the members that ended in the window.
 * Device memory taken for a call: 2 * *plain_len bytes (released before it returns) and 32 bytes per chunk.
 * bdx_fq_inflate_window_close: waits for the context's stream and frees the object (NULL is allowed). */
typedef struct bdx_fq_inflate_window bdx_fq_inflate_window;
int32_t bdx_fq_inflate_window_open(bdx_ctx *ctx, int32_t chunk_bytes, bdx_fq_inflate_window **w);
int32_t bdx_fq_inflate_window_feed(bdx_fq_inflate_window *w, const uint8_t *d_comp, int64_t comp_len, int32_t last,
                                   uint8_t *d_out, int64_t out_cap, int64_t *consumed, int64_t *plain_len, int64_t *info);
int32_t bdx_fq_inflate_window_close(bdx_fq_inflate_window *w);

/* Introspection for bench/tests: name of the kernel path a classify call will take, and numbers of the
 * last launch.  "generic": exact kernel only; "bitpar+verify": bit-vector sweep of every pair, then the exact
 * stage; "qgram+bitpar+verify": single-piece q-gram seeds in front of the sweep; "qgram2+bitpar+verify":
 * two-intact-pieces ("diagonal") seeds in front of the sweep.  All paths give identical results. */
const char *bdx_kernel_path(const bdx_ctx *ctx);

/* How many bdx_classify_host calls went through the WINDOW UPLOAD: when the passes only look at a short column
 * window of long reads (ref_search_range "1:200" on 10 kbp reads), the host entry point copies just each read's
 * window to the device (the union over the passes of final_search_range, classification.jl:795-809, resolved per
 * read exactly like the kernels do) instead of the whole read.  Results are identical; PCIe traffic follows the
 * window. */
int64_t bdx_window_uploads(const bdx_ctx *ctx);

/* How many (pass, exact-kernel launch) pairs ran with the diagonal-band DP enabled (traceback / weighted-cost
 * configs whose barcodes all have 24 or all have 32 bases: the exact stage then computes only the diagonals an
 * alignment within the budget can touch, semiglobal_alignment_core classification.jl:238-445 restricted to them).
 * Results are identical either way; the counter exists so that tests can tell which form ran. */
int64_t bdx_band_launches(const bdx_ctx *ctx);

/* How many launches of the WAVE-AUTONOMOUS kernel this context made (bdx_wave.hip): known-score configs (ScoreOnly,
 * unit costs) with plain A/C/G/T barcodes and ranges "1:end" — the reference's default call and the headline
 * benchmark — get their verdicts from a kernel in which every wavefront walks its own tile of reads (seed scan,
 * bit-vector sweeps, replay of find_best_matching_bc, classification.jl:632-713); reads it cannot answer go to the
 * general kernel.  Results are identical either way (env BDX_NO_WAVE switches it off); the counter exists so that
 * tests can tell which kernel ran. */
int64_t bdx_wave_launches(const bdx_ctx *ctx);

/* How many launches of the same kernel's PAIRS mode this context made (bdx_pairs.hip): tiered configs (budgets too large
 * for selective single seeds, e.g. the reference's default max_error_rate 0.2 on 24-nt barcodes) gather the reads tier 1
 * could not settle and filter them at the full budgets by the two-intact-pieces lemma, ahead of the general kernel.
 * Results are identical either way (env BDX_NO_PAIRS switches it off); a test-visibility counter like the one above. */
int64_t bdx_pair_launches(const bdx_ctx *ctx);

/* How many bdx_classify_host calls uploaded their batch in chunks on a copy stream beside the previous chunk's kernels
 * (large batches of configs with heavier kernels; env BDX_NO_PIPELINE switches it off).  Results are identical. */
int64_t bdx_pipelined_calls(const bdx_ctx *ctx);

/* How many bdx_classify_host calls brought their result vectors back through the context's page-locked staging buffer with
 * several host threads copying them out (large batches whose output arrays are pageable; env BDX_NO_STAGED_DOWNLOAD switches
 * it off — the runtime's own pageable copies then).  Results are identical; replaces nothing in the reference (its workers
 * write into Julia arrays, core.jl:243-267) — this is the PCIe side of the drop-in boundary. */
int64_t bdx_staged_downloads(const bdx_ctx *ctx);

/* Reads the first filter launch of the LAST classify call (the wave kernel, or tier 1) handed on to the next kernel through
 * its device-side list — the reads it could not answer itself (table overflows, reads outside its class, tier 1's open
 * verdicts).  Synchronises the context's stream; a test-visibility counter (C2: one read in ten million since the wave kernel
 * sweeps a read whose record tables overflow over every barcode itself, env BDX_NO_WAVE_FALLBACK switches that off).
 * -1: the device could not be read. */
int64_t bdx_last_list_reads(bdx_ctx *ctx);

/* Reads the pairs mode of the LAST classify call handed on through its own device-side list (tier 1's list is its input):
 * the length of the list the full-budget stage walks behind it.  Synchronises the context's stream; a test-visibility
 * counter like bdx_last_list_reads.  -1: the device could not be read. */
int64_t bdx_last_mid_reads(bdx_ctx *ctx);

/* Hand-over windows the exact kernel refused because they do not end inside the read ("not a window": defence in
 * depth behind the filter kernels, classification.jl:238-445 then runs over the whole pass window).  A correct
 * producer / consumer pair never leaves one: the counter must read 0 (synchronises the stream); the test-suite runs
 * with BDX_POISON, which fills every hand-over buffer with 0xA5 before each call, and checks it.
 * bdx_debug_rejected_windows_total: the same, summed over every context this process has destroyed. */
int64_t bdx_rejected_windows(bdx_ctx *ctx);
int64_t bdx_debug_rejected_windows_total(void);

/* The classify kernels the LAST classify call enqueued (a bdx_classify_host call: all of its chunks), as the launchers
 * saw them — a test-visibility log like the counters above; it adds no synchronisation.  One line per launch, fields
 * separated by tabs: family (wave | pairs | bitpar | generic), the instantiation as the code object names it (e.g.
 * "bdx_wave_kernel<32, 20, 5, 8, false, 0, 0, false, 0, false, false>"), workgroups, threads per workgroup, reads per
 * tile, the units the tiles are dealt over (waves of the grid for wave / pairs, workgroups for bitpar; 0: no tile loop),
 * the reads it was given and a list flag (1: it walks a device-side list of at most that many reads).
 * Copies at most cap - 1 bytes and a NUL into buf (buf may be NULL when cap is 0); returns the length of the whole log. */
int64_t bdx_last_launches(const bdx_ctx *ctx, char *buf, int64_t cap);

typedef struct {
    int32_t threads_per_block;
    int32_t lds_bytes_per_block;
    int64_t blocks;
    int32_t reads_per_block;
    int32_t filter_used;          /* BDX_FILTER_* actually in effect */
    int32_t max_m;
    int64_t launches;             /* kernel launches so far on this context */
} bdx_launch_info_t;
int32_t bdx_launch_info(const bdx_ctx *ctx, bdx_launch_info_t *out);

#ifdef __cplusplus
}
#endif
#endif
