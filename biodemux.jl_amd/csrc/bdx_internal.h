// bdx_internal.h — structures shared between the host side (the create-time planner bdx_plan.cpp, the per-call planner
// bdx_call.cpp, the C-ABI translation unit bdx_abi.cpp) and the gfx950 kernels (bdx_device.hip).  Not part of the public ABI.
// The seam between bdx_abi.cpp's enqueue and the classify launchers is at the end: what one call hands every launcher
// (BdxBatch, BdxHandOver, BdxDevList / BdxTierArgs), the launchers, and the layout of the call's scratch words (BdxScratch).
// A launcher decides no grid and no LDS size: both stand in the sized plan it is given (bdx_call.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/biodemux_hip.h"

// Integer domain of the device DP.  The reference computes in Int64 with
// INF_INT = typemax(Int) ÷ 4 (classification.jl:7); every DP value is bounded by
// (max_m + 2) * max|cost| + allowed_error, so with the limits enforced in bdx_create
// (|cost| <= BDX_MAX_COST, max_m <= BDX_MAX_M, |allowed_error| < 2^27) int32 arithmetic
// is exact and BDX_INF32 + value never overflows.
#define BDX_INF32 0x3FFFFFFF
#define BDX_MAX_COST 32767
#define BDX_MAX_M 8192
#define BDX_MAX_RATE 1.0e4
#define BDX_WCAP 4       // column-window entries per read and pass handed from the filter to the exact kernel
#define BDX_REG_ROWS 32  // barcodes up to this length run the register-resident exact DP

// Developer switches.  Read from the environment ONCE, in bdx_create (read_tuning); none of them
// changes a result — they only select between kernel paths that must agree (the parity tests run them).
struct BdxTuning {
    int no_known = 0;     // BDX_NO_KNOWN: no reducer replay, every config runs split (filter -> exact kernel)
    int no_seed = 0;      // BDX_NO_SEED: no q-gram seeds at all
    int no_diag = 0;      // BDX_NO_DIAG: no two-intact-pieces variant
    int no_windows = 0;   // BDX_NO_WINDOWS: split mode without column windows
    int no_slot = 0;      // BDX_NO_SLOT: long reads use flat staging instead of window slots
    int lds_dp = 0;       // BDX_LDS_DP: exact kernel with LDS columns instead of the register DP
    int bitpar_r = 0;     // BDX_BITPAR_R: forced tile size of the fused kernel
    long long grid = 0;   // BDX_GRID: forced persistent grid
    int diag_min_b = 48;  // BDX_DIAG_MIN_B: barcode threshold of the diagonal filter
    int no_window_upload = 0;  // BDX_NO_WINDOW_UPLOAD: the host entry point always uploads whole reads
    int seed_hash_l2 = 0;  // BDX_SEED_HASH_L2: the piece hash table stays in global memory
    int seed_bm_log2 = 0;  // BDX_SEED_BM_LOG2: size of the seed bitmap (log2 of its bits)
    int no_clean = 0;     // BDX_NO_CLEAN: exact kernel's register DP always in its predicated by-construction form
    int tier_q = 0;       // BDX_TIER_Q: piece length (5..8) the capped budgets of tier 1 are derived from (default: chosen per config)
    int no_pipeline = 0;  // BDX_NO_PIPELINE: the host entry point uploads large batches in one piece
    int no_dense = 0;     // BDX_NO_DENSE: plain-sweep kernels keep the 4-entry slots / window entries also for short barcodes
    int no_band = 0;      // BDX_NO_BAND: the exact kernel never takes the diagonal-band DP
    int poison = 0;       // BDX_POISON: every hand-over buffer is filled with 0xA5 before each classify call (tests: a consumer that reads what no producer wrote gets garbage on every run, not only when the allocator happens to hand back dirty memory)
    int tier0_div = 0;    // BDX_TIER0_DIV: tier 0's list is planned for n_reads / this many reads (default 16; 1: the whole batch)
    int no_kend = 0;      // BDX_NO_KEND: trim_side = 5 configs never take the known-end form of the wave kernel (filter + exact kernel instead)
    int no_pairs = 0;     // BDX_NO_PAIRS: never the pairs-mode kernel (bdx_pairs.hip) between tier 1 and the general kernel
    int no_win = 0;       // BDX_NO_WIN: never the window mode of the wave kernel (bdx_wave_win.hip): reads with a short column window stage whole tiles or stay on the general kernel
    int no_wave = 0;      // BDX_NO_WAVE: never the wave-autonomous kernel (bdx_wave.hip): the general fused kernel answers every read
    int wave_rw = 0;      // BDX_WAVE_RW / BDX_WAVE_WAVES: forced tile size / waves per workgroup of the wave kernel (tuning)
    int wave_waves = 0;
    int no_carry = 0;     // BDX_NO_CARRY: tier 1 of a dual config hands a listed read on without the pass it settled (the pairs mode evaluates both passes again)
    int no_staged_download = 0;  // BDX_NO_STAGED_DOWNLOAD: large result vectors go back with the runtime's own pageable copies
    int wave_maxres = 0;  // BDX_WAVE_MAXRES: resident waves per compute unit the wave kernel's geometry may plan for (default 16 = four per SIMD: the kernels need 114-128 VGPRs; tuning: the occupancy experiment of DESIGN §4)
    int cu_count = 0;     // BDX_CU_COUNT: pretend the device has this many compute units (tests of the grid sizing)
    int no_tier = 0;      // BDX_NO_TIER: no tiered budgets (every read filtered at the full budget)
    int debug = 0;        // BDX_DEBUG: honoured only by builds with -DBDX_TUNING (phase skips: results are wrong)
    int no_band_roll = 0;    // BDX_NO_BAND_ROLL: barcodes beyond 32 rows never take the exact kernel's rolling diagonal band
    int no_known_exact = 0;  // BDX_NO_KNOWN_EXACT: :exact configs stay outside the known classes
    int no_kaln = 0;         // BDX_NO_KALN: never the known-alignment forms (kend = 3) of the wave kernel and its pairs mode
    int trace_launch = 0;    // BDX_TRACE_LAUNCH: the planner says on stderr where it turned a filter set away from the wave kernel
    double wave_chance = NAN;  // BDX_WAVE_CHANCE: chance seed hits per read up to which a set gets wave tables (default 6, tier 1: 3; tuning)
    int pairs_nw = 0;        // BDX_PAIRS_NW: at least this many words per barcode mask in the pairs mode (tuning)
};

struct BdxDevRange {
    long long start_offset;
    long long end_offset;
    int start_from_end;
    int end_from_end;
};

// resolve(), classification.jl:96-100, with Julia's UnitRange normalisation (empty a:b has
// last == a-1; the callers use last(range), :800-801).
__host__ __device__ __forceinline__ void bdx_resolve_range(const BdxDevRange &dr, long long len, long long &first, long long &last) {
    long long s = dr.start_from_end ? len + dr.start_offset : dr.start_offset;
    long long e = dr.end_from_end ? len + dr.end_offset : dr.end_offset;
    long long a = s > 1 ? s : 1;
    long long b = e < len ? e : len;
    if (b < a) b = a - 1;
    first = a;
    last = b;
}

// LDS of a compute unit, and how many workgroups of `lds` bytes share it: LDS is allocated in 1280-byte granules
// (measured: 54128 B -> 2 per CU, 51872 B -> 3)
#define BDX_LDS_MAX ((size_t)160 * 1024)
inline int bdx_lds_residency(size_t lds) { return lds ? (int)(BDX_LDS_MAX / (((lds + 1279) / 1280) * 1280)) : (int)BDX_LDS_MAX; }

struct BdxDevPass {
    BdxDevRange ref_search, bc_start, bc_end;
    int trim_side;
    int n_barcodes;
    int explicit_window;
    int cand_words;  // ceil(n_barcodes / 32)
    long long win_first, win_last, win_max_start, win_min_end;
    const uint8_t *bc_bytes;    // device
    const uint32_t *bc_off;     // device, n_barcodes + 1
    const int32_t *bc_len_no_N; // device
};

struct BdxDevCfg {
    int algorithm;
    int is_dual;
    double max_error_rate;
    double min_delta;
    int match, mismatch, indel;
    int has_nindel, nindel;
    int need_traceback;
    int end_only_ok;   // per launch: the caller did not ask for pass_start (an end-only DP may serve trim_side 5)
    int max_m;
    int force_lds_dp;   // testing: use the LDS-resident DP even for short barcodes (env BDX_LDS_DP)
    int any_traceback;  // origin array needed (trim or summary in any pass)
    int counts_stride2; // max(1, B2 when dual)
    int n_counts;
    // "window upload" of the host entry point (long reads with short column windows): seq / off hold only each
    // read's window bytes; vlen[i] is the read's true length, vlo[i] the 0-based position its first uploaded byte
    // stands for.  Position p of read i lives at seq[off[i] + p - vlo[i]].  NULL: ordinary batches.
    const int32_t *vlen;
    const int32_t *vlo;
    // per launch of the exact kernel, split mode with column windows: the budget (unit operations) the fused kernel's
    // tracked sweeps used for every barcode of the pass and the lookback it subtracted from the first end column;
    // with both the exact kernel rebuilds [e_lo, e_hi] and runs the diagonal-band DP (sg_core_band).  -1: off.
    int band_kb[2];
    int band_lb[2];
    int dense_w;       // per launch: the column windows are a dense table wins[pass][read][barcode] (lo + 1024 | hi << 16), wcnt = 254
    int band_m;        // the common barcode length the band bodies run with (8, 10, 12, 16, 20, 24 or 32)
    int band_hcap;     // rolling band (sg_band_roll, barcodes beyond 32 rows in the clean class): diagonals a lane's LDS cells hold; 0: off
    unsigned int *dbg_rejected;  // device counter: hand-over windows the exact kernel refused as "not a window" (must stay 0)
    BdxDevPass pass[2];
};

struct BdxDevOut {
    int32_t *bc1, *bc2, *keep_start, *keep_end;
    int32_t *pass_start, *pass_end, *pass_raw, *pass_bc;
    double *pass_score, *pass_delta;
};

// DemuxStats histograms (classification.jl:827-865), accumulated by the exact kernel when the config asks for
// statistics (summary = true): per pass three int64 tables [rows][n_barcodes] — start position (row = start - 1
// + pos_bias: origins may lie before the read), length end - start + 1, and the integer numerator of
// the score (the host maps it to round(raw / norm, digits = 2), :835).  Row-major by KEY so that a longer read
// in a later batch only appends rows.
struct BdxDevStats {
    unsigned long long *pos[2], *len[2], *raw[2];
    long long rows;       // rows of pos (0: no statistics)
    int raw_rows;
    // len and raw live TRANSPOSED on the device, [barcode][key] with the key stride a multiple of 16 counters: nearly
    // every match of a barcode has the same length and one of two or three scores, so in [key][barcode] order the
    // whole batch would hammer the half dozen cache lines of those rows (measured: 1.0 of 3.2 ms per 2 M reads);
    // per barcode the hot keys share one line of their own.  bdx_get_stats hands them out as [key][barcode].
    int len_rows, len_stride, raw_stride;
    int pos_bias;         // = max barcode length
    unsigned int *overflow;  // set when a key does not fit (cannot happen with rows sized from the batch)
};

// Launch geometry chosen on the host for the generic (unfiltered / verify) kernel.
struct BdxGenericPlan {
    int threads;         // 64 / 128 / 256
    int reg_rows;        // 24 / 32: register-resident exact DP (no DP columns in LDS); 0: LDS columns
    int clean;           // register DP in its clean-class form (sg_core_clean): in-domain costs, start / end ranges "1:end"
    int uniform_m;       //   ... and every barcode has exactly reg_rows rows
    int uniform_len;     //   ... every barcode of the config has this length and band bodies exist for it (else 0)
    int band_roll;       // barcodes beyond 32 rows inside the clean class: the exact DP is the rolling diagonal band (sg_band_roll), dp_rows = its H + 1
    int same_len;        // every barcode of the config has the same length (the filter's first end column can be rebuilt from a hand-over row)
    int dp_rows;         // generic kernel: max_m + 1, or 1 in register mode
    int dp_rows_fused;   // fused kernel's in-kernel exact stage always keeps LDS columns: max_m + 1
    int stage_bytes;     // LDS bytes reserved for staged read bytes (0 = read from HBM/L2 directly)
    int bc_stage_bytes;  // LDS bytes for the staged barcode bytes of both passes (0 = not staged)
    int hist_entries;    // LDS histogram entries (0 = global atomics)
    size_t lds_bytes;
    int n_cu;            // compute units of the device (list-mode grid: 4 workgroups per unit)
};

// Bit-parallel (Myers) pre-filter: tables built on the host in bdx_plan.cpp, used by
// bdx_bitpar.hip.  enabled == 0 -> the config is outside the filter's domain.
struct BdxBitparPlan {
    int enabled;
    int reads_per_block;   // R: 256 / 128 / 64 / 32 / 16
    int stage_bytes;       // capacity of each staging area (raw bytes, symbol codes)
    int read_len_hint;     // the read length the geometry was planned for
    int r_cap;             // ... and the tile-size cap the batch size implied
    int diag_nw;           // diagonal variant: index words per key for this read length (5: <= 152 bases, 10: <= 312)
    int diag_qcap;         //   ... and sweep-queue entries to provide per read
    int read_len_hint_for_lds;  // same value, set before sizing (used for the seed work areas)
    int slot_bytes;        // > 0: window-slot staging (long reads with a short column window)
    int dense_w;           // per launch: split mode of the plain-sweep kernel hands the column windows over as a dense [read][barcode] table
    int dense_d;           // known-score class, plain-sweep kernels: byte table of every candidate's d (few barcodes, many genuine candidates)
    int slot_cap;          // known-score class: survivors per read and pass the replay takes (4 .. 32, from the expected number of genuine candidates)
    int seed_span;         // bases per read the seed scan covers (read length, or the window in slot mode)
    int ncode_N;           // symbol code of 'N' (255 if no barcode contains it)
    int ncodes;            // symbol codes incl. the trailing "other" code (<= 16)
    long long grid_override;  // (unused: BdxTuning::grid is applied where the grid is decided, bdx_call.cpp)
    int n_cu;              // compute units of the device: the persistent grid is n_cu x the LDS-limited residency
    int short_lb[2];       // per launch and pass: short lookback of the restricted runs (score / end-only clean-class passes)
    int dbg;               // BdxTuning::debug (only builds with -DBDX_TUNING look at it)
    int known_ok[2];       // pass qualifies for the known-score class (see bdx_bitpar.hip)
    int kb_uniform[2];  // the budget every barcode of the pass has in this filter set, or -1 (mixed)
    int tier_capped;       // tier 1: some barcode's budget was capped below its full budget
    double tier_slo[2];    //   ... per pass the smallest score a barcode beyond its capped budget can have (else +Inf)
    int bpad[2];           // barcode stride of peq[code][barcode], multiple of 32
    int *d_tile_counter;           // device int, zeroed before each launch
    const uint8_t *d_lut;          // device, 256 bytes
    int word_bytes;                // 4: 32-bit sweep words (barcodes <= 32 nt); 8: 64-bit (33..64 nt); 16: 128-bit (65..128 nt)
    const void *d_peq[2];          // device, [ncodes][bpad] sweep words
    const void *d_pvinit[2];       // device, [B]: top-aligned mask of the barcode's rows
    const int32_t *d_kb[2];        // device, [B]: max unit edit operations of a recordable alignment
    long long grid;                // per launch (bdx_call.cpp): workgroups
    size_t lds_bytes;              //   ... and LDS bytes of each
};

// q-gram seeding in front of the sweep (pigeonhole): tables built in bdx_plan.cpp.
struct BdxSeedPlan {
    int enabled;
    int q;                 // seed length in bases (5..8); key = 2 bits per base
    int bm_words;          // bitmap words (hashed: bit index = (key * 0x9E3779B1) >> (32 - bm_log2))
    int bm_log2;
    int rcap;              // sweep records per read (power of two)
    int qmul;              // sweep-record queue entries per read (the hit queue has twice as many)
    int hash_in_lds;       // hash table small enough to live in LDS
    int hash_log2;         // hash slots = 1 << hash_log2; entry = key << 16 | pass << 15 | (barcode + 1)
    int n_always[2];       // barcodes swept unconditionally (wildcards / too-short pieces)
    const uint32_t *d_bitmap;
    const uint32_t *d_hash;
    const uint8_t *d_hash_ps;      // piece start offset (bases) of every hash entry
    const uint16_t *d_always[2];
    // two-intact-pieces ("diagonal") variant for budgets too large for single seeds (see bdx_bitpar.hip)
    int diag;                      // 1: q = 4 inverted index per read + per-pair diagonal test instead of bitmap / hash
    int diag_kmax;                 // largest operation budget among the seeded barcodes
    double diag_flag_coef;         // expected flagged pairs per read = coef * ((L - 3) / 256)^2 / (L + 24) for reads of L bases
    const uint32_t *d_dmeta[2];    // per barcode: pieces | piece length << 8 (0 = swept unconditionally)
    const uint32_t *d_dkeys[2];    // per barcode: 2 words, 8 bits per piece key (first 4 bases of the piece)
};

// Wave-autonomous seeded kernel (bdx_wave.hip): the single-seed filter + reducer replay of known-score configs whose
// barcodes are plain A/C/G/T, every wave on a tile of its own (no workgroup barriers), bytes transcoded arithmetically.
// Tables are built next to the seed tables of a filter set (bdx_plan.cpp, build_wave_tables); the geometry per batch.
struct BdxWavePlan {
    int enabled;           // config-level eligibility of this filter set
    uint32_t *d_carry = nullptr;  // per launch (dual tiered known-class configs, min_delta = 0): tier 1 leaves the winning survivor of the ONE pass it settled
                                  // for a read it lists here (indexed by read; two state bits ride on the list entry) and the pairs mode takes it over
    int q;                 // seed length (6..8)
    int n_ent;             // seed table entries (one per (key, barcode, piece start))
    int n_barcodes;        // of all passes together (the barcodes of pass 1 are numbered behind those of pass 0)
    int b0;                // barcodes of pass 0
    int split;             // the set's config is outside the known-score class: the kernel only filters (candidate masks + column windows for the exact kernel)
    int bm_bytes;          // direct bitmap over the 4^q keys
    int track_from;        // columns [0, track_from) of a sweep cannot end an alignment within any barcode's budget
    const uint8_t *d_bitmap;
    const uint16_t *d_rank;      // [bm_bytes / 4]: keys present below each 32-bit word of the bitmap
    const uint32_t *d_ent;       // barcode + 1 | piece start << 11 | next entry of the same key << 16
    const uint32_t *d_peq8;      // [B][9] (stride 9 dwords): rows A, C, T, G ((byte >> 1) & 3), 4..7 = symbols no barcode contains
    const uint32_t *d_peq8r;     // the same for the reversed barcodes (known-trim class: trim_side = 3 passes are swept right to left)
    const uint32_t *d_meta;      // [B]: m | kb << 8 | lone-survivor accept threshold << 16
    const uint32_t *d_settle;    // [B]: tier 1 settle bits of a lone survivor per distance (no_delta | with_delta << 16)
    // per batch (size_wave)
    int rw;                // reads per wave tile (32 / 16 / 8)
    int waves;             // waves per workgroup
    int blocks;            // persistent grid
    int span_cap;          // bytes of a tile's span the images hold
    int read_len_hint;     // the read length the geometry was planned for
    int hq_cap, sq_cap;    // entries of a tile's hit queue / sweep list (from the expected chance hits per read)
    int cand_words;        // split mode: candidate mask words per read (both passes)
    int scan_gpr;          // ranged single-pass configs (per batch): groups of sixteen positions scanned per read, 0: the whole flat image
    int ranged;            // some pass has a ref_search_range other than the whole read: per-read column windows in the kernel
    int winm;              // per batch: window mode (bdx_wave_win.hip): scattered tiles that hold only each read's ref_search_range window (`slot` positions per read)
    int kend;              // known-trim class (any trim side per pass): the non-split kernel with position keys — 1: trim sides 5 / none (bdx_wave_end.hip), 2: with reversed
                           // sweeps for trim_side = 3 (bdx_wave_rev.hip), 3: the known-ALIGNMENT class — both positions of every winner by anchored sweeps, statistics (bdx_wave_aln.hip)
    double chance;         // expected chance seed hits per 150-base read (config)
    // pairs mode (two-intact-pieces filter over a gathered list of reads; bdx_pairs.hip): d_bitmap holds the piece
    // tables [kb + 2][256] of barcode masks, there is no hash
    int pairs_kb;          // 0: single seeds; 3 / 4: two intact 4-base pieces within that many diagonals (the largest budget); 8 / 9: two intact
                           // pieces on the SAME diagonal, of six 4-base / eight 3-base pieces (configs whose indels cost more than their mismatches)
    int pairs_spread;      // pairs mode: columns a flagged alignment can lie off its diagonal (classic: the budget; same-diagonal variants: the largest number of indels)
    int nw;                // words of a barcode mask
    int groups;            // groups of 128 barcodes (more than 128 barcodes: one set of piece tables per group, nw = 4)
    int slot;              // pairs mode: flat positions per read of a (scattered) tile: the read length + 15 (its address mod 16), rounded up to 16
    int cpr;               // 16-diagonal chunks scanned per read
    // per launch (bdx_call.cpp)
    long long grid;        // workgroups: `blocks`, but no more than give every wave a tile
    size_t lds_bytes;      // the tables + one work area per wave
    int dbg;               // BdxTuning::debug as this kernel reads it (the pairs mode: shifted down by eight bits)
};

// ---- what one classify call hands its launchers ----
// The batch: one per bdx_classify_device call.  A launch that must not count (a filter in split form) gets uncounted().
struct BdxBatch {
    const uint8_t *seq;
    const long long *off;
    long long n_reads;
    BdxDevOut out;
    unsigned long long *counts;
    hipStream_t stream;
    BdxBatch uncounted() const { return BdxBatch{seq, off, n_reads, out, nullptr, stream}; }
};

// The split-mode hand-over from a filter (fused kernel, wave kernel, pairs mode) to the exact kernel, per pass: candidate
// masks [read][cand_words], column windows with their entry counts (null: the call runs without windows), and whether the
// restricted runs take the short lookback.  A single-pass call has cand_words[1] = 0 and pass 0's buffers in both places.
// A launch that is no part of a hand-over gets an empty one (BdxHandOver{}).
struct BdxHandOver {
    int cand_words[2];
    uint32_t *cand[2];
    uint32_t *wins[2];
    uint8_t *wcnt[2];
    int short_lb[2];
};

// A list of read numbers on the device with its length.  ids == nullptr: no list (an input: every read of the batch).
struct BdxDevList {
    uint32_t *ids;
    unsigned int *count;
};

// The lists of a launch: it runs over in.ids[0 .. *in.count) (list mode) and appends the reads it cannot settle to out.
// tier1: the launch is tier 1 of the tiered budgets; slo: per pass the smallest score a barcode beyond its capped budget can have.
struct BdxTierArgs {
    BdxDevList in, out;
    int tier1;
    double slo[2];
};

// index sub-batch of the fused kernel's diagonal variant at the narrow index width (bdx_bitpar.hip)
#ifndef BDX_DIAG_SB_NARROW
#define BDX_DIAG_SB_NARROW 8
#endif
// LDS bytes of a workgroup of the fused kernel (bdx_call.cpp; mirrors the carve-up at the head of bdx_bitpar_kernel)
size_t bdx_bitpar_lds_bytes(const BdxDevCfg &cfg, const BdxBitparPlan &bp, const BdxGenericPlan &gp,
                            const BdxSeedPlan *sp = nullptr);
// Implemented in bdx_bitpar.hip.  exc: the known-score form lists the reads it hands to the exact kernel after all
// (no list: split form — masks and windows of every read into `ho`, no verdicts).
hipError_t bdx_launch_bitpar(const BdxDevCfg &cfg, const BdxGenericPlan &gp, const BdxBitparPlan &bp, const BdxSeedPlan &sp, const BdxBatch &b,
                             const BdxHandOver &ho, const BdxDevList &exc, const BdxTierArgs &t);
// max read length of a device-resident batch (one tiny kernel; result written to *d_out)
hipError_t bdx_launch_maxlen(const long long *d_off, long long n_reads, int *d_out, hipStream_t stream);
hipError_t bdx_launch_copy(void *d_dst, const void *src_mapped, size_t bytes, hipStream_t stream, void *d_zero = nullptr, int zero_bytes = 0);

// The wave-autonomous kernel (bdx_wave_kernel.h) is compiled in six translation units, one set of instantiations each.
// Implemented in bdx_wave.hip (the known-score and plain split-mode instantiations: whole ranges, one pass).
// LDS bytes of the shared tables / of one wave's work area (must mirror the kernel's carve-up); the planner (bdx_plan.cpp)
// and the launchers share this one copy
inline size_t bdx_wave_table_bytes(const BdxWavePlan &wp, int hist_entries) {
    auto al = [](size_t x) { return (x + 31) & ~(size_t)31; };
    return al((size_t)wp.bm_bytes) + al(wp.pairs_kb > 0 ? 0 : (size_t)wp.bm_bytes / 2) + al((size_t)wp.n_ent * 4) + al((size_t)wp.n_barcodes * 36) +
           al(wp.kend >= 2 ? (size_t)wp.n_barcodes * 36 : 0) + 2 * al((size_t)wp.n_barcodes * 4) + al((size_t)hist_entries * 4);
}
inline size_t bdx_wave_area_bytes(int rw, int span_cap, bool pairs, int hq_cap, int sq_cap, int cand_words, bool winm = false) {
    const size_t nvec = (size_t)span_cap >> 4;
    const size_t recs = pairs ? 0 : 2 * (size_t)rw * 8 * 4;  // record tables
    const size_t fixed = (size_t)(((rw + 1) * 4 + 15) / 16 * 16) + recs + (size_t)rw * 16 + 3 * (size_t)rw * 4 + 256 +
                         ((pairs || winm) ? 2 * (size_t)rw * 4 + 16 + 2 * (size_t)rw * 20 : 0) + ((winm || pairs) ? (size_t)rw * 4 + 2 * (size_t)rw * 4 : 0);
    const size_t o = fixed + ((nvec + 2 + 3) & ~(size_t)3) * 4 + ((2 * nvec + 6 + 3) & ~(size_t)3) * 4 + ((size_t)hq_cap + (pairs ? 0 : (size_t)sq_cap) + (size_t)rw * (size_t)cand_words) * 4;
    return (o + 31) & ~(size_t)31;
}
// ... of the plan `wp` (window mode keeps no candidate words)
inline size_t bdx_wave_area_bytes(const BdxWavePlan &wp) {
    return wp.winm ? bdx_wave_area_bytes(wp.rw, wp.span_cap, false, wp.hq_cap, wp.sq_cap, 0, true)
                   : bdx_wave_area_bytes(wp.rw, wp.span_cap, wp.pairs_kb > 0, wp.hq_cap, wp.sq_cap, wp.cand_words + (wp.ranged ? 4 : 0));
}
// (ho: the split form's outputs, else empty; t.out: the reads the kernel does not answer)
hipError_t bdx_launch_wave(const BdxDevCfg &cfg, const BdxWavePlan &wp, int hist_entries, const BdxBatch &b, const BdxHandOver &ho, const BdxTierArgs &t);
// Implemented in bdx_wave_end.hip (the known-end class: its forward-sweep instantiations are there, the reversed ones in
// bdx_wave_rev.hip, the known-alignment ones in bdx_wave_aln.hip).  (stats / pass_start: the known-alignment class only, kend = 3)
hipError_t bdx_launch_wave_end(const BdxDevCfg &cfg, const BdxWavePlan &wp, int hist_entries, const BdxBatch &b, const BdxTierArgs &t, const BdxDevStats *stats);
// Implemented in bdx_wave_win.hip (the window-mode instantiations: single-pass known-score configs whose column window is much
// shorter than their reads — only the windows are fetched).
hipError_t bdx_launch_wave_win(const BdxDevCfg &cfg, const BdxWavePlan &wp, int hist_entries, const BdxBatch &b, const BdxTierArgs &t);
// Implemented in bdx_pairs.hip (the pairs-mode instantiations; those of the known-end class with reversed sweeps are in
// bdx_wave_rev.hip, the known-alignment ones in bdx_wave_aln.hip).
// (the listed reads t.in are fetched straight from the batch; no input list: every read of the batch)
hipError_t bdx_launch_pairs(const BdxDevCfg &cfg, const BdxWavePlan &wp, int hist_entries, const BdxBatch &b, const BdxHandOver &ho, const BdxTierArgs &t,
                            const BdxDevStats *stats);

// Implemented in bdx_device.hip.  blocks: the grid (CallPlan); zero_words: the call's last launch clears these scratch words.
hipError_t bdx_launch_generic(const BdxDevCfg &cfg, const BdxGenericPlan &plan, const BdxBatch &b, const BdxHandOver &ho, const BdxTierArgs &t,
                              const BdxDevStats *stats, long long blocks, uint32_t *zero_words);
// Launch log of the classify call in progress on this thread (bdx_last_launches; bdx_abi.cpp): the launchers note every
// classify kernel they enqueue while bdx_launch_logging() holds.  tile: reads per tile; units: what the tiles are dealt
// over (0: no tile loop); list: `reads` is the capacity of a device-side list.
bool bdx_launch_logging();
void bdx_note_launch(const char *family, const char *kernel, long long blocks, int threads, int tile, long long units, long long reads, int list);
// One 512-byte half of the context's 1 KiB scratch block (bdx_ctx::d_maxlen).  The halves alternate between calls and a
// call's last launch clears the other one's words behind `head` (bdx_abi.cpp), which then needs no memset of its own.
struct BdxScratch {
    int head[16];                 // word 0 of half 0 receives bdx_launch_maxlen's result; never cleared by a launch
    int tile_queue[16];           // tile queue of the call's full-budget fused launch
    unsigned int exc_count;       // reads the known-score fused kernel hands to the exact kernel ...
    unsigned int tune_stats[3];   //   ... and its tuning statistics (builds with -DBDX_TUNING)
    unsigned int pad0[12];
    unsigned int front_count;     // length of the front stage's / tier 1's list
    unsigned int pad1[15];
    int tile_queue_t1[16];        // tile queue of tier 1's fused launch
    unsigned int mid_count;       // length of the pairs mode's list
    unsigned int pad2[47];
};
static_assert(offsetof(BdxScratch, tile_queue) == 64 && offsetof(BdxScratch, exc_count) == 128 && offsetof(BdxScratch, tune_stats) == 132 &&
                  offsetof(BdxScratch, front_count) == 192 && offsetof(BdxScratch, tile_queue_t1) == 256 && offsetof(BdxScratch, mid_count) == 320 &&
                  sizeof(BdxScratch) == 512,
              "the kernels and bdx_last_list_reads find the scratch words at these offsets");
// the words a launch clears: everything behind `head`
constexpr int BDX_SCRATCH_WORDS = (int)((sizeof(BdxScratch) - offsetof(BdxScratch, tile_queue)) / 4);
static_assert(BDX_SCRATCH_WORDS == 112, "bytes [64, 512) of a half");
hipError_t bdx_generic_set_lds_limit(size_t bytes);
// test switch BDX_POISON: checks (and sanitises) one hand-over between a producer and its consumer (bdx_device.hip)
// (list: checked when given; pass >= 0: also that pass's windows and masks in `ho` for these reads)
hipError_t bdx_launch_poison_check(const BdxBatch &b, const BdxDevList &list, const BdxHandOver &ho, int pass, int n_barcodes, int check_list, unsigned int *dbg);
