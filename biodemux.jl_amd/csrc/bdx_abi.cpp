// bdx_abi.cpp — C-ABI of libbiodemux_hip.so (see include/biodemux_hip.h for the contract and
// the reference lines each entry point replaces).  Host-side only: validation, table upload,
// launch planning (the host entry point, bdx_classify_host, is bdx_host.cpp).  All arithmetic of the hot path runs in the gfx950
// kernels of bdx_device.hip / bdx_filter.hip; there is NO CPU fallback — without a usable
// HIP device every entry point fails with BDX_E_DEVICE.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <new>
#include <string>
#include <vector>

#include "bdx_ctx.h"

thread_local std::string g_create_error;
static std::atomic<long long> g_rejected_windows{0};  // summed over the contexts destroyed so far (see bdx_debug_rejected_windows_total)
static thread_local std::string *t_launch_log = nullptr;  // the log of the classify call in progress on this thread

bool bdx_launch_logging() { return t_launch_log != nullptr; }

void bdx_note_launch(const char *family, const char *kernel, long long blocks, int threads, int tile, long long units, long long reads, int list) {
    if (!t_launch_log) return;
    char line[256];
    snprintf(line, sizeof line, "%s\t%s\t%lld\t%d\t%d\t%lld\t%lld\t%d\n", family, kernel, blocks, threads, tile, units, reads, list);
    *t_launch_log += line;
}

int bdx_fail(bdx_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx)
        ctx->err = buf;
    else
        g_create_error = buf;
    return code;
}

namespace {

#define fail bdx_fail

BdxTuning read_tuning() {
    BdxTuning t;
    t.no_known = getenv("BDX_NO_KNOWN") != nullptr;
    t.no_seed = getenv("BDX_NO_SEED") != nullptr;
    t.no_diag = getenv("BDX_NO_DIAG") != nullptr;
    t.no_windows = getenv("BDX_NO_WINDOWS") != nullptr;
    t.no_slot = getenv("BDX_NO_SLOT") != nullptr;
    t.lds_dp = getenv("BDX_LDS_DP") != nullptr;
    t.no_tier = getenv("BDX_NO_TIER") != nullptr;
    t.no_wave = getenv("BDX_NO_WAVE") != nullptr;
    t.no_win = getenv("BDX_NO_WIN") != nullptr;
    t.no_pairs = getenv("BDX_NO_PAIRS") != nullptr;
    t.no_kend = getenv("BDX_NO_KEND") != nullptr;
    if (const char *e = getenv("BDX_TIER0_DIV")) t.tier0_div = atoi(e);
    t.poison = getenv("BDX_POISON") != nullptr;
    if (const char *e = getenv("BDX_WAVE_RW")) t.wave_rw = atoi(e);
    if (const char *e = getenv("BDX_WAVE_WAVES")) t.wave_waves = atoi(e);
    if (const char *e = getenv("BDX_WAVE_MAXRES")) t.wave_maxres = atoi(e);
    t.no_staged_download = getenv("BDX_NO_STAGED_DOWNLOAD") != nullptr;
    t.no_carry = getenv("BDX_NO_CARRY") != nullptr;
    if (const char *e = getenv("BDX_CU_COUNT")) t.cu_count = atoi(e);
    t.no_clean = getenv("BDX_NO_CLEAN") != nullptr;
    t.no_band = getenv("BDX_NO_BAND") != nullptr;
    t.no_dense = getenv("BDX_NO_DENSE") != nullptr;
    t.no_pipeline = getenv("BDX_NO_PIPELINE") != nullptr;
    if (const char *e = getenv("BDX_TIER_Q")) t.tier_q = atoi(e);
    t.no_window_upload = getenv("BDX_NO_WINDOW_UPLOAD") != nullptr;
    t.seed_hash_l2 = getenv("BDX_SEED_HASH_L2") != nullptr;
    if (const char *e = getenv("BDX_SEED_BM_LOG2")) t.seed_bm_log2 = atoi(e);
    if (const char *e = getenv("BDX_BITPAR_R")) t.bitpar_r = atoi(e);
    if (const char *e = getenv("BDX_GRID")) t.grid = atoll(e);
    if (const char *e = getenv("BDX_DIAG_MIN_B")) t.diag_min_b = atoi(e);
#ifdef BDX_TUNING
    if (const char *e = getenv("BDX_DEBUG")) t.debug = atoi(e);
#endif
    // BDX_NO_WAVE_FALLBACK: known-score forms of the wave kernel list a read whose record tables overflow instead of sweeping
    // it over every barcode themselves (results identical; bdx_last_list_reads shows the difference) — bit 30 of the kernels' dbg word
    if (getenv("BDX_NO_WAVE_FALLBACK")) t.debug |= 1 << 30;
    return t;
}

BdxDevRange cvt_range(const bdx_range_t &r) {
    BdxDevRange d;
    d.start_offset = r.start_offset;
    d.end_offset = r.end_offset;
    d.start_from_end = r.start_from_end != 0;
    d.end_from_end = r.end_from_end != 0;
    return d;
}

const size_t LDS_MAX = 160 * 1024;

// Launch planning for the exact-evaluation kernel: per-lane DP (+origin) columns, barcode
// tables, count histogram and the read staging area must fit the CU's 160 KiB of LDS.
int plan_generic(bdx_ctx *ctx) {
    const BdxDevCfg &d = ctx->dev;
    BdxGenericPlan &p = ctx->plan;
    // SimpleScoring barcodes of <= 32 rows run the register-resident DP: no LDS columns at all
    p.reg_rows = (!d.has_nindel && d.algorithm == BDX_ALG_SEMIGLOBAL && !d.force_lds_dp)
                     ? (d.max_m <= 24 ? 24 : (d.max_m <= 32 ? 32 : 0)) : 0;
    // clean class (bdx_core.h sg_core_clean): costs match >= 0, mismatch / indel >= 1, and barcode_start_range /
    // barcode_end_range that resolve to 1:n for every read (no offset from either end) — then neither binds
    p.clean = 0;
    p.uniform_m = 0;
    p.uniform_len = 0;
    if (p.reg_rows && !ctx->tune.no_clean && d.match >= 0 && d.mismatch >= 1 && d.indel >= 1) {
        bool free_ranges = true, uniform = true;
        int len0 = -1;
        bool same_len = true;
        for (int k = 0; k < (d.is_dual ? 2 : 1); ++k) {
            const bdx_pass_t &ps = ctx->cfg.pass[k];
            const auto whole = [](const bdx_range_t &r) { return !r.start_from_end && r.start_offset <= 1 && r.end_from_end && r.end_offset >= 0; };
            free_ranges = free_ranges && ps.explicit_window == 0 && whole(ps.barcode_start_range) && whole(ps.barcode_end_range);
            for (int b = 0; b < ps.n_barcodes; ++b) {
                const int m = (int)(ps.bc_off[b + 1] - ps.bc_off[b]);
                uniform = uniform && m == p.reg_rows;
                if (len0 < 0) len0 = m;
                same_len = same_len && m == len0;
            }
        }
        p.clean = free_ranges;
        p.uniform_m = free_ranges && uniform;
        // the diagonal-band bodies exist for these barcode lengths (every barcode of the config alike)
        const bool band_len = len0 == 8 || len0 == 10 || len0 == 12 || len0 == 16 || len0 == 20 || len0 == 24 || len0 == 32;
        p.uniform_len = (free_ranges && same_len && band_len) ? len0 : 0;
    }
    // Barcodes beyond the register DP's 32 rows inside the clean class: the rolling diagonal band (bdx_core.h sg_band_roll) —
    // H = two operation budgets at the configured rate + 9 end columns per chunk — instead of max_m + 1 LDS rows per lane
    // (80-nt barcodes with trimming: 648 B per lane = ONE 128-lane workgroup per CU; 26 cells: two 256-lane workgroups).
    p.band_roll = 0;
    p.same_len = 0;
    ctx->dev.band_hcap = 0;
    // (only behind a filter: without hand-over windows — filter off, barcodes beyond the sweep's 128 rows — every candidate
    // would be walked over its whole window in chunks, three times the full matrix, where sg_core's cut-off visits a few rows
    // per column: 160-nt barcodes unfiltered 0.3 -> 0.03 M reads/s, measured; bdx_create plans again once the filter is known)
    if (!p.reg_rows && d.max_m > 32 && !d.has_nindel && d.algorithm == BDX_ALG_SEMIGLOBAL && !d.force_lds_dp && !ctx->tune.no_clean &&
        !ctx->band_roll_off && !getenv("BDX_NO_BAND_ROLL") && d.match >= 0 && d.mismatch >= 1 && d.indel >= 1) {
        bool free_ranges = true, same_len = true;
        int len0 = -1, kb_max = 0;
        const int cmin = d.mismatch < d.indel ? d.mismatch : d.indel;
        for (int k = 0; k < (d.is_dual ? 2 : 1); ++k) {
            const bdx_pass_t &ps = ctx->cfg.pass[k];
            const auto whole = [](const bdx_range_t &r) { return !r.start_from_end && r.start_offset <= 1 && r.end_from_end && r.end_offset >= 0; };
            free_ranges = free_ranges && ps.explicit_window == 0 && whole(ps.barcode_start_range) && whole(ps.barcode_end_range);
            for (int b = 0; b < ps.n_barcodes; ++b) {
                const int m = (int)(ps.bc_off[b + 1] - ps.bc_off[b]);
                if (len0 < 0) len0 = m;
                same_len = same_len && m == len0;
                const int kb = (int)std::floor(d.max_error_rate * (double)m) / cmin;  // (ae as the device computes it, :254; the threshold only tightens)
                kb_max = kb > kb_max ? kb : kb_max;
            }
        }
        // H: at least two budgets + 9 end columns per chunk; up to four budgets + 9 (a clean occurrence has end columns within
        // the budget on either side: one chunk) while two 256-lane workgroups still fit a CU (8 bytes per cell and lane)
        int hcap = 2 * kb_max + 9;
        {
            size_t bc_bytes = 0;
            int nb = 0;
            for (int k = 0; k < (d.is_dual ? 2 : 1); ++k) {
                bc_bytes += ctx->cfg.pass[k].bc_off[ctx->cfg.pass[k].n_barcodes];
                nb += ctx->cfg.pass[k].n_barcodes;
            }
            // (what the workgroup keeps in LDS besides the cells — barcode bytes and tables, the counter histogram — as below)
            const size_t other = (bc_bytes <= 32 * 1024 ? bc_bytes : 0) + (size_t)nb * 8 + (size_t)(d.n_counts <= 2048 ? d.n_counts : 2048) * 4 + 256;
            const size_t room = other + 2048 < (size_t)76 * 1024 ? (size_t)76 * 1024 - other - 2048 : 0;
            const int fit2 = (int)(room / (256 * (d.any_traceback ? 8 : 4))) - 1;  // cells per lane of a workgroup that shares the CU with another one
            const int want = 4 * kb_max + 9;
            const int roomy = want < fit2 ? want : fit2;
            if (roomy > hcap) hcap = roomy;
        }
        if (free_ranges && hcap + 1 < d.max_m + 1 && d.max_error_rate >= 0.0 && d.max_error_rate <= 1.0) {
            p.band_roll = 1;
            p.same_len = same_len ? 1 : 0;
            ctx->dev.band_hcap = hcap;
        }
    }
    p.dp_rows = p.reg_rows ? 1 : (p.band_roll ? ctx->dev.band_hcap + 1 : d.max_m + 1);
    p.dp_rows_fused = d.max_m + 1;
    const size_t per_thread = (size_t)p.dp_rows * 4 * (d.any_traceback ? 2 : 1);
    const int B0 = d.pass[0].n_barcodes, B1 = d.is_dual ? d.pass[1].n_barcodes : 0;
    size_t bc_total = 0;
    for (int k = 0; k < (d.is_dual ? 2 : 1); ++k) bc_total += ctx->cfg.pass[k].bc_off[ctx->cfg.pass[k].n_barcodes];
    p.bc_stage_bytes = bc_total <= 32 * 1024 ? (int)((bc_total + 15) & ~(size_t)15) : 0;
    p.hist_entries = d.n_counts <= 2048 ? d.n_counts : 2048;  // LDS histogram: the scalars + the first per-barcode slots (>= 4)
    const size_t fixed = (size_t)(B0 + 1 + B1 + 1 + B0 + B1) * 4 + 16 + (size_t)p.bc_stage_bytes + 16 +
                         (size_t)p.hist_entries * 4 + 16;
    const int tries[3] = {256, 128, 64};
    for (int t : tries) {
        const size_t need = fixed + per_thread * (size_t)t;
        if (need + 4096 > LDS_MAX && !(t == 64 && need <= LDS_MAX)) continue;
        p.threads = t;
        // Read staging: aim for two resident workgroups per CU (<= 80 KiB each) when that
        // still leaves room for ~192 B per read; otherwise take what is left of the CU.
        // two workgroups per CU (the exact kernels are compiled for two waves per SIMD); the rolling band keeps clear of the last
        // granules (measured on the fused kernel: three workgroups of 54 128 B do not share a CU, three of 51 872 B do)
        const size_t share = p.band_roll ? 77 * 1024 : 80 * 1024;
        size_t budget = need < share ? share - need : 0;
        // (the rolling band is bound by the latency of its LDS chain: resident waves first — two workgroups per CU with whatever
        // staging still fits, reads that do not fit come straight from L2)
        if (budget < (size_t)t * 192 && !(p.band_roll && need <= share)) budget = LDS_MAX - need;
        size_t stage = budget > 64 * 1024 ? 64 * 1024 : budget;
        stage &= ~(size_t)15;
        if (stage < 1024 || p.bc_stage_bytes == 0) stage = 0;
        p.stage_bytes = (int)stage;
        p.lds_bytes = need + stage;
        return BDX_OK;
    }
    return fail(ctx, BDX_E_INVALID,
                "barcodes too long for the on-chip DP columns: max length %d needs %zu B of LDS per lane "
                "(limit: 64 lanes within 160 KiB)",
                d.max_m, per_thread);
}

// ---- tiered budgets --------------------------------------------------------------------------
// Single q-gram seeds are only selective when a barcode's kb + 1 pieces keep >= 8 bases (C2: kb = 2 on 24 nt).
// The reference's default rate 0.2 allows kb = 4 there, which needs the much costlier two-intact-pieces
// filter — although nearly every read that carries a barcode carries it with 0..2 errors.  Tier 1 therefore
// filters with budgets CAPPED at kb1 = m / 8 - 1: it finds, losslessly, every barcode within kb1 operations
// (exact unit distances).  Both reducers of the reference only ever look at the smallest (and second
// smallest) score, so whenever tier 1 finds a barcode and no barcode it cannot see could tie or beat it
// (bdx_bitpar.hip, "tier settle rule"), the read's verdict is final; only the other reads — those without a
// barcode, or with one beyond kb1 — are filtered again at the full budget (tier 0, in list mode).
long long tier_cap(const bdx_ctx *ctx, int m) {
    if (ctx->cur == 0) return (1LL << 40);
    if (ctx->tier_cap_fixed >= 0) return ctx->tier_cap_fixed;  // (the pairs tier)
    const int q = ctx->tier_q >= 5 && ctx->tier_q <= 8 ? ctx->tier_q : 8;
    const int c = m / q - 1;
    return c > 0 ? c : 0;
}

// ---- bit-parallel pre-filter: eligibility and tables (see bdx_bitpar.hip for the argument) ----
int build_bitpar_tables(bdx_ctx *ctx) {
    const bdx_config_t &c = ctx->cfg;
    BdxBitparPlan &bp = ctx->F().bplan;
    bp = BdxBitparPlan{};
    bp.tier_slo[0] = bp.tier_slo[1] = HUGE_VAL;
    if (c.filter == BDX_FILTER_OFF) return BDX_OK;
    const int npass = c.is_dual ? 2 : 1;
    // cost domain: every edit operation must cost >= 1 and a match >= 0
    int cmin = 1;
    if (c.algorithm == BDX_ALG_SEMIGLOBAL) {
        cmin = c.mismatch < c.indel ? c.mismatch : c.indel;
        if (c.has_nindel && c.nindel < cmin) cmin = c.nindel;
        if (c.match < 0 || cmin < 1) return BDX_OK;
    }
    const bool n_wild = (c.algorithm == BDX_ALG_SEMIGLOBAL && c.has_nindel) || c.algorithm == BDX_ALG_HAMMING;
    // alphabet = distinct barcode bytes (<= 15: the IUPAC letters), everything else shares the "other" code
    int code_of[256];
    for (int i = 0; i < 256; ++i) code_of[i] = -1;
    int K = 0;
    size_t cand_words = 0;
    size_t wb = 4;
    for (int k = 0; k < npass; ++k) {
        const bdx_pass_t &p = c.pass[k];
        cand_words += (size_t)(p.n_barcodes + 31) / 32;
        for (int b = 0; b < p.n_barcodes; ++b) {
            const uint32_t m = p.bc_off[b + 1] - p.bc_off[b];
            if (m > 128) return BDX_OK;  // one sweep word per barcode: 32 bits, 64 for barcodes of 33..64 nt, 128 for 65..128 nt
            if (m > 64) wb = 16;
            else if (m > 32 && wb < 8) wb = 8;
            for (uint32_t i = 0; i < m; ++i) {
                const uint8_t ch = p.bc_bytes[p.bc_off[b] + i];
                if (code_of[ch] < 0) {
                    if (K == 15) return BDX_OK;
                    code_of[ch] = K++;
                }
            }
        }
    }
    if (cand_words > 128) return BDX_OK;  // <= 4096 barcodes per config (both passes together)
    bp.ncodes = K + 1;
    bp.ncode_N = code_of['N'] >= 0 ? code_of['N'] : 255;
    std::vector<uint8_t> lut(256);
    for (int i = 0; i < 256; ++i) lut[i] = (uint8_t)(code_of[i] < 0 ? K : code_of[i]);
    size_t bytes = 256;
    bp.word_bytes = (int)wb;
    size_t o_peq[2] = {0, 0}, o_pv[2] = {0, 0}, o_kb[2] = {0, 0};
    for (int k = 0; k < npass; ++k) {
        const int B = c.pass[k].n_barcodes;
        bp.bpad[k] = 32;  // power of two >= B: peq row address = code << log2(4*bpad)
        while (bp.bpad[k] < B) bp.bpad[k] <<= 1;
        if ((size_t)bp.ncodes * bp.bpad[k] * wb > 96 * 1024) return BDX_OK;  // the table lives in LDS
        bytes = (bytes + 15) & ~(size_t)15;
        o_peq[k] = bytes;
        bytes += (size_t)bp.ncodes * bp.bpad[k] * wb;
        o_pv[k] = bytes;
        bytes += (size_t)B * wb;
        o_kb[k] = bytes;
        bytes += (size_t)B * 4;
    }
    std::vector<uint8_t> blob(bytes, 0);
    memcpy(blob.data(), lut.data(), 256);
    for (int k = 0; k < npass; ++k) {
        const bdx_pass_t &p = c.pass[k];
        uint8_t *peq = blob.data() + o_peq[k];
        uint8_t *pv = blob.data() + o_pv[k];
        int32_t *kb = (int32_t *)(blob.data() + o_kb[k]);
        const int bits = (int)wb * 8;
        bp.kb_uniform[k] = -2;  // (unset)
        typedef unsigned __int128 u128;
        const auto put = [&](uint8_t *dst, size_t idx, u128 v) {
            if (wb == 16)
                memcpy(dst + idx * 16, &v, 16);
            else if (wb == 8)
                ((uint64_t *)dst)[idx] = (uint64_t)v;
            else
                ((uint32_t *)dst)[idx] = (uint32_t)v;
        };
        for (int b = 0; b < p.n_barcodes; ++b) {
            const int m = (int)(p.bc_off[b + 1] - p.bc_off[b]);
            const int shift = bits - m;
            const u128 all = bits == 128 ? ~(u128)0 : (((u128)1 << bits) - 1);
            const u128 rows = m == bits ? all : ((((u128)1 << m) - 1) << shift);
            const u128 pad = ~rows & all;  // virtual rows below the barcode: match everything, D stays 0
            put(pv, (size_t)b, rows);
            for (int code = 0; code < bp.ncodes; ++code) {
                u128 mask = pad;
                for (int i = 0; i < m; ++i) {
                    const uint8_t ch = p.bc_bytes[p.bc_off[b] + i];
                    const bool wild = n_wild && ch == 'N';
                    if (wild || (code < K && code_of[ch] == code)) mask |= (u128)1 << (shift + i);
                }
                put(peq, (size_t)code * bp.bpad[k] + b, mask);
            }
            // allowed_error at the initial threshold, exactly as the device computes it
            long long ae;
            if (c.algorithm == BDX_ALG_EXACT)
                ae = 0;
            else if (c.algorithm == BDX_ALG_HAMMING)
                ae = (long long)std::floor(c.max_error_rate * (double)m);
            else
                ae = (long long)std::floor(c.max_error_rate * (double)(c.has_nindel ? p.bc_len_no_N[b] : m));
            long long kfull = ae < 0 ? -1 : ae / cmin;
            long long kcap = kfull;
            if (kcap > tier_cap(ctx, m)) kcap = tier_cap(ctx, m);
            kb[b] = (int32_t)kcap;
            bp.kb_uniform[k] = bp.kb_uniform[k] == -2 ? (int)kcap : (bp.kb_uniform[k] == (int)kcap ? (int)kcap : -1);
            if (kcap < kfull) {
                // the smallest score a barcode tier 1 cannot see may have: (kb1 + 1) operations of cost >= cmin
                // each, over this barcode's normalisation (computed as the device computes a score)
                const double norm = (c.algorithm == BDX_ALG_SEMIGLOBAL && c.has_nindel) ? (double)p.bc_len_no_N[b] : (double)m;
                const double lo = (double)((kcap + 1) * cmin) / norm;
                if (lo < bp.tier_slo[k]) bp.tier_slo[k] = lo;
                bp.tier_capped = 1;
            }
        }
    }
    HIP_TRY(ctx, ctx->F().bp_tables.ensure(bytes));
    HIP_TRY(ctx, hipMemcpy(ctx->F().bp_tables.p, blob.data(), bytes, hipMemcpyHostToDevice));
    const uint8_t *base = (const uint8_t *)ctx->F().bp_tables.p;
    bp.d_lut = base;
    for (int k = 0; k < npass; ++k) {
        bp.d_peq[k] = base + o_peq[k];
        bp.d_pvinit[k] = base + o_pv[k];
        bp.d_kb[k] = (const int32_t *)(base + o_kb[k]);
    }
    // Reducer replay capacity: short barcodes at high rates have many GENUINE candidates per read (a 10-mer within two
    // edits of a random 150-base read is common: ~25 of 96 barcodes), and a read with more survivors than the replay
    // holds costs a full exact DP per candidate.  Expected candidates per read ~ sum over barcodes of
    // 150 * V(m, kb) / 4^m with V = sum_{e <= kb} C(m, e) 8^e (3 substitutions, 4 insertions, 1 deletion per site).
    {
        double expected = 0.0;
        for (int k = 0; k < npass; ++k) {
            const bdx_pass_t &p = c.pass[k];
            const int32_t *kbh = (const int32_t *)(blob.data() + o_kb[k]);
            for (int b = 0; b < p.n_barcodes; ++b) {
                const int m = (int)(p.bc_off[b + 1] - p.bc_off[b]);
                if (kbh[b] < 0 || m > 20) continue;
                double v = 0.0, term = 1.0;
                for (int e = 0; e <= kbh[b] && e <= m; ++e) {
                    v += term;
                    term *= 8.0 * (double)(m - e) / (double)(e + 1);
                }
                expected += 150.0 * v / std::pow(4.0, (double)m);
            }
        }
        bp.slot_cap = expected < 1.0 ? 4 : expected < 2.5 ? 8 : expected < 8.0 ? 16 : 32;
        int total_b = 0;
        for (int k = 0; k < npass; ++k) total_b += c.pass[k].n_barcodes;
        bp.dense_d = expected >= 1.0 && total_b <= 256 && !ctx->tune.no_dense;  // (used by the kernels without seeds only; they then keep four slots)
    }
    // known-score class (config level): SimpleScoring with unit costs, ScoreOnly output.
    // (:exact with whole ranges IS the class at a budget of 0: exact_align, classification.jl:485-548, returns (0.0, s, s + m - 1)
    // for an occurrence — the leftmost, or the rightmost with trim_side = 3 — else Inf: the value, the end of the first column
    // at distance 0 and the largest origin of a distance-0 alignment; raw bytes are compared, N is a literal: SimpleScoring.
    // With a ref_search_range its meaning differs — allowed START positions, SURVEY Q11 — so only whole ranges qualify.)
    const auto whole_rng = [](const bdx_range_t &r) { return !r.start_from_end && r.start_offset <= 1 && r.end_from_end && r.end_offset >= 0; };
    for (int k = 0; k < npass; ++k) {
        const bool score_only = c.pass[k].trim_side == 0 && !c.need_traceback;
        const bool unit_sg = c.algorithm == BDX_ALG_SEMIGLOBAL && !c.has_nindel && c.match == 0 && c.mismatch == 1 && c.indel == 1;
        const bool exact_whole = c.algorithm == BDX_ALG_EXACT && c.pass[k].explicit_window == 0 && whole_rng(c.pass[k].ref_search_range) &&
                                 whole_rng(c.pass[k].barcode_start_range) && whole_rng(c.pass[k].barcode_end_range) && !getenv("BDX_NO_KNOWN_EXACT");
        bp.known_ok[k] = (unit_sg || exact_whole) && score_only && c.pass[k].explicit_window != BDX_WINDOW_ALIGN_ONE && !ctx->tune.no_known;
    }
    bp.enabled = 1;
    return BDX_OK;
}


// ---- q-gram seeding (pigeonhole) in front of the sweep -------------------------------------
// A recordable alignment of barcode b has at most kb[b] edit operations (see the sweep), so of
// kb[b]+1 disjoint pieces of the barcode at least one occurs in the read unchanged; a fortiori
// the first q bases of that piece do.  Pairs without any such seed hit cannot be candidates and
// are not swept.  Keys use 2 bits per base (symbol code & 3): equal bytes give equal keys, other
// bytes may alias — that only adds sweeps, never removes one.
int build_seed_tables(bdx_ctx *ctx, bool strict, bool alt = false) {
    const bdx_config_t &c = ctx->cfg;
    BdxSeedPlan &sp = alt ? ctx->F().splan_alt : ctx->F().splan;
    DevBuf &tables = alt ? ctx->F().seed_tables_alt : ctx->F().seed_tables;
    sp = BdxSeedPlan{};
    if (!ctx->F().bplan.enabled || c.filter == BDX_FILTER_BITPAR || ctx->tune.no_seed) return BDX_OK;
    const int npass = c.is_dual ? 2 : 1;
    int cmin = 1;
    if (c.algorithm == BDX_ALG_SEMIGLOBAL) {
        cmin = c.mismatch < c.indel ? c.mismatch : c.indel;
        if (c.has_nindel && c.nindel < cmin) cmin = c.nindel;
    }
    const bool n_wild = (c.algorithm == BDX_ALG_SEMIGLOBAL && c.has_nindel) || c.algorithm == BDX_ALG_HAMMING;
    // same symbol coding as the sweep
    int code_of[256];
    for (int i = 0; i < 256; ++i) code_of[i] = -1;
    int K = 0;
    for (int k = 0; k < npass; ++k)
        for (uint32_t i = 0; i < c.pass[k].bc_off[c.pass[k].n_barcodes]; ++i) {
            const uint8_t ch = c.pass[k].bc_bytes[i];
            if (code_of[ch] < 0) code_of[ch] = K++;
        }
    struct Piece { int pass, b, start; };
    std::vector<Piece> pieces;
    std::vector<uint16_t> always[2];
    int q = 8;
    int total_bc = 0;
    for (int k = 0; k < npass; ++k) {
        const bdx_pass_t &p = c.pass[k];
        if (p.n_barcodes > 32767) return BDX_OK;
        total_bc += p.n_barcodes;
        for (int b = 0; b < p.n_barcodes; ++b) {
            const int m = (int)(p.bc_off[b + 1] - p.bc_off[b]);
            long long ae;
            if (c.algorithm == BDX_ALG_EXACT) ae = 0;
            else if (c.algorithm == BDX_ALG_HAMMING) ae = (long long)std::floor(c.max_error_rate * (double)m);
            else ae = (long long)std::floor(c.max_error_rate * (double)(c.has_nindel ? p.bc_len_no_N[b] : m));
            if (ae < 0) continue;  // can never be recorded: neither seeded nor swept
            long long kb = ae / cmin;
            if (kb > tier_cap(ctx, m)) kb = tier_cap(ctx, m);
            bool wild = false;
            for (int i = 0; i < m; ++i) wild |= n_wild && p.bc_bytes[p.bc_off[b] + i] == 'N';
            const long long L = m / (kb + 1);
            if (wild || L < 5) {
                always[k].push_back((uint16_t)b);
                continue;
            }
            if (L < q) q = (int)L;
            for (long long t = 0; t <= kb; ++t) pieces.push_back(Piece{k, b, (int)(t * L)});
        }
    }
    if (pieces.empty()) return BDX_OK;
    if ((int)(always[0].size() + always[1].size()) * 4 > total_bc) return BDX_OK;  // seeding would not pay
    if (pieces.size() > 16384) return BDX_OK;
    // selectivity: expected seed-hit pairs per read of ~150 bases must be well below B
    const double space = std::pow(4.0, q);
    const double expected = 150.0 * (double)pieces.size() / space + 1.0 + (double)(always[0].size() + always[1].size());
    if (expected * 3.0 > (double)total_bc) return BDX_OK;
    // strict: single seeds only when they are really selective (q = 7, 8 in practice).  With ~14 falsely
    // seeded barcodes per read (q = 6 at B = 96) the hit queue / record tables cost more than the
    // two-intact-pieces variant, which is tried next (measured at kb = 3: 7.5 ms vs 5.7 ms per 2 M reads).
    if (strict && expected > 7.0) return BDX_OK;
    sp.q = q;
    // hashed bitmap with >= 96 bits per key (<= ~1 % false hits per position), at most the key space
    // itself (then it is exact).  Too many false hits overflow the hit queue, and an overflow costs a
    // whole-read sweep of every barcode.
    sp.bm_log2 = 5;
    while ((1u << sp.bm_log2) < pieces.size() * 96 && sp.bm_log2 < 2 * q) sp.bm_log2++;
    // sweep records per read: the true barcode(s) plus the expected falsely seeded ones, generously
    {
        const double false_pairs = 150.0 * (double)pieces.size() / space;
        sp.rcap = 8;
        while (sp.rcap < 64 && (double)sp.rcap < 4.0 + 4.0 * false_pairs) sp.rcap *= 2;
        // queues: the planted pair plus the chance pairs, with slack for the spread between the reads of a tile
        sp.qmul = sp.rcap >= 16 ? 8 : 4;
        const int want = (int)std::ceil((1.0 + false_pairs) * 1.5 + 1.0);  // (C2: 4 — one more entry per read would cost the fourth workgroup per CU)
        if (want > sp.qmul) sp.qmul = want > 48 ? 48 : want;
    }
    if (ctx->tune.seed_bm_log2 > 0) sp.bm_log2 = ctx->tune.seed_bm_log2 < 2 * q ? ctx->tune.seed_bm_log2 : 2 * q;
    sp.bm_words = (1 << sp.bm_log2) / 32;
    sp.hash_log2 = 8;
    while ((1u << sp.hash_log2) < pieces.size() * 2) sp.hash_log2++;
    sp.hash_in_lds = ((size_t)5 << sp.hash_log2) <= 8 * 1024;  // larger tables are probed in L2 (a few probes per read)
    if (ctx->tune.seed_hash_l2) sp.hash_in_lds = 0;
    std::vector<uint32_t> bitmap(sp.bm_words, 0), hash((size_t)1 << sp.hash_log2, 0);
    std::vector<uint8_t> hash_ps((size_t)1 << sp.hash_log2, 0);
    const uint32_t hmask = (1u << sp.hash_log2) - 1;
    for (const Piece &pc : pieces) {
        const bdx_pass_t &p = c.pass[pc.pass];
        uint32_t key = 0;
        for (int i = 0; i < q; ++i) key |= (uint32_t)(code_of[p.bc_bytes[p.bc_off[pc.b] + pc.start + i]] & 3) << (2 * i);
        // same cheap fold as the kernel's scan (direct index when the bitmap spans the key space)
        const uint32_t hb = sp.bm_log2 >= 2 * q ? key : ((key ^ (key >> sp.bm_log2)) & ((1u << sp.bm_log2) - 1u));
        bitmap[hb >> 5] |= 1u << (hb & 31);
        const uint32_t entry = (key << 16) | ((uint32_t)pc.pass << 15) | (uint32_t)(pc.b + 1);
        uint32_t slot = (key * 0x9E3779B1u) >> (32 - sp.hash_log2);
        // one entry per (key, barcode, piece start): two pieces of one barcode may share a key
        bool dup = false;
        while (hash[slot] != 0) {
            if (hash[slot] == entry && hash_ps[slot] == (uint8_t)pc.start) { dup = true; break; }
            slot = (slot + 1) & hmask;
        }
        if (!dup) {
            hash[slot] = entry;
            hash_ps[slot] = (uint8_t)pc.start;
        }
    }
    size_t bytes = bitmap.size() * 4 + hash.size() * 4 + ((hash_ps.size() + 15) & ~(size_t)15);
    const size_t o_always[2] = {bytes, bytes + ((always[0].size() * 2 + 15) & ~(size_t)15)};
    bytes = o_always[1] + ((always[1].size() * 2 + 15) & ~(size_t)15) + 16;
    std::vector<uint8_t> blob(bytes, 0);
    memcpy(blob.data(), bitmap.data(), bitmap.size() * 4);
    memcpy(blob.data() + bitmap.size() * 4, hash.data(), hash.size() * 4);
    memcpy(blob.data() + bitmap.size() * 4 + hash.size() * 4, hash_ps.data(), hash_ps.size());
    for (int k = 0; k < 2; ++k)
        if (!always[k].empty()) memcpy(blob.data() + o_always[k], always[k].data(), always[k].size() * 2);
    HIP_TRY(ctx, tables.ensure(bytes));
    HIP_TRY(ctx, hipMemcpy(tables.p, blob.data(), bytes, hipMemcpyHostToDevice));
    const uint8_t *base = (const uint8_t *)tables.p;
    sp.d_bitmap = (const uint32_t *)base;
    sp.d_hash = (const uint32_t *)(base + bitmap.size() * 4);
    sp.d_hash_ps = base + bitmap.size() * 4 + hash.size() * 4;
    for (int k = 0; k < 2; ++k) {
        sp.n_always[k] = (int)always[k].size();
        sp.d_always[k] = (const uint16_t *)(base + o_always[k]);
    }
    sp.enabled = 1;
    return BDX_OK;
}

// ---- two-intact-pieces ("diagonal") seeding for budgets where single pieces are too short -----
// With kb operations allowed, kb+2 disjoint pieces of the barcode leave at least TWO untouched; they
// occur in the read on diagonals (read position - barcode offset) that differ by at most kb (the
// indels between them), and the alignment starts within kb of either diagonal.  The kernel keeps,
// per read, an inverted index of its 4-mers (256 keys x position bits) and tests every (read,
// barcode) pair with a handful of word operations per piece; only pairs with two such pieces are
// swept, over the columns [d_min - kb - 1, d_max + m + kb + 1).  Lossless for the same reason as the
// single-piece seeds: it only skips pairs whose unit distance exceeds kb.
int build_diag_tables(bdx_ctx *ctx) {
    const bdx_config_t &c = ctx->cfg;
    BdxSeedPlan &sp = ctx->F().splan;
    if (sp.enabled || !ctx->F().bplan.enabled || c.filter == BDX_FILTER_BITPAR || ctx->tune.no_seed || ctx->tune.no_diag ||
        ctx->F().bplan.word_bytes != 4)  // (the diagonal variant has 32-bit sweep words)
        return BDX_OK;
    const int npass = c.is_dual ? 2 : 1;
    int cmin = 1;
    if (c.algorithm == BDX_ALG_SEMIGLOBAL) {
        cmin = c.mismatch < c.indel ? c.mismatch : c.indel;
        if (c.has_nindel && c.nindel < cmin) cmin = c.nindel;
    }
    const bool n_wild = (c.algorithm == BDX_ALG_SEMIGLOBAL && c.has_nindel) || c.algorithm == BDX_ALG_HAMMING;
    int code_of[256];
    for (int i = 0; i < 256; ++i) code_of[i] = -1;
    int K = 0;
    for (int k = 0; k < npass; ++k)
        for (uint32_t i = 0; i < c.pass[k].bc_off[c.pass[k].n_barcodes]; ++i) {
            const uint8_t ch = c.pass[k].bc_bytes[i];
            if (code_of[ch] < 0) code_of[ch] = K++;
        }
    std::vector<uint32_t> meta[2], keys[2];
    std::vector<uint16_t> always[2];
    int total_bc = 0, kmax = 0;
    double flagged = 0.0;  // expected falsely flagged pairs per read of ~150 bases
    double flag_coef = 0.0;
    for (int k = 0; k < npass; ++k) {
        const bdx_pass_t &p = c.pass[k];
        if (p.n_barcodes > 32767) return BDX_OK;
        total_bc += p.n_barcodes;
        meta[k].assign((size_t)p.n_barcodes, 0u);
        keys[k].assign((size_t)p.n_barcodes * 2, 0u);
        for (int b = 0; b < p.n_barcodes; ++b) {
            const int m = (int)(p.bc_off[b + 1] - p.bc_off[b]);
            long long ae;
            if (c.algorithm == BDX_ALG_EXACT) ae = 0;
            else if (c.algorithm == BDX_ALG_HAMMING) ae = (long long)std::floor(c.max_error_rate * (double)m);
            else ae = (long long)std::floor(c.max_error_rate * (double)(c.has_nindel ? p.bc_len_no_N[b] : m));
            if (ae < 0) continue;  // can never be recorded: neither seeded nor swept (meta 0 and not in `always`)
            const long long kb = ae / cmin;
            bool wild = false;
            for (int i = 0; i < m; ++i) wild |= n_wild && p.bc_bytes[p.bc_off[b] + i] == 'N';
            const long long P = kb + 2;
            const long long L = m / P;
            if (wild || L < 4 || P > 8 || kb > 6 || (P - 1) * L > 28) {
                always[k].push_back((uint16_t)b);
                continue;
            }
            if (kb > kmax) kmax = (int)kb;
            meta[k][b] = (uint32_t)P | ((uint32_t)L << 8);
            uint64_t kk = 0;
            for (long long t = 0; t < P; ++t) {
                uint32_t key = 0;
                for (int i = 0; i < 4; ++i) key |= (uint32_t)(code_of[p.bc_bytes[p.bc_off[b] + t * L + i]] & 3) << (2 * i);
                kk |= (uint64_t)key << (8 * t);
            }
            keys[k][2 * b] = (uint32_t)kk;
            keys[k][2 * b + 1] = (uint32_t)(kk >> 32);
            const double hits = 147.0 / 256.0;  // occurrences of one 4-mer in the read
            flagged += (double)(P * (P - 1) / 2) * hits * hits * (double)(2 * kb + 1) / (150.0 + m);
            flag_coef += (double)(P * (P - 1) / 2) * (double)(2 * kb + 1);
        }
    }
    const size_t n_always = always[0].size() + always[1].size();
    if (n_always == (size_t)total_bc) return BDX_OK;
    if (n_always * 4 > (size_t)total_bc) return BDX_OK;
    // worth it only if clearly fewer pairs are swept (a flagged pair costs ~ a quarter of a whole-read sweep)
    if ((flagged + (double)n_always) * 2.0 > (double)total_bc) return BDX_OK;
    // ... and only for enough barcodes: the index forces 4..8-read tiles, whose per-tile latency costs about
    // as much as sweeping ~40 barcodes over a whole 150-base read (measured: 1.44 us/read + 0.017 us/pair
    // against 0.054 us/pair of the plain sweep)
    {
        if (total_bc < ctx->tune.diag_min_b) return BDX_OK;  // 48 unless overridden for tuning experiments
    }
    const double coef_keep = flag_coef;
    size_t bytes = 0;
    size_t o_meta[2], o_keys[2], o_always[2];
    for (int k = 0; k < 2; ++k) {
        o_meta[k] = bytes;
        bytes += (meta[k].size() * 4 + 15) & ~(size_t)15;
        o_keys[k] = bytes;
        bytes += (keys[k].size() * 4 + 15) & ~(size_t)15;
        o_always[k] = bytes;
        bytes += (always[k].size() * 2 + 15) & ~(size_t)15;
    }
    bytes += 16;
    std::vector<uint8_t> blob(bytes, 0);
    for (int k = 0; k < 2; ++k) {
        if (!meta[k].empty()) memcpy(blob.data() + o_meta[k], meta[k].data(), meta[k].size() * 4);
        if (!keys[k].empty()) memcpy(blob.data() + o_keys[k], keys[k].data(), keys[k].size() * 4);
        if (!always[k].empty()) memcpy(blob.data() + o_always[k], always[k].data(), always[k].size() * 2);
    }
    HIP_TRY(ctx, ctx->F().seed_tables.ensure(bytes));
    HIP_TRY(ctx, hipMemcpy(ctx->F().seed_tables.p, blob.data(), bytes, hipMemcpyHostToDevice));
    const uint8_t *base = (const uint8_t *)ctx->F().seed_tables.p;
    sp = BdxSeedPlan{};
    sp.diag_flag_coef = coef_keep;
    for (int k = 0; k < 2; ++k) {
        sp.d_dmeta[k] = (const uint32_t *)(base + o_meta[k]);
        sp.d_dkeys[k] = (const uint32_t *)(base + o_keys[k]);
        sp.n_always[k] = (int)always[k].size();
        sp.d_always[k] = (const uint16_t *)(base + o_always[k]);
    }
    sp.q = 4;
    sp.diag = 1;
    sp.diag_kmax = kmax;
    sp.rcap = 8;
    sp.enabled = 1;
    return BDX_OK;
}

// ---- wave-autonomous kernel (bdx_wave.hip): tables of one filter set ------------------------------
// Eligible: single pass in the known-score class (ScoreOnly, unit costs), strict single seeds for every barcode
// (no barcode swept unconditionally), barcodes of plain A / C / G / T up to 32 nt, and ranges that resolve to 1:n
// for every read (then final_search_range = 1:n, max_start_pos = n, min_end_pos = 1: neither binds, DESIGN.md
// §3.1).  Same pieces, keys and budgets as build_seed_tables / build_bitpar_tables of the set — only the symbol
// coding differs: the kernel transcodes arithmetically, code = (byte >> 1) & 3 (A 0, C 1, T 2, G 3).
// (developer aid: with BDX_TRACE_LAUNCH set, build_wave_tables says where it turned a filter set away)
#define WAVE_NO() (getenv("BDX_TRACE_LAUNCH") ? (void)fprintf(stderr, "[bdx] no wave tables for set %d: bdx_abi.cpp:%d\n", ctx->cur, __LINE__) : (void)0, BDX_OK)
int build_wave_tables(bdx_ctx *ctx) {
    const bdx_config_t &c = ctx->cfg;
    BdxFilterSet &F = ctx->F();
    BdxWavePlan &wp = F.wplan;
    wp = BdxWavePlan{};
    const BdxBitparPlan &bp = F.bplan;
    const BdxSeedPlan &sp = F.splan;
    const int npass = c.is_dual ? 2 : 1;
    if (ctx->tune.no_wave || !bp.enabled || !sp.enabled || sp.diag || bp.word_bytes != 4 || sp.n_always[0] != 0 || sp.n_always[1] != 0 ||
        sp.q < 6 || sp.q > 8 || (c.algorithm == BDX_ALG_SEMIGLOBAL && c.has_nindel))
        return WAVE_NO();
    // known-score configs: the kernel replays the reducer itself (single pass); everything else in the filters' domain:
    // "split" — it only filters, candidate masks and column windows go to the exact kernel (either pass count)
    bool split = false;
    for (int k = 0; k < npass; ++k) split |= !bp.known_ok[k];
    // :hamming / :exact (always split: their scans run in the exact kernel, restricted to the hand-over windows): the
    // budget is floor(rate * m) substitutions / 0, one operation costs 1
    const bool sgm = c.algorithm == BDX_ALG_SEMIGLOBAL;
    // the known classes' config condition: unit-cost SimpleScoring, or :exact (whole ranges: checked below / in build_bitpar_tables)
    const bool kclass = (sgm && !c.has_nindel && c.match == 0 && c.mismatch == 1 && c.indel == 1) || (c.algorithm == BDX_ALG_EXACT && !getenv("BDX_NO_KNOWN_EXACT"));
    int cmin = sgm ? (c.mismatch < c.indel ? c.mismatch : c.indel) : 1;
    if (cmin < 1 || (sgm && c.match < 0)) return WAVE_NO();
    const auto whole = [](const bdx_range_t &r) { return !r.start_from_end && r.start_offset <= 1 && r.end_from_end && r.end_offset >= 0; };
    int Btot = 0, cwt = 0;
    bool ranged = false;
    for (int k = 0; k < npass; ++k) {
        const bdx_pass_t &p = c.pass[k];
        // (a ref_search_range is allowed for :semiglobal: the kernel resolves every read's column window itself, classification.jl:795-807;
        // start / end ranges that could bind stay on the general kernel)
        if (p.explicit_window != 0 || !whole(p.barcode_start_range) || !whole(p.barcode_end_range)) return WAVE_NO();
        if (!whole(p.ref_search_range)) {
            if (c.algorithm != BDX_ALG_SEMIGLOBAL) return WAVE_NO();
            ranged = true;
        }
        if (p.n_barcodes < 1) return WAVE_NO();
        for (uint32_t i = 0; i < p.bc_off[p.n_barcodes]; ++i) {
            const uint8_t ch = p.bc_bytes[i];
            if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') return WAVE_NO();
        }
        Btot += p.n_barcodes;
        cwt += (p.n_barcodes + 31) / 32;
    }
    if (Btot > 1024 || (split && cwt > 16)) return WAVE_NO();  // (split mode keeps the candidate words of a read in LDS: up to 512 barcodes)
    const int q = sp.q;
    struct Piece { int g, start; const uint8_t *bc; };
    std::vector<Piece> pieces;
    std::vector<uint32_t> meta((size_t)Btot, 0u), peq8((size_t)Btot * 9, 0u), settle((size_t)Btot, 0u);  // (stride 9: bank spread, see the kernel)
    std::vector<uint32_t> peq8r((size_t)Btot * 9, 0u);  // the reversed barcodes (known-trim class: trim_side = 3 passes are swept right to left)
    int track = 1 << 20, g = 0;
    for (int k = 0; k < npass; ++k) {
        const bdx_pass_t &p = c.pass[k];
        for (int b = 0; b < p.n_barcodes; ++b, ++g) {
            const int m = (int)(p.bc_off[b + 1] - p.bc_off[b]);
            if (m < 1 || m > 32) return WAVE_NO();
            const uint8_t *bc = p.bc_bytes + p.bc_off[b];
            const int shift = 32 - m;
            const uint32_t rows = m == 32 ? 0xFFFFFFFFu : (((1u << m) - 1u) << shift);
            const uint32_t pad = ~rows;  // virtual rows below the barcode: match everything, D stays 0
            for (int code = 0; code < 8; ++code) {
                uint32_t mask = pad;
                if (code < 4)
                    for (int i = 0; i < m; ++i)
                        if (((bc[i] >> 1) & 3) == code) mask |= 1u << (shift + i);
                peq8[(size_t)g * 9 + code] = mask;
                uint32_t maskr = pad;
                if (code < 4)
                    for (int i = 0; i < m; ++i)
                        if (((bc[m - 1 - i] >> 1) & 3) == code) maskr |= 1u << (shift + i);
                peq8r[(size_t)g * 9 + code] = maskr;
            }
            const long long ae = c.algorithm == BDX_ALG_EXACT ? 0 : (long long)std::floor(c.max_error_rate * (double)m);  // (normalisation = m)
            if (ae < 0) {  // can never be recorded: neither seeded nor swept (budget field 255)
                meta[(size_t)g] = (uint32_t)m | (255u << 8) | (255u << 16);
                continue;
            }
            long long kb = ae / cmin;
            if (kb > tier_cap(ctx, m)) kb = tier_cap(ctx, m);
            if (kb > 15) return WAVE_NO();  // (a record keeps the diagonals of its hits as 2 kb + 1 bits)
            const long long L = m / (kb + 1);
            if (L < q) return WAVE_NO();  // (cannot happen: the set's q is the shortest piece)
            // lone-survivor tables of the replay (bdx_wave.hip): the reference accepts a survivor with distance d iff
            // d <= floor(max_error_rate * m) (:254) and score = d / m <= max_error_rate (:658 / :696) — both Float64, both
            // evaluated here exactly as the device would; tier 1 settles it iff score < slo (and, with_delta, the bound
            // slo - score >= min_delta proves "not ambiguous")
            int dmax = 255;
            uint32_t sbits = 0;
            for (long long d = 0; d <= kb && d <= 15; ++d) {
                const double score = (double)d / (double)m;
                if (d <= ae && score <= c.max_error_rate) dmax = (int)d;
                const double slo = bp.tier_slo[k];
                if (score < slo) {
                    sbits |= 1u << d;
                    if ((slo - score) >= c.min_delta) sbits |= 1u << (16 + d);
                }
            }
            settle[(size_t)g] = sbits;
            meta[(size_t)g] = (uint32_t)m | ((uint32_t)kb << 8) | ((uint32_t)dmax << 16);
            if (m - (int)kb - 1 < track) track = m - (int)kb - 1;
            for (long long t = 0; t <= kb; ++t) pieces.push_back(Piece{g, (int)(t * L), bc});
        }
    }
    if (pieces.empty() || pieces.size() > 8192) return WAVE_NO();
    // the per-read record table holds eight (barcode, diagonal cluster) records: the planted one(s) plus the chance pairs must nearly always fit
    {
        // chance seed hits per 150-base read: the hit queue and the sweep list of a tile are sized from it (size_wave)
        // (measured, 24-nt barcodes, 2 M reads: B = 192 / 384 / 768 at rate 0.1 — chance 1.3 / 2.6 / 5.3 — 1.99 -> 4.85, 1.49 -> 3.52,
        // 0.94 -> 1.62 G reads/s against the general kernel; as tier 1 of rate 0.2: 0.92 -> 1.22, 0.50 -> 0.64, 0.25 -> 0.17: whatever
        // overflows there costs a full-budget evaluation)
        double limit = ctx->cur == 1 ? 3.0 : 6.0;
        if (const char *e = getenv("BDX_WAVE_CHANCE")) limit = atof(e);  // (tuning experiment)
        wp.chance = 150.0 * (double)pieces.size() / std::pow(4.0, (double)q);
        if (wp.chance > limit) return WAVE_NO();
    }
    wp.q = q;
    wp.n_barcodes = Btot;
    wp.b0 = c.pass[0].n_barcodes;
    wp.split = split ? 1 : 0;
    wp.ranged = ranged ? 1 : 0;
    wp.cand_words = split ? cwt : (c.is_dual ? 4 : 0);  // (known-score dual configs: four survivor slots of pass 1 per read in that area)
    wp.bm_bytes = (1 << (2 * q)) / 8;
    wp.track_from = track < 0 ? 0 : (track > 28 ? 28 : track);
    // seed table: the bitmap is exact (one bit per key of the 4^q key space), so a hit's entry is found by the RANK of its
    // key among the keys present (prefix count per bitmap word + a popcount); pieces that share a key are chained
    std::vector<uint8_t> bitmap((size_t)wp.bm_bytes, 0);
    struct Ent { uint32_t key; int g, start; };
    std::vector<Ent> ents;
    for (const Piece &pc : pieces) {
        uint32_t key = 0;
        for (int i = 0; i < q; ++i) key |= (uint32_t)((pc.bc[pc.start + i] >> 1) & 3) << (2 * i);
        bool dup = false;  // one entry per (key, barcode, piece start)
        for (const Ent &e : ents) dup |= e.key == key && e.g == pc.g && e.start == pc.start;
        if (dup) continue;
        bitmap[key >> 3] |= (uint8_t)(1u << (key & 7));
        ents.push_back(Ent{key, pc.g, pc.start});
    }
    std::stable_sort(ents.begin(), ents.end(), [](const Ent &x, const Ent &y) { return x.key < y.key; });
    std::vector<uint32_t> ent;  // heads (one per key, in key order) first, chained entries behind them
    std::vector<uint32_t> chain;
    {
        std::vector<size_t> head_of;  // index into ents of every head
        for (size_t i = 0; i < ents.size(); ++i)
            if (i == 0 || ents[i].key != ents[i - 1].key) head_of.push_back(i);
        const size_t D = head_of.size();
        if (ents.size() >= 65536) return WAVE_NO();
        ent.assign(ents.size(), 0u);
        size_t next_free = D;
        for (size_t h = 0; h < D; ++h) {
            const size_t first = head_of[h], last = h + 1 < D ? head_of[h + 1] : ents.size();
            size_t at = h;
            for (size_t i = first; i < last; ++i) {
                const size_t nxt = i + 1 < last ? next_free++ : 0;
                ent[at] = (uint32_t)(ents[i].g + 1) | ((uint32_t)ents[i].start << 11) | ((uint32_t)nxt << 16);
                at = nxt;
            }
        }
    }
    std::vector<uint16_t> rank((size_t)wp.bm_bytes / 4, 0);
    {
        uint32_t run = 0;
        for (size_t w = 0; w < rank.size(); ++w) {
            rank[w] = (uint16_t)run;
            uint32_t word;
            memcpy(&word, bitmap.data() + 4 * w, 4);
            run += (uint32_t)__builtin_popcount(word);
        }
    }
    wp.n_ent = (int)ent.size();
    // the tables must leave room for at least eight waves' work areas at the smallest tile
    if (bdx_wave_table_bytes(wp, ctx->plan.hist_entries) > 64 * 1024) return WAVE_NO();
    auto al = [](size_t x) { return (x + 63) & ~(size_t)63; };
    const size_t o_bm = 0, o_rank = al(bitmap.size()), o_ent = o_rank + al(rank.size() * 2), o_peq = o_ent + al(ent.size() * 4),
                 o_meta = o_peq + al(peq8.size() * 4), o_settle = o_meta + al(meta.size() * 4), o_peqr = o_settle + al(settle.size() * 4),
                 bytes = o_peqr + al(peq8r.size() * 4);
    std::vector<uint8_t> blob(bytes, 0);
    memcpy(blob.data() + o_bm, bitmap.data(), bitmap.size());
    memcpy(blob.data() + o_rank, rank.data(), rank.size() * 2);
    memcpy(blob.data() + o_ent, ent.data(), ent.size() * 4);
    memcpy(blob.data() + o_peq, peq8.data(), peq8.size() * 4);
    memcpy(blob.data() + o_meta, meta.data(), meta.size() * 4);
    memcpy(blob.data() + o_settle, settle.data(), settle.size() * 4);
    memcpy(blob.data() + o_peqr, peq8r.data(), peq8r.size() * 4);
    HIP_TRY(ctx, F.wave_tables.ensure(bytes));
    HIP_TRY(ctx, hipMemcpy(F.wave_tables.p, blob.data(), bytes, hipMemcpyHostToDevice));
    const uint8_t *base = (const uint8_t *)F.wave_tables.p;
    wp.d_bitmap = base + o_bm;
    wp.d_rank = (const uint16_t *)(base + o_rank);
    wp.d_ent = (const uint32_t *)(base + o_ent);
    wp.d_peq8 = (const uint32_t *)(base + o_peq);
    wp.d_meta = (const uint32_t *)(base + o_meta);
    wp.d_settle = (const uint32_t *)(base + o_settle);
    wp.d_peq8r = (const uint32_t *)(base + o_peqr);
    wp.enabled = 1;
    // Known-trim class: the known-score conditions with a trim side in some pass (either pass count, no summary).  What a trim
    // side makes observable is one position per pass — trim_side = 5: the alignment's END (keep_start = end + 1,
    // classification.jl:912-914; the reference keeps the leftmost end of the best score, :142-153: strict `<`); trim_side = 3: its
    // START (keep_end = max(1, start) - 1, :910-911; the largest start among the alignments of the best score, :142-153 tie rule
    // + :310-321 origin order) — and the sweep delivers both (bdx_wave.hip, KEND: the lowering mask of a left-to-right sweep /
    // of a right-to-left sweep with the reversed barcode).  Such a config gets its verdicts from the non-split kernel whenever
    // the caller does not ask for per-pass start positions (nor for end positions of a trim_side = 3 pass).
    F.wplan_k = BdxWavePlan{};
    bool trims_ok = true;
    for (int k = 0; k < npass; ++k) trims_ok = trims_ok && c.pass[k].explicit_window != BDX_WINDOW_ALIGN_ONE;
    if (split && kclass && trims_ok && !c.need_traceback &&
        !ctx->tune.no_known && !ctx->tune.no_kend) {
        bool fits = true;  // entry = barcode << 22 | d << 16 | position key
        for (uint32_t x : meta) fits = fits && (((x >> 8) & 255u) == 255u || ((x >> 8) & 255u) < 64u);
        if (fits && c.pass[0].n_barcodes <= 1023 && (!c.is_dual || c.pass[1].n_barcodes <= 1023)) {
            F.wplan_k = wp;
            F.wplan_k.split = 0;
            F.wplan_k.cand_words = c.is_dual ? 4 : 0;  // (the four survivor slots of pass 1)
            F.wplan_k.kend = 1;
            for (int k = 0; k < npass; ++k)
                if (c.pass[k].trim_side == 3) F.wplan_k.kend = 2;  // (reversed sweeps: bdx_wave_rev.hip)
        }
    }
    // Known-alignment class: the same conditions with `summary` allowed — start AND end of every pass's winner come out of one
    // more (anchored) sweep per pass and read, so per-pass positions and the DemuxStats histograms need no exact kernel either
    // (bdx_wave_aln.hip); taken per launch when the caller wants positions the known-trim class does not know, or statistics.
    F.wplan_a = BdxWavePlan{};
    // (:exact reports the occurrence's positions whatever the output policy, classification.jl:485-548: its score-only form only
    // serves callers that do not ask for them — the others take this class per launch, bdx_classify_device)
    if ((split || c.algorithm == BDX_ALG_EXACT) && kclass && trims_ok && !ctx->tune.no_known &&
        !ctx->tune.no_kend && !getenv("BDX_NO_KALN")) {
        bool fits = true;
        for (uint32_t x : meta) fits = fits && (((x >> 8) & 255u) == 255u || ((x >> 8) & 255u) < 64u);
        if (fits && c.pass[0].n_barcodes <= 1023 && (!c.is_dual || c.pass[1].n_barcodes <= 1023)) {
            F.wplan_a = wp;
            F.wplan_a.split = 0;
            F.wplan_a.cand_words = c.is_dual ? 4 : 0;
            F.wplan_a.kend = 3;
        }
    }
    return BDX_OK;
}

#undef WAVE_NO
// Geometry of the wave kernel for a batch: the tile size and workgroup shape that keep the most waves resident
// per compute unit (tables once per workgroup + one work area per wave within 160 KiB, at most 16 waves: the
// kernel is compiled for four waves per SIMD).  false: this batch runs the general kernel.
bool size_wave(bdx_ctx *ctx, BdxWavePlan &wp, int read_len, long long n_reads);
bool size_wave(bdx_ctx *ctx, int set, int read_len, long long n_reads) { return size_wave(ctx, ctx->fs[set].wplan, read_len, n_reads); }
bool size_wave(bdx_ctx *ctx, BdxWavePlan &wp, int read_len, long long n_reads) {
    wp.winm = 0;
    if (!wp.enabled || ctx->dev.vlen) return false;  // (window uploads stage per-read slots: general kernel)
    if (read_len < 1) read_len = 1;
    const size_t tables = bdx_wave_table_bytes(wp, ctx->plan.hist_entries);
    const int rws[3] = {32, 16, 8};
    int best_waves = 0;
    for (int rw : rws) {
        if (ctx->tune.wave_rw && rw != ctx->tune.wave_rw) continue;
        // small batches: at least one tile per resident wave before the tile grows
        if (!ctx->tune.wave_rw && rw > 8 && n_reads / rw < (long long)ctx->n_cu * 16) continue;
        const long long span = (((long long)rw * read_len + 64 + 15) & ~15LL);
        if (span > 10 * 1024) continue;  // a tile's bytes wait in registers: at most ten 16-byte vectors per lane
        // queues: the planted barcode's pieces (up to kb + 1 = 3 hits, one or two records) + the chance hits, with slack
        const int hq_cap = rw * (int)std::ceil(std::max(6.0, 4.0 + 2.5 * wp.chance));
        const int sq_cap = rw * (int)std::ceil(std::max(3.0, 1.8 + 1.6 * wp.chance));
        const size_t area = bdx_wave_area_bytes(rw, (int)span, false, hq_cap, sq_cap, wp.cand_words + (wp.ranged ? 4 : 0));
        const int maxres = ctx->tune.wave_maxres > 0 ? ctx->tune.wave_maxres : 16;
        const int shapes[4] = {8, 16, 4, ctx->tune.wave_waves};  // (a forced shape may be any wave count up to 16)
        for (int w : shapes) {
            if (w < 1 || w > 16 || (ctx->tune.wave_waves && w != ctx->tune.wave_waves)) continue;
            const size_t lds = tables + (size_t)w * area;
            if (lds > LDS_MAX) continue;
            int per_cu = (int)(LDS_MAX / (((lds + 1279) / 1280) * 1280));  // 1280-byte LDS granules
            if (per_cu * w > maxres) per_cu = maxres / w;
            if (per_cu < 1) continue;
            const int resident = per_cu * w;
            if (resident > best_waves) {
                best_waves = resident;
                wp.rw = rw;
                wp.waves = w;
                wp.blocks = per_cu * ctx->n_cu;
                wp.span_cap = (int)span;
                wp.hq_cap = hq_cap;
                wp.sq_cap = sq_cap;
            }
        }
        if (best_waves >= 12) break;  // a larger tile at (nearly) full residency beats a smaller one
    }
    if (best_waves < 4) return false;
    wp.read_len_hint = read_len;
    // ranged single-pass configs: the seed scan only walks the groups of sixteen positions that overlap a read's window when
    // the window (resolved at the planned read length, classification.jl:795-800) is much shorter than the read
    wp.scan_gpr = 0;
    if (wp.ranged) {
        const int npw = ctx->dev.is_dual ? 2 : 1;
        long long gpr = 0;
        for (int k = 0; k < npw; ++k) {
            const BdxDevRange &dr = ctx->dev.pass[k].ref_search;
            long long f = dr.start_from_end ? read_len + dr.start_offset : dr.start_offset;
            long long l = dr.end_from_end ? read_len + dr.end_offset : dr.end_offset;
            if (f < 1) f = 1;
            if (l > read_len) l = read_len;
            const long long wlen = l >= f ? l - f + 1 : 0;
            const long long g = (wlen + 15) / 16 + 1;
            if (g > gpr) gpr = g;
        }
        if (gpr * npw * 16 * 10 <= (long long)read_len * 7 && (long long)wp.rw * npw * gpr < 2048) wp.scan_gpr = (int)gpr;
    }
    return true;
}

// Window mode of the wave kernel (bdx_wave_win.hip) for a batch: single-pass known-score configs whose ref_search_range
// window — resolved at the planned read length (classification.jl:795-800) — is at most half the read: the tiles are
// scattered, every read's slot holds just its window (+ up to 15 positions in front: the loads are aligned 16-byte vectors).
// This is what lets 10 kbp reads with a 200-column window (BASELINE config 5) take the wave kernel at all: a tile's bytes
// wait in registers, which bounds a contiguous tile at 10 KB.
bool size_wave_win(bdx_ctx *ctx, BdxWavePlan &wp, int read_len, long long n_reads) {
    wp.winm = 0;
    if (!wp.enabled || ctx->dev.vlen || !wp.ranged || wp.split || wp.kend || ctx->dev.is_dual || ctx->tune.no_wave || ctx->tune.no_win) return false;
    if (read_len < 1) read_len = 1;
    const BdxDevRange &dr = ctx->dev.pass[0].ref_search;
    {
        const long long LIM = 1LL << 28;  // (the kernel resolves the windows in 32-bit arithmetic)
        if (dr.start_offset < -LIM || dr.start_offset > LIM || dr.end_offset < -LIM || dr.end_offset > LIM) return false;
    }
    long long f = dr.start_from_end ? read_len + dr.start_offset : dr.start_offset;
    long long l = dr.end_from_end ? read_len + dr.end_offset : dr.end_offset;
    if (f < 1) f = 1;
    if (l > read_len) l = read_len;
    const long long wlen = l >= f ? l - f + 1 : 0;
    if (wlen < 1 || wlen * 2 > read_len) return false;
    const int slot = (int)((wlen + 15 + 15) & ~15LL);
    const size_t tables = bdx_wave_table_bytes(wp, ctx->plan.hist_entries);
    const double chance = wp.chance * (double)wlen / 150.0;
    int best_waves = 0;
    const int rws[2] = {32, 16};
    for (int rw : rws) {
        if (ctx->tune.wave_rw && rw != ctx->tune.wave_rw) continue;
        if (!ctx->tune.wave_rw && rw > 16 && n_reads / rw < (long long)ctx->n_cu * 16) continue;  // small batches: a tile per resident wave first
        const int vecs = rw * (slot >> 4);
        if (!((rw == 32 && vecs <= 64 * 7) || (rw == 16 && vecs <= 64 * 4))) continue;  // (instantiated register budgets)
        const int span = rw * slot + 16;
        const int hq_cap = rw * (int)std::ceil(std::max(6.0, 4.0 + 2.5 * chance));
        const int sq_cap = rw * (int)std::ceil(std::max(3.0, 1.8 + 1.6 * chance));
        const size_t area = bdx_wave_area_bytes(rw, span, false, hq_cap, sq_cap, 0, true);
        const int shapes[3] = {16, 8, 4};  // (tried: 32-read tiles on 12 waves per CU — C5 0.329 vs 0.314 ms with 16-read tiles on 16 waves)
        for (int w : shapes) {
            if (ctx->tune.wave_waves && w != ctx->tune.wave_waves) continue;
            const size_t lds = tables + (size_t)w * area;
            if (lds > LDS_MAX) continue;
            int per_cu = (int)(LDS_MAX / (((lds + 1279) / 1280) * 1280));
            if (per_cu * w > 16) per_cu = 16 / w;
            if (per_cu * w > best_waves) {
                best_waves = per_cu * w;
                wp.rw = rw;
                wp.waves = w;
                wp.blocks = per_cu * ctx->n_cu;
                wp.span_cap = span;
                wp.hq_cap = hq_cap;
                wp.sq_cap = sq_cap;
            }
        }
        if (best_waves >= 12) break;
    }
    if (best_waves < 4) return false;
    wp.slot = slot;
    wp.read_len_hint = read_len;
    wp.scan_gpr = 0;
    wp.winm = 1;
    return true;
}

// ---- pairs mode of the wave kernel (bdx_pairs.hip): tables of the FULL-budget set --------------------------------
// Between tier 1 and the general kernel of a tiered config: the reads tier 1 lists are gathered into slots and filtered
// by the two-intact-pieces lemma on barcode masks (one table entry per (piece, 4-base key): the barcodes whose piece has
// that key).  Eligible: the conditions of build_wave_tables on alphabet, lengths and ranges; every barcode's budget kb
// at most 4 with 4 (kb + 2) <= m (kb + 2 disjoint 4-base pieces at offsets 0, 4, ..); at most 128 barcodes.
int build_pair_tables(bdx_ctx *ctx) {
    const bdx_config_t &c = ctx->cfg;
    BdxFilterSet &F = ctx->F();
    BdxWavePlan &wp = F.pplan;
    wp = BdxWavePlan{};
    const BdxBitparPlan &bp = F.bplan;
    const int npass = c.is_dual ? 2 : 1;
    // (a capped set gets pair tables only as the pairs tier: budgets capped at tier_cap_fixed operations)
    if (ctx->tune.no_wave || ctx->tune.no_pairs || !bp.enabled || bp.word_bytes != 4 || (bp.tier_capped && ctx->tier_cap_fixed < 0) || c.filter != BDX_FILTER_AUTO ||
        (c.algorithm == BDX_ALG_SEMIGLOBAL && c.has_nindel))
        return BDX_OK;
    bool split = false;
    for (int k = 0; k < npass; ++k) split |= !bp.known_ok[k];
    const bool sgm = c.algorithm == BDX_ALG_SEMIGLOBAL;
    const bool kclass = (sgm && !c.has_nindel && c.match == 0 && c.mismatch == 1 && c.indel == 1) || (c.algorithm == BDX_ALG_EXACT && !getenv("BDX_NO_KNOWN_EXACT"));
    const int cmin = sgm ? (c.mismatch < c.indel ? c.mismatch : c.indel) : 1;
    if (cmin < 1 || (sgm && c.match < 0)) return BDX_OK;
    // the pairs tier (capped set): the filter only has to be lossless for alignments of COST <= cap x cmin — a barcode it does not
    // flag costs more, i.e. at least (cap + 1) cmin = the tier's slo (costs are integers; the tier exists for mismatch = cmin = 1)
    const long long cost_cap = (ctx->cur == 1 && ctx->tier_cap_fixed >= 0) ? (long long)ctx->tier_cap_fixed * cmin : (1LL << 40);
    const auto whole = [](const bdx_range_t &r) { return !r.start_from_end && r.start_offset <= 1 && r.end_from_end && r.end_offset >= 0; };
    int Btot = 0, cwt = 0;
    bool ranged = false;
    for (int k = 0; k < npass; ++k) {
        const bdx_pass_t &p = c.pass[k];
        // (a ref_search_range is allowed for :semiglobal: the kernel resolves every read's column window itself, classification.jl:795-807;
        // start / end ranges that could bind stay on the general kernel)
        if (p.explicit_window != 0 || !whole(p.barcode_start_range) || !whole(p.barcode_end_range)) return BDX_OK;
        if (!whole(p.ref_search_range)) {
            if (c.algorithm != BDX_ALG_SEMIGLOBAL) return BDX_OK;
            ranged = true;
        }
        if (p.n_barcodes < 1) return BDX_OK;
        for (uint32_t i = 0; i < p.bc_off[p.n_barcodes]; ++i) {
            const uint8_t ch = p.bc_bytes[i];
            if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') return BDX_OK;
        }
        Btot += p.n_barcodes;
        cwt += (p.n_barcodes + 31) / 32;
    }
    // more than 128 barcodes (known-score configs only: split mode keeps four mask words per read): groups of 128 barcodes,
    // each with its own piece tables of four-word masks
    if (Btot > 512 || (split && (cwt > 4 || Btot > 128))) return BDX_OK;
    const int groups = (Btot + 127) / 128;
    int nw = groups > 1 ? 4 : (Btot + 31) / 32;
    if (const char *e = getenv("BDX_PAIRS_NW")) nw = atoi(e) > nw ? atoi(e) : nw;  // (tuning experiment)
    if (nw > 4) nw = 4;
    const int estride = nw <= 2 ? 8 : 16;
    std::vector<uint32_t> meta((size_t)Btot, 0u), peq8((size_t)Btot * 9, 0u), settle((size_t)Btot, 0u), peq8r((size_t)Btot * 9, 0u);
    int kmax = 0, track = 1 << 20, mmin = 1 << 20, g = 0;
    struct Bc { int g, m, kb; const uint8_t *bc; };
    std::vector<Bc> bcs;
    // SAME-DIAGONAL variants (split configs whose indels cost more than their mismatches — the reference's demo2 options:
    // mismatch 1, indel 2, budget 6 of 24): an alignment with g indels lies on at most g + 1 diagonals and has at most
    // e(g) = g + floor((ae - g indel) / mismatch) operations; with P disjoint pieces, P - e(g) >= g + 2 for every possible g
    // puts two intact pieces on ONE diagonal (an intact piece cannot span an indel) — far more selective than "two pieces
    // within kb diagonals", and valid beyond the classic variant's 4 (kb + 2) <= m.  Tried per piece length: 4 bases
    // (six pieces), then 3 (eight).  The alignment then lies within g_max columns of that diagonal (`spread`).
    // Order of preference: six 4-base pieces on one diagonal (strictly more selective than the classic variant), the classic
    // variant (two 4-base pieces within kb diagonals) where its conditions hold, eight 3-base pieces on one diagonal.
    bool classic_ok = true;
    for (int k = 0; k < npass; ++k)
        for (int b = 0; b < c.pass[k].n_barcodes; ++b) {
            const int m = (int)(c.pass[k].bc_off[b + 1] - c.pass[k].bc_off[b]);
            const long long ae = std::min(cost_cap, c.algorithm == BDX_ALG_EXACT ? 0 : (long long)std::floor(c.max_error_rate * (double)m));
            if (ae >= 0 && (ae / cmin > 4 || 4 * (ae / cmin + 2) > m)) classic_ok = false;
        }
    int sd_pl = 0, sd_spread = 0;
    if (split && sgm && c.mismatch >= 1 && c.indel >= 1 && groups == 1) {
        for (int pl = 4; pl >= 3 && !sd_pl; --pl) {
            if (pl == 3 && classic_ok) break;
            bool ok = true;
            int spread = 0;
            for (int k = 0; k < npass && ok; ++k) {
                const bdx_pass_t &p = c.pass[k];
                for (int b = 0; b < p.n_barcodes && ok; ++b) {
                    const int m = (int)(p.bc_off[b + 1] - p.bc_off[b]);
                    const long long ae = std::min(cost_cap, (long long)std::floor(c.max_error_rate * (double)m));
                    if (ae < 0) continue;
                    const int P = std::min(pl == 4 ? 6 : 8, m / pl);
                    const long long gmax = ae / c.indel;
                    for (long long gg = 0; gg <= gmax && ok; ++gg) {
                        const long long e = gg + (ae - gg * c.indel) / c.mismatch;
                        ok = (long long)P - e >= gg + 2;
                    }
                    if (gmax > spread) spread = (int)gmax;
                    if (ae / cmin > 15 || m - (int)(ae / cmin) - 1 < 12) ok = false;  // (sweep budget field / score tracking from column 12)
                }
            }
            if (ok && spread <= 8) {
                sd_pl = pl;
                sd_spread = spread;
            }
        }
    }
    for (int k = 0; k < npass; ++k) {
        const bdx_pass_t &p = c.pass[k];
        for (int b = 0; b < p.n_barcodes; ++b, ++g) {
            const int m = (int)(p.bc_off[b + 1] - p.bc_off[b]);
            if (m < 1 || m > 32) return BDX_OK;
            const uint8_t *bc = p.bc_bytes + p.bc_off[b];
            const int shift = 32 - m;
            const uint32_t rows = m == 32 ? 0xFFFFFFFFu : (((1u << m) - 1u) << shift);
            const uint32_t pad = ~rows;
            for (int code = 0; code < 8; ++code) {
                uint32_t mask = pad;
                if (code < 4)
                    for (int i = 0; i < m; ++i)
                        if (((bc[i] >> 1) & 3) == code) mask |= 1u << (shift + i);
                peq8[(size_t)g * 9 + code] = mask;
                uint32_t maskr = pad;  // (the reversed barcode: known-trim class, see build_wave_tables)
                if (code < 4)
                    for (int i = 0; i < m; ++i)
                        if (((bc[m - 1 - i] >> 1) & 3) == code) maskr |= 1u << (shift + i);
                peq8r[(size_t)g * 9 + code] = maskr;
            }
            const long long ae = std::min(cost_cap, c.algorithm == BDX_ALG_EXACT ? 0 : (long long)std::floor(c.max_error_rate * (double)m));
            if (ae < 0) {  // can never be recorded: in no table entry, never swept
                meta[(size_t)g] = (uint32_t)m | (255u << 8) | (255u << 16);
                continue;
            }
            const long long kb = ae / cmin;
            if (!sd_pl && (kb > 4 || 4 * (kb + 2) > m)) return BDX_OK;
            int dmax = 255;
            for (long long d = 0; d <= kb; ++d)  // lone-survivor accept threshold of the replay, as in build_wave_tables
                if (d <= ae && (double)d / (double)m <= c.max_error_rate) dmax = (int)d;
            meta[(size_t)g] = (uint32_t)m | ((uint32_t)kb << 8) | ((uint32_t)dmax << 16) | ((uint32_t)sd_spread << 24);
            if ((int)kb > kmax) kmax = (int)kb;
            if (m - (int)kb - 1 < track) track = m - (int)kb - 1;
            if (m < mmin) mmin = m;
            bcs.push_back(Bc{g, m, (int)kb, bc});
        }
    }
    if (bcs.empty() || track < 12) return BDX_OK;
    const int KB = sd_pl == 4 ? 8 : sd_pl == 3 ? 9 : kmax <= 3 ? 3 : 4;  // (the kernel's variant number)
    const int PL = sd_pl ? sd_pl : 4, P = sd_pl == 4 ? 6 : sd_pl == 3 ? 8 : KB + 2, NK = 1 << (2 * PL);
    std::vector<uint32_t> tab((size_t)groups * P * NK * (size_t)(estride / 4), 0u);
    for (const Bc &x : bcs) {
        const int np = sd_pl ? std::min(P, x.m / PL) : x.kb + 2;  // pieces of this barcode
        for (int t = 0; t < np; ++t) {
            uint32_t key = 0;
            for (int i = 0; i < PL; ++i) key |= (uint32_t)((x.bc[PL * t + i] >> 1) & 3) << (2 * i);
            const int grp = x.g >> 7, gl = x.g & 127;
            tab[(((size_t)grp * P + (size_t)t) * NK + key) * (size_t)(estride / 4) + (size_t)(gl >> 5)] |= 1u << (gl & 31);
        }
    }
    wp.q = 4;
    wp.n_barcodes = Btot;
    wp.b0 = c.pass[0].n_barcodes;
    wp.split = split ? 1 : 0;
    wp.bm_bytes = (int)(tab.size() * 4);
    wp.n_ent = 0;
    wp.track_from = track > 28 ? 28 : track;
    wp.pairs_kb = KB;
    wp.pairs_spread = sd_pl ? sd_spread : KB;
    wp.nw = nw;
    wp.groups = groups;
    wp.ranged = ranged ? 1 : 0;
    wp.cand_words = split ? cwt : (c.is_dual ? 4 : 0);  // (known-score dual configs: the survivor slots of pass 1)
    if (bdx_wave_table_bytes(wp, ctx->plan.hist_entries) > 112 * 1024) return BDX_OK;  // (at least four waves' work areas must fit beside the tables)
    auto al = [](size_t x) { return (x + 63) & ~(size_t)63; };
    const size_t o_tab = 0, o_peq = al(tab.size() * 4), o_meta = o_peq + al(peq8.size() * 4), o_settle = o_meta + al(meta.size() * 4),
                 o_peqr = o_settle + al(settle.size() * 4), bytes = o_peqr + al(peq8r.size() * 4);
    std::vector<uint8_t> blob(bytes, 0);
    memcpy(blob.data() + o_tab, tab.data(), tab.size() * 4);
    memcpy(blob.data() + o_peq, peq8.data(), peq8.size() * 4);
    memcpy(blob.data() + o_meta, meta.data(), meta.size() * 4);
    memcpy(blob.data() + o_settle, settle.data(), settle.size() * 4);
    memcpy(blob.data() + o_peqr, peq8r.data(), peq8r.size() * 4);
    HIP_TRY(ctx, F.pair_tables.ensure(bytes));
    HIP_TRY(ctx, hipMemcpy(F.pair_tables.p, blob.data(), bytes, hipMemcpyHostToDevice));
    const uint8_t *base = (const uint8_t *)F.pair_tables.p;
    wp.d_bitmap = base + o_tab;
    wp.d_rank = (const uint16_t *)base;  // (never read)
    wp.d_ent = (const uint32_t *)base;
    wp.d_peq8 = (const uint32_t *)(base + o_peq);
    wp.d_meta = (const uint32_t *)(base + o_meta);
    wp.d_settle = (const uint32_t *)(base + o_settle);
    wp.d_peq8r = (const uint32_t *)(base + o_peqr);
    ctx->pair_mmin = mmin;
    wp.enabled = 1;
    // known-trim class (see build_wave_tables): the listed reads of a config with trim sides get verdict and keep range from
    // the pairs mode too, in its non-split form
    F.pplan_k = BdxWavePlan{};
    bool trims_ok = true;
    for (int k = 0; k < npass; ++k) trims_ok = trims_ok && c.pass[k].explicit_window != BDX_WINDOW_ALIGN_ONE;
    if (split && kclass && trims_ok && !c.need_traceback &&
        !ctx->tune.no_known && !ctx->tune.no_kend && groups == 1 && wp.pairs_kb <= 4) {  // (the same-diagonal variants only exist in split mode)
        F.pplan_k = wp;
        F.pplan_k.split = 0;
        F.pplan_k.cand_words = c.is_dual ? 4 : 0;
        F.pplan_k.kend = 1;
        for (int k = 0; k < npass; ++k)
            if (c.pass[k].trim_side == 3) F.pplan_k.kend = 2;
    }
    F.pplan_a = BdxWavePlan{};  // known-alignment class (build_wave_tables): the same with `summary` allowed
    if (split && kclass && trims_ok && !ctx->tune.no_known &&
        !ctx->tune.no_kend && !getenv("BDX_NO_KALN") && groups == 1 && wp.pairs_kb <= 4) {
        F.pplan_a = wp;
        F.pplan_a.split = 0;
        F.pplan_a.cand_words = c.is_dual ? 4 : 0;
        F.pplan_a.kend = 3;
    }
    return BDX_OK;
}

// Geometry of the pairs mode for a batch: 16-read tiles of slots of `read_len` rounded up to 16 bytes.
bool size_pairs(bdx_ctx *ctx, BdxWavePlan &wp, int read_len);
bool size_pairs(bdx_ctx *ctx, int read_len) { return size_pairs(ctx, ctx->fs[0].pplan, read_len); }
bool size_pairs(bdx_ctx *ctx, BdxWavePlan &wp, int read_len) {
    if (!wp.enabled || ctx->dev.vlen) return false;
    if (read_len < 1) read_len = 1;
    // a read's slot in the tile's images: its bytes are fetched as aligned 16-byte vectors, so it starts up to 15 positions in
    const int slot = (read_len + 15 + 15) & ~15;
    const int rw = 16;
    const int span = rw * slot + 16;
    if (span > 6 * 1024 + 16) return false;  // (instantiated: three and six 16-byte vectors per lane)
    int cpr = ((15 + read_len - ctx->pair_mmin + wp.pairs_spread + 8) >> 4) + 1;  // (diagonals are counted from the slot's start)
    if (read_len < ctx->pair_mmin) cpr = 1;
    if (cpr > slot / 16) cpr = slot / 16;
    if (cpr < 1) cpr = 1;
    const size_t tables = bdx_wave_table_bytes(wp, ctx->plan.hist_entries);
    // (31 chance flags per read at 96 barcodes and kb = 4: the queue holds a 16-read tile's worth; with more barcodes it is
    // drained several times per tile; a tile whose queue runs over between two drains is handed on / swept whole)
    // (same-diagonal variants: ~80 chance flags per read at 96 barcodes of eight 3-base pieces — the queue is drained inside the scan)
    wp.hq_cap = wp.groups > 1 ? 1024 : wp.pairs_kb >= 8 ? 1280 : 56 * rw;
    wp.sq_cap = 0;
    const size_t area = bdx_wave_area_bytes(rw, span, true, wp.hq_cap, 0, wp.cand_words + (wp.ranged ? 4 : 0));
    int best = 0;
    const int shapes[3] = {16, 8, 4};
    for (int w : shapes) {
        if (ctx->tune.wave_waves && w != ctx->tune.wave_waves) continue;
        const size_t lds = tables + (size_t)w * area;
        if (lds > LDS_MAX) continue;
        int per_cu = (int)(LDS_MAX / (((lds + 1279) / 1280) * 1280));
        if (per_cu * w > 16) per_cu = 16 / w;
        if (per_cu * w > best) {
            best = per_cu * w;
            wp.waves = w;
            wp.blocks = per_cu * ctx->n_cu;
        }
    }
    if (best < 4) return false;
    wp.rw = rw;
    wp.span_cap = span;
    wp.slot = slot;
    wp.cpr = cpr;
    wp.read_len_hint = read_len;
    return true;
}

// Geometry of the fused kernel for a given typical read length: the largest R whose LDS
// footprint still lets two workgroups share a CU (8 waves/CU), else whatever fits.
// set: the filter set planned (0: full budgets, 1: tier 1).
// force_slot: list mode (tier 0 of the tiered budgets) — the reads are scattered, every read is staged into a slot
bool size_bitpar(bdx_ctx *ctx, int set, int read_len, long long n_reads, bool force_slot = false) {
    BdxFilterSet &F = ctx->fs[set];
    BdxBitparPlan &bp = F.bplan;
    if (!bp.enabled) return false;
    if (read_len < 1) read_len = 1;
    if (ctx->dev.vlen) force_slot = true;  // window upload: only each read's window is there
    // small batches: keep >= ~1024 tiles in flight (4 per CU) before growing the tile
    int r_cap = 256;
    while (r_cap > 16 && n_reads / r_cap < 4LL * ctx->n_cu) r_cap >>= 1;
    if (bp.read_len_hint == read_len && bp.r_cap == r_cap && bp.reads_per_block > 0 && (bp.slot_bytes > 0 || !force_slot)) return true;
    bp.r_cap = r_cap;
    const int forced = ctx->tune.bitpar_r;
    // Pick the R that keeps the most waves resident per CU (the sweep is latency-bound):
    // workgroups/CU = min(8, floor(160 KiB / LDS(R))) with 4 waves each; ties -> larger R
    // (fewer table reloads).  R = 16 is only taken when nothing larger fits.
    // Column-window bound for this read length: the union over the passes of
    // final_search_range (classification.jl:799-800), resolved exactly like the device does.
    // Window lengths are non-decreasing in n, so the bound at the hint covers shorter reads.
    int wmax = read_len;
    {
        long long ulo = (1LL << 40), uhi = 0;
        const int npass = ctx->dev.is_dual ? 2 : 1;
        for (int k = 0; k < npass; ++k) {
            const BdxDevPass &P = ctx->dev.pass[k];
            long long f, l;
            if (P.explicit_window) {
                f = P.win_first;
                l = P.win_last;
            } else {
                auto res = [&](const BdxDevRange &dr, long long &a, long long &b) {
                    long long s = dr.start_from_end ? read_len + dr.start_offset : dr.start_offset;
                    long long e = dr.end_from_end ? read_len + dr.end_offset : dr.end_offset;
                    a = s > 1 ? s : 1;
                    b = e < read_len ? e : read_len;
                    if (b < a) b = a - 1;
                };
                long long rf, rl, bf, bl, ef, el;
                res(P.ref_search, rf, rl);
                res(P.bc_start, bf, bl);
                res(P.bc_end, ef, el);
                f = rf > bf ? rf : bf;
                l = rl < el ? rl : el;
            }
            if (f < 1) f = 1;
            if (l > read_len) l = read_len;
            if (l < f) continue;
            long long h = ctx->dev.algorithm == BDX_ALG_SEMIGLOBAL ? l : l + ctx->dev.max_m - 1;
            if (h > read_len) h = read_len;
            if (f - 1 < ulo) ulo = f - 1;
            if (h > uhi) uhi = h;
        }
        if (uhi > ulo) wmax = (int)(uhi - ulo);
        else wmax = 16;
    }
    const bool slot_mode = force_slot || ((long long)wmax * 2 + 96 <= (long long)read_len && !ctx->tune.no_slot);
    const int slot = slot_mode ? ((wmax + 15 + 16 + 15) & ~15) : 0;
    bp.slot_bytes = slot;
    bp.seed_span = slot_mode ? wmax : read_len;
    if (F.splan.enabled && F.splan.diag) {
        // index width for this read length, and the sweep queue for the expected number of flagged pairs
        if (bp.seed_span > 312) {  // the widest index holds 320 positions: weak single seeds if they apply, else the plain sweep
            F.splan = F.splan_alt;  // (disabled if weak seeds do not apply either)
            F.splan_alt = BdxSeedPlan{};
            return size_bitpar(ctx, set, read_len, n_reads, force_slot);
        }
        bp.diag_nw = bp.seed_span <= 152 ? 5 : 10;
        const double L = (double)(bp.seed_span < 32 ? 32 : bp.seed_span);
        const double flagged = F.splan.diag_flag_coef * ((L - 3.0) / 256.0) * ((L - 3.0) / 256.0) / (L + 24.0) +
                               (double)(F.splan.n_always[0] + F.splan.n_always[1]);
        bp.diag_qcap = (int)(flagged * 1.3) + 12;  // per read (a sub-batch shares 4..8 reads' worth)
    }
    const bool diag = F.splan.enabled && F.splan.diag;
    const int tries[7] = {256, 128, 64, 32, 16, 8, 4};
    int best_R = 0, best_blocks = 0, best_stage = 0;
    for (int R : tries) {
        if (diag ? R > 32 : R < 16) continue;  // the diagonal variant indexes 8 reads at a time (40 KiB): small tiles
        if (forced && R != forced) continue;
        if (!forced && R > r_cap) continue;
        if (bp.word_bytes == 16 && (R > 64 || R < 16)) continue;  // (128-bit sweep words: instantiated for tiles of 64 / 32 / 16 reads)
        if (!forced && !F.splan.enabled && R > 64 && read_len <= 1024) continue;  // sweep-all: 64-read tiles measured best
        size_t st = slot_mode ? (size_t)R * (size_t)slot : (size_t)R * (size_t)read_len + 64;
        st = (st + 15) & ~(size_t)15;
        if (st > (size_t)1 << 20) continue;
        bp.reads_per_block = R;
        bp.stage_bytes = (int)st;
        bp.read_len_hint_for_lds = read_len;
        const size_t lds = bdx_bitpar_lds_bytes(ctx->dev, bp, ctx->plan, &F.splan);
        if (lds > LDS_MAX) continue;
        int blocks = (int)(LDS_MAX / (((lds + 1279) / 1280) * 1280));  // LDS is allocated in 1280-byte granules (measured: 54128 B -> 2 per CU, 51872 B -> 3)
        // Measured on MI355X (tools/probe.py): tile size matters more than residency once 3
        // workgroups (12 waves) share a CU — larger tiles fill the 256 lanes of the sparse
        // sweep / exact stages better.  Rank: >= 3 resident (largest R wins), then 2, then 1.
        const int rank = blocks >= 3 ? 3 : blocks;
        if (!diag && R == 16 && best_R) continue;
        if (rank > best_blocks) {
            best_blocks = rank;
            best_R = R;
            best_stage = (int)st;
        }
    }
    if (best_R && diag && best_blocks < 2) {
        // the index leaves room for one workgroup per CU only (very many barcodes): weak single seeds if they
        // apply, else the plain sweep
        F.splan = F.splan_alt;  // (disabled if weak seeds do not apply either)
        F.splan_alt = BdxSeedPlan{};
        return size_bitpar(ctx, set, read_len, n_reads, force_slot);
    }
    if (best_R) {
        bp.reads_per_block = best_R;
        bp.stage_bytes = best_stage;
        bp.read_len_hint = read_len;
        bp.read_len_hint_for_lds = read_len;
        return true;
    }
    if (F.splan.enabled) {
        // the seed tables do not fit next to everything else (very many barcodes): the two-intact-pieces index
        // gives way to the weak single seeds kept beside it; those give way to the plain sweep; plan again
        if (F.splan.diag && F.splan_alt.enabled) {
            F.splan = F.splan_alt;
            F.splan_alt = BdxSeedPlan{};
        } else {
            F.splan.enabled = 0;
        }
        return size_bitpar(ctx, set, read_len, n_reads, force_slot);
    }
    bp.reads_per_block = 0;
    bp.read_len_hint = 0;
    return false;
}

int validate(const bdx_config_t *c) {
    if (!c) return fail(nullptr, BDX_E_INVALID, "config is NULL");
    if (c->abi_version != BDX_ABI_VERSION)
        return fail(nullptr, BDX_E_INVALID, "ABI version mismatch: header %u, library %u", c->abi_version,
                    (unsigned)BDX_ABI_VERSION);
    if (c->struct_size != sizeof(bdx_config_t))
        return fail(nullptr, BDX_E_INVALID, "bdx_config_t size mismatch: caller %u, library %zu", c->struct_size,
                    sizeof(bdx_config_t));
    if (c->algorithm < BDX_ALG_SEMIGLOBAL || c->algorithm > BDX_ALG_EXACT)
        return fail(nullptr, BDX_E_INVALID, "unknown matching_algorithm %d", c->algorithm);
    if (!std::isfinite(c->max_error_rate) || std::fabs(c->max_error_rate) > BDX_MAX_RATE)
        return fail(nullptr, BDX_E_INVALID, "max_error_rate must be finite and |rate| <= %g", BDX_MAX_RATE);
    if (!std::isfinite(c->min_delta)) return fail(nullptr, BDX_E_INVALID, "min_delta must be finite");
    const int costs[4] = {c->match, c->mismatch, c->indel, c->has_nindel ? c->nindel : 1};
    for (int v : costs)
        if (v > BDX_MAX_COST || v < -BDX_MAX_COST)
            return fail(nullptr, BDX_E_INVALID, "scoring costs must lie in [-%d, %d]", BDX_MAX_COST, BDX_MAX_COST);
    if (c->algorithm == BDX_ALG_SEMIGLOBAL) {
        // the reference divides by indel / min(indel, nindel) (classification.jl:170-176);
        // a zero divisor raises DivideError there for every read.
        const int div = c->has_nindel ? (c->indel < c->nindel ? c->indel : c->nindel) : c->indel;
        if (div == 0) return fail(nullptr, BDX_E_INVALID, "indel (and nindel) must be non-zero (DivideError in the reference)");
    }
    const int npass = c->is_dual ? 2 : 1;
    for (int k = 0; k < npass; ++k) {
        const bdx_pass_t &p = c->pass[k];
        // core.jl:308-313
        if (p.trim_side != 0 && p.trim_side != 3 && p.trim_side != 5)
            return fail(nullptr, BDX_E_INVALID, "trim_side%s must be 3 or 5, got %d", k ? "2" : "", p.trim_side);
        if (p.n_barcodes < 1) return fail(nullptr, BDX_E_INVALID, "pass %d has no barcodes", k + 1);
        if (!p.bc_bytes || !p.bc_off || !p.bc_len_no_N)
            return fail(nullptr, BDX_E_INVALID, "pass %d barcode tables are NULL", k + 1);
        if (p.bc_off[0] != 0) return fail(nullptr, BDX_E_INVALID, "bc_off[0] must be 0");
        for (int i = 0; i < p.n_barcodes; ++i) {
            if (p.bc_off[i + 1] < p.bc_off[i]) return fail(nullptr, BDX_E_INVALID, "bc_off must be non-decreasing");
            const uint32_t m = p.bc_off[i + 1] - p.bc_off[i];
            if (m == 0)
                return fail(nullptr, BDX_E_INVALID, "barcode %d of pass %d is empty (outside the supported domain)", i + 1, k + 1);
            if (m > BDX_MAX_M)
                return fail(nullptr, BDX_E_INVALID, "barcode %d of pass %d is longer than %d", i + 1, k + 1, BDX_MAX_M);
            if (p.bc_len_no_N[i] < 0 || p.bc_len_no_N[i] > (int32_t)m)
                return fail(nullptr, BDX_E_INVALID, "bc_len_no_N[%d] out of range", i);
        }
        if (p.explicit_window < 0 || p.explicit_window > BDX_WINDOW_ALIGN_ONE)
            return fail(nullptr, BDX_E_INVALID, "explicit_window must be 0, 1 or 2");
        if (p.explicit_window) {
            const int64_t lim = (int64_t)1 << 30;
            const int64_t w[4] = {p.win_first, p.win_last, p.win_max_start_pos, p.win_min_end_pos};
            for (int64_t v : w)
                if (v > lim || v < -lim) return fail(nullptr, BDX_E_INVALID, "explicit window values must be within +-2^30");
        }
    }
    return BDX_OK;
}

int upload_tables(bdx_ctx *ctx) {
    const bdx_config_t &c = ctx->cfg;
    BdxDevCfg &d = ctx->dev;
    d.algorithm = c.algorithm;
    d.is_dual = c.is_dual != 0;
    d.max_error_rate = c.max_error_rate;
    d.min_delta = c.min_delta;
    d.match = c.match;
    d.mismatch = c.mismatch;
    d.indel = c.indel;
    d.has_nindel = c.has_nindel != 0;
    d.nindel = c.has_nindel ? c.nindel : 0;
    d.need_traceback = c.need_traceback != 0;
    d.force_lds_dp = ctx->tune.lds_dp;
    d.band_kb[0] = d.band_kb[1] = -1;
    d.band_m = 0;
    d.dense_w = 0;
    d.band_lb[0] = d.band_lb[1] = 0;
    d.max_m = 1;
    d.any_traceback = d.need_traceback;
    const int npass = d.is_dual ? 2 : 1;
    for (int k = 0; k < 2; ++k) {
        BdxDevPass &P = d.pass[k];
        memset(&P, 0, sizeof P);
        if (k >= npass) continue;
        const bdx_pass_t &p = c.pass[k];
        P.ref_search = cvt_range(p.ref_search_range);
        P.bc_start = cvt_range(p.barcode_start_range);
        P.bc_end = cvt_range(p.barcode_end_range);
        P.trim_side = p.trim_side;
        P.n_barcodes = p.n_barcodes;
        P.cand_words = (p.n_barcodes + 31) / 32;
        P.explicit_window = p.explicit_window;
        P.win_first = p.win_first;
        P.win_last = p.win_last;
        P.win_max_start = p.win_max_start_pos;
        P.win_min_end = p.win_min_end_pos;
        if (p.trim_side != 0) d.any_traceback = 1;
        const size_t nbytes = p.bc_off[p.n_barcodes];
        for (int i = 0; i < p.n_barcodes; ++i) {
            const int m = (int)(p.bc_off[i + 1] - p.bc_off[i]);
            if (m > d.max_m) d.max_m = m;
        }
        HIP_TRY(ctx, ctx->bc_bytes[k].ensure(nbytes + 16));
        HIP_TRY(ctx, ctx->bc_off[k].ensure((size_t)(p.n_barcodes + 1) * 4));
        HIP_TRY(ctx, ctx->bc_nn[k].ensure((size_t)p.n_barcodes * 4));
        HIP_TRY(ctx, hipMemcpy(ctx->bc_bytes[k].p, p.bc_bytes, nbytes, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(ctx->bc_off[k].p, p.bc_off, (size_t)(p.n_barcodes + 1) * 4, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(ctx->bc_nn[k].p, p.bc_len_no_N, (size_t)p.n_barcodes * 4, hipMemcpyHostToDevice));
        P.bc_bytes = (const uint8_t *)ctx->bc_bytes[k].p;
        P.bc_off = (const uint32_t *)ctx->bc_off[k].p;
        P.bc_len_no_N = (const int32_t *)ctx->bc_nn[k].p;
    }
    d.counts_stride2 = d.is_dual ? (d.pass[1].n_barcodes > 1 ? d.pass[1].n_barcodes : 1) : 1;
    const long long nc = 4LL + (long long)d.pass[0].n_barcodes * d.counts_stride2;
    if (nc > (1LL << 28)) return fail(ctx, BDX_E_INVALID, "sample_counts table too large (%lld entries)", nc);
    d.n_counts = (int)nc;
    // allowed_error = floor(rate * normalisation) must stay inside the int32 DP domain
    if (std::fabs(c.max_error_rate) * (double)d.max_m >= (double)(1 << 27))
        return fail(ctx, BDX_E_INVALID, "max_error_rate * barcode length exceeds the supported range");
    HIP_TRY(ctx, ctx->counts_own.ensure((size_t)d.n_counts * 8));
    HIP_TRY(ctx, hipMemset(ctx->counts_own.p, 0, (size_t)d.n_counts * 8));
    ctx->counts = (unsigned long long *)ctx->counts_own.p;
    return BDX_OK;
}

}  // namespace

int bdx_stats_reserve(bdx_ctx *ctx, long long rows, bool exact) {
    if (!ctx->dev.need_traceback || rows <= ctx->st_rows) return BDX_OK;
    long long want = rows;
    if (!exact) {  // generous steps: a batch with slightly longer reads must not re-allocate every time
        want = ctx->st_rows ? ctx->st_rows + ctx->st_rows / 2 : 0;
        if (want < rows) want = rows;
        want = (want + 63) & ~63LL;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // zeroing and copying run on the context's stream (the kernels that add to the tables do, and a non-blocking or
    // caller-supplied stream has no implicit order with the NULL stream); old tables are freed after one more sync
    const int npass = ctx->dev.is_dual ? 2 : 1;
    std::vector<DevBuf> retired;
    auto retire_all = [&]() {
        (void)hipStreamSynchronize(ctx->stream);
        for (DevBuf &b : retired) b.release();
        retired.clear();
    };
    if (!ctx->st_len_fixed) {
        // the transposed len table grows by its key stride: every barcode's run of counters moves to the new pitch
        const int old_stride = bdx_stats_stride(ctx, 1);
        const int old_rows = ctx->st_len_rows;
        ctx->st_len_rows = (int)(want > 0x3FFFFFF0LL ? 0x3FFFFFF0LL : want);
        const int new_stride = bdx_stats_stride(ctx, 1);
        for (int p = 0; p < npass; ++p) {
            const size_t B = (size_t)ctx->dev.pass[p].n_barcodes;
            DevBuf nb;
            hipError_t e1 = nb.ensure((size_t)new_stride * B * 8);
            if (e1 == hipSuccess) e1 = hipMemsetAsync(nb.p, 0, (size_t)new_stride * B * 8, ctx->stream);
            if (e1 == hipSuccess && old_rows > 0 && ctx->st_tab[p][1].p)
                e1 = hipMemcpy2DAsync(nb.p, (size_t)new_stride * 8, ctx->st_tab[p][1].p, (size_t)old_stride * 8, (size_t)old_stride * 8, B,
                                      hipMemcpyDeviceToDevice, ctx->stream);
            if (e1 != hipSuccess) {
                retire_all();
                nb.release();
                ctx->st_len_rows = old_rows;
                return fail(ctx, BDX_E_DEVICE, "growing the statistics tables failed: %s", hipGetErrorString(e1));
            }
            retired.push_back(ctx->st_tab[p][1]);
            ctx->st_tab[p][1] = nb;
        }
    }
    for (int p = 0; p < npass; ++p)
        for (int w = 0; w < 1; ++w) {  // pos (raw has a fixed height; len: above)
            const size_t old_bytes = bdx_stats_phys_words(ctx, p, w, ctx->st_rows) * 8;
            const size_t new_bytes = bdx_stats_phys_words(ctx, p, w, want) * 8;
            DevBuf nb;
            hipError_t e1 = nb.ensure(new_bytes);
            if (e1 == hipSuccess) e1 = hipMemsetAsync(nb.p, 0, new_bytes, ctx->stream);
            if (e1 == hipSuccess && old_bytes) e1 = hipMemcpyAsync(nb.p, ctx->st_tab[p][w].p, old_bytes, hipMemcpyDeviceToDevice, ctx->stream);
            if (e1 != hipSuccess) {
                retire_all();
                nb.release();
                return fail(ctx, BDX_E_DEVICE, "growing the statistics tables failed: %s", hipGetErrorString(e1));
            }
            retired.push_back(ctx->st_tab[p][w]);
            ctx->st_tab[p][w] = nb;  // row-major by key: the old table is a prefix of the new one
        }
    retire_all();
    ctx->st_rows = want;
    return BDX_OK;
}

namespace {

// statistics tables whose size is known from the config: the raw-score table (and the overflow flag)
int init_stats(bdx_ctx *ctx) {
    if (!ctx->dev.need_traceback) return BDX_OK;
    const bdx_config_t &c = ctx->cfg;
    const int npass = c.is_dual ? 2 : 1;
    double top = 0.0;  // the largest recordable numerator: floor(rate * normalisation) at the initial threshold
    for (int k = 0; k < npass; ++k)
        for (int b = 0; b < c.pass[k].n_barcodes; ++b) {
            const int m = (int)(c.pass[k].bc_off[b + 1] - c.pass[k].bc_off[b]);
            const double norm = (c.algorithm == BDX_ALG_SEMIGLOBAL && c.has_nindel) ? (double)c.pass[k].bc_len_no_N[b] : (double)m;
            const double ae = c.algorithm == BDX_ALG_EXACT ? 0.0 : std::floor(c.max_error_rate * norm);
            if (ae > top) top = ae;
        }
    if (top > (double)(1 << 20))
        return fail(ctx, BDX_E_INVALID, "summary statistics support scores up to %d; max_error_rate * barcode length gives %g", 1 << 20, top);
    ctx->st_raw_rows = (int)top + 1;
    // Clean-class configs (and :hamming / :exact): an alignment spans at most m columns plus its insertions (<= m),
    // leading deletions count through the origin: end - start + 1 <= 2 m — a fixed height.  Otherwise (start / end
    // ranges that bind: the band's seeded cells carry origins of their own) only start >= 1 - m and end <= n hold:
    // the table grows with the reads like the position table.
    // (:semiglobal with a ref_search_range that starts inside the read: an alignment out of the reference's initial column keeps the
    // origin 1 - i whatever the window's first column is, classification.jl:278-283 — its length end - start + 1 reaches n + m:
    // found by round 4's known-alignment tests, "a statistics key fell outside its table" on ref_search_range = "end-90:end")
    bool sg_window = false;
    if (c.algorithm == BDX_ALG_SEMIGLOBAL)
        for (int p = 0; p < npass; ++p) {
            const bdx_range_t &r = c.pass[p].ref_search_range;
            sg_window = sg_window || r.start_from_end || r.start_offset > 1 || c.pass[p].explicit_window != 0;
        }
    ctx->st_len_fixed = (ctx->plan.clean || ctx->plan.band_roll || c.algorithm != BDX_ALG_SEMIGLOBAL) && !sg_window;
    ctx->st_len_rows = ctx->st_len_fixed ? 2 * ctx->dev.max_m + 2 : 0;
    for (int p = 0; p < npass; ++p)
        for (int w = (ctx->st_len_fixed ? 1 : 2); w < 3; ++w) {
            const size_t bytes = bdx_stats_phys_words(ctx, p, w, 0) * 8;
            HIP_TRY(ctx, ctx->st_tab[p][w].ensure(bytes));
            HIP_TRY(ctx, hipMemsetAsync(ctx->st_tab[p][w].p, 0, bytes, ctx->stream));
        }
    HIP_TRY(ctx, ctx->st_flag.ensure(256));
    HIP_TRY(ctx, hipMemsetAsync(ctx->st_flag.p, 0, 256, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (ordered on the stream the kernels use, and done before create returns)
    return BDX_OK;
}

}  // namespace


extern "C" {

int32_t bdx_abi_version(void) { return BDX_ABI_VERSION; }

const char *bdx_last_error(const bdx_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int32_t bdx_create(const bdx_config_t *config, bdx_ctx **out) {
    if (!out) return fail(nullptr, BDX_E_INVALID, "out is NULL");
    *out = nullptr;
    int rc = validate(config);
    if (rc != BDX_OK) return rc;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, BDX_E_DEVICE, "no HIP device available (%s); this library has no CPU fallback",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (config->device < 0 || config->device >= ndev)
        return fail(nullptr, BDX_E_INVALID, "device ordinal %d out of range (0..%d)", config->device, ndev - 1);
    bdx_ctx *ctx = new (std::nothrow) bdx_ctx();
    if (!ctx) return fail(nullptr, BDX_E_DEVICE, "out of host memory");
    ctx->cfg = *config;
    ctx->device = config->device;
    ctx->tune = read_tuning();  // the environment is consulted here and nowhere else
    auto bail = [&](int code) {
        g_create_error = ctx->err;
        bdx_destroy(ctx);
        return code;
    };
    if (hipSetDevice(ctx->device) != hipSuccess) {
        ctx->err = "hipSetDevice failed";
        return bail(BDX_E_DEVICE);
    }
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
        ctx->err = "hipStreamCreate failed";
        return bail(BDX_E_DEVICE);
    }
    ctx->stream = ctx->own_stream;
    {
        // the device's shape comes from the device (a partitioned part has fewer compute units than a full MI355X)
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus < 1) cus = 256;
        ctx->n_cu = ctx->tune.cu_count > 0 ? ctx->tune.cu_count : cus;
    }
    rc = upload_tables(ctx);
    if (rc != BDX_OK) return bail(rc);
    if (ctx->d_dbg.ensure(256) != hipSuccess || hipMemset(ctx->d_dbg.p, 0, 256) != hipSuccess) {
        ctx->err = "hipMalloc failed";
        return bail(BDX_E_DEVICE);
    }
    ctx->dev.dbg_rejected = (unsigned int *)ctx->d_dbg.p;
    rc = plan_generic(ctx);  // needs the caller's host tables: run before they are dropped
    if (rc != BDX_OK) return bail(rc);
    ctx->plan.n_cu = ctx->n_cu;
    rc = init_stats(ctx);
    if (rc != BDX_OK) return bail(rc);
    rc = build_bitpar_tables(ctx);
    if (rc != BDX_OK) return bail(rc);
    if (ctx->plan.band_roll && !ctx->F().bplan.enabled) {  // no filter, no hand-over windows: the rolling band would walk whole windows
        ctx->band_roll_off = true;
        rc = plan_generic(ctx);
        if (rc != BDX_OK) return bail(rc);
        ctx->plan.n_cu = ctx->n_cu;
    }
    rc = build_seed_tables(ctx, true);
    if (rc != BDX_OK) return bail(rc);
    rc = build_diag_tables(ctx);
    if (rc != BDX_OK) return bail(rc);
    if (!ctx->F().splan.enabled) {  // neither: moderately selective single seeds still beat sweeping every pair
        rc = build_seed_tables(ctx, false);
        if (rc != BDX_OK) return bail(rc);
    } else if (ctx->F().splan.diag) {  // the fallback of size_bitpar when the index does not fit a batch
        rc = build_seed_tables(ctx, false, true);
        if (rc != BDX_OK) return bail(rc);
    }
    rc = build_wave_tables(ctx);
    if (rc != BDX_OK) return bail(rc);
    rc = build_pair_tables(ctx);
    if (rc != BDX_OK) return bail(rc);
    // tier 1 (capped budgets, strict single seeds) beside a full-budget set that is NOT already strict single seeds
    {
        const BdxFilterSet &full = ctx->fs[0];
        const bool strict_full = full.splan.enabled && !full.splan.diag && full.splan.q >= 7;
        // (the unit-level API's hand-made windows stay on the plain path)
        bool plain_windows = true;
        for (int k = 0; k < (config->is_dual ? 2 : 1); ++k) {
            plain_windows = plain_windows && config->pass[k].explicit_window == 0;
            // N-scoring with real wildcards: position-dependent indel costs — "an alignment's result does not depend on
            // the running threshold" is only argued (and fuzzed) for uniform costs; such configs stay on one tier
            if (config->algorithm == BDX_ALG_SEMIGLOBAL && config->has_nindel)
                for (uint32_t i = 0; i < config->pass[k].bc_off[config->pass[k].n_barcodes]; ++i)
                    if (config->pass[k].bc_bytes[i] == 'N') plain_windows = false;
        }
        if (full.bplan.enabled && plain_windows && !strict_full && !ctx->tune.no_tier && config->filter == BDX_FILTER_AUTO) {
            // Piece length behind tier 1's capped budgets, cap(m) = m / q - 1: 8-base seeds are the most selective; 7- or
            // 6-base pieces raise the cap of some lengths by one (14-15 and 21-23 bases with q = 7, 12-13 with q = 6), so
            // that tier 1 settles reads with one more error and tier 0 — a plain sweep or the two-intact-pieces kernel —
            // sees far fewer reads (m = 14, B = 96, rate 0.2: 444 -> 724 M reads/s), as long as the chance hits per
            // read stay few and no cap goes beyond 2 (measured: caps of 3 — m = 24 with q = 6, m = 28 with q = 7 — cost
            // more in tier 1 than they save in tier 0, at 24 and at 96 barcodes).
            {
                int cmin = 1;
                if (config->algorithm == BDX_ALG_SEMIGLOBAL) {
                    cmin = config->mismatch < config->indel ? config->mismatch : config->indel;
                    if (config->has_nindel && config->nindel < cmin) cmin = config->nindel;
                    if (cmin < 1) cmin = 1;
                }
                long long best_caps = -1;
                int best_q = 8;
                const double limit[9] = {0, 0, 0, 0, 0, 0, 8.0, 4.0, 1e30};
                for (int q = 8; q >= 6; --q) {
                    long long caps = 0, pieces = 0, cap_max = 0;
                    for (int k = 0; k < (config->is_dual ? 2 : 1); ++k)
                        for (int b = 0; b < config->pass[k].n_barcodes; ++b) {
                            const int m = (int)(config->pass[k].bc_off[b + 1] - config->pass[k].bc_off[b]);
                            const double norm = (config->algorithm == BDX_ALG_SEMIGLOBAL && config->has_nindel) ? (double)config->pass[k].bc_len_no_N[b] : (double)m;
                            const long long ae = config->algorithm == BDX_ALG_EXACT ? 0 : (long long)std::floor(config->max_error_rate * norm);
                            if (ae < 0) continue;
                            long long cap = m / q - 1;
                            if (cap < 0) cap = 0;
                            if (cap > ae / cmin) cap = ae / cmin;
                            caps += cap;
                            pieces += cap + 1;
                            if (cap > cap_max) cap_max = cap;
                        }
                    const double chance = 150.0 * (double)pieces / std::pow(4.0, (double)q);
                    // a cap lifted from 0 to 1 pays at once, 1 -> 2 a little, 2 -> 3 never did (measured, B = 24 and 96)
                    if (q < 8 && cap_max > (q == 6 ? 1 : 2)) continue;
                    if (chance <= limit[q] && caps > best_caps) {
                        best_caps = caps;
                        best_q = q;
                    }
                }
                ctx->tier_q = best_q;
            }
            if (ctx->tune.tier_q >= 5 && ctx->tune.tier_q <= 8) ctx->tier_q = ctx->tune.tier_q;
            ctx->cur = 1;
            rc = build_bitpar_tables(ctx);
            if (rc == BDX_OK && ctx->fs[1].bplan.enabled && ctx->fs[1].bplan.tier_capped) {
                rc = build_seed_tables(ctx, true);
                // very many barcodes: moderately selective 8-base seeds (a dozen chance pairs per read) still beat
                // the full-budget filter by far
                if (rc == BDX_OK && !ctx->fs[1].splan.enabled) rc = build_seed_tables(ctx, false);
                if (rc == BDX_OK && ctx->fs[1].splan.enabled && ctx->fs[1].splan.q < ctx->tier_q) ctx->fs[1].splan.enabled = 0;
                if (rc == BDX_OK) rc = build_wave_tables(ctx);
            }
            ctx->cur = 0;
            if (rc != BDX_OK) return bail(rc);
            ctx->tiered = ctx->fs[1].bplan.enabled && ctx->fs[1].bplan.tier_capped && ctx->fs[1].splan.enabled;
            // with_delta and a min_delta beyond the score of an unseen barcode: not even a perfect match can be
            // proven unambiguous at the capped budgets (only a visible runner-up could settle a read) — tier 1
            // would be a pass over the whole batch for next to nothing
            if (ctx->tiered && config->min_delta != 0.0)
                for (int k = 0; k < (config->is_dual ? 2 : 1); ++k)
                    if (!(ctx->fs[1].bplan.tier_slo[k] >= config->min_delta)) ctx->tiered = 0;
        }
    }
    // The PAIRS TIER: a split config with min_delta whose seed tier proves nothing (above), mismatch = cmin = 1 and indels dearer —
    // the reference's demo2 options (mismatch 1, indel 2, rate 0.25, min_delta 0.15): tier 1 = the same-diagonal pairs mode with
    // six 4-base pieces over the WHOLE batch at budgets capped at 4 (3) operations — ~3 chance flags per read instead of the ~90 of
    // the full-budget variant — followed by the exact kernel, which settles every read whose winner leaves min_delta of room below
    // slo = (cap + 1) / m (a perfect match or one mismatch under demo2's options: ~75 % of the reads) and lists the rest for tier 0.
    if (!ctx->tiered && ctx->fs[0].bplan.enabled && ctx->fs[0].pplan.enabled && ctx->fs[0].pplan.split && !ctx->tune.no_tier && !ctx->tune.no_pairs &&
        config->filter == BDX_FILTER_AUTO && config->algorithm == BDX_ALG_SEMIGLOBAL && !config->has_nindel && config->mismatch == 1 &&
        config->indel >= 2 && config->match == 0 && config->min_delta != 0.0) {
        bool plain = true;
        for (int k = 0; k < (config->is_dual ? 2 : 1); ++k) plain = plain && config->pass[k].explicit_window == 0;
        for (int cap = 4; cap >= 3 && plain && !ctx->tiered; --cap) {
            ctx->tier_cap_fixed = cap;
            ctx->cur = 1;
            ctx->fs[1].splan = BdxSeedPlan{};
            ctx->fs[1].wplan = BdxWavePlan{};
            rc = build_bitpar_tables(ctx);
            bool ok = rc == BDX_OK && ctx->fs[1].bplan.enabled && ctx->fs[1].bplan.tier_capped;
            for (int k = 0; ok && k < (config->is_dual ? 2 : 1); ++k) ok = ctx->fs[1].bplan.tier_slo[k] >= config->min_delta;
            if (ok) rc = build_pair_tables(ctx);
            ok = ok && rc == BDX_OK && ctx->fs[1].pplan.enabled && ctx->fs[1].pplan.pairs_kb == 8 && ctx->fs[1].pplan.split;
            ctx->cur = 0;
            if (rc != BDX_OK) return bail(rc);
            if (ok) {
                ctx->tiered = 1;
                ctx->pairs_tier = 1;
            } else {
                ctx->tier_cap_fixed = -1;
                ctx->fs[1].bplan.enabled = 0;
            }
        }
    }
    ctx->path = ctx->F().bplan.enabled ? (ctx->F().splan.enabled ? (ctx->F().splan.diag ? "qgram2+bitpar+verify" : "qgram+bitpar+verify") : "bitpar+verify") : "generic";
    if (ctx->tiered) ctx->path = "tier1:qgram+bitpar > " + ctx->path;
    ctx->filter_used = ctx->F().bplan.enabled ? (ctx->F().splan.enabled ? BDX_FILTER_QGRAM : BDX_FILTER_BITPAR) : BDX_FILTER_OFF;
    if (ctx->F().bplan.enabled) {
        if (ctx->d_maxlen.ensure(1024) != hipSuccess) {
            ctx->err = "hipMalloc failed";
            return bail(BDX_E_DEVICE);
        }
    }
    // the copied config must not keep pointing at caller memory
    for (int k = 0; k < 2; ++k) {
        ctx->cfg.pass[k].bc_bytes = nullptr;
        ctx->cfg.pass[k].bc_off = nullptr;
        ctx->cfg.pass[k].bc_len_no_N = nullptr;
    }
    if (bdx_generic_set_lds_limit(LDS_MAX) != hipSuccess) {
        ctx->err = "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed";
        return bail(BDX_E_DEVICE);
    }
    *out = ctx;
    return BDX_OK;
}

void bdx_destroy(bdx_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->own_stream) {
        (void)hipStreamSynchronize(ctx->own_stream);
        (void)hipStreamDestroy(ctx->own_stream);
    }
    if (ctx->copy_stream) {
        (void)hipStreamSynchronize(ctx->copy_stream);
        for (hipEvent_t &e : ctx->copy_events)
            if (e) (void)hipEventDestroy(e);
        (void)hipStreamDestroy(ctx->copy_stream);
    }
    if (ctx->d_dbg.p) {
        unsigned int rej[2] = {0, 0};
        if (hipMemcpy(rej, ctx->d_dbg.p, sizeof rej, hipMemcpyDeviceToHost) == hipSuccess) g_rejected_windows += (long long)rej[0] + rej[1];
    }
    ctx->d_dbg.release();
    for (int k = 0; k < 2; ++k) {
        ctx->bc_bytes[k].release();
        ctx->bc_off[k].release();
        ctx->bc_nn[k].release();
        ctx->d_cand[k].release();
        ctx->d_wins[k].release();
        ctx->d_wcnt[k].release();
    }
    ctx->counts_own.release();
    for (BdxFilterSet &f : ctx->fs) {
        f.bp_tables.release();
        f.seed_tables.release();
        f.seed_tables_alt.release();
        f.wave_tables.release();
        f.pair_tables.release();
    }
    ctx->d_wlist.release();
    ctx->d_tier.release();
    ctx->d_carry.release();
    ctx->d_maxlen.release();
    ctx->d_exc.release();
    ctx->d_seq.release();
    ctx->d_off.release();
    ctx->d_out_i32.release();
    ctx->d_out_f64.release();
    ctx->d_vlen.release();
    ctx->d_vlo.release();
    ctx->h_stage.release();
    ctx->h_in.release();
    ctx->h_back.release();
    if (ctx->back_events_made)
        for (hipEvent_t &e : ctx->back_events)
            if (e) (void)hipEventDestroy(e);
    ctx->back_events_made = false;
    bdx_comm_release(ctx);
    ctx->counts_sum.release();
    for (int p = 0; p < 2; ++p)
        for (int w = 0; w < 3; ++w) {
            ctx->st_tab[p][w].release();
            ctx->st_sum[p][w].release();
        }
    ctx->st_flag.release();
    for (DevBuf &b : ctx->fq) b.release();
    for (DevBuf &b : ctx->dfl) b.release();
    for (DevBuf &b : ctx->inf) b.release();
    delete ctx;
}

int32_t bdx_set_stream(bdx_ctx *ctx, void *hip_stream) {
    if (!ctx) return BDX_E_INVALID;
    const hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    if (s != ctx->stream) {
        // the scratch half the next call takes was cleared by a launch on the old stream, which the new one is not ordered
        // after: the next call clears its scratch words itself
        ctx->scratch_clean[0] = ctx->scratch_clean[1] = false;
        ctx->scratch_zeroed = false;
    }
    ctx->stream = s;
    return BDX_OK;
}

int32_t bdx_set_read_length_hint(bdx_ctx *ctx, int32_t typical_read_length) {
    if (!ctx) return BDX_E_INVALID;
    ctx->user_len_hint = typical_read_length > 0 ? typical_read_length : 0;
    return BDX_OK;
}

int32_t bdx_sync(bdx_ctx *ctx) {
    if (!ctx) return BDX_E_INVALID;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return BDX_OK;
}

// ---- one filtered classify call: plan (every size_* call), reserve (buffers, poison, scratch), enqueue ----------------
// The fused kernel filters; the exact DP runs at full width in the generic kernel:
//  * split (trimming / summary / weighted costs / N-scoring / Hamming / exact): every read's candidate mask (+ column
//    windows) goes through HBM, the generic kernel gives every verdict;
//  * known-score configs: the fused kernel also gives the verdict of (nearly) every read by replaying the reducer; the few
//    it cannot settle are listed and evaluated by the generic kernel in list mode;
//  * tiered budgets (known-score configs whose full budget is too large for selective single seeds): tier 1 — capped
//    budgets, single seeds — runs over the whole batch and settles every read whose verdict cannot depend on a barcode
//    beyond the cap; tier 0 — the full budget — then runs in list mode over the rest.
// A call runs up to five stages in this order: front, tier 1's exact launch, middle, full-budget filter, exact.

// Front stage.  Tiered: tier 1 over every read of the batch — bitpar (the fused kernel), wave / wave_win / wave_end (the wave
// kernel answers what it can settle and lists the rest), wave_split (the wave kernel as a filter: tier 1's exact launch settles
// and lists), pairs (the same-diagonal pairs mode as a filter).  Plain configs: wave, wave_win or wave_end in front of the same
// filter set in list mode.
enum class Front { none, bitpar, wave, wave_win, wave_split, wave_end, pairs };
// Middle stage: the pairs mode of the wave kernel (bdx_pairs.hip).  end: known-end / known-alignment form over tier 1's
// list; list: known-score form over it; split: tier 0's filter over it; all: the only filter, over every read.
enum class Middle { none, end, list, split, all };
enum class Full { none, wave_split, bitpar };  // the full-budget filter (none: the pairs mode already filtered)
enum class Exact { known, split, split_list };  // the generic kernel: over the fused kernel's hand-over list / dense / over a list

struct CallPlan {
    int npass = 1, tier_len = 0, batch_len = 0;  // tier_len > 0: tiered; batch_len: the read length the launches were planned for
    bool split = false, windows = false, dense_w = false;
    int short_lb[2] = {0, 0};
    Front front = Front::none;
    bool t1_exact = false;  // tier 1's exact launch
    Middle middle = Middle::none;
    Full full = Full::bitpar;
    Exact exact = Exact::known;
    bool carry = false, aln = false;  // carried passes (d_carry); the known-end forms run as the known-alignment class
    BdxWavePlan *wfront = nullptr, *wmid = nullptr;  // the wave plans the front / middle stage launch
};

static int plan_call(bdx_ctx *ctx, const BdxDevOut &o, bool stats, long long n_reads, int batch_len, int tier_len, CallPlan &p) {
    if (n_reads > 0xFFFFFFF0LL) return fail(ctx, BDX_E_INVALID, "more than 2^32 reads in one batch");
    const BdxDevCfg &dev = ctx->dev;
    BdxFilterSet &f0 = ctx->fs[0], &f1 = ctx->fs[1];
    const bool tiered = tier_len > 0;
    p.npass = dev.is_dual ? 2 : 1;
    p.tier_len = tier_len;
    p.batch_len = batch_len;
    for (int k = 0; k < p.npass; ++k) p.split |= !f0.bplan.known_ok[k];
    // (:exact returns the occurrence's start and end whatever the output policy: a caller that wants them gets the launch in
    // its split form — known-alignment class first, exact kernel for what that lists)
    if (dev.algorithm == BDX_ALG_EXACT && (o.pass_start != nullptr || o.pass_end != nullptr)) p.split = true;
    p.windows = p.split && !ctx->tune.no_windows;
    // dense window table of the plain-sweep kernel (few barcodes, many genuine candidates per read; columns fit 16 bits)
    p.dense_w = p.windows && f0.bplan.dense_d && !f0.splan.enabled && batch_len <= 60000 && !ctx->tune.no_dense;
    // restricted runs of passes that only report score (+ end) through the clean-class DP start m + kb columns before
    // the first end column (orc_selftest_clean_short_lookback); everything else keeps 2 (m + kb) + 1
    for (int k = 0; k < p.npass; ++k) {
        const int ts = dev.pass[k].trim_side;
        p.short_lb[k] = (ctx->plan.clean || ctx->plan.band_roll) && dev.algorithm == BDX_ALG_SEMIGLOBAL && !dev.need_traceback &&
                        (ts == 0 || (ts == 5 && o.pass_start == nullptr));
    }
    for (BdxFilterSet &f : ctx->fs) {
        f.bplan.short_lb[0] = p.short_lb[0];
        f.bplan.short_lb[1] = p.short_lb[1];
        f.bplan.n_cu = ctx->n_cu;
    }
    // Wave-autonomous kernel (bdx_wave.hip) in front of the general one: it answers the reads of the known-score
    // class and lists the rest — as tier 1 of a tiered config, or (plain configs) ahead of the same filter set
    // in list mode.  The list-mode plan is made first: if it cannot be made, the general kernel runs alone.
    // (window mode first: reads much longer than their column window — only the windows are fetched)
    if (!p.split && !dev.vlen) {
        BdxWavePlan &wp = tiered ? f1.wplan : f0.wplan;
        if ((size_wave_win(ctx, wp, batch_len, n_reads) || size_wave(ctx, wp, batch_len, n_reads)) &&
            (tiered || size_bitpar(ctx, 0, batch_len, n_reads, true))) {
            p.front = wp.winm ? Front::wave_win : Front::wave;
            p.wfront = &wp;
        }
        if (!tiered && p.front == Front::none) (void)size_bitpar(ctx, 0, batch_len, n_reads);  // (restore the dense plan)
    }
    // Known-end class (trim_side = 5, single pass, no start positions or statistics wanted): the same kernel in its
    // known-end form answers the reads it can settle, trimmed keep range included; the listed rest goes through the
    // split path (filter in list mode -> exact kernel in list mode).
    bool trim3 = false;  // (a trim_side = 3 pass of the known-trim class knows its start only)
    for (int k = 0; k < p.npass; ++k) trim3 |= dev.pass[k].trim_side == 3;
    const bool kend_ok = p.split && p.windows && !dev.vlen && !p.dense_w && o.pass_start == nullptr && !stats && !(trim3 && o.pass_end != nullptr);
    // known-alignment class: the caller wants positions the known-trim class does not know, or the statistics tables
    p.aln = p.split && p.windows && !dev.vlen && !p.dense_w && !kend_ok && ctx->fs[tiered ? 1 : 0].wplan_a.enabled;
    if (kend_ok || p.aln) {
        BdxWavePlan &wk = tiered ? (p.aln ? f1.wplan_a : f1.wplan_k) : (p.aln ? f0.wplan_a : f0.wplan_k);
        if (size_wave(ctx, wk, batch_len, n_reads)) {
            if (tiered || size_bitpar(ctx, 0, batch_len, n_reads, true)) {
                p.front = Front::wave_end;
                p.wfront = &wk;
            } else {
                (void)size_bitpar(ctx, 0, batch_len, n_reads);  // (restore the dense plan)
            }
        }
    }
    // split configs (trimming, summary, weighted costs): the wave kernel as the FILTER of a dense launch — candidate
    // masks and column windows in the formats of the general kernel's split mode, every verdict from the exact
    // kernel as before.  Tiered: tier 1 (all reads); plain: the only filter launch.
    bool wsplit0 = false;
    if (p.split && p.windows && !dev.vlen && p.front == Front::none) {
        if (tiered && f1.wplan.split && size_wave(ctx, 1, batch_len, n_reads)) p.front = Front::wave_split;
        if (!tiered) wsplit0 = f0.wplan.split && !p.dense_w && size_wave(ctx, 0, batch_len, n_reads);
    }
    // the pairs tier: tier 1's filter is the same-diagonal pairs mode over every read of the batch
    if (tiered && p.front != Front::wave_end && ctx->pairs_tier && p.split && p.windows && !p.dense_w && !dev.vlen &&
        size_pairs(ctx, f1.pplan, batch_len))
        p.front = Front::pairs;
    if (tiered && p.front == Front::none) p.front = Front::bitpar;
    p.t1_exact = tiered && p.split && p.front != Front::wave_end;
    // Carried passes: tier 1 of a dual known-class config lists a read when ONE of its passes is open; the pass it settled goes
    // along (two state bits on the list entry + the pass's winning survivor in d_carry[read]) and the pairs mode only looks for
    // the other pass's barcodes — about half of its sweeps for C4.  Only when the pairs mode in its known form is what reads
    // tier 1's list (nothing else understands the state bits), reads fit 30 bits and min_delta = 0 (a lone carried winner
    // then IS the pass's result).
    // (the known-trim / known-alignment forms and the plain known-score form of a dual config without trimming)
    if (tiered && (p.front == Front::wave_end || p.front == Front::wave) && dev.is_dual && dev.min_delta == 0.0 && !ctx->tune.no_carry &&
        n_reads < (1LL << 30) && o.pass_start == nullptr && o.pass_end == nullptr && o.pass_raw == nullptr && o.pass_bc == nullptr &&
        o.pass_score == nullptr && o.pass_delta == nullptr) {
        BdxWavePlan &pp = p.front == Front::wave_end ? (p.aln ? f0.pplan_a : f0.pplan_k) : f0.pplan;
        p.carry = size_pairs(ctx, pp, tier_len) && pp.groups <= 1 && pp.pairs_kb <= 4 && !pp.split;
    }
    if (tiered) {
        // tier 0 walks the list: scattered reads -> slot staging
        // (tier 0 sees a fraction of the batch — 10..25 % in the bench configs: its tile size is planned for a sixteenth of
        // the batch, so that the list of a small batch still spreads over the device — C5, 400 k reads: tiles of 16 instead
        // of 128 reads, 0.42 -> 0.38 ms; batches of millions of reads keep their tiles)
        long long n_list_est = n_reads / (ctx->tune.tier0_div > 0 ? ctx->tune.tier0_div : 16);
        if (n_list_est < 1) n_list_est = 1;
        if (!size_bitpar(ctx, 0, tier_len, n_list_est, true)) return fail(ctx, BDX_E_DEVICE, "internal: tier 0 cannot be planned in list mode");
    }
    // Pairs mode of the wave kernel between tier 1 and the general kernel: the listed reads are gathered into slots and
    // filtered at the full budgets by the two-intact-pieces lemma.  Known-score configs: it answers them (what it cannot
    // answer goes on to the general kernel in list mode); split configs: it is tier 0's filter (masks + windows of the
    // listed reads for the exact kernel).  Known-end class: the pairs mode answers the listed reads itself (verdict +
    // trimmed keep range); what it cannot answer goes on to the split path in list mode.
    // Same-diagonal pairs mode as the ONLY filter of a split config without tiers (weighted costs whose full budget is beyond
    // every seeded variant — the reference's demo2 options): every read of the batch is laid out in slots and scanned;
    // masks + windows of all reads go to the exact kernel's dense launch.
    BdxWavePlan &pk = p.aln ? f0.pplan_a : f0.pplan_k;
    p.wmid = &f0.pplan;
    if (tiered && (kend_ok || p.aln) && size_pairs(ctx, pk, tier_len)) {
        p.middle = Middle::end;
        p.wmid = &pk;
    } else if (tiered && (!p.split || p.windows) && !p.dense_w && size_pairs(ctx, tier_len)) {
        p.middle = p.split ? Middle::split : Middle::list;
    } else if (!tiered && p.split && p.windows && !p.dense_w && !wsplit0 && p.front != Front::wave_end && !dev.vlen && f0.pplan.enabled &&
               f0.pplan.pairs_kb >= 8 && f0.pplan.split && size_pairs(ctx, batch_len)) {
        p.middle = Middle::all;
    }
    p.full = (p.middle == Middle::split || p.middle == Middle::all) ? Full::none : wsplit0 ? Full::wave_split : Full::bitpar;
    p.exact = !p.split ? Exact::known : p.front != Front::none ? Exact::split_list : Exact::split;
    return BDX_OK;
}

// Buffers of the plan's hand-overs, the test switch's fills, this call's half of the scratch block and the per-launch
// fields of the plans.
static int reserve(bdx_ctx *ctx, const CallPlan &p, long long n_reads) {
    const bool tiered = p.tier_len > 0;
    const size_t list_bytes = (size_t)n_reads * 4 + 64;
    for (int k = 0; k < p.npass; ++k) {
        HIP_TRY(ctx, ctx->d_cand[k].ensure((size_t)n_reads * ctx->dev.pass[k].cand_words * 4 + 64));
        if (p.windows) {
            size_t per_read = (size_t)BDX_WCAP * 3;
            if (p.dense_w && (size_t)ctx->dev.pass[k].n_barcodes > per_read) per_read = (size_t)ctx->dev.pass[k].n_barcodes;
            HIP_TRY(ctx, ctx->d_wins[k].ensure((size_t)n_reads * per_read * 4 + 64));
            HIP_TRY(ctx, ctx->d_wcnt[k].ensure((size_t)n_reads + 64));
        }
    }
    if (!p.split) HIP_TRY(ctx, ctx->d_exc.ensure(list_bytes));
    if (tiered) HIP_TRY(ctx, ctx->d_tier.ensure(list_bytes));
    if ((!tiered && p.front != Front::none) || p.middle == Middle::end || p.middle == Middle::list) HIP_TRY(ctx, ctx->d_wlist.ensure(list_bytes));
    for (BdxFilterSet &f : ctx->fs)
        f.wplan.d_carry = f.pplan.d_carry = f.wplan_k.d_carry = f.wplan_a.d_carry = f.pplan_k.d_carry = f.pplan_a.d_carry = nullptr;
    if (p.carry) {
        HIP_TRY(ctx, ctx->d_carry.ensure(list_bytes));
        p.wfront->d_carry = p.wmid->d_carry = (uint32_t *)ctx->d_carry.p;
    }
    if (ctx->tune.poison) {
        // test switch: whatever a consumer reads without a producer having written it is garbage on EVERY run
        // every hand-over buffer is filled with 0xA5; between each producer and its consumer a checker kernel
        // (bdx_poison_check_kernel) then looks at exactly the elements the consumer is going to read — an element that
        // still holds the fill was never written: counted (bdx_rejected_windows) and made harmless
        DevBuf *bufs[] = {&ctx->d_cand[0], &ctx->d_cand[1], &ctx->d_wins[0], &ctx->d_wins[1], &ctx->d_wcnt[0], &ctx->d_wcnt[1],
                          &ctx->d_exc, &ctx->d_tier, &ctx->d_wlist, &ctx->d_carry};
        for (DevBuf *b : bufs)
            if (b->p) HIP_TRY(ctx, hipMemsetAsync(b->p, 0xA5, b->cap, ctx->stream));
    }
    // scratch words (d_maxlen, 1 KiB): +64 tile queue, +128 hand-over count (+132.. tuning statistics),
    // +192 tier-0 list length, +256 tile queue of the second launch, +320 the pairs mode's list length; one memset clears them all
    // (the block's two halves alternate between calls: this call's last launch clears the other half for the next call,
    // which then needs no memset of its own — 5 us of fill + a launch gap per call, 1 % of a 10 M-read C2 step)
    const int spar = ctx->scratch_par & 1;
    char *scratch = (char *)ctx->d_maxlen.p + 512 * spar;
    if (!ctx->scratch_zeroed && !ctx->scratch_clean[spar]) HIP_TRY(ctx, hipMemsetAsync(scratch + 64, 0, 4 * BDX_SCRATCH_WORDS, ctx->stream));
    ctx->scratch_zeroed = false;
    ctx->scratch_clean[spar] = false;  // (a call that fails half-way leaves it that way: the next one clears it itself)
    for (int set = tiered ? 1 : 0; set >= 0; --set) {
        BdxBitparPlan &b = ctx->fs[set].bplan;
        b.d_tile_counter = (int *)(scratch + (set ? 256 : 64));
        b.dense_w = set ? 0 : p.dense_w;
        b.grid_override = ctx->tune.grid;
        b.dbg = ctx->tune.debug;
    }
    return BDX_OK;
}

static int enqueue(bdx_ctx *ctx, const CallPlan &p, const uint8_t *seq, const long long *off, long long n_reads, const BdxDevOut &o,
                   const BdxDevStats *stp) {
    const BdxFilterSet &f0 = ctx->fs[0], &f1 = ctx->fs[1];
    const bool tiered = p.tier_len > 0, two = p.npass > 1;
    const int spar = ctx->scratch_par & 1;
    char *scratch = (char *)ctx->d_maxlen.p + 512 * spar;
    uint32_t *zero_next = (uint32_t *)((char *)ctx->d_maxlen.p + 512 * (1 - spar) + 64);
    uint32_t *c0 = (uint32_t *)ctx->d_cand[0].p, *c1 = two ? (uint32_t *)ctx->d_cand[1].p : c0;
    uint32_t *w0 = p.windows ? (uint32_t *)ctx->d_wins[0].p : nullptr, *w1 = p.windows && two ? (uint32_t *)ctx->d_wins[1].p : w0;
    uint8_t *n0 = p.windows ? (uint8_t *)ctx->d_wcnt[0].p : nullptr, *n1 = p.windows && two ? (uint8_t *)ctx->d_wcnt[1].p : n0;
    uint32_t *exc_list = p.split ? nullptr : (uint32_t *)ctx->d_exc.p;
    unsigned int *exc_count = (unsigned int *)(scratch + 128);
    // what the front stage cannot settle: tier 1 lists into d_tier, a plain front stage into d_wlist; the pairs mode into d_wlist
    uint32_t *front_list = (uint32_t *)(tiered ? ctx->d_tier.p : ctx->d_wlist.p), *mid_list = (uint32_t *)ctx->d_wlist.p;
    unsigned int *front_count = (unsigned int *)(scratch + 192), *mid_count = (unsigned int *)(scratch + 320);
    const double *slo = f1.bplan.tier_slo;
    BdxWaveSplit wsp{};
    for (int k = 0; k < 2; ++k) {
        wsp.cw[k] = k < p.npass ? ctx->dev.pass[k].cand_words : 0;
        wsp.cand_out[k] = k ? c1 : c0;
        wsp.wins_out[k] = k ? w1 : w0;
        wsp.wcnt_out[k] = k ? n1 : n0;
        wsp.short_lb[k] = p.short_lb[k];
    }
    // diagonal-band DP of the exact kernel (sg_core_band): clean class, every barcode of the config with the same
    // number of rows and of the pass with the same budget, column windows handed over by tracked sweeps
    const auto band_cfg = [&](const BdxFilterSet &f) {
        BdxDevCfg dv = ctx->dev;
        dv.dense_w = (&f == &ctx->fs[0]) && p.dense_w;
        for (int k = 0; k < p.npass; ++k) {
            const int kb = f.bplan.kb_uniform[k];
            // (rolling band, barcodes beyond 32 rows: any uniform budget; the first end column is rebuilt from the hand-over row
            // when every barcode has the same length — band_lb is made of max_m)
            const bool on = ctx->plan.band_roll ? (p.windows && ctx->plan.same_len && kb >= 0)
                                                : (p.windows && ctx->plan.clean && ctx->plan.uniform_len > 0 && !ctx->tune.no_band &&
                                                   ctx->dev.algorithm == BDX_ALG_SEMIGLOBAL && kb >= 0 && kb <= 4);
            dv.band_m = ctx->plan.uniform_len;
            dv.band_kb[k] = on ? kb : -1;
            if (on && !ctx->plan.band_roll) ctx->band_launches += 1;
            dv.band_lb[k] = p.short_lb[k] ? ctx->dev.max_m + kb : 2 * (ctx->dev.max_m + kb) + 1;
        }
        return dv;
    };
    // test switch BDX_POISON: between a producer and its consumer, every element the consumer will read must have
    // been written (bdx_poison_check_kernel); `with_windows`: also the window hand-over of both passes for these reads
    const auto poison_check = [&](const uint32_t *list, const unsigned int *count, bool check_list, bool with_windows, bool packed = false) -> hipError_t {
        if (!ctx->tune.poison) return hipSuccess;
        unsigned int *dbg = (unsigned int *)ctx->d_dbg.p;
        uint32_t *l = (uint32_t *)list;
        if (!with_windows || !p.windows)
            return l ? bdx_launch_poison_check(l, count, n_reads, nullptr, nullptr, nullptr, 0, 0, (check_list ? 1 : 0) | (packed ? 2 : 0), dbg, ctx->stream) : hipSuccess;
        for (int k = 0; k < p.npass; ++k) {
            hipError_t e = bdx_launch_poison_check(l, count, n_reads, k ? w1 : w0, k ? n1 : n0, k ? c1 : c0, ctx->dev.pass[k].cand_words,
                                                   ctx->dev.pass[k].n_barcodes, (check_list && k == 0) ? 1 : 0, dbg, ctx->stream);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };
    // one launcher per kernel family; `filter`: the split form (masks + windows into wsp, no verdicts, no list)
    const auto counted = [](hipError_t e, int64_t &launches) { if (e == hipSuccess) launches += 1; return e; };
    const int he = ctx->plan.hist_entries, dbg = ctx->tune.debug;
    const auto bitpar = [&](const BdxFilterSet &f, const BdxTierArgs *t) {
        return bdx_launch_bitpar(ctx->dev, ctx->plan, f.bplan, f.splan, seq, off, n_reads, o, ctx->counts, c0, c1, ctx->stream, w0, w1, n0, n1,
                                 p.split ? 1 : 0, exc_list, exc_count, t);
    };
    const auto wave = [&](const BdxWavePlan &wp, int tier1, bool filter) {
        return counted(bdx_launch_wave(ctx->dev, wp, he, seq, off, n_reads, o, filter ? nullptr : ctx->counts, tier1,
                                       tier1 ? slo[0] : 0.0, filter ? nullptr : front_list, filter ? nullptr : front_count, ctx->stream, dbg,
                                       filter ? &wsp : nullptr, tier1 ? slo[1] : 0.0),
                       ctx->wave_launches);
    };
    const auto wave_win = [&](const BdxWavePlan &wp, int tier1) {
        return counted(bdx_launch_wave_win(ctx->dev, wp, he, seq, off, n_reads, o, ctx->counts, tier1, tier1 ? slo[0] : 0.0, front_list,
                                           front_count, ctx->stream, dbg),
                       ctx->wave_launches);
    };
    const auto wave_end = [&](const BdxWavePlan &wp, int tier1) {
        return counted(bdx_launch_wave_end(ctx->dev, wp, he, seq, off, n_reads, o, ctx->counts, tier1, tier1 ? slo[0] : 0.0, front_list,
                                           front_count, ctx->stream, dbg, tier1 ? slo[1] : 0.0, p.aln ? stp : nullptr),
                       ctx->wave_launches);
    };
    const auto pairs = [&](const BdxWavePlan &wp, const uint32_t *in_list, const unsigned int *in_count, bool filter, const BdxDevStats *st) {
        return counted(bdx_launch_pairs(ctx->dev, wp, he, seq, off, n_reads, in_list, in_count, o, filter ? nullptr : ctx->counts,
                                        filter ? nullptr : mid_list, filter ? nullptr : mid_count, ctx->stream, dbg >> 8, filter ? &wsp : nullptr, st),
                       ctx->pair_launches);
    };
    const auto generic = [&](const BdxDevCfg &dv, const uint32_t *list, const unsigned int *count, const BdxTierArgs *t, const double *t_slo,
                             uint32_t *zero) {
        return bdx_launch_generic(dv, ctx->plan, seq, off, n_reads, o, ctx->counts, c0, two ? c1 : nullptr, ctx->stream, w0, two ? w1 : nullptr, n0,
                                  two ? n1 : nullptr, list, count, stp, t, t_slo, zero);
    };

    BdxTierArgs t1{1, (uint32_t *)ctx->d_tier.p, front_count, nullptr, nullptr};
    BdxTierArgs t0{0, nullptr, nullptr, nullptr, nullptr};
    // 1. front stage
    switch (p.front) {
        case Front::none: break;
        case Front::bitpar: HIP_TRY(ctx, bitpar(f1, &t1)); break;
        case Front::wave: HIP_TRY(ctx, wave(*p.wfront, tiered, false)); break;
        case Front::wave_win: HIP_TRY(ctx, wave_win(*p.wfront, tiered)); break;
        case Front::wave_split: HIP_TRY(ctx, wave(f1.wplan, 0, true)); break;  // (the exact kernel settles and lists)
        case Front::wave_end: HIP_TRY(ctx, wave_end(*p.wfront, tiered)); break;  // verdicts + trimmed keep range of what it settles
        case Front::pairs: HIP_TRY(ctx, pairs(f1.pplan, nullptr, nullptr, true, nullptr)); break;
    }
    // 2. tier 1's exact launch: it answers what tier 1 settles and lists the rest (known-score / known-end configs: the filter kernel did)
    if (p.t1_exact) {
        HIP_TRY(ctx, poison_check(nullptr, nullptr, false, true));
        HIP_TRY(ctx, generic(band_cfg(f1), nullptr, nullptr, &t1, f1.bplan.tier_slo, nullptr));
    }
    if (p.front != Front::none) {  // tier 0 / the plain front stage's filter set walks the list
        t0.in_list = front_list;
        t0.in_count = front_count;
        HIP_TRY(ctx, poison_check(t0.in_list, t0.in_count, true, false, p.carry));
    }
    // 3. middle stage
    switch (p.middle) {
        case Middle::none: break;
        case Middle::end: HIP_TRY(ctx, pairs(*p.wmid, t0.in_list, t0.in_count, false, p.aln ? stp : nullptr)); break;
        case Middle::list: HIP_TRY(ctx, pairs(*p.wmid, t0.in_list, t0.in_count, false, nullptr)); break;
        case Middle::split: HIP_TRY(ctx, pairs(*p.wmid, t0.in_list, t0.in_count, true, nullptr)); break;
        case Middle::all: HIP_TRY(ctx, pairs(*p.wmid, nullptr, nullptr, true, nullptr)); break;
    }
    if (p.middle == Middle::end || p.middle == Middle::list) {  // what the pairs mode cannot answer goes on in list mode
        t0.in_list = mid_list;
        t0.in_count = mid_count;
        HIP_TRY(ctx, poison_check(mid_list, mid_count, true, false));
    }
    // 4. full-budget filter
    switch (p.full) {
        case Full::none: break;  // (the pairs mode already wrote the masks and windows)
        case Full::wave_split: HIP_TRY(ctx, wave(f0.wplan, 0, true)); break;
        case Full::bitpar: HIP_TRY(ctx, bitpar(f0, p.front != Front::none ? &t0 : nullptr)); break;
    }
    // 5. exact stage (its last launch clears the other scratch half for the next call)
    switch (p.exact) {
        case Exact::known:
            HIP_TRY(ctx, poison_check(exc_list, exc_count, true, false));
            HIP_TRY(ctx, generic(ctx->dev, exc_list, exc_count, nullptr, nullptr, zero_next));
            break;
        case Exact::split:
            HIP_TRY(ctx, poison_check(nullptr, nullptr, false, true));
            HIP_TRY(ctx, generic(band_cfg(f0), nullptr, nullptr, nullptr, nullptr, zero_next));
            break;
        case Exact::split_list:  // (tiered: list mode over the reads tier 1 handed on)
            HIP_TRY(ctx, poison_check(t0.in_list, t0.in_count, false, true));
            HIP_TRY(ctx, generic(band_cfg(f0), t0.in_list, t0.in_count, nullptr, nullptr, zero_next));
            break;
    }
    // (the call's last launch is enqueued: the other half will hold zeros when the next call's kernels start)
    ctx->scratch_clean[1 - spar] = true;
    ctx->scratch_par = 1 - spar;
#ifdef BDX_TUNING
    if (ctx->tune.debug & 128) {  // tuning statistics of the fused kernel (see bdx_bitpar.hip)
            unsigned int st[4] = {0, 0, 0, 0}, tl = 0;
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, hipMemcpy(st, exc_count, sizeof(st), hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(&tl, scratch + 192, sizeof(tl), hipMemcpyDeviceToHost));
            fprintf(stderr, "[bdx] handed over %u reads; %u windowed sweeps, %u columns, %u tiles with a fallback read; tier 0 list %u (of %lld reads)\n",
                    st[0], st[1], st[2], st[3], tl, (long long)n_reads);
    }
#endif
    return BDX_OK;
}

// ctx->path of a filtered call: its stages, front first
static std::string call_path(const bdx_ctx *ctx, const CallPlan &p) {
    const BdxSeedPlan &sp = ctx->fs[0].splan;
    std::string s = sp.enabled ? (sp.diag ? "qgram2+bitpar+verify" : "qgram+bitpar+verify") : "bitpar+verify";
    if (p.full == Full::wave_split) s = "wave+verify";
    switch (p.middle) {
        case Middle::none: break;
        case Middle::end: s = (p.aln ? "pairs(aln) > " : "pairs(end) > ") + s; break;
        case Middle::list: s = "pairs > " + s; break;
        case Middle::split: s = "pairs+verify"; break;
        case Middle::all: s = "pairs(diag)+verify"; break;
    }
    static const char *const front[] = {"", "qgram+bitpar", "wave", "wave(win)", "wave", "wave(end)", "pairs(diag)"};
    if (p.front == Front::none) return s;
    return std::string(p.tier_len > 0 ? "tier1:" : "") + (p.front == Front::wave_end && p.aln ? "wave(aln)" : front[(int)p.front]) + " > " + s;
}

int32_t bdx_classify_device(bdx_ctx *ctx, const uint8_t *d_seq_bytes, const int64_t *d_seq_off, int64_t n_reads,
                            const bdx_outputs_t *d_out) {
    if (!ctx) return BDX_E_INVALID;
    if (!ctx->log_host_call) ctx->launch_log.clear();
    if (n_reads < 0) return fail(ctx, BDX_E_INVALID, "n_reads is negative");
    if (n_reads == 0) return BDX_OK;
    if (!d_seq_bytes || !d_seq_off || !d_out) return fail(ctx, BDX_E_INVALID, "NULL device pointer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the launchers note what they enqueue into this call's log (test visibility: bdx_last_launches)
    struct LogScope {
        std::string *prev;
        explicit LogScope(std::string *log) : prev(t_launch_log) { t_launch_log = log; }
        ~LogScope() { t_launch_log = prev; }
    } log_scope(&ctx->launch_log);
    const BdxDevOut o{d_out->bc1,      d_out->bc2,      d_out->keep_start, d_out->keep_end,   d_out->pass_start,
                      d_out->pass_end, d_out->pass_raw, d_out->pass_bc,    d_out->pass_score, d_out->pass_delta};
    BdxDevStats st{};
    const BdxDevStats *stp = nullptr;
    int measured_len = -1;
    if (ctx->virt_maxlen > 0) {
        measured_len = ctx->virt_maxlen;  // window upload: the host has seen every length
    } else if (ctx->host_maxlen > 0) {
        measured_len = ctx->host_maxlen;  // host entry point: the offsets were on the host anyway
    } else if (ctx->dev.need_traceback) {
        // statistics tables are sized from the batch's true maximum read length (a hint is only a hint)
        HIP_TRY(ctx, ctx->d_maxlen.ensure(1024));
        HIP_TRY(ctx, bdx_launch_maxlen((const long long *)d_seq_off, n_reads, (int *)ctx->d_maxlen.p, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&measured_len, ctx->d_maxlen.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (ctx->dev.need_traceback) {
        int rc = bdx_stats_reserve(ctx, (long long)measured_len + ctx->dev.max_m + 2);
        if (rc != BDX_OK) return rc;
        for (int p = 0; p < 2; ++p) {
            st.pos[p] = (unsigned long long *)ctx->st_tab[p][0].p;
            st.len[p] = (unsigned long long *)ctx->st_tab[p][1].p;
            st.raw[p] = (unsigned long long *)ctx->st_tab[p][2].p;
        }
        st.rows = ctx->st_rows;
        st.raw_rows = ctx->st_raw_rows;
        st.len_rows = ctx->st_len_rows;
        st.len_stride = bdx_stats_stride(ctx, 1);
        st.raw_stride = bdx_stats_stride(ctx, 2);
        st.pos_bias = ctx->dev.max_m;
        st.overflow = (unsigned int *)ctx->st_flag.p;
        stp = &st;
    }
    bool filtered = false;
    int tier_len = 0;  // > 0: tiered budgets apply to this batch (the read length both tiers were planned for)
    int batch_len = 0;  // the read length the filtered launches were planned for
    if (ctx->fs[0].bplan.enabled) {
        int len = ctx->virt_maxlen > 0 ? ctx->virt_maxlen : ctx->user_len_hint;
        if (len <= 0 && measured_len >= 0) len = measured_len > 0 ? measured_len : 1;
        if (len <= 0) {  // measure the batch: one tiny kernel + a 4-byte copy
            int host_len = 0;
            HIP_TRY(ctx, bdx_launch_maxlen((const long long *)d_seq_off, n_reads, (int *)ctx->d_maxlen.p, ctx->stream));
            HIP_TRY(ctx, hipMemcpyAsync(&host_len, ctx->d_maxlen.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            len = host_len;
        }
        batch_len = len;
        filtered = size_bitpar(ctx, 0, len, n_reads);
        // both tiers must be plannable for this batch, else the full budget alone
        if (filtered && ctx->tiered && size_bitpar(ctx, 1, len, n_reads)) tier_len = len;
    }
    if (filtered) {
        CallPlan p;
        int rc = plan_call(ctx, o, stp != nullptr, n_reads, batch_len, tier_len, p);
        if (rc == BDX_OK) rc = reserve(ctx, p, n_reads);
        if (rc == BDX_OK) rc = enqueue(ctx, p, d_seq_bytes, (const long long *)d_seq_off, n_reads, o, stp);
        if (rc != BDX_OK) return rc;
        ctx->last_blocks = (n_reads + ctx->fs[0].bplan.reads_per_block - 1) / ctx->fs[0].bplan.reads_per_block;
        ctx->path = call_path(ctx, p);
        ctx->filter_used = ctx->fs[0].splan.enabled ? BDX_FILTER_QGRAM : BDX_FILTER_BITPAR;
    } else {
        HIP_TRY(ctx, bdx_launch_generic(ctx->dev, ctx->plan, d_seq_bytes, (const long long *)d_seq_off, n_reads, o,
                                        ctx->counts, nullptr, nullptr, ctx->stream, nullptr, nullptr, nullptr, nullptr, nullptr,
                                        nullptr, stp));
        ctx->last_blocks = (n_reads + ctx->plan.threads - 1) / ctx->plan.threads;
        ctx->path = "generic";
        ctx->filter_used = BDX_FILTER_OFF;
    }
    ctx->launches += 1;
    return BDX_OK;
}

int64_t bdx_counts_len(const bdx_ctx *ctx) { return ctx ? ctx->dev.n_counts : 0; }

int32_t bdx_get_counts(bdx_ctx *ctx, int64_t *out, int64_t n) {
    if (!ctx || !out) return BDX_E_INVALID;
    if (n < ctx->dev.n_counts) return fail(ctx, BDX_E_INVALID, "counts buffer too small: need %d", ctx->dev.n_counts);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->counts, (size_t)ctx->dev.n_counts * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return BDX_OK;
}

int32_t bdx_reset_counts(bdx_ctx *ctx) {
    if (!ctx) return BDX_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(ctx->counts, 0, (size_t)ctx->dev.n_counts * 8, ctx->stream));
    if (ctx->dev.need_traceback)
        for (int p = 0; p < (ctx->dev.is_dual ? 2 : 1); ++p)
            for (int w = 0; w < 3; ++w)
                if (ctx->st_tab[p][w].p)
                    HIP_TRY(ctx, hipMemsetAsync(ctx->st_tab[p][w].p, 0, bdx_stats_phys_words(ctx, p, w, ctx->st_rows) * 8, ctx->stream));
    return BDX_OK;
}

int32_t bdx_stats_shape(const bdx_ctx *ctx, int32_t pass, int32_t which, int64_t *rows, int64_t *key0, int64_t *n_barcodes) {
    if (!ctx) return BDX_E_INVALID;
    if (pass < 0 || pass > 1 || which < BDX_STATS_POS || which > BDX_STATS_RAW) return BDX_E_INVALID;
    const bool on = ctx->dev.need_traceback && (pass == 0 || ctx->dev.is_dual);
    if (rows) *rows = !on ? 0 : (which == BDX_STATS_RAW ? ctx->st_raw_rows : which == BDX_STATS_LEN ? ctx->st_len_rows : ctx->st_rows);
    if (key0) *key0 = which == BDX_STATS_POS ? 1 - (int64_t)ctx->dev.max_m : 0;
    if (n_barcodes) *n_barcodes = on ? ctx->dev.pass[pass].n_barcodes : 0;
    return BDX_OK;
}

int32_t bdx_get_stats(bdx_ctx *ctx, int32_t pass, int32_t which, int32_t reduced, int64_t *out, int64_t n_words) {
    if (!ctx || !out) return BDX_E_INVALID;
    if (pass < 0 || pass > 1 || which < BDX_STATS_POS || which > BDX_STATS_RAW) return fail(ctx, BDX_E_INVALID, "bad statistics table selector");
    if (!ctx->dev.need_traceback || (pass == 1 && !ctx->dev.is_dual)) return fail(ctx, BDX_E_STATE, "the config collects no statistics for this pass (need_traceback = 0)");
    // the shape handed out is the CURRENT one (bdx_stats_shape); the summed twins were filled at the shape of the last
    // all-reduce — fewer pos rows, and for a growing length table fewer keys at a smaller pitch: rows / keys appended
    // since then read as zero
    const size_t B = (size_t)ctx->dev.pass[pass].n_barcodes;
    const size_t words = bdx_stats_words(ctx, pass, which, ctx->st_rows);
    if ((size_t)n_words < words) return fail(ctx, BDX_E_INVALID, "statistics buffer too small: need %zu words", words);
    const DevBuf &src = reduced ? ctx->st_sum[pass][which] : ctx->st_tab[pass][which];
    if (reduced && !src.p) return fail(ctx, BDX_E_STATE, "bdx_allreduce_counts has not been called");
    const long long pos_rows = reduced ? ctx->st_sum_rows : ctx->st_rows;
    const size_t keys_now = which == BDX_STATS_RAW ? (size_t)ctx->st_raw_rows : (size_t)ctx->st_len_rows;
    const size_t keys_src = which == BDX_STATS_LEN && reduced ? (size_t)ctx->st_sum_len_rows : keys_now;
    const size_t stride_src = (keys_src + 15) & ~(size_t)15;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned int flag = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&flag, ctx->st_flag.p, sizeof flag, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<int64_t> phys;  // len / raw: [barcode][key stride] on the device
    if (which == BDX_STATS_POS) {
        const size_t have = (size_t)pos_rows * B;
        if (have) HIP_TRY(ctx, hipMemcpyAsync(out, src.p, have * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (words > have) memset(out + have, 0, (words - have) * 8);
    } else {
        phys.resize(stride_src * B);
        if (!phys.empty()) HIP_TRY(ctx, hipMemcpyAsync(phys.data(), src.p, phys.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (flag) return fail(ctx, BDX_E_STATE, "a statistics key fell outside its table (internal sizing error)");
    if (which != BDX_STATS_POS) {
        for (size_t k = 0; k < keys_now; ++k)
            for (size_t b = 0; b < B; ++b) out[k * B + b] = k < keys_src ? phys[b * stride_src + k] : 0;
    }
    return BDX_OK;
}

void *bdx_counts_device_ptr(bdx_ctx *ctx) { return ctx ? (void *)ctx->counts : nullptr; }

int32_t bdx_set_counts_buffer(bdx_ctx *ctx, void *d_counts) {
    if (!ctx) return BDX_E_INVALID;
    ctx->counts = d_counts ? (unsigned long long *)d_counts : (unsigned long long *)ctx->counts_own.p;
    return BDX_OK;
}

const char *bdx_kernel_path(const bdx_ctx *ctx) { return ctx ? ctx->path.c_str() : ""; }

int64_t bdx_window_uploads(const bdx_ctx *ctx) { return ctx ? ctx->window_uploads : 0; }

int64_t bdx_band_launches(const bdx_ctx *ctx) { return ctx ? ctx->band_launches : 0; }

int64_t bdx_wave_launches(const bdx_ctx *ctx) { return ctx ? ctx->wave_launches : 0; }
int64_t bdx_pair_launches(const bdx_ctx *ctx) { return ctx ? ctx->pair_launches : 0; }

int64_t bdx_pipelined_calls(const bdx_ctx *ctx) { return ctx ? ctx->pipelined_calls : 0; }
int64_t bdx_staged_downloads(const bdx_ctx *ctx) { return ctx ? ctx->staged_downloads : 0; }
int64_t bdx_last_list_reads(bdx_ctx *ctx) {
    if (!ctx || !ctx->d_maxlen.p) return 0;
    if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return -1;
    unsigned int v = 0;
    // (the scratch half of the LAST call: the halves alternate, the last launch of a call clears the other one)
    const char *last = (const char *)ctx->d_maxlen.p + 512 * (1 - (ctx->scratch_par & 1)) + 192;
    if (hipMemcpy(&v, last, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)v;
}

int64_t bdx_rejected_windows(bdx_ctx *ctx) {
    if (!ctx || !ctx->d_dbg.p) return 0;
    unsigned int rej[2] = {0, 0};  // [0] refused by the exact kernel, [1] found unwritten by the poison checker
    if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
        hipMemcpy(rej, ctx->d_dbg.p, sizeof rej, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    return (int64_t)rej[0] + (int64_t)rej[1];
}

int64_t bdx_debug_rejected_windows_total(void) { return (int64_t)g_rejected_windows.load(); }

int64_t bdx_last_launches(const bdx_ctx *ctx, char *buf, int64_t cap) {
    const std::string empty;
    const std::string &log = ctx ? ctx->launch_log : empty;
    if (buf && cap > 0) {
        const size_t n = std::min((size_t)(cap - 1), log.size());
        memcpy(buf, log.data(), n);
        buf[n] = '\0';
    }
    return (int64_t)log.size();
}

int32_t bdx_launch_info(const bdx_ctx *ctx, bdx_launch_info_t *out) {
    if (!ctx || !out) return BDX_E_INVALID;
    const bool f = ctx->filter_used != BDX_FILTER_OFF && ctx->F().bplan.reads_per_block > 0;
    out->threads_per_block = f ? 256 : ctx->plan.threads;
    out->lds_bytes_per_block = f ? (int32_t)bdx_bitpar_lds_bytes(ctx->dev, ctx->F().bplan, ctx->plan, &ctx->F().splan) : (int32_t)ctx->plan.lds_bytes;
    out->blocks = ctx->last_blocks;
    out->reads_per_block = f ? ctx->F().bplan.reads_per_block : ctx->plan.threads;
    out->filter_used = ctx->filter_used;
    out->max_m = ctx->dev.max_m;
    out->launches = ctx->launches;
    return BDX_OK;
}

}  // extern "C"
