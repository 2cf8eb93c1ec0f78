// bdx_abi.cpp — C-ABI of libbiodemux_hip.so (see include/biodemux_hip.h for the contract and
// the reference lines each entry point replaces).  Host-side only: validation, upload of what the create-time planner
// (bdx_plan.cpp) produced, reserve and enqueue of what the per-call planner (bdx_call.cpp) decided — bdx_classify_batch, which both entry points end in (the host entry point, bdx_classify_host, is bdx_host.cpp).  All arithmetic of the hot path runs in the gfx950
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

#include "bdx_call.h"
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
    t.no_band_roll = getenv("BDX_NO_BAND_ROLL") != nullptr;
    t.no_known_exact = getenv("BDX_NO_KNOWN_EXACT") != nullptr;
    t.no_kaln = getenv("BDX_NO_KALN") != nullptr;
    t.trace_launch = getenv("BDX_TRACE_LAUNCH") != nullptr;
    if (const char *e = getenv("BDX_WAVE_CHANCE")) t.wave_chance = atof(e);
    if (const char *e = getenv("BDX_PAIRS_NW")) t.pairs_nw = atoi(e);
    return t;
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

// One table on the device: `bytes` of src in a buffer of at least bytes + room.
int upload(bdx_ctx *ctx, DevBuf &buf, const void *src, size_t bytes, size_t room = 0) {
    HIP_TRY(ctx, buf.ensure(bytes + room));
    HIP_TRY(ctx, hipMemcpy(buf.p, src, bytes, hipMemcpyHostToDevice));
    return BDX_OK;
}

const uint8_t *at(const DevBuf &t, size_t off) { return (const uint8_t *)t.p + off; }

void bind(BdxBitparPlan &bp, const DevBuf &t, const BdxBitparOff &o, int npass) {
    if (!bp.enabled) return;
    bp.d_lut = at(t, o.lut);
    for (int k = 0; k < npass; ++k) {
        bp.d_peq[k] = at(t, o.peq[k]);
        bp.d_pvinit[k] = at(t, o.pvinit[k]);
        bp.d_kb[k] = (const int32_t *)at(t, o.kb[k]);
    }
}

void bind(BdxSeedPlan &sp, const DevBuf &t, const BdxSeedOff &o) {
    if (!sp.enabled) return;
    if (!sp.diag) {
        sp.d_bitmap = (const uint32_t *)at(t, o.bitmap);
        sp.d_hash = (const uint32_t *)at(t, o.hash);
        sp.d_hash_ps = at(t, o.hash_ps);
    }
    for (int k = 0; k < 2; ++k) {
        sp.d_always[k] = (const uint16_t *)at(t, o.always[k]);
        if (!sp.diag) continue;
        sp.d_dmeta[k] = (const uint32_t *)at(t, o.dmeta[k]);
        sp.d_dkeys[k] = (const uint32_t *)at(t, o.dkeys[k]);
    }
}

void bind(BdxWavePlan &wp, const DevBuf &t, const BdxWaveOff &o) {
    if (!wp.enabled) return;
    wp.d_bitmap = at(t, o.bitmap);
    wp.d_rank = (const uint16_t *)at(t, o.rank);
    wp.d_ent = (const uint32_t *)at(t, o.ent);
    wp.d_peq8 = (const uint32_t *)at(t, o.peq8);
    wp.d_meta = (const uint32_t *)at(t, o.meta);
    wp.d_settle = (const uint32_t *)at(t, o.settle);
    wp.d_peq8r = (const uint32_t *)at(t, o.peq8r);
}

// Everything the planner produced goes to the device here: the barcode arrays, the counters, and per filter set every
// table a plan left enabled refers to (also one a rejected tier attempt left behind: the call planner walks both sets); then
// the plans' pointers are bound from base + offset.
int upload_plan(bdx_ctx *ctx, const bdx_config_t &c, const BdxPlanOut &po) {
    ctx->dev = po.dev;
    ctx->plan = po.plan;
    static_cast<BdxPlanChoice &>(*ctx) = po;
    const int npass = c.is_dual ? 2 : 1;
    int rc = BDX_OK;
    for (int k = 0; k < npass; ++k) {
        const bdx_pass_t &p = c.pass[k];
        BdxDevPass &P = ctx->dev.pass[k];
        if ((rc = upload(ctx, ctx->bc_bytes[k], p.bc_bytes, p.bc_off[p.n_barcodes], 16)) != BDX_OK) return rc;
        if ((rc = upload(ctx, ctx->bc_off[k], p.bc_off, (size_t)(p.n_barcodes + 1) * 4)) != BDX_OK) return rc;
        if ((rc = upload(ctx, ctx->bc_nn[k], p.bc_len_no_N, (size_t)p.n_barcodes * 4)) != BDX_OK) return rc;
        P.bc_bytes = (const uint8_t *)ctx->bc_bytes[k].p;
        P.bc_off = (const uint32_t *)ctx->bc_off[k].p;
        P.bc_len_no_N = (const int32_t *)ctx->bc_nn[k].p;
    }
    HIP_TRY(ctx, ctx->counts_own.ensure((size_t)ctx->dev.n_counts * 8));
    HIP_TRY(ctx, hipMemset(ctx->counts_own.p, 0, (size_t)ctx->dev.n_counts * 8));
    ctx->counts = (unsigned long long *)ctx->counts_own.p;
    for (int s = 0; s < 2; ++s) {
        BdxFilterSet &F = ctx->fs[s];
        const BdxPlanSet &P = po.fs[s];
        static_cast<BdxSetPlans &>(F) = P;
        const struct { DevBuf &buf; const BdxBlob &blob; int used; } tables[5] = {
            {F.bp_tables, P.bp_tables, F.bplan.enabled},
            {F.seed_tables, P.seed_tables, F.splan.enabled},
            {F.seed_tables_alt, P.seed_tables_alt, F.splan_alt.enabled},
            {F.wave_tables, P.wave_tables, F.wplan.enabled | F.wplan_k.enabled | F.wplan_a.enabled},
            {F.pair_tables, P.pair_tables, F.pplan.enabled | F.pplan_k.enabled | F.pplan_a.enabled}};
        for (const auto &t : tables)
            if (t.used && (rc = upload(ctx, t.buf, t.blob.bytes.data(), t.blob.bytes.size())) != BDX_OK) return rc;
        bind(F.bplan, F.bp_tables, P.bp_off, npass);
        bind(F.splan, F.seed_tables, P.seed_off);
        bind(F.splan_alt, F.seed_tables_alt, P.seed_alt_off);
        for (BdxWavePlan *wp : {&F.wplan, &F.wplan_k, &F.wplan_a}) bind(*wp, F.wave_tables, P.wave_off);
        for (BdxWavePlan *wp : {&F.pplan, &F.pplan_k, &F.pplan_a}) bind(*wp, F.pair_tables, P.pair_off);
    }
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
    std::vector<DevBuf> retired;  // old tables: freed once the stream is idle (a new table of a failed step dies after the same wait)
    auto retire_all = [&]() {
        (void)hipStreamSynchronize(ctx->stream);
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
                ctx->st_len_rows = old_rows;
                return fail(ctx, BDX_E_DEVICE, "growing the statistics tables failed: %s", hipGetErrorString(e1));
            }
            retired.push_back(std::move(ctx->st_tab[p][1]));
            ctx->st_tab[p][1] = std::move(nb);
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
                return fail(ctx, BDX_E_DEVICE, "growing the statistics tables failed: %s", hipGetErrorString(e1));
            }
            retired.push_back(std::move(ctx->st_tab[p][w]));
            ctx->st_tab[p][w] = std::move(nb);  // row-major by key: the old table is a prefix of the new one
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
    // (band_roll_off: inside the rolling band's class, though without a filter the exact kernel keeps its LDS columns)
    ctx->st_len_fixed = (ctx->plan.clean || ctx->plan.band_roll || ctx->band_roll_off || c.algorithm != BDX_ALG_SEMIGLOBAL) && !sg_window;
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
    ctx->tune = read_tuning();  // the environment is consulted here and nowhere else (the planner gets this struct)
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
    {
        BdxPlanOut po;  // host only: which kernels, which tables (bdx_plan.cpp); needs the caller's host tables
        rc = bdx_plan(*config, ctx->tune, ctx->n_cu, po);
        if (rc != BDX_OK) {
            ctx->err = po.err;
            return bail(rc);
        }
        rc = upload_plan(ctx, *config, po);
        if (rc != BDX_OK) return bail(rc);
    }
    if (ctx->d_dbg.ensure(256) != hipSuccess || hipMemset(ctx->d_dbg.p, 0, 256) != hipSuccess) {
        ctx->err = "hipMalloc failed";
        return bail(BDX_E_DEVICE);
    }
    ctx->dev.dbg_rejected = (unsigned int *)ctx->d_dbg.p;
    rc = init_stats(ctx);
    if (rc != BDX_OK) return bail(rc);
    if (ctx->fs[0].bplan.enabled) {
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
    if (bdx_generic_set_lds_limit(BDX_LDS_MAX) != hipSuccess) {
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
    if (ctx->back_events_made)
        for (hipEvent_t &e : ctx->back_events)
            if (e) (void)hipEventDestroy(e);
    bdx_comm_release(ctx);
    delete ctx;  // (every DevBuf / PinnedBuf of the context frees itself, on the device selected above and after its streams are idle)
}

int32_t bdx_set_stream(bdx_ctx *ctx, void *hip_stream) {
    if (!ctx) return BDX_E_INVALID;
    const hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    // the scratch half the next call takes was cleared by a launch on the old stream, which the new one is not ordered
    // after: the next call clears its scratch words itself
    if (s != ctx->stream) ctx->turn.stream_changed();
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

// ---- one filtered classify call, after its plan (bdx_plan_call, bdx_call.cpp): reserve (buffers, poison, scratch), enqueue ------

// Buffers of the plan's hand-overs, the test switch's fills, this call's half of the scratch block and the per-launch
// fields of the plans.
static int reserve(bdx_ctx *ctx, CallPlan &p, long long n_reads, bool scratch_cleared) {
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
    if (p.carry) {
        HIP_TRY(ctx, ctx->d_carry.ensure(list_bytes));
        p.wfront.d_carry = p.wmid.d_carry = (uint32_t *)ctx->d_carry.p;
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
    // this call's half of the scratch block (BdxScratch): one memset clears its words — unless the last call's final launch
    // already did: the halves alternate, so a call needs no memset of its own (5 us of fill + a launch gap per call, 1 % of a
    // 10 M-read C2 step)
    BdxScratch *const scratch = ctx->scratch();
    if (ctx->turn.begin_call(scratch_cleared)) HIP_TRY(ctx, hipMemsetAsync(scratch->tile_queue, 0, 4 * BDX_SCRATCH_WORDS, ctx->stream));
    for (int set = tiered ? 1 : 0; set >= 0; --set) {
        BdxBitparPlan &b = set ? p.t1 : p.fused;
        b.d_tile_counter = set ? scratch->tile_queue_t1 : scratch->tile_queue;
        b.dense_w = set ? 0 : p.dense_w;
        b.dbg = ctx->tune.debug;
    }
    return BDX_OK;
}

// dev: the call's copy of the device config (a window upload's per-read pointers are in it)
static int enqueue(bdx_ctx *ctx, const CallPlan &p, const BdxDevCfg &dev, const BdxBatch &b, const BdxDevStats *stp) {
    const BdxFilterSet &f0 = ctx->fs[0], &f1 = ctx->fs[1];
    const bool tiered = p.tier_len > 0;
    BdxScratch *const scratch = ctx->scratch();
    // the hand-over buffers: a single-pass call names pass 0's twice, windows only when the call runs with them
    BdxHandOver ho{};
    for (int k = 0; k < 2; ++k) {
        const int buf = k < p.npass ? k : 0;
        ho.cand_words[k] = k < p.npass ? dev.pass[k].cand_words : 0;
        ho.cand[k] = (uint32_t *)ctx->d_cand[buf].p;
        ho.wins[k] = p.windows ? (uint32_t *)ctx->d_wins[buf].p : nullptr;
        ho.wcnt[k] = p.windows ? (uint8_t *)ctx->d_wcnt[buf].p : nullptr;
        ho.short_lb[k] = p.short_lb[k];
    }
    // what the known-score fused kernel hands to the exact kernel; what the front stage cannot settle: tier 1 lists into d_tier,
    // a plain front stage into d_wlist; the pairs mode into d_wlist
    const BdxDevList none{}, exc{p.split ? nullptr : (uint32_t *)ctx->d_exc.p, &scratch->exc_count};
    const BdxDevList front{(uint32_t *)(tiered ? ctx->d_tier.p : ctx->d_wlist.p), &scratch->front_count}, mid{(uint32_t *)ctx->d_wlist.p, &scratch->mid_count};
    const double *slo = f1.bplan.tier_slo;
    const BdxTierArgs no_lists{}, tier1{none, front, 1, {slo[0], slo[1]}};
    const BdxTierArgs front_out = tiered ? tier1 : BdxTierArgs{none, front, 0, {0.0, 0.0}};  // a front stage that settles and lists
    const auto over = [&](const BdxDevList &in, const BdxDevList &out) { return BdxTierArgs{in, out, 0, {0.0, 0.0}}; };
    // the device config of a launch of the generic kernel: the band fields are the plan's
    const auto with_band = [&](const BdxBandPlan &bd) {
        BdxDevCfg dv = dev;
        dv.dense_w = bd.dense_w;
        dv.band_m = bd.m;
        for (int k = 0; k < 2; ++k) dv.band_kb[k] = bd.kb[k], dv.band_lb[k] = bd.lb[k];
        return dv;
    };
    // test switch BDX_POISON: between a producer and its consumer, every element the consumer will read must have
    // been written (bdx_poison_check_kernel); `with_windows`: also the window hand-over of both passes for these reads
    const auto poison_check = [&](const BdxDevList &list, bool check_list, bool with_windows, bool packed = false) -> hipError_t {
        if (!ctx->tune.poison) return hipSuccess;
        unsigned int *dbg = (unsigned int *)ctx->d_dbg.p;
        if (!with_windows || !p.windows) return list.ids ? bdx_launch_poison_check(b, list, ho, -1, 0, (check_list ? 1 : 0) | (packed ? 2 : 0), dbg) : hipSuccess;
        for (int k = 0; k < p.npass; ++k) {
            hipError_t e = bdx_launch_poison_check(b, list, ho, k, dev.pass[k].n_barcodes, (check_list && k == 0) ? 1 : 0, dbg);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };
    // `filter`: a wave / pairs launch in its split form (masks + windows into the hand-over, no verdicts, no counts, no list)
    const auto counted = [](hipError_t e, int64_t &launches) { if (e == hipSuccess) launches += 1; return e; };
    const int he = ctx->plan.hist_entries;
    const auto wave = [&](const BdxWavePlan &wp, bool filter) {
        return counted(filter ? bdx_launch_wave(dev, wp, he, b.uncounted(), ho, no_lists) : bdx_launch_wave(dev, wp, he, b, BdxHandOver{}, front_out), ctx->wave_launches);
    };
    const auto pairs = [&](const BdxWavePlan &wp, const BdxDevList &in, bool filter, const BdxDevStats *st) {
        return counted(filter ? bdx_launch_pairs(dev, wp, he, b.uncounted(), ho, over(in, none), st) : bdx_launch_pairs(dev, wp, he, b, BdxHandOver{}, over(in, mid), st),
                       ctx->pair_launches);
    };
    const auto generic = [&](const BdxBandPlan &bd, const BdxTierArgs &t, long long blocks, bool last) {
        // (the call's last launch clears the other scratch half for the next call)
        const hipError_t e = bdx_launch_generic(with_band(bd), ctx->plan, b, ho, t, stp, blocks, last ? (uint32_t *)ctx->scratch(true)->tile_queue : nullptr);
        if (e == hipSuccess) ctx->band_launches += bd.launches;
        return e;
    };

    BdxDevList todo = none;  // the list the next stage walks (none: every read of the batch)
    // 1. front stage
    switch (p.front) {
        case Front::none: break;
        case Front::bitpar: HIP_TRY(ctx, bdx_launch_bitpar(dev, ctx->plan, p.t1, bdx_seed_plan(f1, p.seed[1]), b, ho, exc, tier1)); break;
        case Front::wave: HIP_TRY(ctx, wave(p.wfront, false)); break;
        case Front::wave_win: HIP_TRY(ctx, counted(bdx_launch_wave_win(dev, p.wfront, he, b, front_out), ctx->wave_launches)); break;
        case Front::wave_split: HIP_TRY(ctx, wave(p.wfront, true)); break;  // (the exact kernel settles and lists)
        case Front::wave_end:  // verdicts + trimmed keep range of what it settles
            HIP_TRY(ctx, counted(bdx_launch_wave_end(dev, p.wfront, he, b, front_out, p.aln ? stp : nullptr), ctx->wave_launches));
            break;
        case Front::pairs: HIP_TRY(ctx, pairs(p.wfront, none, true, nullptr)); break;
    }
    // 2. tier 1's exact launch: it answers what tier 1 settles and lists the rest (known-score / known-end configs: the filter kernel did)
    if (p.t1_exact) {
        HIP_TRY(ctx, poison_check(none, false, true));
        HIP_TRY(ctx, generic(p.band_t1, tier1, p.t1_exact_blocks, false));
    }
    if (p.front != Front::none) {  // tier 0 / the plain front stage's filter set walks the list
        todo = front;
        HIP_TRY(ctx, poison_check(todo, true, false, p.carry));
    }
    // 3. middle stage
    switch (p.middle) {
        case Middle::none: break;
        case Middle::end: HIP_TRY(ctx, pairs(p.wmid, todo, false, p.aln ? stp : nullptr)); break;
        case Middle::list: HIP_TRY(ctx, pairs(p.wmid, todo, false, nullptr)); break;
        case Middle::split: HIP_TRY(ctx, pairs(p.wmid, todo, true, nullptr)); break;
        case Middle::all: HIP_TRY(ctx, pairs(p.wmid, none, true, nullptr)); break;
    }
    if (p.middle == Middle::end || p.middle == Middle::list) {  // what the pairs mode cannot answer goes on in list mode
        todo = mid;
        HIP_TRY(ctx, poison_check(todo, true, false));
    }
    // 4. full-budget filter (in list mode it runs with its own set's thresholds: nothing lies beyond a full budget)
    switch (p.full) {
        case Full::none: break;  // (the pairs mode already wrote the masks and windows)
        case Full::wave_split: HIP_TRY(ctx, wave(p.wfull, true)); break;
        case Full::bitpar: {
            const BdxTierArgs listed{todo, none, 0, {p.fused.tier_slo[0], p.fused.tier_slo[1]}};
            HIP_TRY(ctx, bdx_launch_bitpar(dev, ctx->plan, p.fused, bdx_seed_plan(f0, p.seed[0]), b, ho, exc, p.front != Front::none ? listed : no_lists));
            break;
        }
    }
    // 5. exact stage
    switch (p.exact) {
        case Exact::known:
            HIP_TRY(ctx, poison_check(exc, true, false));
            HIP_TRY(ctx, generic(p.band_exact, over(exc, none), p.exact_blocks, true));
            break;
        case Exact::split:
            HIP_TRY(ctx, poison_check(none, false, true));
            HIP_TRY(ctx, generic(p.band_exact, no_lists, p.exact_blocks, true));
            break;
        case Exact::split_list:  // (tiered: list mode over the reads tier 1 handed on)
            HIP_TRY(ctx, poison_check(todo, false, true));
            HIP_TRY(ctx, generic(p.band_exact, over(todo, none), p.exact_blocks, true));
            break;
    }
    ctx->turn.finish_call();  // (the other half will hold zeros when the next call's kernels start)
#ifdef BDX_TUNING
    if (ctx->tune.debug & 128) {  // tuning statistics of the fused kernel (see bdx_bitpar.hip)
            unsigned int st[4] = {0, 0, 0, 0}, tl = 0;
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, hipMemcpy(st, &scratch->exc_count, sizeof(st), hipMemcpyDeviceToHost));  // (with the three statistics words behind it)
            HIP_TRY(ctx, hipMemcpy(&tl, &scratch->front_count, sizeof(tl), hipMemcpyDeviceToHost));
            fprintf(stderr, "[bdx] handed over %u reads; %u windowed sweeps, %u columns, %u tiles with a fallback read; tier 0 list %u (of %lld reads)\n",
                    st[0], st[1], st[2], st[3], tl, b.n_reads);
    }
#endif
    return BDX_OK;
}

}  // extern "C"

// ---- one classify call: the batch's read length, the statistics tables, plan, reserve, enqueue ---------------------------------
int bdx_classify_batch(bdx_ctx *ctx, const BdxBatchIn &in) {
    if (!in.append_log) ctx->launch_log.clear();
    const long long n_reads = in.n_reads;
    // the launchers note what they enqueue into this call's log (test visibility: bdx_last_launches)
    struct LogScope {
        std::string *prev;
        explicit LogScope(std::string *log) : prev(t_launch_log) { t_launch_log = log; }
        ~LogScope() { t_launch_log = prev; }
    } log_scope(&ctx->launch_log);
    const BdxDevOut o{in.out.bc1,      in.out.bc2,      in.out.keep_start, in.out.keep_end,   in.out.pass_start,
                      in.out.pass_end, in.out.pass_raw, in.out.pass_bc,    in.out.pass_score, in.out.pass_delta};
    // the batch's read length (bdx_batch_len holds the rule); measured here and nowhere else: one tiny kernel, a 4-byte copy
    // and a stream synchronisation
    const bool window_upload = in.vlen != nullptr;
    const auto batch_len = [&](int measured) {
        return bdx_batch_len(window_upload ? in.known_maxlen : 0, window_upload ? 0 : in.known_maxlen, ctx->user_len_hint, ctx->dev.need_traceback != 0,
                             ctx->fs[0].bplan.enabled != 0, measured);
    };
    BdxBatchLen bl = batch_len(-1);
    if (bl.measure) {
        int measured = 0;
        HIP_TRY(ctx, ctx->d_maxlen.ensure(1024));
        HIP_TRY(ctx, bdx_launch_maxlen((const long long *)in.d_off, n_reads, (int *)ctx->d_maxlen.p, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(&measured, ctx->d_maxlen.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        bl = batch_len(measured < 0 ? 0 : measured);
    }
    BdxDevStats st{};
    const BdxDevStats *stp = nullptr;
    if (ctx->dev.need_traceback) {
        // (sized from the batch's true maximum read length: a hint is only a hint)
        int rc = bdx_stats_reserve(ctx, (long long)bl.longest + ctx->dev.max_m + 2);
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
    const BdxCallEnv env{ctx->dev, ctx->plan, ctx->fs[0], ctx->fs[1], *ctx, ctx->tune, ctx->n_cu};
    BdxCallArgs args;
    args.n_reads = n_reads;
    args.read_len = bl.planned;
    args.window_upload = window_upload;
    void *const vectors[10] = {o.bc1, o.bc2, o.keep_start, o.keep_end, o.pass_start, o.pass_end, o.pass_raw, o.pass_bc, o.pass_score, o.pass_delta};
    for (int i = 0; i < 10; ++i) args.wanted |= vectors[i] ? 1u << i : 0u;
    args.stats = stp != nullptr;
    CallPlan &p = ctx->last;
    std::string why;
    int rc = bdx_plan_call(env, args, ctx->seed, p, why);
    if (rc != BDX_OK) return fail(ctx, rc, "%s", why.c_str());
    BdxDevCfg dev = ctx->dev;  // the launches' config: what bdx_create produced + this batch's window-upload pointers
    dev.vlen = in.vlen;
    dev.vlo = in.vlo;
    const BdxBatch batch{in.d_seq, (const long long *)in.d_off, n_reads, o, ctx->counts, ctx->stream};
    if (p.filtered) {
        rc = reserve(ctx, p, n_reads, in.scratch_cleared);
        if (rc == BDX_OK) rc = enqueue(ctx, p, dev, batch, stp);
        if (rc != BDX_OK) return rc;
        ctx->last_blocks = (n_reads + p.fused.reads_per_block - 1) / p.fused.reads_per_block;
        ctx->path = p.path;
        ctx->filter_used = bdx_seed_plan(ctx->fs[0], p.seed[0]).enabled ? BDX_FILTER_QGRAM : BDX_FILTER_BITPAR;
    } else {
        HIP_TRY(ctx, bdx_launch_generic(dev, ctx->plan, batch, BdxHandOver{}, BdxTierArgs{}, stp, p.exact_blocks, nullptr));
        ctx->last_blocks = p.exact_blocks;
        ctx->path = "generic";
        ctx->filter_used = BDX_FILTER_OFF;
    }
    ctx->launches += 1;
    return BDX_OK;
}

extern "C" {

int32_t bdx_classify_device(bdx_ctx *ctx, const uint8_t *d_seq_bytes, const int64_t *d_seq_off, int64_t n_reads,
                            const bdx_outputs_t *d_out) {
    if (!ctx) return BDX_E_INVALID;
    ctx->launch_log.clear();
    if (n_reads < 0) return fail(ctx, BDX_E_INVALID, "n_reads is negative");
    if (n_reads == 0) return BDX_OK;
    if (!d_seq_bytes || !d_seq_off || !d_out) return fail(ctx, BDX_E_INVALID, "NULL device pointer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BdxBatchIn in;  // (nothing known of the batch: the library measures what it needs)
    in.d_seq = d_seq_bytes;
    in.d_off = d_seq_off;
    in.n_reads = n_reads;
    in.out = *d_out;
    return bdx_classify_batch(ctx, in);
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
    if (hipMemcpy(&v, &ctx->scratch(true)->front_count, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)v;
}

int64_t bdx_last_mid_reads(bdx_ctx *ctx) {
    if (!ctx || !ctx->d_maxlen.p) return 0;
    if (hipSetDevice(ctx->device) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return -1;
    unsigned int v = 0;
    if (hipMemcpy(&v, &ctx->scratch(true)->mid_count, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return -1;
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
    const CallPlan &p = ctx->last;  // (filtered: the last call ran the fused kernel's path)
    const bool f = ctx->filter_used != BDX_FILTER_OFF && p.filtered;
    out->threads_per_block = f ? 256 : ctx->plan.threads;
    out->lds_bytes_per_block = f ? (int32_t)p.lds_bytes : (int32_t)ctx->plan.lds_bytes;
    out->blocks = ctx->last_blocks;
    out->reads_per_block = f ? p.fused.reads_per_block : ctx->plan.threads;
    out->filter_used = ctx->filter_used;
    out->max_m = ctx->dev.max_m;
    out->launches = ctx->launches;
    return BDX_OK;
}

}  // extern "C"
