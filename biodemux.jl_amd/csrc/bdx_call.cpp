// bdx_call.cpp — the per-call planner: every geometry and every stage of one classify call, decided before its first launch.
// Pure arithmetic over what bdx_create produced (BdxCallEnv) and the batch at hand (BdxCallArgs): the sizers take a
// create-time plan by const reference and fill a sized copy, nothing in the environment is written.  The one state a call
// leaves behind is the seed choice per filter set (BdxSeedChoice, bdx_call.h).
#include "bdx_call.h"

#include <algorithm>
#include <cmath>
#include <initializer_list>

namespace {

struct Batch {  // a sizer's view of the call
    const BdxCallEnv &env;
    bool window_upload;
};

// One tile size of the wave kernel (rw reads, span bytes, queues of hq / sq entries; `area`: a wave's work area) against the
// workgroup shapes `shapes` (waves per workgroup; `forced`: only that one): the tables once + one area per wave must fit
// the LDS, at most maxres waves stay resident per compute unit.  A shape that keeps more waves resident than `best` goes
// into wp.
void try_tile(const BdxCallEnv &env, BdxWavePlan &wp, int &best, size_t tables, size_t area, std::initializer_list<int> shapes, int maxres, int rw,
              int span, int hq, int sq) {
    for (int w : shapes) {
        if (w < 1 || w > 16 || (env.tune.wave_waves && w != env.tune.wave_waves)) continue;
        const size_t lds = tables + (size_t)w * area;
        if (lds > BDX_LDS_MAX) continue;
        int per_cu = bdx_lds_residency(lds);
        if (per_cu * w > maxres) per_cu = maxres / w;
        if (per_cu * w <= best) continue;
        best = per_cu * w;
        wp.rw = rw;
        wp.waves = w;
        wp.blocks = per_cu * env.n_cu;
        wp.span_cap = span;
        wp.hq_cap = hq;
        wp.sq_cap = sq;
    }
}

// queues of a tile: the planted barcode's pieces (up to kb + 1 = 3 hits, one or two records) + the chance hits, with slack
int hit_queue(int rw, double chance) { return rw * (int)std::ceil(std::max(6.0, 4.0 + 2.5 * chance)); }
int sweep_list(int rw, double chance) { return rw * (int)std::ceil(std::max(3.0, 1.8 + 1.6 * chance)); }

// columns of a range resolved at the planned read length (classification.jl:795-800)
long long window_len(const BdxDevRange &dr, int read_len) {
    long long f, l;
    bdx_resolve_range(dr, read_len, f, l);
    return l - f + 1;
}

// Geometry of the wave kernel for a batch: the tile size and workgroup shape that keep the most waves resident
// per compute unit (tables once per workgroup + one work area per wave within 160 KiB, at most 16 waves: the
// kernel is compiled for four waves per SIMD).  false: this batch runs the general kernel.
bool size_wave(const Batch &b, const BdxWavePlan &src, int read_len, long long n_reads, BdxWavePlan &wp) {
    const BdxCallEnv &env = b.env;
    wp = src;
    wp.winm = 0;
    if (!wp.enabled || b.window_upload) return false;  // (window uploads stage per-read slots: general kernel)
    const size_t tables = bdx_wave_table_bytes(wp, env.plan.hist_entries);
    const int rws[3] = {32, 16, 8};
    int best_waves = 0;
    for (int rw : rws) {
        if (env.tune.wave_rw && rw != env.tune.wave_rw) continue;
        // small batches: at least one tile per resident wave before the tile grows
        if (!env.tune.wave_rw && rw > 8 && n_reads / rw < (long long)env.n_cu * 16) continue;
        const long long span = (((long long)rw * read_len + 64 + 15) & ~15LL);
        if (span > 10 * 1024) continue;  // a tile's bytes wait in registers: at most ten 16-byte vectors per lane
        const int hq = hit_queue(rw, wp.chance), sq = sweep_list(rw, wp.chance);
        const size_t area = bdx_wave_area_bytes(rw, (int)span, false, hq, sq, wp.cand_words + (wp.ranged ? 4 : 0));
        const int maxres = env.tune.wave_maxres > 0 ? env.tune.wave_maxres : 16;
        try_tile(env, wp, best_waves, tables, area, {8, 16, 4, env.tune.wave_waves}, maxres, rw, (int)span, hq, sq);  // (a forced shape may be any wave count up to 16)
        if (best_waves >= 12) break;  // a larger tile at (nearly) full residency beats a smaller one
    }
    if (best_waves < 4) return false;
    wp.read_len_hint = read_len;
    // ranged single-pass configs: the seed scan only walks the groups of sixteen positions that overlap a read's window when
    // the window (resolved at the planned read length, classification.jl:795-800) is much shorter than the read
    wp.scan_gpr = 0;
    if (wp.ranged) {
        const int npw = env.dev.is_dual ? 2 : 1;
        long long gpr = 0;
        for (int k = 0; k < npw; ++k) gpr = std::max(gpr, (window_len(env.dev.pass[k].ref_search, read_len) + 15) / 16 + 1);
        if (gpr * npw * 16 * 10 <= (long long)read_len * 7 && (long long)wp.rw * npw * gpr < 2048) wp.scan_gpr = (int)gpr;
    }
    return true;
}

// Window mode of the wave kernel (bdx_wave_win.hip) for a batch: single-pass known-score configs whose ref_search_range
// window — resolved at the planned read length (classification.jl:795-800) — is at most half the read: the tiles are
// scattered, every read's slot holds just its window (+ up to 15 positions in front: the loads are aligned 16-byte vectors).
// This is what lets 10 kbp reads with a 200-column window (BASELINE config 5) take the wave kernel at all: a tile's bytes
// wait in registers, which bounds a contiguous tile at 10 KB.
bool size_wave_win(const Batch &b, const BdxWavePlan &src, int read_len, long long n_reads, BdxWavePlan &wp) {
    const BdxCallEnv &env = b.env;
    wp = src;
    wp.winm = 0;
    if (!wp.enabled || b.window_upload || !wp.ranged || wp.split || wp.kend || env.dev.is_dual || env.tune.no_wave || env.tune.no_win) return false;
    const BdxDevRange &dr = env.dev.pass[0].ref_search;
    const long long LIM = 1LL << 28;  // (the kernel resolves the windows in 32-bit arithmetic)
    if (dr.start_offset < -LIM || dr.start_offset > LIM || dr.end_offset < -LIM || dr.end_offset > LIM) return false;
    const long long wlen = window_len(dr, read_len);
    if (wlen < 1 || wlen * 2 > read_len) return false;
    const int slot = (int)((wlen + 15 + 15) & ~15LL);
    const size_t tables = bdx_wave_table_bytes(wp, env.plan.hist_entries);
    const double chance = wp.chance * (double)wlen / 150.0;
    int best_waves = 0;
    const int rws[2] = {32, 16};
    for (int rw : rws) {
        if (env.tune.wave_rw && rw != env.tune.wave_rw) continue;
        if (!env.tune.wave_rw && rw > 16 && n_reads / rw < (long long)env.n_cu * 16) continue;  // small batches: a tile per resident wave first
        const int vecs = rw * (slot >> 4);
        if (!((rw == 32 && vecs <= 64 * 7) || (rw == 16 && vecs <= 64 * 4))) continue;  // (instantiated register budgets)
        const int span = rw * slot + 16;
        const int hq = hit_queue(rw, chance), sq = sweep_list(rw, chance);
        const size_t area = bdx_wave_area_bytes(rw, span, false, hq, sq, 0, true);
        // (tried: 32-read tiles on 12 waves per CU — C5 0.329 vs 0.314 ms with 16-read tiles on 16 waves)
        try_tile(env, wp, best_waves, tables, area, {16, 8, 4}, 16, rw, span, hq, sq);
        if (best_waves >= 12) break;
    }
    if (best_waves < 4) return false;
    wp.slot = slot;
    wp.read_len_hint = read_len;
    wp.scan_gpr = 0;
    wp.winm = 1;
    return true;
}

// Geometry of the pairs mode for a batch: 16-read tiles of slots of `read_len` rounded up to 16 bytes.
bool size_pairs(const Batch &b, const BdxWavePlan &src, int read_len, BdxWavePlan &wp) {
    const BdxCallEnv &env = b.env;
    wp = src;
    if (!wp.enabled || b.window_upload) return false;
    // a read's slot in the tile's images: its bytes are fetched as aligned 16-byte vectors, so it starts up to 15 positions in
    const int slot = (read_len + 15 + 15) & ~15;
    const int rw = 16;
    const int span = rw * slot + 16;
    if (span > 6 * 1024 + 16) return false;  // (instantiated: three and six 16-byte vectors per lane)
    const int mmin = env.choice.pair_mmin;
    int cpr = ((15 + read_len - mmin + wp.pairs_spread + 8) >> 4) + 1;  // (diagonals are counted from the slot's start)
    if (read_len < mmin) cpr = 1;
    if (cpr > slot / 16) cpr = slot / 16;
    if (cpr < 1) cpr = 1;
    const size_t tables = bdx_wave_table_bytes(wp, env.plan.hist_entries);
    // (31 chance flags per read at 96 barcodes and kb = 4: the queue holds a 16-read tile's worth; with more barcodes it is
    // drained several times per tile; a tile whose queue runs over between two drains is handed on / swept whole)
    // (same-diagonal variants: ~80 chance flags per read at 96 barcodes of eight 3-base pieces — the queue is drained inside the scan)
    const int hq = wp.groups > 1 ? 1024 : wp.pairs_kb >= 8 ? 1280 : 56 * rw;
    const size_t area = bdx_wave_area_bytes(rw, span, true, hq, 0, wp.cand_words + (wp.ranged ? 4 : 0));
    int best = 0;
    try_tile(env, wp, best, tables, area, {16, 8, 4}, 16, rw, span, hq, 0);
    if (best < 4) return false;
    wp.slot = slot;
    wp.cpr = cpr;
    wp.read_len_hint = read_len;
    return true;
}

// Column-window bound for a read length: the union over the passes of final_search_range (classification.jl:799-800),
// resolved exactly like the device does.  Window lengths are non-decreasing in n, so the bound at the planned length
// covers shorter reads.
int window_bound(const BdxDevCfg &dev, int read_len) {
    long long ulo = (1LL << 40), uhi = 0;
    for (int k = 0; k < (dev.is_dual ? 2 : 1); ++k) {
        const BdxDevPass &P = dev.pass[k];
        long long f = P.win_first, l = P.win_last;
        if (!P.explicit_window) {
            long long rf, rl, bf, bl, ef, el;
            bdx_resolve_range(P.ref_search, read_len, rf, rl);
            bdx_resolve_range(P.bc_start, read_len, bf, bl);
            bdx_resolve_range(P.bc_end, read_len, ef, el);
            f = std::max(rf, bf);
            l = std::min(rl, el);
        }
        f = std::max(f, 1LL);
        l = std::min(l, (long long)read_len);
        if (l < f) continue;
        const long long h = std::min(dev.algorithm == BDX_ALG_SEMIGLOBAL ? l : l + dev.max_m - 1, (long long)read_len);
        ulo = std::min(ulo, f - 1);
        uhi = std::max(uhi, h);
    }
    return uhi > ulo ? (int)(uhi - ulo) : 16;
}

enum class Fit { yes, no, demote };  // demote: the seed plan in effect is what stands in the way

// One attempt at the fused kernel's geometry under the seed plan `sp`: the R that keeps the most waves resident per CU
// (the sweep is latency-bound): workgroups/CU = min(8, floor(160 KiB / LDS(R))) with 4 waves each; ties -> larger R
// (fewer table reloads).  R = 16 is only taken when nothing larger fits.
Fit fit_bitpar(const BdxCallEnv &env, const BdxSeedPlan &sp, int read_len, int wmax, bool slot_mode, BdxBitparPlan &bp) {
    const int slot = slot_mode ? ((wmax + 15 + 16 + 15) & ~15) : 0;
    bp.slot_bytes = slot;
    bp.seed_span = slot_mode ? wmax : read_len;
    const bool diag = sp.enabled && sp.diag;
    if (diag) {
        // index width for this read length, and the sweep queue for the expected number of flagged pairs
        if (bp.seed_span > 312) return Fit::demote;  // the widest index holds 320 positions
        bp.diag_nw = bp.seed_span <= 152 ? 5 : 10;
        const double L = (double)(bp.seed_span < 32 ? 32 : bp.seed_span);
        const double flagged = sp.diag_flag_coef * ((L - 3.0) / 256.0) * ((L - 3.0) / 256.0) / (L + 24.0) + (double)(sp.n_always[0] + sp.n_always[1]);
        bp.diag_qcap = (int)(flagged * 1.3) + 12;  // per read (a sub-batch shares 4..8 reads' worth)
    }
    const int forced = env.tune.bitpar_r;
    const int tries[7] = {256, 128, 64, 32, 16, 8, 4};
    int best_R = 0, best_blocks = 0, best_stage = 0;
    bp.read_len_hint_for_lds = read_len;
    for (int R : tries) {
        if (diag ? R > 32 : R < 16) continue;  // the diagonal variant indexes 8 reads at a time (40 KiB): small tiles
        if (forced && R != forced) continue;
        if (!forced && R > bp.r_cap) continue;
        if (bp.word_bytes == 16 && (R > 64 || R < 16)) continue;  // (128-bit sweep words: instantiated for tiles of 64 / 32 / 16 reads)
        if (!forced && !sp.enabled && R > 64 && read_len <= 1024) continue;  // sweep-all: 64-read tiles measured best
        size_t st = slot_mode ? (size_t)R * (size_t)slot : (size_t)R * (size_t)read_len + 64;
        st = (st + 15) & ~(size_t)15;
        if (st > (size_t)1 << 20) continue;
        bp.reads_per_block = R;
        bp.stage_bytes = (int)st;
        const size_t lds = bdx_bitpar_lds_bytes(env.dev, bp, env.plan, &sp);
        if (lds > BDX_LDS_MAX) continue;
        // Measured on MI355X (tools/probe.py): tile size matters more than residency once 3
        // workgroups (12 waves) share a CU — larger tiles fill the 256 lanes of the sparse
        // sweep / exact stages better.  Rank: >= 3 resident (largest R wins), then 2, then 1.
        const int rank = std::min(bdx_lds_residency(lds), 3);
        if (!diag && R == 16 && best_R) continue;
        if (rank > best_blocks) {
            best_blocks = rank;
            best_R = R;
            best_stage = (int)st;
        }
    }
    if (best_R && diag && best_blocks < 2) return Fit::demote;  // the index leaves room for one workgroup per CU only (very many barcodes)
    if (!best_R) return sp.enabled ? Fit::demote : Fit::no;     // the seed tables do not fit next to everything else
    bp.reads_per_block = best_R;
    bp.stage_bytes = best_stage;
    bp.read_len_hint = read_len;
    return Fit::yes;
}

// Geometry of the fused kernel for a given typical read length.
// set: the filter set planned (0: full budgets, 1: tier 1).
// force_slot: list mode (tier 0 of the tiered budgets) — the reads are scattered, every read is staged into a slot
// A seed plan that stands in the way is demoted for good: the two-intact-pieces index gives way to the weak single seeds
// kept beside it, those to the plain sweep.
bool size_bitpar(const Batch &b, int set, BdxSeedChoice &choice, int read_len, long long n_reads, bool force_slot, BdxBitparPlan &bp) {
    const BdxCallEnv &env = b.env;
    const BdxSetPlans &F = set ? env.f1 : env.f0;
    if (!F.bplan.enabled) return false;
    if (b.window_upload) force_slot = true;  // window upload: only each read's window is there
    // small batches: keep >= ~1024 tiles in flight (4 per CU) before growing the tile
    int r_cap = 256;
    while (r_cap > 16 && n_reads / r_cap < 4LL * env.n_cu) r_cap >>= 1;
    const int wmax = window_bound(env.dev, read_len);
    const bool slot_mode = force_slot || ((long long)wmax * 2 + 96 <= (long long)read_len && !env.tune.no_slot);
    for (;;) {
        bp = F.bplan;
        bp.r_cap = r_cap;
        bp.n_cu = env.n_cu;
        const BdxSeedPlan sp = bdx_seed_plan(F, choice);
        const Fit fit = fit_bitpar(env, sp, read_len, wmax, slot_mode, bp);
        if (fit != Fit::demote) return fit == Fit::yes;
        choice = (choice == BDX_SEED_MAIN && sp.diag && F.splan_alt.enabled) ? BDX_SEED_ALT : BDX_SEED_NONE;
    }
}

// ---- the grid and LDS bytes of a launch ----
// Fused kernel, a persistent grid: enough workgroups to fill every compute unit at the LDS-limited residency (the tile queue
// balances it), or what BDX_GRID forces; never more than there are tiles.
void grid_bitpar(const BdxCallEnv &env, const BdxSeedPlan &sp, long long n_reads, BdxBitparPlan &bp) {
    bp.lds_bytes = bdx_bitpar_lds_bytes(env.dev, bp, env.plan, &sp);
    const long long tiles = (n_reads + bp.reads_per_block - 1) / bp.reads_per_block;
    const long long per_cu = std::min(std::max(bdx_lds_residency(bp.lds_bytes), 1), 8);
    const long long blocks = env.tune.grid > 0 ? env.tune.grid : (long long)(env.n_cu > 0 ? env.n_cu : 256) * per_cu;
    bp.grid = std::max(std::min(blocks, tiles), 1LL);
}

// Wave kernel over contiguous tiles: the plan's workgroups, but no more than give every wave one tile; the pairs mode (its
// reads are a list of unknown length): the plan's.  At least one.
void grid_wave(const BdxCallEnv &env, long long n_reads, BdxWavePlan &wp) {
    wp.lds_bytes = bdx_wave_table_bytes(wp, env.plan.hist_entries) + (size_t)wp.waves * bdx_wave_area_bytes(wp);
    const long long tiles = (n_reads + wp.rw - 1) / wp.rw, useful = (tiles + wp.waves - 1) / wp.waves;
    wp.grid = std::max(wp.pairs_kb > 0 ? (long long)wp.blocks : std::min<long long>(wp.blocks, useful), 1LL);
}

// Generic kernel: a thread per read; over a list the grid strides, four workgroups per compute unit.  false: more workgroups
// than a grid holds.
bool grid_generic(const BdxGenericPlan &gp, long long n_reads, bool list, long long &blocks) {
    blocks = (n_reads + gp.threads - 1) / gp.threads;
    if (blocks > 0x7FFFFFFFLL) return false;
    if (list) blocks = std::min(blocks, 4LL * (gp.n_cu > 0 ? gp.n_cu : 256));
    return true;
}

// The band fields of a launch of the generic kernel that filter set `set` hands its windows to.
// (rolling band, barcodes beyond 32 rows: any uniform budget; the first end column is rebuilt from the hand-over row when
// every barcode has the same length — lb is made of max_m)
BdxBandPlan plan_band(const BdxCallEnv &env, const CallPlan &p, int set) {
    const BdxGenericPlan &gp = env.plan;
    BdxBandPlan bd;
    bd.dense_w = set == 0 && p.dense_w;
    bd.m = gp.uniform_len;
    for (int k = 0; k < p.npass; ++k) {
        const int kb = (set ? env.f1 : env.f0).bplan.kb_uniform[k];
        const bool on = gp.band_roll ? (p.windows && gp.same_len && kb >= 0)
                                     : (p.windows && gp.clean && gp.uniform_len > 0 && !env.tune.no_band && env.dev.algorithm == BDX_ALG_SEMIGLOBAL &&
                                        kb >= 0 && kb <= 4);
        bd.kb[k] = on ? kb : -1;
        bd.launches += on && !gp.band_roll;
        bd.lb[k] = p.short_lb[k] ? env.dev.max_m + kb : 2 * (env.dev.max_m + kb) + 1;
    }
    return bd;
}

// the stages of a filtered call, front first
std::string call_path(const BdxSeedPlan &sp, const CallPlan &p) {
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

}  // namespace

size_t bdx_bitpar_lds_bytes(const BdxDevCfg &cfg, const BdxBitparPlan &bp, const BdxGenericPlan &gp,
                            const BdxSeedPlan *sp) {
    auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const int R = bp.reads_per_block;
    const int B0 = cfg.pass[0].n_barcodes, B1 = cfg.is_dual ? cfg.pass[1].n_barcodes : 0;
    const int cw0 = cfg.pass[0].cand_words, cw1 = cfg.is_dual ? cfg.pass[1].cand_words : 0;
    size_t o = 0;
    o += al((size_t)gp.hist_entries * 4) + al(256);
    const size_t wb = bp.word_bytes >= 8 ? (size_t)bp.word_bytes : 4;
    o += al((size_t)bp.ncodes * bp.bpad[0] * wb) + al(cfg.is_dual ? (size_t)bp.ncodes * bp.bpad[1] * wb : 0);
    o += al((size_t)B0 * wb) + al((size_t)B1 * wb) + al((size_t)B0 * 4) + al((size_t)B1 * 4);
    o += al((size_t)R * (cw0 + cw1) * 4) + al((size_t)(R + 1) * 4) + 4 * al((size_t)R * 4) + al((size_t)R * 16);
    const bool seeded = sp && sp->enabled;
    const int sc = (!seeded && bp.dense_d) ? 4 : (bp.slot_cap > 4 ? bp.slot_cap : 4);
    o += al((size_t)2 * R * sc * 4) + al((size_t)2 * R * 4) + al((size_t)2 * R);
    o += al((size_t)bp.stage_bytes + 16);
    if (sp && sp->enabled && sp->diag) {
        const int nw = bp.diag_nw > 0 ? bp.diag_nw : 5;
        const int sbmax = nw <= 5 ? BDX_DIAG_SB_NARROW : 4;
        const int SBh = R < sbmax ? R : sbmax;  // index sub-batch (see the kernel)
        o += al((size_t)(bp.stage_bytes >> 2) + 32) + al((size_t)2 * (bp.diag_qcap > 0 ? bp.diag_qcap : 64) * SBh * 4);
        o += al((size_t)R) + 2 * al((size_t)R * 4);
        o += al((size_t)SBh * 256 * nw * 4) + al((size_t)B0 * 4) + al((size_t)B1 * 4) + al((size_t)B0 * 8) + al((size_t)B1 * 8);
    } else if (sp && sp->enabled) {
        o += al((size_t)sp->bm_words * 4) + al((size_t)(bp.stage_bytes >> 2) + 32);
        if (sp->hash_in_lds) o += al((size_t)4 << sp->hash_log2) + al((size_t)1 << sp->hash_log2);
        const size_t sq = (size_t)2 * (sp->qmul >= 4 ? sp->qmul : 4) * R;  // hit-queue entries
        o += al(sq * 4) + al(sq) + 3 * al((size_t)R * sp->rcap * 4);
        o += al((size_t)R) + 2 * al((size_t)R * 4);
    }
    o += al(32);
    if (!(sp && sp->enabled) && cfg.is_dual) o += al((size_t)R);  // act[]
    if (!(sp && sp->enabled) && bp.dense_d) o += al((size_t)R * (B0 + B1));  // dtab[]
    return o;
}

// The fused kernel filters; the exact DP runs at full width in the generic kernel:
//  * split (trimming / summary / weighted costs / N-scoring / Hamming / exact): every read's candidate mask (+ column
//    windows) goes through HBM, the generic kernel gives every verdict;
//  * known-score configs: the fused kernel also gives the verdict of (nearly) every read by replaying the reducer; the few
//    it cannot settle are listed and evaluated by the generic kernel in list mode;
//  * tiered budgets (known-score configs whose full budget is too large for selective single seeds): tier 1 — capped
//    budgets, single seeds — runs over the whole batch and settles every read whose verdict cannot depend on a barcode
//    beyond the cap; tier 0 — the full budget — then runs in list mode over the rest.
int bdx_plan_call(const BdxCallEnv &env, const BdxCallArgs &args, BdxSeedChoice seed[2], CallPlan &p, std::string &err) {
    p = CallPlan{};
    const BdxDevCfg &dev = env.dev;
    const BdxSetPlans &f0 = env.f0, &f1 = env.f1;
    const Batch b{env, args.window_upload};
    const long long n_reads = args.n_reads;
    const int len = args.read_len < 1 ? 1 : args.read_len;
    const auto fail = [&](int code, const char *msg) {
        err = msg;
        return code;
    };
    const char *const too_many = "more reads than one launch of the exact kernel takes";
    p.filtered = size_bitpar(b, 0, seed[0], len, n_reads, false, p.fused);
    if (!p.filtered) return grid_generic(env.plan, n_reads, false, p.exact_blocks) ? BDX_OK : fail(BDX_E_DEVICE, too_many);
    // both tiers must be plannable for this batch, else the full budget alone (a batch of empty reads is never tiered)
    const bool tiered = env.choice.tiered && size_bitpar(b, 1, seed[1], len, n_reads, false, p.t1) && args.read_len > 0;
    if (n_reads > 0xFFFFFFF0LL) return fail(BDX_E_INVALID, "more than 2^32 reads in one batch");
    const unsigned want = args.wanted;
    const bool want_start = (want & BDX_WANT_PASS_START) != 0, want_end = (want & BDX_WANT_PASS_END) != 0;
    p.npass = dev.is_dual ? 2 : 1;
    p.tier_len = tiered ? len : 0;
    p.batch_len = args.read_len;
    for (int k = 0; k < p.npass; ++k) p.split |= !f0.bplan.known_ok[k];
    // (:exact returns the occurrence's start and end whatever the output policy: a caller that wants them gets the launch in
    // its split form — known-alignment class first, exact kernel for what that lists)
    if (dev.algorithm == BDX_ALG_EXACT && (want_start || want_end)) p.split = true;
    p.windows = p.split && !env.tune.no_windows;
    // dense window table of the plain-sweep kernel (few barcodes, many genuine candidates per read; columns fit 16 bits)
    p.dense_w = p.windows && f0.bplan.dense_d && !bdx_seed_plan(f0, seed[0]).enabled && len <= 60000 && !env.tune.no_dense;
    // restricted runs of passes that only report score (+ end) through the clean-class DP start m + kb columns before
    // the first end column (orc_selftest_clean_short_lookback); everything else keeps 2 (m + kb) + 1
    for (int k = 0; k < p.npass; ++k) {
        const int ts = dev.pass[k].trim_side;
        p.short_lb[k] = (env.plan.clean || env.plan.band_roll) && dev.algorithm == BDX_ALG_SEMIGLOBAL && !dev.need_traceback &&
                        (ts == 0 || (ts == 5 && !want_start));
    }
    // A plain config's front stage hands its list to the SAME filter set: scattered reads -> slot staging.  false: that
    // cannot be planned, the general kernel runs alone over the dense batch (under the seed plan the attempt left)
    bool dense_lost = false;
    const auto list_mode = [&]() {
        const BdxSeedChoice before = seed[0];
        BdxBitparPlan listed;
        if (size_bitpar(b, 0, seed[0], len, n_reads, true, listed)) {
            p.fused = listed;
            return true;
        }
        if (seed[0] != before) dense_lost = !size_bitpar(b, 0, seed[0], len, n_reads, false, p.fused);
        return false;
    };
    // Wave-autonomous kernel (bdx_wave.hip) in front of the general one: it answers the reads of the known-score
    // class and lists the rest — as tier 1 of a tiered config, or (plain configs) ahead of the same filter set
    // in list mode.  (window mode first: reads much longer than their column window — only the windows are fetched)
    if (!p.split && !args.window_upload) {
        const BdxWavePlan &wp = tiered ? f1.wplan : f0.wplan;
        if ((size_wave_win(b, wp, len, n_reads, p.wfront) || size_wave(b, wp, len, n_reads, p.wfront)) && (tiered || list_mode()))
            p.front = p.wfront.winm ? Front::wave_win : Front::wave;
    }
    // Known-end class (trim_side = 5, single pass, no start positions or statistics wanted): the same kernel in its
    // known-end form answers the reads it can settle, trimmed keep range included; the listed rest goes through the
    // split path (filter in list mode -> exact kernel in list mode).
    bool trim3 = false;  // (a trim_side = 3 pass of the known-trim class knows its start only)
    for (int k = 0; k < p.npass; ++k) trim3 |= dev.pass[k].trim_side == 3;
    const bool kend_ok = p.split && p.windows && !args.window_upload && !p.dense_w && !want_start && !args.stats && !(trim3 && want_end);
    // known-alignment class: the caller wants positions the known-trim class does not know, or the statistics tables
    p.aln = p.split && p.windows && !args.window_upload && !p.dense_w && !kend_ok && (tiered ? f1 : f0).wplan_a.enabled;
    if (kend_ok || p.aln) {
        const BdxWavePlan &wk = tiered ? (p.aln ? f1.wplan_a : f1.wplan_k) : (p.aln ? f0.wplan_a : f0.wplan_k);
        if (size_wave(b, wk, len, n_reads, p.wfront) && (tiered || list_mode())) p.front = Front::wave_end;
    }
    // split configs (trimming, summary, weighted costs): the wave kernel as the FILTER of a dense launch — candidate
    // masks and column windows in the formats of the general kernel's split mode, every verdict from the exact
    // kernel as before.  Tiered: tier 1 (all reads); plain: the only filter launch.
    bool wsplit0 = false;
    if (p.split && p.windows && !args.window_upload && p.front == Front::none) {
        if (tiered && f1.wplan.split && size_wave(b, f1.wplan, len, n_reads, p.wfront)) p.front = Front::wave_split;
        if (!tiered) wsplit0 = f0.wplan.split && !p.dense_w && size_wave(b, f0.wplan, len, n_reads, p.wfull);
    }
    // the pairs tier: tier 1's filter is the same-diagonal pairs mode over every read of the batch
    if (tiered && p.front != Front::wave_end && env.choice.pairs_tier && p.split && p.windows && !p.dense_w && !args.window_upload) {
        BdxWavePlan pt;
        if (size_pairs(b, f1.pplan, len, pt)) {
            p.front = Front::pairs;
            p.wfront = pt;
        }
    }
    if (dense_lost) return fail(BDX_E_DEVICE, "internal: the dense launch cannot be planned under the demoted seed plan");
    if (tiered && p.front == Front::none) p.front = Front::bitpar;
    p.t1_exact = tiered && p.split && p.front != Front::wave_end;
    // Pairs mode of the wave kernel between tier 1 and the general kernel: the listed reads are gathered into slots and
    // filtered at the full budgets by the two-intact-pieces lemma.  Known-score configs: it answers them (what it cannot
    // answer goes on to the general kernel in list mode); split configs: it is tier 0's filter (masks + windows of the
    // listed reads for the exact kernel).  Known-end class: the pairs mode answers the listed reads itself (verdict +
    // trimmed keep range); what it cannot answer goes on to the split path in list mode.
    // Same-diagonal pairs mode as the ONLY filter of a split config without tiers (weighted costs whose full budget is beyond
    // every seeded variant — the reference's demo2 options): every read of the batch is laid out in slots and scanned;
    // masks + windows of all reads go to the exact kernel's dense launch.
    if (tiered && (kend_ok || p.aln) && size_pairs(b, p.aln ? f0.pplan_a : f0.pplan_k, len, p.wmid)) {
        p.middle = Middle::end;
    } else if (tiered && (!p.split || p.windows) && !p.dense_w && size_pairs(b, f0.pplan, len, p.wmid)) {
        p.middle = p.split ? Middle::split : Middle::list;
    } else if (!tiered && p.split && p.windows && !p.dense_w && !wsplit0 && p.front != Front::wave_end && !args.window_upload && f0.pplan.enabled &&
               f0.pplan.pairs_kb >= 8 && f0.pplan.split && size_pairs(b, f0.pplan, len, p.wmid)) {
        p.middle = Middle::all;
    }
    // Carried passes: tier 1 of a dual known-class config lists a read when ONE of its passes is open; the pass it settled goes
    // along (two state bits on the list entry + the pass's winning survivor in d_carry[read]) and the pairs mode only looks for
    // the other pass's barcodes — about half of its sweeps for C4.  Only when the pairs mode in its known form is what reads
    // tier 1's list (nothing else understands the state bits), reads fit 30 bits and min_delta = 0 (a lone carried winner
    // then IS the pass's result).
    // (the known-trim / known-alignment forms and the plain known-score form of a dual config without trimming)
    p.carry = tiered && (p.front == Front::wave_end || p.front == Front::wave) && dev.is_dual && dev.min_delta == 0.0 && !env.tune.no_carry &&
              n_reads < (1LL << 30) && !(want & BDX_WANT_PER_PASS) && (p.middle == Middle::end || p.middle == Middle::list) &&
              p.wmid.groups <= 1 && p.wmid.pairs_kb <= 4 && !p.wmid.split;
    if (tiered) {
        // tier 0 walks the list: scattered reads -> slot staging
        // (tier 0 sees a fraction of the batch — 10..25 % in the bench configs: its tile size is planned for a sixteenth of
        // the batch, so that the list of a small batch still spreads over the device — C5, 400 k reads: tiles of 16 instead
        // of 128 reads, 0.42 -> 0.38 ms; batches of millions of reads keep their tiles)
        long long n_list_est = n_reads / (env.tune.tier0_div > 0 ? env.tune.tier0_div : 16);
        if (n_list_est < 1) n_list_est = 1;
        if (!size_bitpar(b, 0, seed[0], len, n_list_est, true, p.fused)) return fail(BDX_E_DEVICE, "internal: tier 0 cannot be planned in list mode");
    }
    p.full = (p.middle == Middle::split || p.middle == Middle::all) ? Full::none : wsplit0 ? Full::wave_split : Full::bitpar;
    p.exact = !p.split ? Exact::known : p.front != Front::none ? Exact::split_list : Exact::split;
    for (BdxBitparPlan *bp : {&p.t1, &p.fused}) {
        bp->short_lb[0] = p.short_lb[0];
        bp->short_lb[1] = p.short_lb[1];
    }
    p.seed[0] = seed[0];
    p.seed[1] = seed[1];
    const BdxSeedPlan sp = bdx_seed_plan(f0, seed[0]);
    // every launch's grid and LDS bytes; the developer switches' word as the wave kernels read it
    grid_bitpar(env, sp, n_reads, p.fused);
    p.lds_bytes = p.fused.lds_bytes;
    if (p.front == Front::bitpar) grid_bitpar(env, bdx_seed_plan(f1, seed[1]), n_reads, p.t1);
    const auto wave_launch = [&](bool launched, BdxWavePlan &wp) {
        if (!launched) return;
        grid_wave(env, n_reads, wp);
        wp.dbg = wp.pairs_kb > 0 ? env.tune.debug >> 8 : env.tune.debug;
    };
    wave_launch(p.front != Front::none && p.front != Front::bitpar, p.wfront);
    wave_launch(p.middle != Middle::none, p.wmid);
    wave_launch(p.full == Full::wave_split, p.wfull);
    if (!grid_generic(env.plan, n_reads, false, p.t1_exact_blocks) || !grid_generic(env.plan, n_reads, p.exact != Exact::split, p.exact_blocks))
        return fail(BDX_E_DEVICE, too_many);
    p.band_t1 = p.band_exact = BdxBandPlan{dev.dense_w, dev.band_m, {dev.band_kb[0], dev.band_kb[1]}, {dev.band_lb[0], dev.band_lb[1]}, 0};
    if (p.t1_exact) p.band_t1 = plan_band(env, p, 1);
    if (p.exact != Exact::known) p.band_exact = plan_band(env, p, 0);
    p.path = call_path(sp, p);
    return BDX_OK;
}

BdxBatchLen bdx_batch_len(int window_len, int host_len, int hint, bool stats, bool filter, int measured) {
    const int known = window_len > 0 ? window_len : host_len > 0 ? host_len : 0;
    const bool wanted = !known && (stats || (filter && hint <= 0));
    const int longest = known ? known : (wanted ? measured : -1);
    int planned = 0;
    if (filter) planned = window_len > 0 ? window_len : hint > 0 ? hint : std::max(longest, 1);
    return BdxBatchLen{wanted && measured < 0, longest, planned};
}
