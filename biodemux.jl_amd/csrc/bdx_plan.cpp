// bdx_plan.cpp — the create-time planner behind bdx_create (bdx_plan.h): the launch plan of the exact kernel, the table
// builders of every filter family and the tier selection.  Host-only and free of the environment: everything comes from
// the caller's config, a BdxTuning and the compute-unit count; every table leaves as a host blob with the offsets its
// plan's pointers take.  tests/plan_host.cpp runs it on a CPU (tests/test_plan_cpu.py, also under ASan / UBSan).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>

#include "bdx_plan.h"

namespace {

const size_t LDS_MAX = BDX_LDS_MAX;

bool whole(const bdx_range_t &r) { return !r.start_from_end && r.start_offset <= 1 && r.end_from_end && r.end_offset >= 0; }

BdxDevRange cvt_range(const bdx_range_t &r) { return BdxDevRange{r.start_offset, r.end_offset, r.start_from_end != 0, r.end_from_end != 0}; }

int bc_len(const bdx_pass_t &p, int b) { return (int)(p.bc_off[b + 1] - p.bc_off[b]); }

// ---- the per-barcode budget, as the device computes it ------------------------------------------------------------
// cost of the cheapest edit operation (:hamming / :exact: one substitution costs 1)
int unit_cost(const bdx_config_t &c) {
    if (c.algorithm != BDX_ALG_SEMIGLOBAL) return 1;
    int cmin = c.mismatch < c.indel ? c.mismatch : c.indel;
    if (c.has_nindel && c.nindel < cmin) cmin = c.nindel;
    return cmin;
}
// allowed_error at the initial threshold (classification.jl:254); negative: the barcode can never be recorded.
// len_norm: normalise by the barcode's length whatever the scoring (the wave / pairs tables and the rolling band, which
// N-scoring never reaches); else by bc_len_no_N under N-scoring.
long long allowed_error(const bdx_config_t &c, const bdx_pass_t &p, int b, bool len_norm = false) {
    if (c.algorithm == BDX_ALG_EXACT) return 0;
    const bool no_N = c.algorithm == BDX_ALG_SEMIGLOBAL && c.has_nindel && !len_norm;
    return (long long)std::floor(c.max_error_rate * (double)(no_N ? p.bc_len_no_N[b] : bc_len(p, b)));
}
bool n_wildcards(const bdx_config_t &c) { return (c.algorithm == BDX_ALG_SEMIGLOBAL && c.has_nindel) || c.algorithm == BDX_ALG_HAMMING; }
bool has_wildcard(const bdx_config_t &c, const bdx_pass_t &p, int b) {
    bool wild = false;
    for (int i = 0; i < bc_len(p, b); ++i) wild |= n_wildcards(c) && p.bc_bytes[p.bc_off[b] + i] == 'N';
    return wild;
}

// alphabet = the distinct barcode bytes, coded in the order they appear; false: more than `limit` of them
bool code_alphabet(const bdx_config_t &c, int code_of[256], int &K, int limit) {
    for (int i = 0; i < 256; ++i) code_of[i] = -1;
    K = 0;
    for (int k = 0; k < (c.is_dual ? 2 : 1); ++k)
        for (uint32_t i = 0; i < c.pass[k].bc_off[c.pass[k].n_barcodes]; ++i) {
            const uint8_t ch = c.pass[k].bc_bytes[i];
            if (code_of[ch] < 0) {
                if (K == limit) return false;
                code_of[ch] = K++;
            }
        }
    return true;
}

// sweep rows of the wave kernel for one barcode: codes A 0, C 1, T 2, G 3 ((byte >> 1) & 3), 4..7 = symbols no barcode
// contains; virtual rows below the barcode match everything, D stays 0.  reversed: the barcode read right to left.
void peq8_rows(const uint8_t *bc, int m, bool reversed, uint32_t *row) {
    const int shift = 32 - m;
    const uint32_t rows = m == 32 ? 0xFFFFFFFFu : (((1u << m) - 1u) << shift);
    for (int code = 0; code < 8; ++code) {
        uint32_t mask = ~rows;
        if (code < 4)
            for (int i = 0; i < m; ++i)
                if (((bc[reversed ? m - 1 - i : i] >> 1) & 3) == code) mask |= 1u << (shift + i);
        row[code] = mask;
    }
}

struct Planner {
    const bdx_config_t &c;
    const BdxTuning &tune;
    BdxPlanOut &o;
    int cur = 0;  // the set the table builders work on
    const int npass = c.is_dual ? 2 : 1;
    BdxPlanSet &F() { return o.fs[cur]; }

    int fail(int code, const char *fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        o.err = buf;
        return code;
    }
    // the budget of a barcode in the set being built: unit operations, capped by the tier (and, where given, by a cost cap)
    long long budget(long long ae, int m, bool tier_capped = true) const {
        const long long kb = ae / unit_cost(c);
        return tier_capped && kb > tier_cap(m) ? tier_cap(m) : kb;
    }
    long long tier_cap(int m) const;
    int fill_dev();
    int plan_generic();
    void build_bitpar_tables();
    void build_seed_tables(bool strict, bool alt = false);
    void build_diag_tables();
    struct WaveDomain { bool ok = false, split = false, kclass = false, ranged = false; int Btot = 0, cwt = 0; };
    WaveDomain wave_domain(int limit_b, int limit_cw_split, int trace_set);
    void derive_known(const BdxWavePlan &wp, bool split, bool kclass, bool aln_for_exact, bool fits, BdxWavePlan &k, BdxWavePlan &a);
    void build_wave_tables();
    void build_pair_tables();
    void choose_tier_q();
    int run();
};

// ---- the scalar half of the device config ---------------------------------------------------------------------------
int Planner::fill_dev() {
    BdxDevCfg &d = o.dev;
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
    d.force_lds_dp = tune.lds_dp;
    d.band_kb[0] = d.band_kb[1] = -1;  // (everything else per launch starts at 0, like the pass the config does not have)
    d.max_m = 1;
    d.any_traceback = d.need_traceback;
    for (int k = 0; k < npass; ++k) {
        BdxDevPass &P = d.pass[k];
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
        for (int i = 0; i < p.n_barcodes; ++i) d.max_m = std::max(d.max_m, bc_len(p, i));
    }
    d.counts_stride2 = d.is_dual ? (d.pass[1].n_barcodes > 1 ? d.pass[1].n_barcodes : 1) : 1;
    const long long nc = 4LL + (long long)d.pass[0].n_barcodes * d.counts_stride2;
    if (nc > (1LL << 28)) return fail(BDX_E_INVALID, "sample_counts table too large (%lld entries)", nc);
    d.n_counts = (int)nc;
    // allowed_error = floor(rate * normalisation) must stay inside the int32 DP domain
    if (std::fabs(c.max_error_rate) * (double)d.max_m >= (double)(1 << 27))
        return fail(BDX_E_INVALID, "max_error_rate * barcode length exceeds the supported range");
    return BDX_OK;
}

// Launch planning for the exact-evaluation kernel: per-lane DP (+origin) columns, barcode
// tables, count histogram and the read staging area must fit the CU's 160 KiB of LDS.
int Planner::plan_generic() {
    BdxDevCfg &d = o.dev;
    BdxGenericPlan &p = o.plan;
    // what both DP forms below ask of the config's barcodes and ranges
    bool free_ranges = true, same_len = true;
    int len0 = -1, nb = 0;
    size_t bc_total = 0;
    for (int k = 0; k < npass; ++k) {
        const bdx_pass_t &ps = c.pass[k];
        free_ranges = free_ranges && ps.explicit_window == 0 && whole(ps.barcode_start_range) && whole(ps.barcode_end_range);
        for (int b = 0; b < ps.n_barcodes; ++b) {
            if (len0 < 0) len0 = bc_len(ps, b);
            same_len = same_len && bc_len(ps, b) == len0;
        }
        bc_total += ps.bc_off[ps.n_barcodes];
        nb += ps.n_barcodes;
    }
    const bool clean_costs = d.match >= 0 && d.mismatch >= 1 && d.indel >= 1;
    const bool simple_sg = !d.has_nindel && d.algorithm == BDX_ALG_SEMIGLOBAL && !d.force_lds_dp;
    // SimpleScoring barcodes of <= 32 rows run the register-resident DP: no LDS columns at all
    p.reg_rows = simple_sg ? (d.max_m <= 24 ? 24 : (d.max_m <= 32 ? 32 : 0)) : 0;
    // clean class (bdx_core.h sg_core_clean): costs match >= 0, mismatch / indel >= 1, and barcode_start_range /
    // barcode_end_range that resolve to 1:n for every read (no offset from either end) — then neither binds
    p.clean = 0;
    p.uniform_m = 0;
    p.uniform_len = 0;
    if (p.reg_rows && !tune.no_clean && clean_costs) {
        p.clean = free_ranges;
        p.uniform_m = free_ranges && same_len && len0 == p.reg_rows;
        // the diagonal-band bodies exist for these barcode lengths (every barcode of the config alike)
        const bool band_len = len0 == 8 || len0 == 10 || len0 == 12 || len0 == 16 || len0 == 20 || len0 == 24 || len0 == 32;
        p.uniform_len = (free_ranges && same_len && band_len) ? len0 : 0;
    }
    // Barcodes beyond the register DP's 32 rows inside the clean class: the rolling diagonal band (bdx_core.h sg_band_roll) —
    // H = two operation budgets at the configured rate + 9 end columns per chunk — instead of max_m + 1 LDS rows per lane
    // (80-nt barcodes with trimming: 648 B per lane = ONE 128-lane workgroup per CU; 26 cells: two 256-lane workgroups).
    p.band_roll = 0;
    p.same_len = 0;
    d.band_hcap = 0;
    // (only behind a filter: without hand-over windows — filter off, barcodes beyond the sweep's 128 rows — every candidate
    // would be walked over its whole window in chunks, three times the full matrix, where sg_core's cut-off visits a few rows
    // per column: 160-nt barcodes unfiltered 0.3 -> 0.03 M reads/s, measured; run() plans again once the filter is known)
    if (!p.reg_rows && d.max_m > 32 && simple_sg && !tune.no_clean && !o.band_roll_off && !tune.no_band_roll && clean_costs) {
        int kb_max = 0;
        for (int k = 0; k < npass; ++k)
            for (int b = 0; b < c.pass[k].n_barcodes; ++b)  // (the threshold only tightens)
                kb_max = std::max(kb_max, (int)(allowed_error(c, c.pass[k], b, true) / unit_cost(c)));
        // H: at least two budgets + 9 end columns per chunk; up to four budgets + 9 (a clean occurrence has end columns within
        // the budget on either side: one chunk) while two 256-lane workgroups still fit a CU (8 bytes per cell and lane)
        int hcap = 2 * kb_max + 9;
        {
            // (what the workgroup keeps in LDS besides the cells — barcode bytes and tables, the counter histogram — as below)
            const size_t other = (bc_total <= 32 * 1024 ? bc_total : 0) + (size_t)nb * 8 + (size_t)(d.n_counts <= 2048 ? d.n_counts : 2048) * 4 + 256;
            const size_t room = other + 2048 < (size_t)76 * 1024 ? (size_t)76 * 1024 - other - 2048 : 0;
            const int fit2 = (int)(room / (256 * (d.any_traceback ? 8 : 4))) - 1;  // cells per lane of a workgroup that shares the CU with another one
            const int want = 4 * kb_max + 9;
            const int roomy = want < fit2 ? want : fit2;
            if (roomy > hcap) hcap = roomy;
        }
        if (free_ranges && hcap + 1 < d.max_m + 1 && d.max_error_rate >= 0.0 && d.max_error_rate <= 1.0) {
            p.band_roll = 1;
            p.same_len = same_len ? 1 : 0;
            d.band_hcap = hcap;
        }
    }
    p.dp_rows = p.reg_rows ? 1 : (p.band_roll ? d.band_hcap + 1 : d.max_m + 1);
    p.dp_rows_fused = d.max_m + 1;
    const size_t per_thread = (size_t)p.dp_rows * 4 * (d.any_traceback ? 2 : 1);
    const int B0 = d.pass[0].n_barcodes, B1 = d.is_dual ? d.pass[1].n_barcodes : 0;
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
    return fail(BDX_E_INVALID,
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
long long Planner::tier_cap(int m) const {
    if (cur == 0) return (1LL << 40);
    if (o.tier_cap_fixed >= 0) return o.tier_cap_fixed;  // (the pairs tier)
    const int q = o.tier_q >= 5 && o.tier_q <= 8 ? o.tier_q : 8;
    const int cap = m / q - 1;
    return cap > 0 ? cap : 0;
}

// ---- bit-parallel pre-filter: eligibility and tables (see bdx_bitpar.hip for the argument) ----
void Planner::build_bitpar_tables() {
    BdxBitparPlan &bp = F().bplan;
    bp = BdxBitparPlan{};
    bp.tier_slo[0] = bp.tier_slo[1] = HUGE_VAL;
    if (c.filter == BDX_FILTER_OFF) return;
    // cost domain: every edit operation must cost >= 1 and a match >= 0
    const int cmin = unit_cost(c);
    if (c.algorithm == BDX_ALG_SEMIGLOBAL && (c.match < 0 || cmin < 1)) return;
    size_t cand_words = 0, wb = 4;
    for (int k = 0; k < npass; ++k) {
        const bdx_pass_t &p = c.pass[k];
        cand_words += (size_t)(p.n_barcodes + 31) / 32;
        for (int b = 0; b < p.n_barcodes; ++b) {
            const int m = bc_len(p, b);
            if (m > 128) return;  // one sweep word per barcode: 32 bits, 64 for barcodes of 33..64 nt, 128 for 65..128 nt
            if (m > 64) wb = 16;
            else if (m > 32 && wb < 8) wb = 8;
        }
    }
    // alphabet = distinct barcode bytes (<= 15: the IUPAC letters), everything else shares the "other" code
    int code_of[256], K;
    if (!code_alphabet(c, code_of, K, 15)) return;
    if (cand_words > 128) return;  // <= 4096 barcodes per config (both passes together)
    bp.ncodes = K + 1;
    bp.ncode_N = code_of['N'] >= 0 ? code_of['N'] : 255;
    std::vector<uint8_t> lut(256);
    for (int i = 0; i < 256; ++i) lut[i] = (uint8_t)(code_of[i] < 0 ? K : code_of[i]);
    bp.word_bytes = (int)wb;
    for (int k = 0; k < npass; ++k) {
        bp.bpad[k] = 32;  // power of two >= B: peq row address = code << log2(4*bpad)
        while (bp.bpad[k] < c.pass[k].n_barcodes) bp.bpad[k] <<= 1;
        if ((size_t)bp.ncodes * bp.bpad[k] * wb > 96 * 1024) return;  // the table lives in LDS
    }
    BdxBlob &blob = ((F().bp_tables) = BdxBlob{});  // (no return from here on)
    BdxBitparOff &off = F().bp_off;
    off.lut = blob.put(lut);
    std::vector<int32_t> kb[2];
    for (int k = 0; k < npass; ++k) {
        const bdx_pass_t &p = c.pass[k];
        std::vector<uint8_t> peq((size_t)bp.ncodes * bp.bpad[k] * wb, 0), pv((size_t)p.n_barcodes * wb, 0);
        kb[k].assign((size_t)p.n_barcodes, 0);
        const int bits = (int)wb * 8;
        bp.kb_uniform[k] = -2;  // (unset)
        typedef unsigned __int128 u128;
        const auto put = [&](std::vector<uint8_t> &dst, size_t idx, u128 v) { memcpy(dst.data() + idx * wb, &v, wb); };  // (little endian: the low bytes)
        for (int b = 0; b < p.n_barcodes; ++b) {
            const int m = bc_len(p, b);
            const int shift = bits - m;
            const u128 all = bits == 128 ? ~(u128)0 : (((u128)1 << bits) - 1);
            const u128 rows = m == bits ? all : ((((u128)1 << m) - 1) << shift);
            const u128 pad = ~rows & all;  // virtual rows below the barcode: match everything, D stays 0
            put(pv, (size_t)b, rows);
            for (int code = 0; code < bp.ncodes; ++code) {
                u128 mask = pad;
                for (int i = 0; i < m; ++i) {
                    const uint8_t ch = p.bc_bytes[p.bc_off[b] + i];
                    const bool wild = n_wildcards(c) && ch == 'N';
                    if (wild || (code < K && code_of[ch] == code)) mask |= (u128)1 << (shift + i);
                }
                put(peq, (size_t)code * bp.bpad[k] + b, mask);
            }
            const long long ae = allowed_error(c, p, b);
            const long long kfull = ae < 0 ? -1 : ae / cmin;
            const long long kcap = std::min(kfull, tier_cap(m));
            kb[k][b] = (int32_t)kcap;
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
        blob.align(16);
        off.peq[k] = blob.put(peq);
        off.pvinit[k] = blob.put(pv);
        off.kb[k] = blob.put(kb[k]);
    }
    // Reducer replay capacity: short barcodes at high rates have many GENUINE candidates per read (a 10-mer within two
    // edits of a random 150-base read is common: ~25 of 96 barcodes), and a read with more survivors than the replay
    // holds costs a full exact DP per candidate.  Expected candidates per read ~ sum over barcodes of
    // 150 * V(m, kb) / 4^m with V = sum_{e <= kb} C(m, e) 8^e (3 substitutions, 4 insertions, 1 deletion per site).
    {
        double expected = 0.0;
        int total_b = 0;
        for (int k = 0; k < npass; ++k) {
            const bdx_pass_t &p = c.pass[k];
            total_b += p.n_barcodes;
            for (int b = 0; b < p.n_barcodes; ++b) {
                const int m = bc_len(p, b);
                if (kb[k][b] < 0 || m > 20) continue;
                double v = 0.0, term = 1.0;
                for (int e = 0; e <= kb[k][b] && e <= m; ++e) {
                    v += term;
                    term *= 8.0 * (double)(m - e) / (double)(e + 1);
                }
                expected += 150.0 * v / std::pow(4.0, (double)m);
            }
        }
        bp.slot_cap = expected < 1.0 ? 4 : expected < 2.5 ? 8 : expected < 8.0 ? 16 : 32;
        bp.dense_d = expected >= 1.0 && total_b <= 256 && !tune.no_dense;  // (used by the kernels without seeds only; they then keep four slots)
    }
    // known-score class (config level): SimpleScoring with unit costs, ScoreOnly output.
    // (:exact with whole ranges IS the class at a budget of 0: exact_align, classification.jl:485-548, returns (0.0, s, s + m - 1)
    // for an occurrence — the leftmost, or the rightmost with trim_side = 3 — else Inf: the value, the end of the first column
    // at distance 0 and the largest origin of a distance-0 alignment; raw bytes are compared, N is a literal: SimpleScoring.
    // With a ref_search_range its meaning differs — allowed START positions, SURVEY Q11 — so only whole ranges qualify.)
    for (int k = 0; k < npass; ++k) {
        const bdx_pass_t &p = c.pass[k];
        const bool score_only = p.trim_side == 0 && !c.need_traceback;
        const bool unit_sg = c.algorithm == BDX_ALG_SEMIGLOBAL && !c.has_nindel && c.match == 0 && c.mismatch == 1 && c.indel == 1;
        const bool exact_whole = c.algorithm == BDX_ALG_EXACT && p.explicit_window == 0 && whole(p.ref_search_range) &&
                                 whole(p.barcode_start_range) && whole(p.barcode_end_range) && !tune.no_known_exact;
        bp.known_ok[k] = (unit_sg || exact_whole) && score_only && p.explicit_window != BDX_WINDOW_ALIGN_ONE && !tune.no_known;
    }
    bp.enabled = 1;
}

// ---- q-gram seeding (pigeonhole) in front of the sweep -------------------------------------
// A recordable alignment of barcode b has at most kb[b] edit operations (see the sweep), so of
// kb[b]+1 disjoint pieces of the barcode at least one occurs in the read unchanged; a fortiori
// the first q bases of that piece do.  Pairs without any such seed hit cannot be candidates and
// are not swept.  Keys use 2 bits per base (symbol code & 3): equal bytes give equal keys, other
// bytes may alias — that only adds sweeps, never removes one.
void Planner::build_seed_tables(bool strict, bool alt) {
    BdxSeedPlan &sp = alt ? F().splan_alt : F().splan;
    sp = BdxSeedPlan{};
    if (!F().bplan.enabled || c.filter == BDX_FILTER_BITPAR || tune.no_seed) return;
    int code_of[256], K;  // same symbol coding as the sweep
    code_alphabet(c, code_of, K, 256);
    struct Piece { int pass, b, start; };
    std::vector<Piece> pieces;
    std::vector<uint16_t> always[2];
    int q = 8;
    int total_bc = 0;
    for (int k = 0; k < npass; ++k) {
        const bdx_pass_t &p = c.pass[k];
        if (p.n_barcodes > 32767) return;
        total_bc += p.n_barcodes;
        for (int b = 0; b < p.n_barcodes; ++b) {
            const int m = bc_len(p, b);
            const long long ae = allowed_error(c, p, b);
            if (ae < 0) continue;  // can never be recorded: neither seeded nor swept
            const long long kb = budget(ae, m);
            const long long L = m / (kb + 1);
            if (has_wildcard(c, p, b) || L < 5) {
                always[k].push_back((uint16_t)b);
                continue;
            }
            if (L < q) q = (int)L;
            for (long long t = 0; t <= kb; ++t) pieces.push_back(Piece{k, b, (int)(t * L)});
        }
    }
    if (pieces.empty()) return;
    if ((int)(always[0].size() + always[1].size()) * 4 > total_bc) return;  // seeding would not pay
    if (pieces.size() > 16384) return;
    // selectivity: expected seed-hit pairs per read of ~150 bases must be well below B
    const double space = std::pow(4.0, q);
    const double expected = 150.0 * (double)pieces.size() / space + 1.0 + (double)(always[0].size() + always[1].size());
    if (expected * 3.0 > (double)total_bc) return;
    // strict: single seeds only when they are really selective (q = 7, 8 in practice).  With ~14 falsely
    // seeded barcodes per read (q = 6 at B = 96) the hit queue / record tables cost more than the
    // two-intact-pieces variant, which is tried next (measured at kb = 3: 7.5 ms vs 5.7 ms per 2 M reads).
    if (strict && expected > 7.0) return;
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
    if (tune.seed_bm_log2 > 0) sp.bm_log2 = tune.seed_bm_log2 < 2 * q ? tune.seed_bm_log2 : 2 * q;
    sp.bm_words = (1 << sp.bm_log2) / 32;
    sp.hash_log2 = 8;
    while ((1u << sp.hash_log2) < pieces.size() * 2) sp.hash_log2++;
    sp.hash_in_lds = ((size_t)5 << sp.hash_log2) <= 8 * 1024;  // larger tables are probed in L2 (a few probes per read)
    if (tune.seed_hash_l2) sp.hash_in_lds = 0;
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
    BdxBlob &blob = ((alt ? F().seed_tables_alt : F().seed_tables) = BdxBlob{});  // (no return from here on)
    BdxSeedOff &off = alt ? F().seed_alt_off : F().seed_off;
    off.bitmap = blob.put(bitmap);
    off.hash = blob.put(hash);
    off.hash_ps = blob.put(hash_ps, 16);
    for (int k = 0; k < 2; ++k) {
        sp.n_always[k] = (int)always[k].size();
        off.always[k] = blob.put(always[k], 16);
    }
    blob.bytes.resize(blob.bytes.size() + 16, 0);
    sp.enabled = 1;
}

// ---- two-intact-pieces ("diagonal") seeding for budgets where single pieces are too short -----
// With kb operations allowed, kb+2 disjoint pieces of the barcode leave at least TWO untouched; they
// occur in the read on diagonals (read position - barcode offset) that differ by at most kb (the
// indels between them), and the alignment starts within kb of either diagonal.  The kernel keeps,
// per read, an inverted index of its 4-mers (256 keys x position bits) and tests every (read,
// barcode) pair with a handful of word operations per piece; only pairs with two such pieces are
// swept, over the columns [d_min - kb - 1, d_max + m + kb + 1).  Lossless for the same reason as the
// single-piece seeds: it only skips pairs whose unit distance exceeds kb.
void Planner::build_diag_tables() {
    BdxSeedPlan &sp = F().splan;
    if (sp.enabled || !F().bplan.enabled || c.filter == BDX_FILTER_BITPAR || tune.no_seed || tune.no_diag ||
        F().bplan.word_bytes != 4)  // (the diagonal variant has 32-bit sweep words)
        return;
    int code_of[256], K;
    code_alphabet(c, code_of, K, 256);
    std::vector<uint32_t> meta[2], keys[2];
    std::vector<uint16_t> always[2];
    int total_bc = 0, kmax = 0;
    double flagged = 0.0;  // expected falsely flagged pairs per read of ~150 bases
    double flag_coef = 0.0;
    for (int k = 0; k < npass; ++k) {
        const bdx_pass_t &p = c.pass[k];
        if (p.n_barcodes > 32767) return;
        total_bc += p.n_barcodes;
        meta[k].assign((size_t)p.n_barcodes, 0u);
        keys[k].assign((size_t)p.n_barcodes * 2, 0u);
        for (int b = 0; b < p.n_barcodes; ++b) {
            const int m = bc_len(p, b);
            const long long ae = allowed_error(c, p, b);
            if (ae < 0) continue;  // can never be recorded: neither seeded nor swept (meta 0 and not in `always`)
            const long long kb = budget(ae, m, false);  // (a capped set never gets here: its seeds are single pieces)
            const long long P = kb + 2;
            const long long L = m / P;
            if (has_wildcard(c, p, b) || L < 4 || P > 8 || kb > 6 || (P - 1) * L > 28) {
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
    if (n_always == (size_t)total_bc) return;
    if (n_always * 4 > (size_t)total_bc) return;
    // worth it only if clearly fewer pairs are swept (a flagged pair costs ~ a quarter of a whole-read sweep)
    if ((flagged + (double)n_always) * 2.0 > (double)total_bc) return;
    // ... and only for enough barcodes: the index forces 4..8-read tiles, whose per-tile latency costs about
    // as much as sweeping ~40 barcodes over a whole 150-base read (measured: 1.44 us/read + 0.017 us/pair
    // against 0.054 us/pair of the plain sweep)
    if (total_bc < tune.diag_min_b) return;  // 48 unless overridden for tuning experiments
    sp = BdxSeedPlan{};
    sp.diag_flag_coef = flag_coef;
    BdxBlob &blob = ((F().seed_tables) = BdxBlob{});  // (no return from here on)
    BdxSeedOff &off = F().seed_off;
    for (int k = 0; k < 2; ++k) {
        off.dmeta[k] = blob.put(meta[k], 16);
        off.dkeys[k] = blob.put(keys[k], 16);
        sp.n_always[k] = (int)always[k].size();
        off.always[k] = blob.put(always[k], 16);
    }
    blob.bytes.resize(blob.bytes.size() + 16, 0);
    sp.q = 4;
    sp.diag = 1;
    sp.diag_kmax = kmax;
    sp.rcap = 8;
    sp.enabled = 1;
}

// ---- what the wave kernel and its pairs mode ask of a config -------------------------------------------------------------
// Barcodes of plain A / C / G / T, SimpleScoring, and ranges that resolve to 1:n for every read (then final_search_range =
// 1:n, max_start_pos = n, min_end_pos = 1: neither binds); at most limit_b barcodes, and limit_cw_split
// candidate words in split mode.  (developer aid: with BDX_TRACE_LAUNCH set, the planner says where it turned a filter set
// away from the wave tables; trace_set < 0: silent)
#define WAVE_NO(ret) return ((tune.trace_launch && trace_set >= 0) ? (void)fprintf(stderr, "[bdx] no wave tables for set %d: bdx_plan.cpp:%d\n", trace_set, __LINE__) : (void)0, ret)
Planner::WaveDomain Planner::wave_domain(int limit_b, int limit_cw_split, int trace_set) {
    const BdxBitparPlan &bp = F().bplan;
    WaveDomain w;
    if (tune.no_wave || !bp.enabled || bp.word_bytes != 4 || (c.algorithm == BDX_ALG_SEMIGLOBAL && c.has_nindel)) WAVE_NO(w);
    // known-score configs: the kernel replays the reducer itself (single pass); everything else in the filters' domain:
    // "split" — it only filters, candidate masks and column windows go to the exact kernel (either pass count)
    for (int k = 0; k < npass; ++k) w.split |= !bp.known_ok[k];
    // :hamming / :exact (always split: their scans run in the exact kernel, restricted to the hand-over windows): the
    // budget is floor(rate * m) substitutions / 0, one operation costs 1
    const bool sgm = c.algorithm == BDX_ALG_SEMIGLOBAL;
    // the known classes' config condition: unit-cost SimpleScoring, or :exact (whole ranges: checked below / in build_bitpar_tables)
    w.kclass = (sgm && !c.has_nindel && c.match == 0 && c.mismatch == 1 && c.indel == 1) || (c.algorithm == BDX_ALG_EXACT && !tune.no_known_exact);
    if (unit_cost(c) < 1 || (sgm && c.match < 0)) WAVE_NO(w);
    for (int k = 0; k < npass; ++k) {
        const bdx_pass_t &p = c.pass[k];
        // (a ref_search_range is allowed for :semiglobal: the kernel resolves every read's column window itself, classification.jl:795-807;
        // start / end ranges that could bind stay on the general kernel)
        if (p.explicit_window != 0 || !whole(p.barcode_start_range) || !whole(p.barcode_end_range)) WAVE_NO(w);
        if (!whole(p.ref_search_range)) {
            if (!sgm) WAVE_NO(w);
            w.ranged = true;
        }
        if (p.n_barcodes < 1) WAVE_NO(w);
        for (uint32_t i = 0; i < p.bc_off[p.n_barcodes]; ++i) {
            const uint8_t ch = p.bc_bytes[i];
            if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') WAVE_NO(w);
        }
        for (int b = 0; b < p.n_barcodes; ++b)
            if (bc_len(p, b) < 1 || bc_len(p, b) > 32) WAVE_NO(w);
        w.Btot += p.n_barcodes;
        w.cwt += (p.n_barcodes + 31) / 32;
    }
    if (w.Btot > limit_b || (w.split && w.cwt > limit_cw_split)) WAVE_NO(w);
    w.ok = true;
    return w;
}

// Known-trim class: the known-score conditions with a trim side in some pass (either pass count, no summary).  What a trim
// side makes observable is one position per pass — trim_side = 5: the alignment's END (keep_start = end + 1,
// classification.jl:912-914; the reference keeps the leftmost end of the best score, :142-153: strict `<`); trim_side = 3: its
// START (keep_end = max(1, start) - 1, :910-911; the largest start among the alignments of the best score, :142-153 tie rule
// + :310-321 origin order) — and the sweep delivers both (bdx_wave.hip, KEND: the lowering mask of a left-to-right sweep /
// of a right-to-left sweep with the reversed barcode).  Such a config gets its verdicts from the non-split kernel whenever
// the caller does not ask for per-pass start positions (nor for end positions of a trim_side = 3 pass).
// Known-alignment class: the same conditions with `summary` allowed — start AND end of every pass's winner come out of one
// more (anchored) sweep per pass and read, so per-pass positions and the DemuxStats histograms need no exact kernel either
// (bdx_wave_aln.hip); taken per launch when the caller wants positions the known-trim class does not know, or statistics.
// fits: what the form at hand (wave / pairs) asks beyond the class.  aln_for_exact: :exact reports the occurrence's positions
// whatever the output policy (classification.jl:485-548), so its score-only form only serves callers that do not ask for
// them — the others take the known-alignment class per launch (wave tables only).
void Planner::derive_known(const BdxWavePlan &wp, bool split, bool kclass, bool aln_for_exact, bool fits, BdxWavePlan &k, BdxWavePlan &a) {
    k = a = BdxWavePlan{};
    bool ok = kclass && fits && !tune.no_known && !tune.no_kend;
    for (int p = 0; p < npass; ++p) ok = ok && c.pass[p].explicit_window != BDX_WINDOW_ALIGN_ONE;
    if (!ok) return;
    BdxWavePlan known = wp;
    known.split = 0;
    known.cand_words = c.is_dual ? 4 : 0;  // (the four survivor slots of pass 1)
    if (split && !c.need_traceback) {
        k = known;
        k.kend = 1;
        for (int p = 0; p < npass; ++p)
            if (c.pass[p].trim_side == 3) k.kend = 2;  // (reversed sweeps: bdx_wave_rev.hip)
    }
    if ((split || (aln_for_exact && c.algorithm == BDX_ALG_EXACT)) && !tune.no_kaln) {
        a = known;
        a.kend = 3;
    }
}

// ---- wave-autonomous kernel (bdx_wave.hip): tables of one filter set ------------------------------
// Eligible: wave_domain, strict single seeds for every barcode (no barcode swept unconditionally), at most 1024 barcodes.
// Same pieces, keys and budgets as build_seed_tables / build_bitpar_tables of the set — only the symbol
// coding differs: the kernel transcodes arithmetically, code = (byte >> 1) & 3 (A 0, C 1, T 2, G 3).
void Planner::build_wave_tables() {
    const int trace_set = cur;
    BdxWavePlan &wp = F().wplan;
    wp = BdxWavePlan{};
    const BdxBitparPlan &bp = F().bplan;
    const BdxSeedPlan &sp = F().splan;
    if (!sp.enabled || sp.diag || sp.n_always[0] != 0 || sp.n_always[1] != 0 || sp.q < 6 || sp.q > 8) WAVE_NO((void)0);
    const auto [eligible, split, kclass, ranged, Btot, cwt] = wave_domain(1024, 16, cur);  // (split mode keeps the candidate words of a read in LDS: up to 512 barcodes)
    if (!eligible) return;
    const int q = sp.q;
    struct Piece { int g, start; const uint8_t *bc; };
    std::vector<Piece> pieces;
    std::vector<uint32_t> meta((size_t)Btot, 0u), peq8((size_t)Btot * 9, 0u), settle((size_t)Btot, 0u);  // (stride 9: bank spread, see the kernel)
    std::vector<uint32_t> peq8r((size_t)Btot * 9, 0u);  // the reversed barcodes (known-trim class: trim_side = 3 passes are swept right to left)
    int track = 1 << 20, g = 0;
    for (int k = 0; k < npass; ++k) {
        const bdx_pass_t &p = c.pass[k];
        for (int b = 0; b < p.n_barcodes; ++b, ++g) {
            const int m = bc_len(p, b);
            const uint8_t *bc = p.bc_bytes + p.bc_off[b];
            peq8_rows(bc, m, false, &peq8[(size_t)g * 9]);
            peq8_rows(bc, m, true, &peq8r[(size_t)g * 9]);
            const long long ae = allowed_error(c, p, b, true);
            if (ae < 0) {  // can never be recorded: neither seeded nor swept (budget field 255)
                meta[(size_t)g] = (uint32_t)m | (255u << 8) | (255u << 16);
                continue;
            }
            const long long kb = budget(ae, m);
            if (kb > 15) WAVE_NO((void)0);  // (a record keeps the diagonals of its hits as 2 kb + 1 bits)
            const long long L = m / (kb + 1);
            if (L < q) WAVE_NO((void)0);  // (cannot happen: the set's q is the shortest piece)
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
    if (pieces.empty() || pieces.size() > 8192) WAVE_NO((void)0);
    // the per-read record table holds eight (barcode, diagonal cluster) records: the planted one(s) plus the chance pairs must nearly always fit
    {
        // chance seed hits per 150-base read: the hit queue and the sweep list of a tile are sized from it (size_wave)
        // (measured, 24-nt barcodes, 2 M reads: B = 192 / 384 / 768 at rate 0.1 — chance 1.3 / 2.6 / 5.3 — 1.99 -> 4.85, 1.49 -> 3.52,
        // 0.94 -> 1.62 G reads/s against the general kernel; as tier 1 of rate 0.2: 0.92 -> 1.22, 0.50 -> 0.64, 0.25 -> 0.17: whatever
        // overflows there costs a full-budget evaluation)
        const double limit = std::isnan(tune.wave_chance) ? (cur == 1 ? 3.0 : 6.0) : tune.wave_chance;
        wp.chance = 150.0 * (double)pieces.size() / std::pow(4.0, (double)q);
        if (wp.chance > limit) WAVE_NO((void)0);
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
    {
        std::vector<size_t> head_of;  // index into ents of every head
        for (size_t i = 0; i < ents.size(); ++i)
            if (i == 0 || ents[i].key != ents[i - 1].key) head_of.push_back(i);
        const size_t D = head_of.size();
        if (ents.size() >= 65536) WAVE_NO((void)0);
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
    if (bdx_wave_table_bytes(wp, o.plan.hist_entries) > 64 * 1024) WAVE_NO((void)0);
    BdxBlob &blob = ((F().wave_tables) = BdxBlob{});  // (no return from here on)
    BdxWaveOff &off = F().wave_off;
    off.bitmap = blob.put(bitmap, 64);
    off.rank = blob.put(rank, 64);
    off.ent = blob.put(ent, 64);
    off.peq8 = blob.put(peq8, 64);
    off.meta = blob.put(meta, 64);
    off.settle = blob.put(settle, 64);
    off.peq8r = blob.put(peq8r, 64);
    wp.enabled = 1;
    bool fits = c.pass[0].n_barcodes <= 1023 && (!c.is_dual || c.pass[1].n_barcodes <= 1023);  // entry = barcode << 22 | d << 16 | position key
    for (uint32_t x : meta) fits = fits && (((x >> 8) & 255u) == 255u || ((x >> 8) & 255u) < 64u);
    derive_known(wp, split, kclass, true, fits, F().wplan_k, F().wplan_a);
}
#undef WAVE_NO

// ---- pairs mode of the wave kernel (bdx_pairs.hip): tables of the FULL-budget set --------------------------------
// Between tier 1 and the general kernel of a tiered config: the reads tier 1 lists are gathered into slots and filtered
// by the two-intact-pieces lemma on barcode masks (one table entry per (piece, 4-base key): the barcodes whose piece has
// that key).  Eligible: wave_domain; every barcode's budget kb at most 4 with 4 (kb + 2) <= m (kb + 2 disjoint 4-base
// pieces at offsets 0, 4, ..); at most 128 barcodes.
void Planner::build_pair_tables() {
    BdxWavePlan &wp = F().pplan;
    wp = BdxWavePlan{};
    // (a capped set gets pair tables only as the pairs tier: budgets capped at tier_cap_fixed operations)
    if (tune.no_pairs || (F().bplan.tier_capped && o.tier_cap_fixed < 0) || c.filter != BDX_FILTER_AUTO) return;
    // more than 128 barcodes (known-score configs only: split mode keeps four mask words per read): groups of 128 barcodes,
    // each with its own piece tables of four-word masks
    const auto [eligible, split, kclass, ranged, Btot, cwt] = wave_domain(512, 4, -1);
    if (!eligible || (split && Btot > 128)) return;
    const bool sgm = c.algorithm == BDX_ALG_SEMIGLOBAL;
    const int cmin = unit_cost(c);
    // the pairs tier (capped set): the filter only has to be lossless for alignments of COST <= cap x cmin — a barcode it does not
    // flag costs more, i.e. at least (cap + 1) cmin = the tier's slo (costs are integers; the tier exists for mismatch = cmin = 1)
    const long long cost_cap = (cur == 1 && o.tier_cap_fixed >= 0) ? (long long)o.tier_cap_fixed * cmin : (1LL << 40);
    const auto capped_ae = [&](const bdx_pass_t &p, int b) { return std::min(cost_cap, allowed_error(c, p, b, true)); };
    const int groups = (Btot + 127) / 128;
    int nw = groups > 1 ? 4 : (Btot + 31) / 32;
    nw = std::min(4, std::max(nw, tune.pairs_nw));
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
            const long long ae = capped_ae(c.pass[k], b);
            if (ae >= 0 && (ae / cmin > 4 || 4 * (ae / cmin + 2) > bc_len(c.pass[k], b))) classic_ok = false;
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
                    const int m = bc_len(p, b);
                    const long long ae = capped_ae(p, b);
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
            const int m = bc_len(p, b);
            const uint8_t *bc = p.bc_bytes + p.bc_off[b];
            peq8_rows(bc, m, false, &peq8[(size_t)g * 9]);
            peq8_rows(bc, m, true, &peq8r[(size_t)g * 9]);  // (the reversed barcode: known-trim class, see derive_known)
            const long long ae = capped_ae(p, b);
            if (ae < 0) {  // can never be recorded: in no table entry, never swept
                meta[(size_t)g] = (uint32_t)m | (255u << 8) | (255u << 16);
                continue;
            }
            const long long kb = budget(ae, m, false);  // (the cost cap above is the tier's cap)
            if (!sd_pl && (kb > 4 || 4 * (kb + 2) > m)) return;
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
    if (bcs.empty() || track < 12) return;
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
    if (bdx_wave_table_bytes(wp, o.plan.hist_entries) > 112 * 1024) return;  // (at least four waves' work areas must fit beside the tables)
    BdxBlob &blob = ((F().pair_tables) = BdxBlob{});  // (no return from here on)
    BdxWaveOff &off = F().pair_off;
    off.bitmap = off.rank = off.ent = blob.put(tab, 64);  // (rank and entries are never read)
    off.peq8 = blob.put(peq8, 64);
    off.meta = blob.put(meta, 64);
    off.settle = blob.put(settle, 64);
    off.peq8r = blob.put(peq8r, 64);
    o.pair_mmin = mmin;
    wp.enabled = 1;
    // the listed reads of a config with trim sides get verdict and keep range from the pairs mode too, in its non-split form
    // (the same-diagonal variants only exist in split mode)
    derive_known(wp, split, kclass, false, groups == 1 && wp.pairs_kb <= 4, F().pplan_k, F().pplan_a);
}

// Piece length behind tier 1's capped budgets, cap(m) = m / q - 1: 8-base seeds are the most selective; 7- or
// 6-base pieces raise the cap of some lengths by one (14-15 and 21-23 bases with q = 7, 12-13 with q = 6), so
// that tier 1 settles reads with one more error and tier 0 — a plain sweep or the two-intact-pieces kernel —
// sees far fewer reads (m = 14, B = 96, rate 0.2: 444 -> 724 M reads/s), as long as the chance hits per
// read stay few and no cap goes beyond 2 (measured: caps of 3 — m = 24 with q = 6, m = 28 with q = 7 — cost
// more in tier 1 than they save in tier 0, at 24 and at 96 barcodes).
void Planner::choose_tier_q() {
    long long best_caps = -1;
    int best_q = 8;
    const double limit[9] = {0, 0, 0, 0, 0, 0, 8.0, 4.0, 1e30};
    for (int q = 8; q >= 6; --q) {
        long long caps = 0, pieces = 0, cap_max = 0;
        for (int k = 0; k < npass; ++k)
            for (int b = 0; b < c.pass[k].n_barcodes; ++b) {
                const long long ae = allowed_error(c, c.pass[k], b);
                if (ae < 0) continue;
                const long long cap = std::min(std::max(0LL, (long long)bc_len(c.pass[k], b) / q - 1), ae / unit_cost(c));
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
    o.tier_q = tune.tier_q >= 5 && tune.tier_q <= 8 ? tune.tier_q : best_q;
}

// ---- the tier sequence: which builders run for which set --------------------------------------------------------------
int Planner::run() {
    int rc = fill_dev();
    if (rc == BDX_OK) rc = plan_generic();  // needs the caller's host tables
    if (rc != BDX_OK) return rc;
    build_bitpar_tables();
    if (o.plan.band_roll && !F().bplan.enabled) {  // no filter, no hand-over windows: the rolling band would walk whole windows
        o.band_roll_off = true;
        rc = plan_generic();
        if (rc != BDX_OK) return rc;
    }
    build_seed_tables(true);
    build_diag_tables();
    if (!F().splan.enabled) build_seed_tables(false);  // neither: moderately selective single seeds still beat sweeping every pair
    else if (F().splan.diag) build_seed_tables(false, true);  // the fallback of size_bitpar when the index does not fit a batch
    build_wave_tables();
    build_pair_tables();
    // tier 1 (capped budgets, strict single seeds) beside a full-budget set that is NOT already strict single seeds
    const BdxPlanSet &full = o.fs[0];
    BdxPlanSet &t1 = o.fs[1];
    const bool strict_full = full.splan.enabled && !full.splan.diag && full.splan.q >= 7;
    // (the unit-level API's hand-made windows stay on the plain path)
    bool plain_windows = true, wild_N = false;
    for (int k = 0; k < npass; ++k) {
        plain_windows = plain_windows && c.pass[k].explicit_window == 0;
        // N-scoring with real wildcards: position-dependent indel costs — "an alignment's result does not depend on
        // the running threshold" is only argued (and fuzzed) for uniform costs; such configs stay on one tier
        if (c.algorithm == BDX_ALG_SEMIGLOBAL && c.has_nindel)
            for (int b = 0; b < c.pass[k].n_barcodes; ++b) wild_N = wild_N || has_wildcard(c, c.pass[k], b);
    }
    if (full.bplan.enabled && plain_windows && !wild_N && !strict_full && !tune.no_tier && c.filter == BDX_FILTER_AUTO) {
        choose_tier_q();
        cur = 1;
        build_bitpar_tables();
        if (t1.bplan.enabled && t1.bplan.tier_capped) {
            build_seed_tables(true);
            // very many barcodes: moderately selective 8-base seeds (a dozen chance pairs per read) still beat
            // the full-budget filter by far
            if (!t1.splan.enabled) build_seed_tables(false);
            if (t1.splan.enabled && t1.splan.q < o.tier_q) t1.splan.enabled = 0;
            build_wave_tables();
        }
        cur = 0;
        o.tiered = t1.bplan.enabled && t1.bplan.tier_capped && t1.splan.enabled;
        // with_delta and a min_delta beyond the score of an unseen barcode: not even a perfect match can be
        // proven unambiguous at the capped budgets (only a visible runner-up could settle a read) — tier 1
        // would be a pass over the whole batch for next to nothing
        if (o.tiered && c.min_delta != 0.0)
            for (int k = 0; k < npass; ++k)
                if (!(t1.bplan.tier_slo[k] >= c.min_delta)) o.tiered = 0;
    }
    // The PAIRS TIER: a split config with min_delta whose seed tier proves nothing (above), mismatch = cmin = 1 and indels dearer —
    // the reference's demo2 options (mismatch 1, indel 2, rate 0.25, min_delta 0.15): tier 1 = the same-diagonal pairs mode with
    // six 4-base pieces over the WHOLE batch at budgets capped at 4 (3) operations — ~3 chance flags per read instead of the ~90 of
    // the full-budget variant — followed by the exact kernel, which settles every read whose winner leaves min_delta of room below
    // slo = (cap + 1) / m (a perfect match or one mismatch under demo2's options: ~75 % of the reads) and lists the rest for tier 0.
    if (!o.tiered && full.bplan.enabled && full.pplan.enabled && full.pplan.split && !tune.no_tier && !tune.no_pairs &&
        c.filter == BDX_FILTER_AUTO && c.algorithm == BDX_ALG_SEMIGLOBAL && !c.has_nindel && c.mismatch == 1 &&
        c.indel >= 2 && c.match == 0 && c.min_delta != 0.0) {
        for (int cap = 4; cap >= 3 && plain_windows && !o.tiered; --cap) {
            o.tier_cap_fixed = cap;
            cur = 1;
            t1.splan = BdxSeedPlan{};
            t1.wplan = BdxWavePlan{};
            build_bitpar_tables();
            bool ok = t1.bplan.enabled && t1.bplan.tier_capped;
            for (int k = 0; ok && k < npass; ++k) ok = t1.bplan.tier_slo[k] >= c.min_delta;
            if (ok) build_pair_tables();
            ok = ok && t1.pplan.enabled && t1.pplan.pairs_kb == 8 && t1.pplan.split;
            cur = 0;
            if (ok) {
                o.tiered = o.pairs_tier = 1;
            } else {
                o.tier_cap_fixed = -1;
                t1.bplan.enabled = 0;
            }
        }
    }
    o.path = full.bplan.enabled ? (full.splan.enabled ? (full.splan.diag ? "qgram2+bitpar+verify" : "qgram+bitpar+verify") : "bitpar+verify") : "generic";
    if (o.tiered) o.path = "tier1:qgram+bitpar > " + o.path;
    o.filter_used = full.bplan.enabled ? (full.splan.enabled ? BDX_FILTER_QGRAM : BDX_FILTER_BITPAR) : BDX_FILTER_OFF;
    return BDX_OK;
}

}  // namespace

int bdx_plan(const bdx_config_t &c, const BdxTuning &tune, int n_cu, BdxPlanOut &out) {
    out = BdxPlanOut{};
    Planner p{c, tune, out};
    const int rc = p.run();
    out.plan.n_cu = n_cu;
    return rc;
}
