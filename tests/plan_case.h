// plan_case.h — what the stand-alone planner drivers share (tests/plan_host.cpp, tests/call_host.cpp): the case file that
// tests/plan_cases.py writes, and the report of every non-pointer field of the create-time planner's output.
//
// case file, one token list per line:
//   case NAME | cfg algorithm is_dual rate min_delta match mismatch indel has_nindel nindel need_traceback filter | tune KEY VALUE
//   pass trim_side explicit_window win_first win_last win_max_start win_min_end <3 ranges: start end start_from_end end_from_end> B
//   bc SEQ LEN_NO_N (B of them after their pass) | call N_READS READ_LEN WINDOW_UPLOAD WANTED STATS (call_host.cpp only) | end
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bdx_plan.h"

static FILE *g_report = stdout;  // where the report goes (call_host.cpp digests one through a memory stream)

struct Case {
    std::string name;
    bdx_config_t cfg;
    BdxTuning tune;
    int n_cu = 256;
    std::vector<std::pair<std::string, std::string>> tune_kv;
    std::vector<std::string> calls;  // the `call` lines, unparsed
    uint8_t *bytes[2] = {nullptr, nullptr};
    uint32_t *off[2] = {nullptr, nullptr};
    int32_t *nn[2] = {nullptr, nullptr};
    void release() {
        for (int k = 0; k < 2; ++k) {
            free(bytes[k]);
            free(off[k]);
            free(nn[k]);
        }
    }
};

static bool set_tuning(Case &cs, const std::string &key, const std::string &val) {
    BdxTuning &t = cs.tune;
#define T(f) if (key == #f) { t.f = atoi(val.c_str()); return true; }
    T(no_known) T(no_seed) T(no_diag) T(lds_dp) T(diag_min_b) T(seed_hash_l2) T(seed_bm_log2) T(no_clean) T(tier_q) T(no_dense)
    T(no_kend) T(no_pairs) T(no_wave) T(no_tier) T(no_band_roll) T(no_known_exact) T(no_kaln) T(pairs_nw)
    T(no_win) T(no_carry) T(no_windows) T(no_slot) T(tier0_div) T(wave_rw) T(wave_waves) T(wave_maxres) T(bitpar_r)
#undef T
    if (key == "grid") { t.grid = atoll(val.c_str()); return true; }
    if (key == "wave_chance") { t.wave_chance = atof(val.c_str()); return true; }
    if (key == "n_cu") { cs.n_cu = atoi(val.c_str()); return true; }
    return false;
}

static bool read_case(FILE *f, Case &cs) {
    char line[1 << 16];
    int pass = -1;
    std::vector<uint8_t> bytes[2];
    std::vector<uint32_t> off[2];
    std::vector<int32_t> nn[2];
    bool open = false;
    while (fgets(line, sizeof line, f)) {
        char word[64] = "", a[1 << 15] = "", b[64] = "";
        if (sscanf(line, "%63s", word) != 1) continue;
        const std::string w = word;
        if (w == "case") {
            sscanf(line, "%*s %32767s", a);
            cs = Case{};
            cs.name = a;
            memset(&cs.cfg, 0, sizeof cs.cfg);
            cs.cfg.abi_version = BDX_ABI_VERSION;
            cs.cfg.struct_size = sizeof(bdx_config_t);
            open = true;
        } else if (w == "cfg") {
            bdx_config_t &c = cs.cfg;
            if (sscanf(line, "%*s %d %d %lf %lf %d %d %d %d %d %d %d", &c.algorithm, &c.is_dual, &c.max_error_rate, &c.min_delta, &c.match, &c.mismatch,
                       &c.indel, &c.has_nindel, &c.nindel, &c.need_traceback, &c.filter) != 11) { fprintf(stderr, "bad cfg line in %s\n", cs.name.c_str()); exit(3); }
        } else if (w == "tune") {
            sscanf(line, "%*s %32767s %63s", a, b);
            if (!set_tuning(cs, a, b)) { fprintf(stderr, "unknown tuning key %s\n", a); exit(3); }
            cs.tune_kv.emplace_back(a, b);
        } else if (w == "pass") {
            bdx_pass_t &p = cs.cfg.pass[++pass];
            long long v[16];
            int tr, ew, B;
            if (sscanf(line, "%*s %d %d %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %d", &tr, &ew, &v[0], &v[1], &v[2], &v[3], &v[4],
                       &v[5], &v[6], &v[7], &v[8], &v[9], &v[10], &v[11], &v[12], &v[13], &v[14], &v[15], &B) != 19) { fprintf(stderr, "bad pass line in %s\n", cs.name.c_str()); exit(3); }
            p.trim_side = tr;
            p.explicit_window = ew;
            p.win_first = v[0], p.win_last = v[1], p.win_max_start_pos = v[2], p.win_min_end_pos = v[3];
            bdx_range_t *r[3] = {&p.ref_search_range, &p.barcode_start_range, &p.barcode_end_range};
            for (int i = 0; i < 3; ++i) {
                r[i]->start_offset = v[4 + 4 * i];
                r[i]->end_offset = v[5 + 4 * i];
                r[i]->start_from_end = (int32_t)v[6 + 4 * i];
                r[i]->end_from_end = (int32_t)v[7 + 4 * i];
            }
            p.n_barcodes = B;
            off[pass].push_back(0);
        } else if (w == "bc") {
            int n = 0;
            sscanf(line, "%*s %32767s %d", a, &n);
            bytes[pass].insert(bytes[pass].end(), a, a + strlen(a));
            off[pass].push_back((uint32_t)bytes[pass].size());
            nn[pass].push_back(n);
        } else if (w == "call") {
            cs.calls.push_back(line);
        } else if (w == "end") {
            for (int k = 0; k <= pass; ++k) {  // exact sizes: one byte outside is outside the allocation
                cs.bytes[k] = (uint8_t *)malloc(bytes[k].size() ? bytes[k].size() : 1);
                cs.off[k] = (uint32_t *)malloc(off[k].size() * 4);
                cs.nn[k] = (int32_t *)malloc(nn[k].size() ? nn[k].size() * 4 : 1);
                memcpy(cs.bytes[k], bytes[k].data(), bytes[k].size());
                memcpy(cs.off[k], off[k].data(), off[k].size() * 4);
                memcpy(cs.nn[k], nn[k].data(), nn[k].size() * 4);
                cs.cfg.pass[k].bc_bytes = cs.bytes[k];
                cs.cfg.pass[k].bc_off = cs.off[k];
                cs.cfg.pass[k].bc_len_no_N = cs.nn[k];
            }
            return true;
        }
    }
    if (open) { fprintf(stderr, "case %s has no end\n", cs.name.c_str()); exit(3); }
    return false;
}

// ---- the report ---------------------------------------------------------------------------------------------------------
#define I(s, f) fprintf(g_report, "%s." #f " %lld\n", pfx, (long long)(s).f)
#define I2(s, f) fprintf(g_report, "%s." #f " %lld %lld\n", pfx, (long long)(s).f[0], (long long)(s).f[1])
#define D(s, f) fprintf(g_report, "%s." #f " %a\n", pfx, (double)(s).f)

static void report_range(const char *pfx, const char *name, const BdxDevRange &r) {
    fprintf(g_report, "%s.%s %lld %lld %d %d\n", pfx, name, r.start_offset, r.end_offset, r.start_from_end, r.end_from_end);
}

static void report_dev(const BdxDevCfg &d) {
    const char *pfx = "dev";
    I(d, algorithm); I(d, is_dual); D(d, max_error_rate); D(d, min_delta); I(d, match); I(d, mismatch); I(d, indel); I(d, has_nindel); I(d, nindel);
    I(d, need_traceback); I(d, end_only_ok); I(d, max_m); I(d, force_lds_dp); I(d, any_traceback); I(d, counts_stride2); I(d, n_counts);
    I2(d, band_kb); I2(d, band_lb); I(d, dense_w); I(d, band_m); I(d, band_hcap);
    for (int k = 0; k < 2; ++k) {
        const BdxDevPass &P = d.pass[k];
        pfx = k ? "dev.pass1" : "dev.pass0";
        report_range(pfx, "ref_search", P.ref_search);
        report_range(pfx, "bc_start", P.bc_start);
        report_range(pfx, "bc_end", P.bc_end);
        I(P, trim_side); I(P, n_barcodes); I(P, explicit_window); I(P, cand_words); I(P, win_first); I(P, win_last); I(P, win_max_start); I(P, win_min_end);
    }
}

static void report_generic(const BdxGenericPlan &p) {
    const char *pfx = "plan";
    I(p, threads); I(p, reg_rows); I(p, clean); I(p, uniform_m); I(p, uniform_len); I(p, band_roll); I(p, same_len); I(p, dp_rows); I(p, dp_rows_fused);
    I(p, stage_bytes); I(p, bc_stage_bytes); I(p, hist_entries); I(p, lds_bytes); I(p, n_cu);
}

// off: lut, peq[2], pvinit[2], kb[2] (printed for an enabled plan, the passes the config has)
static void report_bitpar(const char *pfx, const BdxBitparPlan &b, const long long off[7], int npass) {
    I(b, enabled); I(b, reads_per_block); I(b, stage_bytes); I(b, read_len_hint); I(b, r_cap); I(b, diag_nw); I(b, diag_qcap); I(b, read_len_hint_for_lds);
    I(b, slot_bytes); I(b, dense_w); I(b, dense_d); I(b, slot_cap); I(b, seed_span); I(b, ncode_N); I(b, ncodes); I(b, grid_override); I(b, n_cu);
    I2(b, short_lb); I(b, dbg); I2(b, known_ok); I2(b, kb_uniform); I(b, tier_capped); fprintf(g_report, "%s.tier_slo %a %a\n", pfx, b.tier_slo[0], b.tier_slo[1]);
    I2(b, bpad); I(b, word_bytes);
    if (!b.enabled) return;
    fprintf(g_report, "%s.off.lut %lld\n", pfx, off[0]);
    for (int k = 0; k < npass; ++k) fprintf(g_report, "%s.off.pass%d %lld %lld %lld\n", pfx, k, off[1 + k], off[3 + k], off[5 + k]);
}

// off: bitmap, hash, hash_ps, always[2], dmeta[2], dkeys[2]
static void report_seed(const char *pfx, const BdxSeedPlan &s, const long long off[9]) {
    I(s, enabled); I(s, q); I(s, bm_words); I(s, bm_log2); I(s, rcap); I(s, qmul); I(s, hash_in_lds); I(s, hash_log2); I2(s, n_always); I(s, diag);
    I(s, diag_kmax); D(s, diag_flag_coef);
    if (!s.enabled) return;
    if (s.diag)
        fprintf(g_report, "%s.off.diag %lld %lld %lld %lld %lld %lld\n", pfx, off[5], off[6], off[7], off[8], off[3], off[4]);
    else
        fprintf(g_report, "%s.off.single %lld %lld %lld %lld %lld\n", pfx, off[0], off[1], off[2], off[3], off[4]);
}

// off: bitmap, rank, ent, peq8, meta, settle, peq8r
static void report_wave(const char *pfx, const BdxWavePlan &w, const long long off[7]) {
    I(w, enabled); I(w, q); I(w, n_ent); I(w, n_barcodes); I(w, b0); I(w, split); I(w, bm_bytes); I(w, track_from); I(w, rw); I(w, waves); I(w, blocks);
    I(w, span_cap); I(w, read_len_hint); I(w, hq_cap); I(w, sq_cap); I(w, cand_words); I(w, scan_gpr); I(w, ranged); I(w, winm); I(w, kend); D(w, chance);
    I(w, pairs_kb); I(w, pairs_spread); I(w, nw); I(w, groups); I(w, slot); I(w, cpr);
    if (w.enabled) fprintf(g_report, "%s.off %lld %lld %lld %lld %lld %lld %lld\n", pfx, off[0], off[1], off[2], off[3], off[4], off[5], off[6]);
}

// every plan of one filter set, with the offsets of its tables
static void report_set(const BdxPlanSet &F, const std::string &set, int npass) {
    const auto name = [&](const char *plan) { return set + "." + plan; };
    const BdxBitparOff &bo = F.bp_off;
    const long long boff[7] = {(long long)bo.lut, (long long)bo.peq[0], (long long)bo.peq[1], (long long)bo.pvinit[0], (long long)bo.pvinit[1], (long long)bo.kb[0], (long long)bo.kb[1]};
    report_bitpar(name("bplan").c_str(), F.bplan, boff, npass);
    const BdxSeedPlan *sps[2] = {&F.splan, &F.splan_alt};
    const BdxSeedOff *sos[2] = {&F.seed_off, &F.seed_alt_off};
    for (int i = 0; i < 2; ++i) {
        const BdxSeedOff &so = *sos[i];
        const long long soff[9] = {(long long)so.bitmap, (long long)so.hash, (long long)so.hash_ps, (long long)so.always[0], (long long)so.always[1],
                                   (long long)so.dmeta[0], (long long)so.dmeta[1], (long long)so.dkeys[0], (long long)so.dkeys[1]};
        report_seed(name(i ? "splan_alt" : "splan").c_str(), *sps[i], soff);
    }
    const BdxWavePlan *wps[6] = {&F.wplan, &F.wplan_k, &F.wplan_a, &F.pplan, &F.pplan_k, &F.pplan_a};
    const char *wnames[6] = {"wplan", "wplan_k", "wplan_a", "pplan", "pplan_k", "pplan_a"};
    for (int i = 0; i < 6; ++i) {
        const BdxWaveOff &wo = i < 3 ? F.wave_off : F.pair_off;
        const long long woff[7] = {(long long)wo.bitmap, (long long)wo.rank, (long long)wo.ent, (long long)wo.peq8, (long long)wo.meta, (long long)wo.settle, (long long)wo.peq8r};
        report_wave(name(wnames[i]).c_str(), *wps[i], woff);
    }
}

