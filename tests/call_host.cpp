// call_host.cpp — stand-alone driver of the per-call planner (csrc/bdx_call.cpp): reads the case file that tests/call_cases.py
// writes (the configs of tests/plan_cases.py, each with a list of `call` lines), runs the create-time planner and then
// bdx_plan_call for every call of the case IN ORDER on one seed choice — a case with several calls is a sequence on one
// context — and prints per call every CallPlan scalar, the path, every geometry field of every plan a stage launches and the
// seed plans in effect afterwards.  A digest of the create-time planner's whole report and tables is printed before and after
// the calls: a call never changes them.  tests/test_call_plan_cpu.py compares the report with tests/golden/call_plans.json and
// runs this same program under ASan / UBSan; tests/test_call_plan_gpu.py compares it with what the library launched.
//
//   call_host CASES [REPEAT | launches]
//     REPEAT > 0: also prints the mean host time of one bdx_plan_call per case on stderr (ns, not compared)
//     launches: also prints the launches every plan holds (report_launches), for the golden file and the comparison with bdx_last_launches
//   call_host lengths FILE   bdx_batch_len's answers, one line per line `WINDOW_LEN HOST_LEN HINT STATS FILTER MEASURED` of FILE:
//                            `measure longest planned` (measure 1: asked again with MEASURED, whose answer the other two are)
//   call_host scratch FILE   BdxScratchTurn over the events of every line of FILE (call, copy: a call whose scratch the copy kernel
//                            cleared, fail: a call that never finishes, plain: an unfiltered call, stream: a stream switch); per
//                            event `memset:mine:other` (memset -: the event begins no call)
//
// (diag_nw / diag_qcap are reported for a launch whose seed plan is the two-intact-pieces index; nothing else reads them)
#include <algorithm>
#include <chrono>

#include "bdx_call.h"
#include "plan_case.h"

static uint64_t fnv(uint64_t h, const void *data, size_t n) {
    const unsigned char *p = (const unsigned char *)data;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001B3ULL;
    return h;
}

// the create-time planner's output as plan_host.cpp reports it (every scalar, every offset) + every table, hashed
static uint64_t digest(const BdxPlanOut &po, int npass) {
    char *text = nullptr;
    size_t n = 0;
    g_report = open_memstream(&text, &n);
    const char *pfx = "top";
    I(po, tiered); I(po, pairs_tier); I(po, tier_q); I(po, tier_cap_fixed); I(po, pair_mmin); I(po, band_roll_off); I(po, filter_used);
    report_dev(po.dev);
    report_generic(po.plan);
    uint64_t h = 0xCBF29CE484222325ULL;
    for (int s = 0; s < 2; ++s) {
        report_set(po.fs[s], s ? "fs1" : "fs0", npass);
        for (const BdxBlob *b : {&po.fs[s].bp_tables, &po.fs[s].seed_tables, &po.fs[s].seed_tables_alt, &po.fs[s].wave_tables, &po.fs[s].pair_tables})
            h = fnv(h, b->bytes.data(), b->bytes.size());
    }
    fclose(g_report);
    g_report = stdout;
    h = fnv(h, text, n);
    free(text);
    return h;
}

static void report_fused(const char *key, const BdxBitparPlan &b, const BdxSeedPlan &sp, size_t lds) {
    const bool diag = sp.enabled && sp.diag;
    printf("%s %d %d %d %d %d %d %d %zu\n", key, b.reads_per_block, b.stage_bytes, b.slot_bytes, b.seed_span, b.r_cap, diag ? b.diag_nw : 0,
           diag ? b.diag_qcap : 0, lds);
}

static void report_tiles(const char *key, const BdxWavePlan &w) {
    printf("%s %d %d %d %d %d %d %d %d %d %d %d\n", key, w.rw, w.waves, w.blocks, w.span_cap, w.hq_cap, w.sq_cap, w.slot, w.cpr, w.scan_gpr, w.winm,
           w.read_len_hint);
}

// c<i>.plan: npass tier_len batch_len split windows dense_w short_lb[2] front t1_exact middle full exact carry aln
// c<i>.fused / .t1: reads_per_block stage_bytes slot_bytes seed_span r_cap diag_nw diag_qcap LDS bytes
// c<i>.wfront / .wmid / .wfull: rw waves blocks span_cap hq_cap sq_cap slot cpr scan_gpr winm read_len_hint
// c<i>.band_t1 / .band_exact: dense_w band_m band_kb[2] band_lb[2] of tier 1's exact launch / the exact stage, and what the launch adds to bdx_band_launches
// c<i>.seed: per set 0: the set's own seed plan, 1: the weak single seeds kept beside it, 2: no seeds
static void report_call(int i, int rc, const std::string &err, const CallPlan &p, const BdxPlanOut &po, const BdxSeedChoice seed[2]) {
    char key[32];
    const auto k = [&](const char *field) {
        snprintf(key, sizeof key, "c%d.%s", i, field);
        return key;
    };
    printf("%s %d\n", k("rc"), rc);
    if (rc != BDX_OK) printf("%s %s\n", k("err"), err.c_str());
    printf("%s %d\n", k("filtered"), (int)p.filtered);
    if (rc == BDX_OK && p.filtered) {
        printf("%s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", k("plan"), p.npass, p.tier_len, p.batch_len, (int)p.split, (int)p.windows, (int)p.dense_w,
               p.short_lb[0], p.short_lb[1], (int)p.front, (int)p.t1_exact, (int)p.middle, (int)p.full, (int)p.exact, (int)p.carry, (int)p.aln);
        printf("%s %s\n", k("path"), p.path.c_str());
        report_fused(k("fused"), p.fused, bdx_seed_plan(po.fs[0], p.seed[0]), p.fused.lds_bytes);
        if (p.front == Front::bitpar) {
            report_fused(k("t1"), p.t1, bdx_seed_plan(po.fs[1], p.seed[1]), p.t1.lds_bytes);
        } else if (p.front != Front::none) {
            report_tiles(k("wfront"), p.wfront);
        }
        if (p.middle != Middle::none) report_tiles(k("wmid"), p.wmid);
        if (p.full == Full::wave_split) report_tiles(k("wfull"), p.wfull);
        const auto band = [&](const char *field, const BdxBandPlan &b) {
            printf("%s %d %d %d %d %d %d %d\n", k(field), b.dense_w, b.m, b.kb[0], b.kb[1], b.lb[0], b.lb[1], b.launches);
        };
        if (p.t1_exact) band("band_t1", p.band_t1);
        band("band_exact", p.band_exact);
    }
    int eff[2];
    for (int s = 0; s < 2; ++s) eff[s] = bdx_seed_plan(po.fs[s], seed[s]).enabled ? (int)seed[s] : (int)BDX_SEED_NONE;
    printf("%s %d %d\n", k("seed"), eff[0], eff[1]);
}

// The launches a plan holds, one line per classify kernel in the order of the stages: family, then blocks, threads, tile and
// list flag as the plan states them (the launchers take the grid from the plan; tests/golden/call_plans.json holds these lines
// as the launchers of the commit before computed them), then the template arguments the plan decides
//   bitpar: R SEED DIAG NW WL | generic: BS reg_rows clean uniform_m band_roll (the ladder of bdx_launch_generic spells the
//   instantiation from these: tests/kernel_lattice.py generic_name) | wave, pairs: RW SPLIT KEND WINM, then what the dispatch
//   ladders of bdx_wave_kernel.h and the leaves in bdx_wave.hip / bdx_wave_win.hip / bdx_pairs.hip read: q track_from span_cap slot
//   gen (split ? ranged : dual || ranged) pairs_kb nw groups (tests/kernel_lattice.py wave_name / pairs_name)
static void report_launches(int i, const CallPlan &p, const BdxPlanOut &po) {
    int j = 0;
    const auto line = [&](const char *family, long long blocks, int threads, int tile, int list, int a, int b, int c, int d, int e) {
        printf("c%d.launch%d %s %lld %d %d %d %d %d %d %d %d\n", i, j++, family, blocks, threads, tile, list, a, b, c, d, e);
    };
    const auto fused = [&](int set, const BdxBitparPlan &b, int list) {
        const BdxSeedPlan sp = bdx_seed_plan(po.fs[set], p.seed[set]);
        const bool diag = sp.enabled && sp.diag;
        line("bitpar", b.grid, 256, b.reads_per_block, list, b.reads_per_block, sp.enabled != 0, diag, diag && b.diag_nw > 5 ? 10 : 5,
             b.word_bytes == 8 ? 1 : b.word_bytes == 16 ? 2 : 0);
    };
    const auto seeded = [&](const char *family, const BdxWavePlan &w, int tile, int list, int winm) {
        const int gen = w.split ? w.ranged != 0 : (po.dev.is_dual || w.ranged != 0);
        printf("c%d.launch%d %s %lld %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", i, j++, family, w.grid, 64 * w.waves, tile, list, tile, w.split, w.kend, winm, w.q,
               w.track_from, w.span_cap, w.slot, gen, w.pairs_kb, w.nw, w.groups);
    };
    const auto wave = [&](const BdxWavePlan &w) { seeded("wave", w, w.rw, 0, w.winm); };
    const auto pairs = [&](const BdxWavePlan &w, int list) { seeded("pairs", w, 16, list, 0); };
    const auto generic = [&](long long blocks, int list) {
        line("generic", blocks, po.plan.threads, po.plan.threads, list, po.plan.threads, po.plan.reg_rows, po.plan.clean, po.plan.uniform_m, po.plan.band_roll);
    };
    if (!p.filtered) return generic(p.exact_blocks, 0);
    if (p.front == Front::bitpar) fused(1, p.t1, 0);
    else if (p.front == Front::pairs) pairs(p.wfront, 0);
    else if (p.front != Front::none) wave(p.wfront);
    if (p.t1_exact) generic(p.t1_exact_blocks, 0);
    if (p.middle != Middle::none) pairs(p.wmid, p.middle != Middle::all);
    if (p.full == Full::wave_split) wave(p.wfull);
    if (p.full == Full::bitpar) fused(0, p.fused, p.front != Front::none);
    generic(p.exact_blocks, p.exact != Exact::split);
}

// ---- the planner under test: one context's worth of state and one call ------------------------------------------------
struct Session {
    const BdxPlanOut &po;
    const Case &cs;
    BdxSeedChoice seed[2] = {BDX_SEED_MAIN, BDX_SEED_MAIN};
    Session(const BdxPlanOut &po_, const Case &cs_) : po(po_), cs(cs_) {}
    BdxCallEnv env() const { return BdxCallEnv{po.dev, po.plan, po.fs[0], po.fs[1], po, cs.tune, cs.n_cu}; }
    int call(const BdxCallArgs &a, CallPlan &p, std::string &err) { return bdx_plan_call(env(), a, seed, p, err); }
};
// ---- end of the planner under test -------------------------------------------------------------------------------------

static BdxCallArgs parse_call(const std::string &line) {
    BdxCallArgs a;
    int wu = 0, stats = 0;
    if (sscanf(line.c_str(), "%*s %lld %d %d %u %d", &a.n_reads, &a.read_len, &wu, &a.wanted, &stats) != 5) { fprintf(stderr, "bad call line: %s", line.c_str()); exit(3); }
    a.window_upload = wu != 0;
    a.stats = stats != 0;
    return a;
}

static void run_case(const Case &cs, int repeat, bool launches) {
    BdxPlanOut po;
    const int rc = bdx_plan(cs.cfg, cs.tune, cs.n_cu, po);
    printf("case %s\nrc %d\n", cs.name.c_str(), rc);
    if (rc != BDX_OK) {
        printf("err %s\n", po.err.c_str());
        return;
    }
    const int npass = cs.cfg.is_dual ? 2 : 1;
    printf("digest.before %016llx\n", (unsigned long long)digest(po, npass));
    Session ses(po, cs);
    for (size_t i = 0; i < cs.calls.size(); ++i) {
        CallPlan p;
        std::string err;
        const BdxCallArgs a = parse_call(cs.calls[i]);
        const int crc = ses.call(a, p, err);
        report_call((int)i, crc, err, p, po, ses.seed);
        if (launches && crc == BDX_OK) report_launches((int)i, p, po);
    }
    printf("digest.after %016llx\n", (unsigned long long)digest(po, npass));
    if (repeat > 0 && !cs.calls.empty()) {  // the last call again and again, on the state the sequence left
        const BdxCallArgs a = parse_call(cs.calls.back());
        CallPlan p;
        std::string err;
        const auto t0 = std::chrono::steady_clock::now();
        long long sink = 0;
        for (int r = 0; r < repeat; ++r) sink += ses.call(a, p, err) + p.fused.reads_per_block;
        const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / repeat;
        fprintf(stderr, "time %s %.0f ns per call (%lld)\n", cs.name.c_str(), ns, sink);
    }
}

static int run_lengths(FILE *f) {
    int w, h, hint, stats, filter, measured, n = 0;
    while (fscanf(f, "%d %d %d %d %d %d", &w, &h, &hint, &stats, &filter, &measured) == 6) {
        BdxBatchLen a = bdx_batch_len(w, h, hint, stats != 0, filter != 0);
        const bool measure = a.measure;
        if (measure) a = bdx_batch_len(w, h, hint, stats != 0, filter != 0, measured);
        if (a.measure) return 4;  // (asked twice)
        printf("%d %d %d\n", (int)measure, a.longest, a.planned);
        ++n;
    }
    printf("length driver ok: %d lines\n", n);
    return 0;
}

static int run_scratch(FILE *f) {
    char line[4096];
    int n = 0;
    while (fgets(line, sizeof line, f)) {
        BdxScratchTurn t;
        std::string out;
        for (char *ev = strtok(line, " \n"); ev; ev = strtok(nullptr, " \n")) {
            const std::string e = ev;
            char memset_needed = '-';
            if (e == "call" || e == "copy" || e == "fail") {
                memset_needed = t.begin_call(e == "copy") ? '1' : '0';
                if (e != "fail") t.finish_call();
            } else if (e == "stream") {
                t.stream_changed();
            } else if (e != "plain") {
                return 4;
            }
            out += (out.empty() ? "" : " ") + std::string(1, memset_needed) + ":" + std::to_string(t.mine()) + ":" + std::to_string(t.other());
        }
        printf("%s\n", out.c_str());
        ++n;
    }
    printf("scratch driver ok: %d lines\n", n);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2 || argc > 3) return 2;
    const bool lengths = argc == 3 && !strcmp(argv[1], "lengths"), scratch = argc == 3 && !strcmp(argv[1], "scratch");
    FILE *f = fopen(argv[lengths || scratch ? 2 : 1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[lengths || scratch ? 2 : 1]); return 3; }
    if (lengths || scratch) {
        const int rc = lengths ? run_lengths(f) : run_scratch(f);
        fclose(f);
        return rc;
    }
    const bool launches = argc == 3 && !strcmp(argv[2], "launches");
    const int repeat = argc == 3 && !launches ? atoi(argv[2]) : 0;
    Case cs;
    int n = 0;
    while (read_case(f, cs)) {
        run_case(cs, repeat, launches);
        cs.release();
        ++n;
    }
    fclose(f);
    printf("call driver ok: %d cases\n", n);
    return 0;
}
