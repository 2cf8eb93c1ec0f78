// plan_host.cpp — stand-alone driver of the create-time planner (csrc/bdx_plan.cpp): reads the case file that
// tests/plan_cases.py writes, plans every case on the CPU, writes every table a plan refers to into a directory and prints
// every non-pointer field of the output (doubles as %a, offsets as integers).  tests/test_plan_cpu.py compares the report
// with tests/golden/plan_tables.json and runs this same program under ASan / UBSan; the barcode arrays are exact-size heap
// blocks (bc_bytes ends its allocation, bc_off has exactly B + 1 entries), so a read outside them is the sanitizer's to report.
//
//   plan_host CASES OUTDIR
//
// (the case file and the report of the scalar fields: tests/plan_case.h)
#include "plan_case.h"

static void report_blob(const std::string &dir, const std::string &name, const std::string &table, const void *data, size_t bytes) {
    const std::string path = dir + "/" + name + "." + table + ".bin";
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(data, 1, bytes, f) != bytes) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(4); }
    fclose(f);
    printf("blob %s %zu\n", table.c_str(), bytes);
}

// ---- one case through the planner ---------------------------------------------------------------------------------------
static void run_case(const Case &cs, const std::string &dir) {
    BdxPlanOut po;
    const int rc = bdx_plan(cs.cfg, cs.tune, cs.n_cu, po);
    printf("case %s\nrc %d\n", cs.name.c_str(), rc);
    if (rc != BDX_OK) {
        printf("err %s\n", po.err.c_str());
        return;
    }
    const char *pfx = "top";
    I(po, tiered); I(po, pairs_tier); I(po, tier_q); I(po, tier_cap_fixed); I(po, pair_mmin); I(po, band_roll_off); I(po, filter_used);
    printf("top.path %s\n", po.path.c_str());
    report_dev(po.dev);
    report_generic(po.plan);
    for (int s = 0; s < 2; ++s) {
        const BdxPlanSet &F = po.fs[s];
        const std::string set = s ? "fs1" : "fs0";
        report_set(F, set, cs.cfg.is_dual ? 2 : 1);
        // the tables some enabled plan refers to
        if (F.bplan.enabled) report_blob(dir, cs.name, set + ".bp_tables", F.bp_tables.bytes.data(), F.bp_tables.bytes.size());
        if (F.splan.enabled) report_blob(dir, cs.name, set + ".seed_tables", F.seed_tables.bytes.data(), F.seed_tables.bytes.size());
        if (F.splan_alt.enabled) report_blob(dir, cs.name, set + ".seed_tables_alt", F.seed_tables_alt.bytes.data(), F.seed_tables_alt.bytes.size());
        if (F.wplan.enabled || F.wplan_k.enabled || F.wplan_a.enabled) report_blob(dir, cs.name, set + ".wave_tables", F.wave_tables.bytes.data(), F.wave_tables.bytes.size());
        if (F.pplan.enabled || F.pplan_k.enabled || F.pplan_a.enabled) report_blob(dir, cs.name, set + ".pair_tables", F.pair_tables.bytes.data(), F.pair_tables.bytes.size());
    }
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 3; }
    Case cs;
    int n = 0;
    while (read_case(f, cs)) {
        run_case(cs, argv[2]);
        cs.release();
        ++n;
    }
    fclose(f);
    printf("plan driver ok: %d cases\n", n);
    return 0;
}
