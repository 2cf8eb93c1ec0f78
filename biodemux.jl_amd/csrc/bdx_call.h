// bdx_call.h — the per-call planner (bdx_call.cpp): which kernels one batch runs on and with which tile, queue and LDS
// geometry, and the grid and LDS bytes of every launch (the launchers decide neither).  Host-only like bdx_plan.cpp: no HIP
// runtime call, no device buffer, no context.  bdx_classify_device (bdx_abi.cpp) runs it once per call and launches from
// the CallPlan it returns; tests/call_host.cpp runs it on a CPU.
#pragma once
#include <string>

#include "bdx_plan.h"

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

// what bdx_create produced (nothing here is written by a call)
struct BdxCallEnv {
    const BdxDevCfg &dev;
    const BdxGenericPlan &plan;
    const BdxSetPlans &f0, &f1;  // full budgets, tier 1
    const BdxPlanChoice &choice;
    const BdxTuning &tune;
    int n_cu;
};

// the vectors of BdxDevOut a caller may want, as bits of BdxCallArgs::wanted (in the struct's order)
enum : unsigned {
    BDX_WANT_BC1 = 1u << 0, BDX_WANT_BC2 = 1u << 1, BDX_WANT_KEEP_START = 1u << 2, BDX_WANT_KEEP_END = 1u << 3, BDX_WANT_PASS_START = 1u << 4,
    BDX_WANT_PASS_END = 1u << 5, BDX_WANT_PASS_RAW = 1u << 6, BDX_WANT_PASS_BC = 1u << 7, BDX_WANT_PASS_SCORE = 1u << 8, BDX_WANT_PASS_DELTA = 1u << 9,
    BDX_WANT_PER_PASS = 0x3F0u
};

struct BdxCallArgs {
    long long n_reads = 0;
    int read_len = 0;            // the read length the batch is planned for (values below 1 count as 1)
    bool window_upload = false;  // seq / off hold only each read's window (BdxDevCfg::vlen)
    unsigned wanted = 0;         // BDX_WANT_* bits
    bool stats = false;          // the statistics tables are collected
};

// The one piece of planning state that outlives a call, per filter set: which seed plan the fused kernel runs with.  A batch
// the two-intact-pieces index does not fit (reads beyond 312 bases, very many barcodes) demotes the set to the weak single
// seeds kept beside it, those to the plain sweep; later batches stay there (monotone).
enum BdxSeedChoice : int { BDX_SEED_MAIN = 0, BDX_SEED_ALT = 1, BDX_SEED_NONE = 2 };

// the seed plan of `f` under a choice (a disabled one for BDX_SEED_NONE); device pointers as bound in `f`
inline BdxSeedPlan bdx_seed_plan(const BdxSetPlans &f, BdxSeedChoice c) {
    return c == BDX_SEED_MAIN ? f.splan : c == BDX_SEED_ALT ? f.splan_alt : BdxSeedPlan{};
}

struct CallPlan {
    bool filtered = false;  // false: the generic kernel alone (of what is below only exact_blocks is set)
    int npass = 1, tier_len = 0, batch_len = 0;  // tier_len > 0: tiered; batch_len: the read length the launches were planned for
    bool split = false, windows = false, dense_w = false;
    int short_lb[2] = {0, 0};
    Front front = Front::none;
    bool t1_exact = false;  // tier 1's exact launch
    Middle middle = Middle::none;
    Full full = Full::bitpar;
    Exact exact = Exact::known;
    bool carry = false, aln = false;  // carried passes (d_carry); the known-end forms run as the known-alignment class
    // sized copies of the plans the stages launch, each with its launch's grid and LDS bytes (BDX_GRID applied); reserve
    // (bdx_abi.cpp) adds the per-launch device pointers
    BdxWavePlan wfront{}, wmid{}, wfull{};  // the wave-kernel front stage, the pairs mode, the wave kernel as the full-budget filter
    BdxBitparPlan t1{}, fused{};            // the fused kernel: tier 1 over the batch; at the full budgets (dense, or over the list)
    BdxSeedChoice seed[2] = {BDX_SEED_MAIN, BDX_SEED_MAIN};  // the seed plans t1 (seed[1]) and fused (seed[0]) were sized with
    long long t1_exact_blocks = 0, exact_blocks = 0;  // grids of the generic kernel: tier 1's exact launch, the exact stage
    size_t lds_bytes = 0;  // LDS of a `fused` workgroup (fused.lds_bytes: what bdx_launch_info reports)
    std::string path;      // the stages, front first (bdx_kernel_path)
};

// Plans one classify call.  seed[set] is read and may be demoted.  BDX_OK with out.filtered = false: the config has no
// filter, or no geometry of the fused kernel fits this batch.  Otherwise the code of a refusal with its message in err.
int bdx_plan_call(const BdxCallEnv &env, const BdxCallArgs &args, BdxSeedChoice seed[2], CallPlan &out, std::string &err);
