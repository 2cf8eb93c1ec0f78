// bdx_call.h — the per-call planner (bdx_call.cpp): which kernels one batch runs on and with which tile, queue and LDS
// geometry, and the grid and LDS bytes of every launch (the launchers decide neither).  Host-only like bdx_plan.cpp: no HIP
// runtime call, no device buffer, no context.  bdx_classify_batch (bdx_abi.cpp) runs it once per call and launches from
// the CallPlan it returns; tests/call_host.cpp runs it on a CPU.  With it, host-only in the same way: the rule for a batch's
// read length (bdx_batch_len) and the turn of the scratch halves (BdxScratchTurn).
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

// what bdx_create produced (nothing here is written by a call: a window upload's per-read pointers go into the call's own
// copy of BdxDevCfg, bdx_abi.cpp)
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

// The exact kernel's diagonal-band DP (sg_core_band) for one launch of the generic kernel, as the launch's BdxDevCfg carries
// it: clean class, every barcode of the config with the same number of rows and of the pass with the same budget, column
// windows handed over by tracked sweeps.  launches: what the launch adds to bdx_band_launches (passes with the band on).
struct BdxBandPlan {
    int dense_w = 0, m = 0;
    int kb[2] = {-1, -1}, lb[2] = {0, 0};
    int launches = 0;
};

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
    BdxBandPlan band_t1{}, band_exact{};              //   ... and their band fields (a launch without the band: the config's own)
    size_t lds_bytes = 0;  // LDS of a `fused` workgroup (fused.lds_bytes: what bdx_launch_info reports)
    std::string path;      // the stages, front first (bdx_kernel_path)
};

// Plans one classify call.  seed[set] is read and may be demoted.  BDX_OK with out.filtered = false: the config has no
// filter, or no geometry of the fused kernel fits this batch.  Otherwise the code of a refusal with its message in err.
int bdx_plan_call(const BdxCallEnv &env, const BdxCallArgs &args, BdxSeedChoice seed[2], CallPlan &out, std::string &err);

// The read length of a batch.  window_len / host_len: the longest read as a window upload / the host entry point has seen it
// (0: not known); hint: bdx_set_read_length_hint; measured: bdx_launch_maxlen's answer, -1 before it was asked.
//   measure  the config collects statistics, or has a filter and neither a window upload nor a hint, and nothing is known:
//            the caller measures on the device and asks again
//   longest  the known, else the measured longest read: the statistics tables are reserved for longest + max_m + 2 rows
//   planned  what the filtered launches are planned for: the window upload's value, else a positive hint (also when the host
//            knows better), else `longest` with values below 1 counted as 1; 0 without a filter
struct BdxBatchLen {
    bool measure;
    int longest, planned;
};
BdxBatchLen bdx_batch_len(int window_len, int host_len, int hint, bool stats, bool filter, int measured = -1);

// Whose turn it is with the two halves of the scratch block (BdxScratch, bdx_internal.h).  A filtered call runs on mine();
// its last launch clears other(), which the next call then takes without a memset of its own.  A call that fails between
// begin_call and finish_call leaves its half dirty and does not turn; an unfiltered call touches nothing.
struct BdxScratchTurn {
    int half = 0;
    bool clean[2] = {false, false};  // the half is known to hold zeros when the next launch on the context's stream starts
    int mine() const { return half; }
    int other() const { return 1 - half; }
    // true: this call clears mine() with a memset (cleared_by_copy: the host entry's copy kernel already did, for this call)
    bool begin_call(bool cleared_by_copy) {
        const bool need_memset = !cleared_by_copy && !clean[half];
        clean[half] = false;
        return need_memset;
    }
    void finish_call() {  // the call's last launch is enqueued
        clean[other()] = true;
        half = other();
    }
    void stream_changed() { clean[0] = clean[1] = false; }  // (the clearing launch ran on a stream the new one is not ordered after)
};
