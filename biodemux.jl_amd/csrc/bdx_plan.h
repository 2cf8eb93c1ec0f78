// bdx_plan.h — the create-time planner (bdx_plan.cpp): which kernel family every config runs on and what the kernels read
// from their tables.  Host-only: no HIP runtime call, no device buffer, no context.  bdx_create (bdx_abi.cpp) runs it, uploads
// every blob it produced and binds the plans' device pointers from base + offset; tests/plan_host.cpp runs it on a CPU.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "bdx_internal.h"

// A table as the device will hold it.  put() appends a vector, fills its size up to a multiple of `unit` with zeros and
// returns the offset it went to; align() fills up to the next multiple of `a` first.
struct BdxBlob {
    std::vector<uint8_t> bytes;
    void align(size_t a) { bytes.resize((bytes.size() + a - 1) & ~(a - 1), 0); }
    template <class T>
    size_t put(const std::vector<T> &v, size_t unit = 1) {
        const size_t at = bytes.size(), n = v.size() * sizeof(T);
        bytes.resize(at + ((n + unit - 1) & ~(unit - 1)), 0);
        if (n) memcpy(bytes.data() + at, v.data(), n);
        return at;
    }
};

// where the pointer fields of a plan point, as byte offsets into the set's table of that kind
struct BdxBitparOff { size_t lut = 0, peq[2] = {0, 0}, pvinit[2] = {0, 0}, kb[2] = {0, 0}; };
struct BdxSeedOff { size_t bitmap = 0, hash = 0, hash_ps = 0, always[2] = {0, 0}, dmeta[2] = {0, 0}, dkeys[2] = {0, 0}; };  // (diag plans: dmeta, dkeys, always)
struct BdxWaveOff { size_t bitmap = 0, rank = 0, ent = 0, peq8 = 0, meta = 0, settle = 0, peq8r = 0; };

// the plans of one filter set (BdxFilterSet of bdx_ctx.h adds the device buffers, BdxPlanSet the host blobs)
struct BdxSetPlans {
    BdxBitparPlan bplan{};
    BdxSeedPlan splan{};
    // weak single seeds kept beside a two-intact-pieces plan: taken when the latter's index does not fit the
    // batch at hand (very many barcodes, reads beyond 312 bases); built at create, while the barcodes are there
    BdxSeedPlan splan_alt{};
    BdxWavePlan wplan{};    // wave-autonomous kernel (bdx_wave.hip) for this set, when the config qualifies
    BdxWavePlan wplan_k{};  // known-trim class (ScoreOnly conditions + trim sides): the same tables, the non-split kernel with position keys
    BdxWavePlan wplan_a{};  // known-alignment class (... + summary statistics / per-pass positions wanted): kend = 3
    BdxWavePlan pplan{};    // the same kernel in pairs mode (bdx_pairs.hip) at this set's full budgets, over listed reads
    BdxWavePlan pplan_k{};  // ... in its known-end form (trim_side = 5 configs)
    BdxWavePlan pplan_a{};  // ... in its known-alignment form (kend = 3)
};

// A table is replaced only by a builder that succeeds, so a plan a rejected tier attempt left enabled keeps the table it
// was built with; the _k / _a plans share their parent's table and offsets.
struct BdxPlanSet : BdxSetPlans {
    BdxBlob bp_tables, seed_tables, seed_tables_alt, wave_tables, pair_tables;
    BdxBitparOff bp_off;
    BdxSeedOff seed_off, seed_alt_off;
    BdxWaveOff wave_off, pair_off;
};

// what the tier selection decided (bdx_ctx carries the same fields: it derives from this)
struct BdxPlanChoice {
    int tiered = 0;     // fs[1] is usable: classify runs tier 1 first, tier 0 on the reads it cannot settle
    int tier_q = 8;     // piece length behind tier 1's capped budgets: cap(m) = m / tier_q - 1
    int tier_cap_fixed = -1;  // >= 0: the pairs tier — tier 1's budgets are capped at this many operations for every barcode and its
                              // filter is the same-diagonal pairs mode over the whole batch (configs whose min_delta the seed tier cannot prove)
    int pairs_tier = 0;
    int pair_mmin = 0;  // shortest barcode of the pairs plan
    bool band_roll_off = false;  // the config has no filter (no hand-over windows) — the exact kernel keeps its by-construction LDS form
    int filter_used = BDX_FILTER_OFF;
    std::string path;
};

struct BdxPlanOut : BdxPlanChoice {
    BdxDevCfg dev{};  // without device pointers
    BdxGenericPlan plan{};
    BdxPlanSet fs[2];  // fs[0] filters at the config's full operation budgets, fs[1] is tier 1 (bdx_plan.cpp, tiered budgets)
    std::string err;   // the message of a refusal
};

// Plans `c` (validated; its barcode arrays are read, nothing is kept) for a device of n_cu compute units.
// Returns BDX_OK, or the code of a refusal with its message in out.err.
int bdx_plan(const bdx_config_t &c, const BdxTuning &tune, int n_cu, BdxPlanOut &out);
