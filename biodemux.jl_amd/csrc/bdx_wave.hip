// bdx_wave.hip — the wave-autonomous kernel (bdx_wave_kernel.h) for known-score configs (the headline form) and for plain split
// mode, both with whole ranges and a single pass (GEN = false), and their launcher.  Dual and ranged configs
// take the general forms, which bdx_wave_end.hip (non-split) and bdx_pairs.hip (split) hold.
#include "bdx_wave_kernel.h"

hipError_t bdx_launch_wave(const BdxDevCfg &cfg, const BdxWavePlan &wp, int hist_entries, const BdxBatch &b, const BdxHandOver &ho, const BdxTierArgs &t) {
    if (b.n_reads <= 0) return hipSuccess;
    WaveArgs a;
    fill_args(a, cfg, wp, hist_entries, b, ho, t);
    a.tier_slo1 = t.slo[1];
    a.dual = (!wp.split && cfg.is_dual) ? 1 : 0;
    if (a.dual && wp.cand_words != 4) return BDX_BAD_PLAN();  // (the survivors of pass 1 live in the candidate-word area: four per read)
    if (wp.pairs_kb > 0) return BDX_BAD_PLAN();
    if (wp.split && (!a.cand_out[0] || !a.wins_out[0] || !a.wcnt_out[0])) return BDX_BAD_PLAN();
    // (known-score dual configs and configs with a ref_search_range take the general form of their kernel)
    if (!wp.split && (a.dual || a.ranged)) return bdx_launch_wave_gen(&a, wp, b.stream);  // (bdx_wave_end.hip)
    if (wp.split && a.ranged) return bdx_launch_wave_split_gen(&a, wp, b.stream);         // (bdx_pairs.hip)
    return seeded_ladder<false>(wp, [&](auto c) {
        using C = decltype(c);
        return wp.split ? launch_wave<C::RW, C::TF, C::NV, C::Q, true, 0, 0, false, 0, false>(a, wp, b.stream)
                        : launch_wave<C::RW, C::TF, C::NV, C::Q, false, 0, 0, false, 0, false>(a, wp, b.stream);
    });
}
