// bdx_wave_end.hip — the known-trim instantiations of the wave-autonomous kernel with forward sweeps (bdx_wave_kernel.h,
// KEND = 1) with the launcher of the whole known-end class, and the general form of the non-split kernel (dual and ranged
// configs: GEN), in a translation unit of their own so that the sets of instantiations compile side by side.
#include "bdx_wave_kernel.h"

// The kernel for configs of the known-end class (ScoreOnly conditions + trim_side = 5, no start positions wanted): same
// launch as bdx_launch_wave for a known-score config, the verdicts carry the trimmed keep range.
hipError_t bdx_launch_wave_end(const BdxDevCfg &cfg, const BdxWavePlan &wp, int hist_entries, const BdxBatch &b, const BdxTierArgs &t, const BdxDevStats *stats) {
    if (b.n_reads <= 0) return hipSuccess;
    if (wp.pairs_kb > 0 || wp.split || !wp.kend || !wp.d_peq8r) return BDX_BAD_PLAN();
    if (wp.kend != 3 && (b.out.pass_start != nullptr || stats != nullptr)) return BDX_BAD_PLAN();  // (only the known-alignment class knows both positions)
    WaveArgs a;
    fill_args(a, cfg, wp, hist_entries, b, BdxHandOver{}, t);
    if (wp.kend != 3 && b.out.pass_end != nullptr && (a.trim0 == 3 || a.trim1 == 3)) return BDX_BAD_PLAN();  // (a trim_side = 3 pass knows its start only)
    if (stats) a.stats = *stats;
    a.tier_slo1 = t.slo[1];
    a.dual = cfg.is_dual ? 1 : 0;
    if (a.dual && wp.cand_words != 4) return BDX_BAD_PLAN();  // (the survivors of pass 1 live in the candidate-word area: four per read)
    if (wp.kend == 3) return bdx_launch_wave_end_aln(&a, wp, b.stream);  // (bdx_wave_aln.hip)
    if ((wp.kend == 2) != (a.trim0 == 3 || a.trim1 == 3)) return BDX_BAD_PLAN();
    if (wp.kend == 2) return bdx_launch_wave_end_rev(&a, wp, b.stream);  // (bdx_wave_rev.hip)
    return launch_seeded<false, 1, true>(a, wp, b.stream);
}

// The general form of the non-split kernel (dual configs, ref_search_range windows) for bdx_launch_wave.
hipError_t bdx_launch_wave_gen(const void *wave_args, const BdxWavePlan &wp, hipStream_t stream) {
    return launch_seeded<false, 0, true>(*(const WaveArgs *)wave_args, wp, stream);
}
