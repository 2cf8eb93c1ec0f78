// bdx_wave_end.hip — the known-trim instantiations of the wave-autonomous kernel with forward sweeps (bdx_wave_kernel.h,
// KEND = 1) with the launcher of the whole known-end class, and the general form of the non-split kernel (dual and ranged
// configs: GEN), in a translation unit of their own so that the sets of instantiations compile side by side.
#include "bdx_wave_kernel.h"

// The kernel for configs of the known-end class (ScoreOnly conditions + trim_side = 5, no start positions wanted): same
// launch as bdx_launch_wave for a known-score config, the verdicts carry the trimmed keep range.
hipError_t bdx_launch_wave_end(const BdxDevCfg &cfg, const BdxWavePlan &wp, int hist_entries, const uint8_t *d_seq, const long long *d_off,
                               long long n_reads, const BdxDevOut &out, unsigned long long *d_counts, int tier1, double tier_slo, uint32_t *list,
                               unsigned int *list_count, hipStream_t stream, int dbg, double tier_slo1, const BdxDevStats *stats) {
    if (n_reads <= 0) return hipSuccess;
    if (wp.pairs_kb > 0 || wp.split || !wp.kend || !wp.d_peq8r) return BDX_BAD_PLAN();
    if (wp.kend != 3 && (out.pass_start != nullptr || stats != nullptr)) return BDX_BAD_PLAN();  // (only the known-alignment class knows both positions)
    WaveArgs a;
    fill_args(a, cfg, wp, hist_entries, out, d_counts, list, list_count, dbg, nullptr);
    if (wp.kend != 3 && out.pass_end != nullptr && (a.trim0 == 3 || a.trim1 == 3)) return BDX_BAD_PLAN();  // (a trim_side = 3 pass knows its start only)
    if (stats) a.stats = *stats;
    a.seq = d_seq;
    a.off = d_off;
    a.n_reads = n_reads;
    a.tier = tier1;
    a.tier_slo = tier_slo;
    a.tier_slo1 = tier_slo1;
    a.dual = cfg.is_dual ? 1 : 0;
    if (a.dual && wp.cand_words != 4) return BDX_BAD_PLAN();  // (the survivors of pass 1 live in the candidate-word area: four per read)
    const size_t lds = bdx_wave_table_bytes(wp, hist_entries) + (size_t)wp.waves * (size_t)a.per_wave;
    const long long blocks = wave_grid(wp, n_reads);
    if (wp.kend == 3) return bdx_launch_wave_end_aln(&a, wp, lds, blocks, stream);  // (bdx_wave_aln.hip)
    if ((wp.kend == 2) != (a.trim0 == 3 || a.trim1 == 3)) return BDX_BAD_PLAN();
    if (wp.kend == 2) return bdx_launch_wave_end_rev(&a, wp, lds, blocks, stream);  // (bdx_wave_rev.hip)
    return launch_seeded<false, 1, true>(a, wp, lds, blocks, stream);
}

// The general form of the non-split kernel (dual configs, ref_search_range windows) for bdx_launch_wave.
hipError_t bdx_launch_wave_gen(const void *wave_args, const BdxWavePlan &wp, size_t lds, long long blocks, hipStream_t stream) {
    return launch_seeded<false, 0, true>(*(const WaveArgs *)wave_args, wp, lds, blocks, stream);
}
