// bdx_wave.hip — the wave-autonomous kernel (bdx_wave_kernel.h) for known-score configs (the headline form) and for plain split
// mode, both with whole ranges and a single pass (GEN = false), its LDS sizing and their launcher.  Dual and ranged configs
// take the general forms, which bdx_wave_end.hip (non-split) and bdx_pairs.hip (split) hold.
#include "bdx_wave_kernel.h"

// LDS bytes of the shared tables / of one wave's work area (must mirror the kernel's carve-up)
size_t bdx_wave_table_bytes(const BdxWavePlan &wp, int hist_entries) {
    auto al = [](size_t x) { return (x + 31) & ~(size_t)31; };
    return al((size_t)wp.bm_bytes) + al(wp.pairs_kb > 0 ? 0 : (size_t)wp.bm_bytes / 2) + al((size_t)wp.n_ent * 4) + al((size_t)wp.n_barcodes * 36) +
           al(wp.kend >= 2 ? (size_t)wp.n_barcodes * 36 : 0) + 2 * al((size_t)wp.n_barcodes * 4) + al((size_t)hist_entries * 4);
}

size_t bdx_wave_area_bytes(int rw, int span_cap, bool pairs, int hq_cap, int sq_cap, int cand_words, bool winm) {
    const size_t nvec = (size_t)span_cap >> 4;
    const size_t recs = pairs ? 0 : 2 * (size_t)rw * 8 * 4;  // record tables
    const size_t fixed = (size_t)(((rw + 1) * 4 + 15) / 16 * 16) + recs + (size_t)rw * 16 + 3 * (size_t)rw * 4 + 256 +
                         ((pairs || winm) ? 2 * (size_t)rw * 4 + 16 + 2 * (size_t)rw * 20 : 0) + ((winm || pairs) ? (size_t)rw * 4 + 2 * (size_t)rw * 4 : 0);
    const size_t o = fixed + ((nvec + 2 + 3) & ~(size_t)3) * 4 + ((2 * nvec + 6 + 3) & ~(size_t)3) * 4 + ((size_t)hq_cap + (pairs ? 0 : (size_t)sq_cap) + (size_t)rw * (size_t)cand_words) * 4;
    return (o + 31) & ~(size_t)31;
}

hipError_t bdx_launch_wave(const BdxDevCfg &cfg, const BdxWavePlan &wp, int hist_entries, const uint8_t *d_seq, const long long *d_off,
                           long long n_reads, const BdxDevOut &out, unsigned long long *d_counts, int tier1, double tier_slo, uint32_t *list,
                           unsigned int *list_count, hipStream_t stream, int dbg, const BdxWaveSplit *sp, double tier_slo1) {
    if (n_reads <= 0) return hipSuccess;
    WaveArgs a;
    fill_args(a, cfg, wp, hist_entries, out, d_counts, list, list_count, dbg, sp);
    a.seq = d_seq;
    a.off = d_off;
    a.n_reads = n_reads;
    a.tier = tier1;
    a.tier_slo = tier_slo;
    a.tier_slo1 = tier_slo1;
    a.dual = (!wp.split && cfg.is_dual) ? 1 : 0;
    if (a.dual && wp.cand_words != 4) return BDX_BAD_PLAN();  // (the survivors of pass 1 live in the candidate-word area: four per read)
    if (wp.pairs_kb > 0) return BDX_BAD_PLAN();
    if (wp.split && (!sp || !a.cand_out[0] || !a.wins_out[0] || !a.wcnt_out[0])) return BDX_BAD_PLAN();
    const size_t lds = bdx_wave_table_bytes(wp, hist_entries) + (size_t)wp.waves * (size_t)a.per_wave;
    const long long blocks = wave_grid(wp, n_reads);
    // (known-score dual configs and configs with a ref_search_range take the general form of their kernel)
    if (!wp.split && (a.dual || a.ranged)) return bdx_launch_wave_gen(&a, wp, lds, blocks, stream);  // (bdx_wave_end.hip)
    if (wp.split && a.ranged) return bdx_launch_wave_split_gen(&a, wp, lds, blocks, stream);         // (bdx_pairs.hip)
    return seeded_ladder<false>(wp, [&](auto c) {
        using C = decltype(c);
        return wp.split ? launch_wave<C::RW, C::TF, C::NV, C::Q, true, 0, 0, false, 0, false>(a, lds, wp.waves, blocks, stream)
                        : launch_wave<C::RW, C::TF, C::NV, C::Q, false, 0, 0, false, 0, false>(a, lds, wp.waves, blocks, stream);
    });
}
