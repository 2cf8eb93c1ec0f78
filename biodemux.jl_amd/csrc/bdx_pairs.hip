// bdx_pairs.hip — the pairs-mode instantiations of the wave-autonomous kernel (bdx_wave_kernel.h, KB > 0) without a known
// end or with a known end and forward sweeps (KEND = 0 / 1), with their launcher, and the general form of the split-mode
// kernel (ranged configs: SPLIT, GEN), in a translation unit of their own so that the sets of instantiations compile side
// by side.
#include "bdx_wave_kernel.h"

// Pairs mode over the reads of a list (t.in, fetched straight from the batch; no input list: every read of the batch): final
// verdicts at the full budgets for the known-score class (what it cannot answer goes to t.out), candidate masks + windows in
// split mode.  (never a tier 1 with a settle rule: t.tier1 / t.slo are not looked at)
hipError_t bdx_launch_pairs(const BdxDevCfg &cfg, const BdxWavePlan &wp, int hist_entries, const BdxBatch &b, const BdxHandOver &ho, const BdxTierArgs &t,
                            const BdxDevStats *stats) {
    if (wp.pairs_kb <= 0 || !b.seq || !b.off || b.n_reads <= 0 || (t.in.ids && !t.in.count)) return BDX_BAD_PLAN();
    WaveArgs a;
    fill_args(a, cfg, wp, hist_entries, b, ho, t);
    if (stats) {
        if (wp.kend != 3) return BDX_BAD_PLAN();
        a.stats = *stats;
    }
    a.tier = 0;
    a.tier_slo = 0.0;
    a.slot = wp.slot;
    a.vps = wp.slot >> 4;
    a.vps_inv = (65536 + a.vps - 1) / a.vps;
    a.max_len = wp.read_len_hint;
    a.cpr = wp.cpr;
    a.cpr_inv = (65536 + wp.cpr - 1) / wp.cpr;
    a.idmap = t.in.ids;
    a.n_dev = t.in.ids ? t.in.count : nullptr;
    a.dual = (!wp.split && cfg.is_dual) ? 1 : 0;
    if (a.dual && wp.cand_words != 4) return BDX_BAD_PLAN();
    if (wp.split && (!a.cand_out[0] || !a.wins_out[0] || !a.wcnt_out[0])) return BDX_BAD_PLAN();
    if (wp.rw * wp.cpr > 32 * 40 || (wp.slot & 15) || wp.slot < 16 || wp.rw * wp.slot + 16 > wp.span_cap) return BDX_BAD_PLAN();
    // (4 (kb + 2) <= m makes m - kb - 1 >= 16: the first twelve columns of a sweep never need the score)
    if ((wp.pairs_kb > 4 && wp.pairs_kb != 8 && wp.pairs_kb != 9) || wp.nw > 4 || wp.track_from < 12 || wp.n_barcodes > 512 || (wp.groups > 1 && (wp.nw != 4 || wp.split || wp.kend))) return BDX_BAD_PLAN();
    if (wp.pairs_kb >= 8 && (!wp.split || wp.groups > 1)) return BDX_BAD_PLAN();
    if (wp.kend && !wp.d_peq8r) return BDX_BAD_PLAN();
    if (wp.kend == 3) {
        if (wp.pairs_kb > 4 || wp.groups > 1 || wp.split) return BDX_BAD_PLAN();
        return bdx_launch_pairs_aln(&a, wp, b.stream);  // (bdx_wave_aln.hip)
    }
    if (wp.kend && b.out.pass_start != nullptr) return BDX_BAD_PLAN();
    if (wp.kend && b.out.pass_end != nullptr && (a.trim0 == 3 || a.trim1 == 3)) return BDX_BAD_PLAN();
    if ((wp.kend == 2) != (wp.kend && (a.trim0 == 3 || a.trim1 == 3))) return BDX_BAD_PLAN();
    if (wp.kend == 2) return bdx_launch_pairs_rev(&a, wp, b.stream);  // (bdx_wave_rev.hip)
    return pairs_ladder<true>(wp, [&](auto c) {
        using C = decltype(c);
        // (same-diagonal variants 8 / 9: weighted costs, i.e. always split mode)
        if constexpr (C::KB >= 8)
            return launch_wave<16, 12, C::NV, 4, true, C::KB, C::NW>(a, wp, b.stream);
        else  // (many groups, MG: always four mask words, which the checks above made sure of)
            return wp.groups > 1 ? launch_wave<16, 12, C::NV, 4, false, C::KB, 4, true>(a, wp, b.stream)
                   : wp.split    ? launch_wave<16, 12, C::NV, 4, true, C::KB, C::NW>(a, wp, b.stream)
                   : wp.kend     ? launch_wave<16, 12, C::NV, 4, false, C::KB, C::NW, false, 1>(a, wp, b.stream)
                                 : launch_wave<16, 12, C::NV, 4, false, C::KB, C::NW>(a, wp, b.stream);
    });
}

// The split-mode kernel with per-read column windows (ref_search_range), for bdx_launch_wave.
hipError_t bdx_launch_wave_split_gen(const void *wave_args, const BdxWavePlan &wp, hipStream_t stream) {
    return launch_seeded<true, 0, true>(*(const WaveArgs *)wave_args, wp, stream);
}
