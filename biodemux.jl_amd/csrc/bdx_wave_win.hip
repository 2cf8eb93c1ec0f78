// bdx_wave_win.hip — the WINDOW-mode instantiations of the wave-autonomous kernel (bdx_wave_kernel.h, WINM: single-pass
// known-score configs whose ref_search_range window is much shorter than their reads — scattered tiles that hold only the
// windows) and their launcher, in a translation unit of their own so that the sets of instantiations compile side by side.
#include "bdx_wave_kernel.h"

// Window mode: a single-pass known-score config whose column window is much shorter than its reads; tier 1 or the only
// wave launch of the config, same outputs and the same list as bdx_launch_wave.
hipError_t bdx_launch_wave_win(const BdxDevCfg &cfg, const BdxWavePlan &wp, int hist_entries, const BdxBatch &b, const BdxTierArgs &t) {
    if (b.n_reads <= 0) return hipSuccess;
    if (!wp.winm || wp.pairs_kb > 0 || wp.split || wp.kend || cfg.is_dual || !wp.ranged || wp.slot < 16 || (wp.slot & 15)) return BDX_BAD_PLAN();
    WaveArgs a;
    fill_args(a, cfg, wp, hist_entries, b, BdxHandOver{}, t);
    a.ranged = 0;     // (the window is resolved by the tile loader: downstream the window IS the read)
    {
        const BdxDevRange &dr = cfg.pass[0].ref_search;
        const long long LIM = 1LL << 28;
        if (dr.start_offset < -LIM || dr.start_offset > LIM || dr.end_offset < -LIM || dr.end_offset > LIM) return BDX_BAD_PLAN();
        a.win_sfe = dr.start_from_end ? 1 : 0;
        a.win_so = (int)dr.start_offset;
        a.win_efe = dr.end_from_end ? 1 : 0;
        a.win_eo = (int)dr.end_offset;
    }
    a.scan_gpr = 0;
    a.slot = wp.slot;
    a.vps = wp.slot >> 4;
    a.vps_inv = (65536 + a.vps - 1) / a.vps;
    a.idmap = nullptr;
    a.n_dev = nullptr;
    if (wp.rw * wp.slot + 16 > wp.span_cap) return BDX_BAD_PLAN();
    return launch_seeded<false, 0, true, true>(a, wp, b.stream);
}
