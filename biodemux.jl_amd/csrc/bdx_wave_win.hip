// bdx_wave_win.hip — the WINDOW-mode instantiations of the wave-autonomous kernel (bdx_wave_kernel.h, WINM: single-pass
// known-score configs whose ref_search_range window is much shorter than their reads — scattered tiles that hold only the
// windows) and their launcher, in a translation unit of their own so that the sets of instantiations compile side by side.
#include "bdx_wave_kernel.h"

// Window mode: a single-pass known-score config whose column window is much shorter than its reads; tier 1 or the only
// wave launch of the config, same outputs and the same list as bdx_launch_wave.
hipError_t bdx_launch_wave_win(const BdxDevCfg &cfg, const BdxWavePlan &wp, int hist_entries, const uint8_t *d_seq, const long long *d_off,
                               long long n_reads, const BdxDevOut &out, unsigned long long *d_counts, int tier1, double tier_slo, uint32_t *list,
                               unsigned int *list_count, hipStream_t stream, int dbg) {
    if (n_reads <= 0) return hipSuccess;
    if (!wp.winm || wp.pairs_kb > 0 || wp.split || wp.kend || cfg.is_dual || !wp.ranged || wp.slot < 16 || (wp.slot & 15)) return BDX_BAD_PLAN();
    WaveArgs a;
    fill_args(a, cfg, wp, hist_entries, out, d_counts, list, list_count, dbg, nullptr);
    a.seq = d_seq;
    a.off = d_off;
    a.n_reads = n_reads;
    a.tier = tier1;
    a.tier_slo = tier_slo;
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
    a.per_wave = (int)bdx_wave_area_bytes(wp.rw, wp.span_cap, false, wp.hq_cap, wp.sq_cap, 0, true);
    const size_t lds = bdx_wave_table_bytes(wp, hist_entries) + (size_t)wp.waves * (size_t)a.per_wave;
    const long long blocks = wave_grid(wp, n_reads);
    if (wp.rw * wp.slot + 16 > wp.span_cap) return BDX_BAD_PLAN();
    return launch_seeded<false, 0, true, true>(a, wp, lds, blocks, stream);
}
