// bdx_wave_aln.hip — the known-ALIGNMENT instantiations of the wave-autonomous kernel (bdx_wave_kernel.h, KEND = 3: start and
// end of every pass's winner by anchored sweeps — per-pass position outputs and the DemuxStats histograms without the exact
// kernel), seeded and pairs mode, for bdx_launch_wave_end and bdx_launch_pairs, in a translation unit of their own so that
// the sets of instantiations compile side by side.
#include "bdx_wave_kernel.h"

hipError_t bdx_launch_wave_end_aln(const void *wave_args, const BdxWavePlan &wp, hipStream_t stream) {
    if (wp.kend != 3) return BDX_BAD_PLAN();
    return launch_seeded<false, 3, true>(*(const WaveArgs *)wave_args, wp, stream);
}

hipError_t bdx_launch_pairs_aln(const void *wave_args, const BdxWavePlan &wp, hipStream_t stream) {
    if (wp.pairs_kb > 4 || wp.nw > 4 || wp.track_from < 12 || wp.groups > 1 || wp.split || wp.kend != 3) return BDX_BAD_PLAN();
    return launch_pairs_form<false, 3>(*(const WaveArgs *)wave_args, wp, stream);
}
