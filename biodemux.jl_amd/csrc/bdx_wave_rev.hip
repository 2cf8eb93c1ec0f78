// bdx_wave_rev.hip — the known-trim instantiations of the wave-autonomous kernel with REVERSED sweeps (bdx_wave_kernel.h,
// KEND = 2: configs with a trim_side = 3 pass), seeded and pairs mode, for bdx_launch_wave_end and bdx_launch_pairs, in a
// translation unit of their own so that the sets of instantiations compile side by side.
#include "bdx_wave_kernel.h"

hipError_t bdx_launch_wave_end_rev(const void *wave_args, const BdxWavePlan &wp, hipStream_t stream) {
    return launch_seeded<false, 2, true>(*(const WaveArgs *)wave_args, wp, stream);
}

hipError_t bdx_launch_pairs_rev(const void *wave_args, const BdxWavePlan &wp, hipStream_t stream) {
    if (wp.pairs_kb > 4 || wp.nw > 4 || wp.track_from < 12 || wp.groups > 1 || wp.split || wp.kend != 2) return BDX_BAD_PLAN();
    return launch_pairs_form<false, 2>(*(const WaveArgs *)wave_args, wp, stream);
}
