"""One context driven through both entry points in turn: what a host call knows of its batch (the longest read, a window
upload's per-read windows, the scratch half its copy kernel cleared, its launch log) is handed to that call as a value and must
not reach the next one.  A window-upload host call, a small-batch host call, a bdx_classify_device call on torch-owned buffers
with no hint (its kernel_path is the one a fresh context reports for the batch), a host call that fails validation, the device
call again, the window upload again — outputs and counters against the oracle after every call, the statistics tables at the
end.  The forms the host calls take are asserted through the library's counters and the thresholds they sit behind, so a
changed threshold cannot turn the sequence into six calls of one kind.  Everything runs on the library's own stream."""
import ctypes as C

import numpy as np
import pytest

import fuzz
import helpers as H
from biodemux_jl_amd import hipabi, synth
from biodemux_jl_amd.classification import DemuxStats
from test_stats_gpu import _same

pytestmark = pytest.mark.gpu
VERDICTS = ("bc1", "bc2", "keep_start", "keep_end")
BCS = synth.make_barcodes(24, 24, seed=20261019, min_hamming=7)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"


def _reads(n, lo, hi, seed):
    """Ragged reads with a barcode planted inside the first 200 columns of most of them."""
    seq, off, _ = synth.make_ragged_reads(BCS, n, lo, hi, seed=seed, plant_lo=0, plant_hi=min(lo - 24, 170))
    return np.ascontiguousarray(seq), np.ascontiguousarray(off)


@pytest.fixture(scope="module")
def batches():
    long_reads, short_reads = _reads(3000, 2000, 2600, 1), _reads(4000, 60, 150, 2)
    for (seq, off), lo, hi in ((long_reads, 2000, 2600), (short_reads, 60, 150)):
        lens = off[1:] - off[:-1]
        assert lens.min() >= lo and lens.max() <= hi and off[0] == 0
    return long_reads, short_reads


def _device_call(hc, tensors, n):
    d_seq, d_off, d_out = tensors
    hc.classify_device(d_seq.data_ptr(), d_off.data_ptr(), n, **{k: v.data_ptr() for k, v in d_out.items()})
    hc.sync()
    return {k: v.cpu().numpy() for k, v in d_out.items()}


@pytest.mark.parametrize("summary", [False, True], ids=["plain", "summary"])
def test_host_and_device_calls_share_a_context(summary, batches):
    import torch

    (lseq, loff), (sseq, soff) = batches
    nl, ns = len(loff) - 1, len(soff) - 1
    cfg = H.bdx.DemuxConfig(bc_seqs=BCS, bc_lengths_no_N=[24] * 24, ids=["b%d" % i for i in range(24)], max_error_rate=0.1,
                            ref_search_range=H.bdx.parse_dynamic_range("1:200"), summary=summary)
    # the forms these lengths select (bdx_classify_host): long reads — at least 512 bases on average and windows (200 columns) +
    # 16 bytes per read that are less than half the bytes: the window upload; short reads — too short for it, and bytes + offsets
    # within 2 MiB: one staged copy whose kernel also clears the call's scratch half
    assert loff[-1] >= nl * 512 and 2 * 200 * nl + 16 * nl <= loff[-1]
    assert soff[-1] < ns * 512 and soff[-1] + (ns + 1) * 8 <= 2 << 20
    # the oracle once per batch; the counters and the statistics of the sequence add up from these
    oracle = {}
    for name, (seq, off) in (("long", (lseq, loff)), ("short", (sseq, soff))):
        oc = H.orc.OracleClassifier(cfg, nthreads=16, want_pass=True)
        oracle[name] = (oc.classify(seq, off), oc.counts.copy())
    stats, total = DemuxStats(), np.zeros_like(oracle["long"][1])

    def expect(name):
        nonlocal total
        exp, counts = oracle[name]
        stats.add_pass_outputs(exp, float(cfg.min_delta))
        total = total + counts
        return exp, total

    dev = torch.device("cuda:0")
    tensors = (torch.from_numpy(sseq).to(dev), torch.from_numpy(soff).to(dev), {k: torch.empty(ns, dtype=torch.int32, device=dev) for k in VERDICTS})
    torch.cuda.synchronize()  # (torch's stream made the tensors; the classifier runs on its own)
    with H.bdx.HipClassifier(cfg, want_pass=False) as fresh:
        fresh_out = _device_call(fresh, tensors, ns)
        fresh_path, fresh_launches = fresh.kernel_path, [(ln["family"], ln["kernel"], ln["blocks"]) for ln in fresh.last_launches]
    assert "wave" in fresh_path or "bitpar" in fresh_path, fresh_path  # a filtered call: it takes a scratch half

    with H.bdx.HipClassifier(cfg, want_pass=False) as hc:
        def check(got, exp, counts, what):
            what = f"{what} [{hc.kernel_path}]"
            fuzz.assert_same(got, {k: exp[k] for k in VERDICTS}, what)
            assert np.array_equal(hc.counts, counts), f"{what}: counters"
            assert hc.rejected_windows == 0 and hc.pipelined_calls == 0, what

        # 1. long reads through the host entry point: the window upload
        exp_long, counts = expect("long")
        check(hc.classify(lseq, loff), exp_long, counts, "1. window upload")
        assert hc.window_uploads == 1
        long_path = hc.kernel_path
        assert (exp_long["bc1"] > 0).mean() > 0.3
        # 2. short reads through the host entry point: the small-batch form
        exp_short, counts = expect("short")
        check(hc.classify(sseq, soff), exp_short, counts, "2. small batch")
        assert hc.window_uploads == 1 and hc.staged_downloads == 0
        assert (exp_short["bc1"] > 0).mean() > 0.3 and (exp_short["bc1"] == 0).any()
        # 3. the same reads through the device entry point, no hint: nothing is left over from the host calls
        _, counts = expect("short")
        first = _device_call(hc, tensors, ns)
        check(first, exp_short, counts, "3. device call")
        assert hc.kernel_path == fresh_path and hc.kernel_path != long_path, (hc.kernel_path, fresh_path, long_path)
        assert [(ln["family"], ln["kernel"], ln["blocks"]) for ln in hc.last_launches] == fresh_launches
        assert all(np.array_equal(first[k], fresh_out[k]) for k in VERDICTS)
        # 4. a host call whose offsets decrease once: refused, nothing counted
        bad = soff.copy()
        bad[ns // 2] = bad[ns // 2 - 1] - 3
        o = hipabi.BdxOutputs()
        outs = {k: np.full(ns, -77, dtype=np.int32) for k in VERDICTS}
        for k, v in outs.items():
            setattr(o, k, v.ctypes.data)
        assert hc.lib.bdx_classify_host(hc.h, sseq.ctypes.data, bad.ctypes.data, ns, C.byref(o)) == -1  # BDX_E_INVALID
        assert b"non-decreasing" in hc.lib.bdx_last_error(hc.h)
        assert np.array_equal(hc.counts, counts)
        # 5. the device call again
        _, counts = expect("short")
        again = _device_call(hc, tensors, ns)
        check(again, exp_short, counts, "5. device call again")
        assert hc.kernel_path == fresh_path and all(np.array_equal(again[k], first[k]) for k in VERDICTS)
        # 6. the long reads again
        _, counts = expect("long")
        check(hc.classify(lseq, loff), exp_long, counts, "6. window upload again")
        assert hc.window_uploads == 2 and hc.kernel_path == long_path
        if summary:
            got = DemuxStats()
            got.add_device_tables(hc.stats_tables(), cfg)
            _same(got, stats)
            assert sum(got.bc1_pos_counts.values()) == int(counts[1]) and max(got.bc1_pos_counts) > 150
