"""GPU checks of the wave kernel's tile deal (csrc/bdx_wave_kernel.h): wave w of the grid walks the tiles w + k x waves of the
grid, every tile exactly once whatever the numbering of the waves, also where the last round is partial or a wave gets no tile.

The C2 barcode set (96 of 24 nt) at rate 0.1 with 32-read tiles of 150-base reads, on a pretended device of three compute units
(BDX_CU_COUNT=3: up to 3 workgroups of 16 waves; one test with 4 waves per workgroup).  The batch sizes give 1, 2, 3, 4, 47, 48,
49, 95, 96, 97 and 48 x 3 + 5 tiles, each with a full and with a ragged last tile: fewer tiles than waves (waves, and with four
waves per workgroup the planner's smaller grid, without a tile) and last rounds of 0, 1, G - 1, G, G + 1 and waves - 1 tiles for
G workgroups.  Every case compares every output and the counter vector bit for bit with the CPU oracle and with the general
kernel alone (BDX_NO_WAVE); counts[0] == n and the per-read vectors catch a tile dealt twice or never.  The launch log must show
the headline form over the whole batch.
"""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

import fuzz
import helpers as H

pytestmark = pytest.mark.gpu

NTHREADS = min(16, os.cpu_count() or 1)
KNOBS = ("BDX_CU_COUNT", "BDX_WAVE_RW", "BDX_WAVE_WAVES", "BDX_GRID", "BDX_NO_WAVE")
OUTPUTS = ("bc1", "bc2", "keep_start", "keep_end")
HEADLINE = "bdx_wave_kernel<32, 20, 5, 8, false, 0, 0, false, 0, false, false>"
TILES = (1, 2, 3, 4, 47, 48, 49, 95, 96, 97, 48 * 3 + 5)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert os.path.exists(H.bdx.LIB_PATH), "HIP extension missing: run __graft_entry__.build()"


@functools.lru_cache(maxsize=None)
def c2_barcodes():
    from biodemux_jl_amd import synth

    return tuple(synth.make_barcodes(96, 24, seed=synth.SEED))


def c2_config(**kw):
    bcs = c2_barcodes()
    base = dict(bc_seqs=list(bcs), bc_lengths_no_N=[24] * 96, ids=[f"bc{i + 1}" for i in range(96)], max_error_rate=0.1)
    base.update(kw)
    return H.bdx.DemuxConfig(**base)


def oracle(cfg, seq, off):
    oc = H.orc.OracleClassifier(cfg, nthreads=NTHREADS, want_pass=False)
    exp = oc.classify(seq, off)
    return {k: exp[k] for k in OUTPUTS}, oc.counts


def run_device(cfg, seq, off, monkeypatch, env, hint=None, shift=0):
    """-> (outputs, counters, launch log, reads handed on, kernel path) of one classify call under the environment `env`; hint /
    shift: through classify_device with that read-length hint and the bytes `shift` bytes past a 16-byte boundary."""
    import torch

    n = len(off) - 1
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        with H.bdx.HipClassifier(cfg, want_pass=False) as hc:
            if hint is None and shift == 0:
                got = hc.classify(seq, off)
                got = {k: got[k] for k in OUTPUTS}
            else:
                dev = torch.device("cuda:0")
                buf = torch.zeros(len(seq) + 64, dtype=torch.uint8, device=dev)
                base = (-buf.data_ptr()) % 16 + shift
                buf[base:base + len(seq)] = torch.from_numpy(seq).to(dev)
                d_off = torch.from_numpy(off).to(dev)
                if hint is not None:
                    hc.set_read_length_hint(hint)
                d_out = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in OUTPUTS}
                hc.classify_device(buf.data_ptr() + base, d_off.data_ptr(), n, **{k: v.data_ptr() for k, v in d_out.items()})
                hc.sync()
                got = {k: v.cpu().numpy() for k, v in d_out.items()}
            return got, hc.counts, hc.last_launches, hc.last_list_reads, hc.kernel_path
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)


def check_case(key, cfg, seq, off, monkeypatch, env, kernel=HEADLINE, units=None, waves=None, listed=0, hint=None, shift=0):
    """Oracle == wave kernel == general kernel alone on every output and the counters; the wave run's first launch is `kernel`
    over the whole batch (`units` waves in all / workgroups of `waves` waves, where given) and hands on `listed` reads."""
    n = len(off) - 1
    exp, counts = oracle(cfg, seq, off)
    got, got_counts, launches, handed, path = run_device(cfg, seq, off, monkeypatch, env, hint=hint, shift=shift)
    what = f"{key} [{path}] {launches}"
    fuzz.assert_same(got, exp, what)
    assert np.array_equal(got_counts, counts) and int(got_counts[0]) == n, what
    first = launches[0]
    assert first["kernel"] == kernel and first["reads"] == n and first["tile"] == 32 and not first["list"], what
    if units is not None:
        assert first["units"] == units and first["threads"] * first["blocks"] == 64 * units, what
    if waves is not None:  # (the grid is the planner's: as many workgroups as it keeps resident, no more than give every wave a tile)
        assert first["threads"] == 64 * waves and first["units"] == first["blocks"] * waves and 1 <= first["blocks"] <= -(-n // (32 * waves)), what
    assert handed == listed, f"{what}: {handed} reads handed on"
    ref, ref_counts, _, _, ref_path = run_device(cfg, seq, off, monkeypatch, dict(env, BDX_NO_WAVE=1), hint=hint, shift=shift)
    assert "wave" not in ref_path, ref_path
    fuzz.assert_same(got, ref, what + " against " + ref_path)
    assert np.array_equal(got_counts, ref_counts), what + " against " + ref_path
    return exp


@functools.lru_cache(maxsize=None)
def _batch():
    from biodemux_jl_amd import synth

    seq, off, _ = synth.make_reads(c2_barcodes(), max(TILES) * 32, 150, seed=synth.SEED + 12)
    return seq, off


def _prefix(n):
    seq, off = _batch()
    return seq[:off[n]].copy(), off[:n + 1].copy()


def _units(tiles, waves):
    return min(3, -(-tiles // waves)) * waves  # (the planner's grid: no more workgroups than give every wave one tile)


@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("tiles", TILES)
def test_every_tile_dealt_once(tiles, ragged, monkeypatch):
    n = 32 * tiles - (13 if ragged else 0)
    seq, off = _prefix(n)
    exp = check_case(("deal", tiles, ragged), c2_config(), seq, off, monkeypatch, {"BDX_CU_COUNT": 3, "BDX_WAVE_RW": 32}, units=_units(tiles, 16))
    if tiles >= 47:
        assert 0.5 < (exp["bc1"] > 0).mean() < 1.0


@pytest.mark.parametrize("tiles,ragged", [(3, True), (13, False), (61, True), (97, False), (149, True)], ids=["3r", "13", "61r", "97", "149r"])
def test_four_waves_per_workgroup(tiles, ragged, monkeypatch):
    """Workgroups of 4 waves, several to a compute unit (the planner's grid: as many as stay resident, no more than give every
    wave a tile): fewer tiles than waves (waves without a tile in the last workgroup), and several rounds with a partial last
    one."""
    n = 32 * tiles - (7 if ragged else 0)
    seq, off = _prefix(n)
    check_case(("deal4", tiles, ragged), c2_config(), seq, off, monkeypatch, {"BDX_CU_COUNT": 3, "BDX_WAVE_RW": 32, "BDX_WAVE_WAVES": 4}, waves=4)
