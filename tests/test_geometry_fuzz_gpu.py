"""The fuzz families and the bench legs at PRODUCTION tile geometry.

The launch planner sizes every persistent kernel from reads per compute unit.  The randomised tests of
test_gpu_parity.py classify 600..1500 reads on a 256-CU device: the wave kernel then runs 8-read tiles, the fused
filter 16-read tiles, and no wave or workgroup ever walks a second tile.  Production batches (2^19 reads per pipeline
batch, 10 M per bench step) take 32-read wave tiles, fused tiles of 128 / 256 reads, and every wave walks many of them.
Here the same generators (new seeds) run with the device shrunk by the developer switches read in bdx_create:

  cu1    BDX_CU_COUNT=1 at ~4 k reads: the largest tiles, many tiles per wave and per fused workgroup
  cu3    BDX_CU_COUNT=3, BDX_WAVE_RW=16, BDX_WAVE_WAVES=4: 16-read tiles dealt unevenly over 3 x 4 x k waves
  grid2  BDX_CU_COUNT=1, BDX_GRID=2: two workgroups drain the fused kernel's tile queue

and everything is compared bit for bit with the oracle.  HipClassifier.last_launches (bdx_last_launches) says what
each call enqueued: every case asserts that the persistent stages it steers walked at least two tiles per wave /
workgroup, every family asserts the union of the shapes it reached, and every name must exist in the code object."""
import functools
import os

import numpy as np
import pytest

import fuzz
import helpers as H
from kernel_lattice import code_object_kernels
from biodemux_jl_amd.classification import DemuxStats

pytestmark = pytest.mark.gpu

NTHREADS = min(16, os.cpu_count() or 1)
# (env, reads, the families whose whole-batch launches must walk >= 2 tiles per wave / workgroup).  cu1: 4 096 reads make
# even 256-read fused tiles >= 16 tiles for the <= 8 workgroups of one CU; cu3 steers the wave kernel's dealing only (the
# fused grid of 3 CUs at a few thousand reads keeps one tile per workgroup: cu1 and grid2 cover that kernel)
SETTINGS = {
    "cu1": ({"BDX_CU_COUNT": "1"}, 4200, {"wave", "pairs", "bitpar"}),
    "cu3": ({"BDX_CU_COUNT": "3", "BDX_WAVE_RW": "16", "BDX_WAVE_WAVES": "4"}, 2400, {"wave", "pairs"}),
    "grid2": ({"BDX_CU_COUNT": "1", "BDX_GRID": "2"}, 2000, {"wave", "pairs", "bitpar"}),
}
KNOBS = ("BDX_CU_COUNT", "BDX_WAVE_RW", "BDX_WAVE_WAVES", "BDX_GRID")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert os.path.exists(H.bdx.LIB_PATH), "HIP extension missing: run __graft_entry__.build()"


# ---- the kernels the code object holds (kernel_lattice.py) ----

def test_code_object_reader_sees_the_instantiation_lattice():
    ks = code_object_kernels()
    wave = [k for k in ks if k.startswith("bdx_wave_kernel<")]
    assert len([k for k in wave if k.startswith("bdx_wave_kernel<32,")]) >= 32, sorted(wave)[:8]
    assert "bdx_bitpar_kernel<256, 256, true, false, 5, 0>" in ks and "bdx_generic_kernel<256, 24, true, true>" in ks


# ---- launches ----
def _check_launches(launches, steer, what):
    """Every recorded name exists in the code object; every whole-batch launch of a steered persistent family walked at
    least two tiles per wave / workgroup (the wave kernel deals its tiles round robin: tiles >= 2 x waves gives EVERY wave
    a second tile; the fused kernel's queue hands out as many on average).  A list launch's length lives on the device."""
    ks = code_object_kernels()
    for ln in launches:
        assert ln["kernel"] in ks, f"{what}: launched {ln['kernel']} is not in the code object"
        if ln["family"] in steer and not ln["list"] and ln["units"] > 0:
            tiles = -(-ln["reads"] // ln["tile"])
            assert tiles >= 2 * ln["units"], f"{what}: vacuous geometry {ln} ({tiles} tiles over {ln['units']} units)"


@functools.lru_cache(maxsize=None)
def _case(gen_name, seed, n):
    return getattr(fuzz, gen_name)(seed, n_reads=n)


@functools.lru_cache(maxsize=None)
def _oracle(gen_name, seed, n, want_pass):
    cfg, seq, off = _case(gen_name, seed, n)
    oc = H.orc.OracleClassifier(cfg, nthreads=NTHREADS, want_pass=want_pass)
    exp = oc.classify(seq, off)
    stats = None
    if want_pass and cfg.summary:
        stats = DemuxStats()
        stats.add_pass_outputs(exp, float(cfg.min_delta))
    return exp, oc.counts, stats


def _same_stats(a: DemuxStats, b: DemuxStats, what):
    for t in ("bc1", "bc2"):
        for k in ("pos_counts", "len_counts", "score_counts", "per_bc_pos_counts", "per_bc_len_counts", "per_bc_score_counts"):
            f = f"{t}_{k}"
            assert getattr(a, f) == getattr(b, f), f"{what}: statistics table {f}"


def _set_knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# family -> seeds (new ones: test_gpu_parity.py runs 0..59, 7100.. and the campaign its own), want_pass variants (those of the
# family's test in test_gpu_parity.py)
FAMILIES = {
    "random_case": (range(31000, 31032), (True,)),
    "random_case_many_barcodes": (range(32000, 32020), (True, False)),
    "random_case_tiers": (range(33000, 33020), (True, False)),
    "random_case_wide": (range(34000, 34016), (True, False)),
    "random_case_band": (range(35000, 35020), (True, False)),
    "random_case_band_long": (range(36000, 36016), (True,)),
}
_SEEN = {f: [] for f in FAMILIES}  # family -> launches of every call
_RAN = {f: set() for f in FAMILIES}  # family -> seeds that ran (the union is checked once all of them did)


def family_shapes(launches) -> dict:
    """The union of what `launches` ran: wave {(form, RW)} (form: the template arguments after RW, TF, NV, Q — split,
    pairs KB / NW, MG, KEND, GEN, WINM), pairs {(KB, NW, KEND)}, fused tile sizes R."""
    wave, pairs, fused = set(), set(), set()
    for ln in launches:
        a = ln["kernel"].split("<")[1].rstrip(">").split(", ")
        if ln["family"] in ("wave", "pairs"):
            wave.add((", ".join(a[4:]), int(a[0])))
            if ln["family"] == "pairs":
                pairs.add((int(a[5]), int(a[6]), int(a[8])))
        elif ln["family"] == "bitpar":
            fused.add(int(a[1]))
    return dict(wave=wave, pairs=pairs, fused=fused)


# Shapes each family must reach (union over its seeds and the three settings; measured on an MI355X): every form of the
# wave kernel listed with the tile sizes it must run, the pairs-mode (KB, NW, KEND) variants, the fused tile sizes.  The
# pairs mode always runs 16-read tiles (size_pairs); other forms take 32-read tiles wherever the planner gives them to a
# production batch of the same per-CU size (configs with large tables keep 16: more resident waves).
EXPECTED_SHAPES = {
    "random_case": dict(
        wave={},
        pairs=set(), fused={16, 32, 64, 128}),
    "random_case_many_barcodes": dict(
        wave={
            "false, 0, 0, false, 0, false, false": {16, 32},
            "false, 0, 0, false, 0, true, false": {16, 32},
            "false, 0, 0, false, 1, true, false": {16, 32},
            "false, 0, 0, false, 2, true, false": {16},
            "false, 0, 0, false, 3, true, false": {16, 32},
            "false, 4, 4, false, 0, true, false": {16},
            "false, 4, 4, true, 0, true, false": {16},
            "true, 0, 0, false, 0, false, false": {16, 32},
            "true, 0, 0, false, 0, true, false": {16, 32},
            "true, 4, 2, false, 0, true, false": {16},
        },
        pairs={(4, 2, 0), (4, 4, 0)}, fused={4, 8, 16, 32, 64}),
    "random_case_tiers": dict(
        wave={
            "false, 0, 0, false, 0, false, false": {16, 32},
            "false, 0, 0, false, 0, true, false": {16},
            "false, 0, 0, false, 3, true, false": {16, 32},
            "false, 3, 3, false, 0, true, false": {16},
            "false, 3, 4, false, 0, true, false": {16},
            "true, 0, 0, false, 0, false, false": {16, 32},
            "true, 0, 0, false, 0, true, false": {16},
            "true, 3, 3, false, 0, true, false": {16},
        },
        pairs={(3, 3, 0), (3, 4, 0)}, fused={4, 16, 32, 64}),
    "random_case_wide": dict(
        wave={
            "false, 0, 0, false, 0, false, false": {16, 32},
            "false, 0, 0, false, 1, true, false": {16, 32},
            "false, 0, 0, false, 3, true, false": {16, 32},
            "false, 3, 4, false, 1, true, false": {16},
            "false, 3, 4, false, 3, true, false": {16},
            "false, 4, 4, false, 0, true, false": {16},
            "false, 4, 4, true, 0, true, false": {16},
            "true, 0, 0, false, 0, false, false": {16},
        },
        pairs={(3, 4, 1), (3, 4, 3), (4, 4, 0)}, fused={4, 8, 16, 32, 64}),
    "random_case_band": dict(
        wave={
            "false, 0, 0, false, 0, false, false": {16, 32},
            "false, 0, 0, false, 0, true, false": {16},
            "false, 0, 0, false, 1, true, false": {16, 32},
            "false, 0, 0, false, 2, true, false": {16, 32},
            "false, 0, 0, false, 3, true, false": {16, 32},
            "false, 3, 3, false, 1, true, false": {16},
            "false, 3, 3, false, 3, true, false": {16},
            "false, 3, 4, false, 2, true, false": {16},
            "false, 3, 4, false, 3, true, false": {16},
            "false, 4, 2, false, 1, true, false": {16},
            "false, 4, 2, false, 2, true, false": {16},
            "false, 4, 2, false, 3, true, false": {16},
            "true, 0, 0, false, 0, false, false": {16, 32},
            "true, 0, 0, false, 0, true, false": {16, 32},
        },
        pairs={(3, 3, 1), (3, 3, 3), (3, 4, 2), (3, 4, 3), (4, 2, 1), (4, 2, 2), (4, 2, 3)}, fused={4, 8, 16, 32, 64}),
    "random_case_band_long": dict(
        wave={},
        pairs=set(), fused={16, 32, 64, 128}),
}


def _family_union_checks(family):
    got = family_shapes(_SEEN[family])
    exp = EXPECTED_SHAPES[family]
    msg = f"{family}: reached {sorted(got['wave'])} pairs {sorted(got['pairs'])} fused {sorted(got['fused'])}"
    for form, rws in exp["wave"].items():
        for rw in rws:
            assert (form, rw) in got["wave"], f"{family}: wave form <{form}> never ran {rw}-read tiles; {msg}"
    for form, rw in got["wave"]:  # (BDX_WAVE_RW=16 of the cu3 setting: every form reached also runs 16-read tiles)
        assert (form, 16) in got["wave"], f"{family}: wave form <{form}> never ran 16-read tiles; {msg}"
    assert got["pairs"] >= exp["pairs"], msg
    assert got["fused"] >= exp["fused"], msg


def run_case(family, seed, monkeypatch):
    """One fuzz case under every setting, with and without per-pass outputs where the family's test does both: bit for
    bit against the oracle (verdicts, per-pass outputs incl. the doubles, counters, the statistics tables of a summary
    config); the launches are checked and collected in _SEEN."""
    want = FAMILIES[family][1]
    for setting, (env, n0, steer) in SETTINGS.items():
        n = n0 + (seed % 7) * 37  # (ragged last tiles)
        cfg, seq, off = _case(family, seed, n)
        _set_knobs(monkeypatch, env)
        for want_pass in want:
            exp, counts, stats = _oracle(family, seed, n, want_pass)
            what = f"{family} seed {seed} {setting} ({n} reads) pass outputs {want_pass}"
            with H.bdx.HipClassifier(cfg, want_pass=want_pass) as hc:
                got = hc.classify(seq, off)
                launches = hc.last_launches
                fuzz.assert_same(got, exp, f"{what} [{hc.kernel_path}] {launches}")
                assert np.array_equal(hc.counts, counts), f"{what}: counters"
                if cfg.summary:
                    ref = stats if stats is not None else _oracle(family, seed, n, True)[2]
                    dev = DemuxStats()
                    dev.add_device_tables(hc.stats_tables(), cfg)
                    _same_stats(dev, ref, what)
                _check_launches(launches, steer, what)
                _SEEN[family].extend(dict(ln, setting=setting) for ln in launches)
    _set_knobs(monkeypatch, {})
    _RAN[family].add(seed)


@pytest.mark.parametrize("family,seed", [(f, s) for f, (seeds, _) in FAMILIES.items() for s in seeds])
def test_fuzz_at_production_geometry(family, seed, monkeypatch):
    run_case(family, seed, monkeypatch)
    if seed == FAMILIES[family][0][-1] and len(_RAN[family]) == len(FAMILIES[family][0]):
        _family_union_checks(family)


def test_batches_of_other_sizes_in_a_row_on_one_context(monkeypatch):
    """One context, one CU: batches of different sizes in a row — the scratch ping-pong, the tile queues and the wave
    plans are reused at multi-tile grids (a larger batch after a smaller one, a tiny one in between)."""
    _set_knobs(monkeypatch, {"BDX_CU_COUNT": "1"})
    for family, seed in (("random_case_many_barcodes", 32100), ("random_case_tiers", 33100), ("random_case_band", 35100)):
        cfg, seq, off = _case(family, seed, 5000)
        oc = H.orc.OracleClassifier(cfg, nthreads=NTHREADS, want_pass=False)
        with H.bdx.HipClassifier(cfg) as hc:
            for lo, hi in ((0, 1800), (1800, 5000), (100, 137), (37, 4400), (4400, 5000)):
                s, o = seq[off[lo]:off[hi]], off[lo:hi + 1] - off[lo]
                exp = oc.classify(s, o)
                got = hc.classify(s, o)
                fuzz.assert_same(got, exp, f"{family} seed {seed} reads {lo}:{hi} [{hc.kernel_path}]")
                _check_launches(hc.last_launches, {"wave", "pairs"} if hi - lo >= 1024 else set(), f"{family} {lo}:{hi}")
            assert np.array_equal(hc.counts, oc.counts), family
    _set_knobs(monkeypatch, {})


# ---- the bench legs: the suite runs the kernels production runs ----
LEGS = ("C2", "C2d", "C4", "C5", "C2t5", "C2r60", "C2dual")
PIPELINE_BATCH = 1 << 19  # core.DEFAULT_BATCH_READS


def _device_launches(cfg, outputs, read_len, d_seq, d_off, n, env, monkeypatch):
    """One classify_device call the way bench.py makes it (read-length hint, the leg's outputs): the outputs (host) and
    the launch log."""
    import torch

    _set_knobs(monkeypatch, env)
    try:
        with H.bdx.HipClassifier(cfg) as hc:
            hc.set_read_length_hint(read_len)
            d_out = {k: torch.empty(n, dtype=torch.int32, device=d_seq.device) for k in outputs}
            hc.classify_device(d_seq.data_ptr(), d_off.data_ptr(), n, **{k: v.data_ptr() for k, v in d_out.items()})
            hc.sync()
            return {k: v.cpu().numpy() for k, v in d_out.items()}, hc.counts, hc.last_launches, hc.kernel_path
    finally:
        _set_knobs(monkeypatch, {})


@pytest.mark.parametrize("leg", LEGS)
def test_bench_leg_scaled_to_one_cu_runs_the_production_kernels(leg, monkeypatch):
    """Each bench leg's workload (bench.build_workload, exactly its outputs): one call at the production size — the bench's
    n and a 2^19-read pipeline batch — on the real device; then n / (its CUs) reads of the same workload at BDX_CU_COUNT=1 must
    enqueue the identical list of instantiations (family + template arguments, in order), and equal the oracle on EVERY
    read.  (The production batch is the scaled one repeated: the plan depends on the reads' count and length, not on what
    they hold.)  No decision of the planner depends on absolute n at these sizes: tier 0's list is planned for n / 16 reads
    (same per-CU ratio in both runs), the carry gate is n < 2^30 for both."""
    import torch

    import bench

    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count  # (256 on an MI355X)
    n_prod = {"C5": 400_000}.get(leg, 10_000_000)
    sizes = sorted({n_prod, min(n_prod, PIPELINE_BATCH)}, reverse=True)
    n_small = n_prod // cus
    wl = bench.build_workload(leg, n_small, 0)
    cfg, seq, off, outputs, read_len = wl["cfg"], wl["seq"], wl["off"], wl["outputs"], wl["read_len"]
    d_small = torch.from_numpy(seq).to(dev)
    reps = -(-n_prod // n_small)
    total = int(off[-1])
    d_seq = d_small.repeat(reps)
    base = torch.from_numpy(off[:-1]).to(dev)
    d_off = (torch.arange(reps, device=dev, dtype=torch.int64)[:, None] * total + base[None, :]).reshape(-1)
    d_off = torch.cat([d_off, torch.tensor([reps * total], device=dev, dtype=torch.int64)])
    for n in sizes:
        _, _, prod, prod_path = _device_launches(cfg, outputs, read_len, d_seq, d_off, n, {}, monkeypatch)
        k = n // cus
        s, o = seq[: off[k]], off[: k + 1]
        got, counts, small, path = _device_launches(cfg, outputs, read_len, torch.from_numpy(s).to(dev), torch.from_numpy(o).to(dev),
                                                    k, {"BDX_CU_COUNT": "1"}, monkeypatch)
        inst = lambda log: [(ln["family"], ln["kernel"]) for ln in log]  # noqa: E731
        assert inst(small) == inst(prod), f"{leg}: {k} reads on 1 CU [{path}] vs {n} on the device [{prod_path}]:\n{small}\n{prod}"
        assert prod, leg
        _check_launches(prod, set(), f"{leg} {n} reads")
        _check_launches(small, {"wave", "pairs"}, f"{leg} {k} reads on 1 CU")
        oc = H.orc.OracleClassifier(cfg, nthreads=NTHREADS, want_pass=False)
        exp = oc.classify(s, o)
        for key in outputs:
            assert got[key].shape == exp[key].shape == (k,), (leg, key)
            bad = np.flatnonzero(got[key] != exp[key])
            assert bad.size == 0, f"{leg} ({k} reads on 1 CU): {key} differs at reads {bad[:8].tolist()}"
        assert np.array_equal(counts, oc.counts), f"{leg} ({k} reads): counters"
