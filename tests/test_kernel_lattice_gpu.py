"""One case per classify instantiation that has a recipe (kernel_lattice.py): on one context, a main batch and an edge
batch built for the instantiation's cell.  Each call must launch exactly that kernel over the whole batch, at two or more
tiles per resident wave with a ragged last tile; the kernel must answer most reads itself; and verdicts, per-pass outputs
(doubles by bit pattern) and counters must equal the oracle bit for bit.  The autouse poison and refused-window fixtures
of conftest.py watch the hand-over of the split forms.  The fused filter's instantiations run as the full-budget launch
of a known-score call, the exact kernel's behind the filter of a split call (or alone): there the whole batch is a thread
per read, three whole workgroups and a ragged one.  Window mode's instantiations run on batches planned at a hinted read
length, the general forms' on dual and ranged configs in each of their argument states, the pairs mode's over the list of
reads tier 1 leaves (check_list_launch)."""
import os

import numpy as np
import pytest

import fuzz
import helpers as H
import kernel_lattice as KL

pytestmark = pytest.mark.gpu

NTHREADS = min(16, os.cpu_count() or 1)
KNOBS = ("BDX_CU_COUNT", "BDX_WAVE_RW", "BDX_WAVE_WAVES", "BDX_GRID") + tuple(k for k in KL.SWITCHES if k != "BDX_CU_COUNT")
assert os.path.exists(H.bdx.LIB_PATH), "HIP extension missing: run __graft_entry__.build()"
CASES = [n for n in KL.classify_kernels() if isinstance(KL.recipe(n), KL.Recipe)]
CELL_CASES = [n for n in KL.classify_kernels() if isinstance(KL.recipe(n), KL.CellRecipe)]
WIN_CASES = [n for n in KL.classify_kernels() if isinstance(KL.recipe(n), KL.WinRecipe)]
GEN_CASES = [n for n in KL.classify_kernels() if isinstance(KL.recipe(n), KL.GenRecipe)]
PAIRS_CASES = [n for n in KL.classify_kernels() if isinstance(KL.recipe(n), KL.PairsRecipe)]
STATS_FIELDS = [f"bc1_{k}" for k in ("pos_counts", "len_counts", "score_counts", "per_bc_pos_counts", "per_bc_len_counts", "per_bc_score_counts")]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert os.path.exists(H.bdx.LIB_PATH), "HIP extension missing: run __graft_entry__.build()"


def _set_knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def check_launches(launches, target, n_reads, what):
    """The target ran over the whole batch (not a list launch), walking >= 2 tiles per unit, the last one ragged; every
    launched name is in the code object."""
    ks = KL.code_object_kernels()
    for ln in launches:
        assert ln["kernel"] in ks, f"{what}: launched {ln['kernel']} is not in the code object"
    whole = [ln for ln in launches if ln["kernel"] == target and not ln["list"]]
    assert whole, f"{what}: {target} did not run over the whole batch: {launches}"
    for ln in whole:
        assert ln["reads"] == n_reads, f"{what}: {ln}"
        tiles = -(-ln["reads"] // ln["tile"])
        assert ln["units"] > 0 and tiles >= 2 * ln["units"], f"{what}: vacuous geometry {ln} ({tiles} tiles over {ln['units']} units)"
        assert ln["reads"] % ln["tile"] == 1, f"{what}: the last tile is not ragged: {ln}"


@pytest.mark.parametrize("name", CASES)
def test_instantiation_equals_the_oracle(name, monkeypatch):
    rc = KL.recipe(name)
    cfg = rc.config()
    _set_knobs(monkeypatch, rc.env)
    oc = H.orc.OracleClassifier(cfg, nthreads=NTHREADS, want_pass=rc.want_pass)
    try:
        with H.bdx.HipClassifier(cfg, want_pass=rc.want_pass) as hc:
            for which in ("main", "edge"):
                seq, off, longest = rc.batch(which)
                n = len(off) - 1
                what = f"{name} {which} batch ({n} reads, longest {longest}, {rc.env})"
                exp = oc.classify(seq, off)
                got = hc.classify(seq, off)
                launches = hc.last_launches
                fuzz.assert_same(got, exp, f"{what} [{hc.kernel_path}] {launches}")
                assert np.array_equal(hc.counts, oc.counts), f"{what}: counters"
                check_launches(launches, name, n, what)
                # not vacuous: the target answers most reads itself, all but a quarter unless the recipe states otherwise
                # (split forms hand every read with a candidate on by design: there the exact kernel's inputs come from
                # the target, and the poison fixture checks them)
                if not rc.derived["split"]:
                    assert hc.last_list_reads <= n // rc.list_div, f"{what}: {hc.last_list_reads} reads listed on"
    finally:
        _set_knobs(monkeypatch, {})


@pytest.mark.parametrize("name", GEN_CASES)
def test_general_instantiation_equals_the_oracle(name, monkeypatch):
    """The general forms: dual configs and configs with a ref_search_range that window mode turns down, known-score (the target
    answers all but a quarter of the reads itself) and split (the target filters for the exact kernel)."""
    rc = KL.recipe(name)
    cfg = rc.config()
    _set_knobs(monkeypatch, rc.env)
    oc = H.orc.OracleClassifier(cfg, nthreads=NTHREADS, want_pass=rc.want_pass)
    try:
        with H.bdx.HipClassifier(cfg, want_pass=rc.want_pass) as hc:
            for which in ("main", "edge"):
                seq, off, longest = rc.batch(which)
                n = len(off) - 1
                what = f"{name} {which} batch ({n} reads, longest {longest}, {rc.state} {rc.range_strs()}, {rc.env})"
                exp = oc.classify(seq, off)
                got = hc.classify(seq, off)
                launches = hc.last_launches
                fuzz.assert_same(got, exp, f"{what} [{hc.kernel_path}] {launches}")
                assert np.array_equal(hc.counts, oc.counts), f"{what}: counters"
                check_launches(launches, name, n, what)
                if not rc.split:
                    assert hc.last_list_reads <= n // rc.list_div, f"{what}: {hc.last_list_reads} reads listed on"
    finally:
        _set_knobs(monkeypatch, {})


@pytest.mark.parametrize("name", WIN_CASES)
def test_window_instantiation_equals_the_oracle(name, monkeypatch):
    """Window mode: both batches are planned at the recipe's read length (the hint a pipeline that knows its reads gives), so
    that the edge batch's reads beyond twice that length meet slots planned without them."""
    rc = KL.recipe(name)
    cfg = rc.config()
    _set_knobs(monkeypatch, rc.env)
    oc = H.orc.OracleClassifier(cfg, nthreads=NTHREADS, want_pass=rc.want_pass)
    try:
        with H.bdx.HipClassifier(cfg, want_pass=rc.want_pass) as hc:
            hc.set_read_length_hint(rc.hint)
            for which in ("main", "edge"):
                seq, off, planned = rc.batch(which)
                n = len(off) - 1
                what = f"{name} {which} batch ({n} reads, planned at {planned}, window {rc.range_str()}, {rc.env})"
                exp = oc.classify(seq, off)
                got = hc.classify(seq, off)
                launches = hc.last_launches
                fuzz.assert_same(got, exp, f"{what} [{hc.kernel_path}] {launches}")
                assert np.array_equal(hc.counts, oc.counts), f"{what}: counters"
                check_launches(launches, name, n, what)
                assert "wave(win)" in hc.kernel_path, f"{what}: {hc.kernel_path}"
                # not vacuous: the target answers all but a quarter of the reads itself
                assert hc.last_list_reads <= n // rc.list_div, f"{what}: {hc.last_list_reads} reads listed on"
    finally:
        _set_knobs(monkeypatch, {})


def check_list_launch(launches, target, listed, n_reads, what):
    """The target ran over a device-side list (list = 1) behind a launch over the whole batch; `listed`, the list's real length
    read back after the call, gives every unit (resident wave) two 16-read tiles and more and leaves a ragged last tile; every
    launched name is in the code object."""
    ks = KL.code_object_kernels()
    for ln in launches:
        assert ln["kernel"] in ks, f"{what}: launched {ln['kernel']} is not in the code object"
    hits = [ln for ln in launches if ln["kernel"] == target and ln["list"]]
    assert len(hits) == 1 and not launches[0]["list"] and launches[0]["reads"] == n_reads, f"{what}: {target} did not run over tier 1's list: {launches}"
    ln = hits[0]
    assert ln["tile"] == 16 and ln["units"] > 0 and ln["reads"] >= listed, f"{what}: {ln}"
    assert listed >= 2 * 16 * ln["units"], f"{what}: vacuous geometry: {listed} listed reads over {ln['units']} units"
    assert listed % 16 != 0, f"{what}: the last tile is not ragged: {listed} listed reads"


@pytest.mark.parametrize("name", PAIRS_CASES)
def test_pairs_instantiation_equals_the_oracle(name, monkeypatch):
    """The pairs mode: the target walks the list of reads tier 1 could not settle.  Known forms must answer all but a quarter of
    their list themselves (bdx_last_mid_reads against bdx_last_list_reads); the KEND 3 / NW 2 cells compare the device's
    statistics tables with DemuxStats.add_pass_outputs of the oracle, the other KEND 3 cells the per-pass outputs."""
    from biodemux_jl_amd.classification import DemuxStats

    rc = KL.recipe(name)
    cfg = rc.config()
    _set_knobs(monkeypatch, rc.env)
    oc = H.orc.OracleClassifier(cfg, nthreads=NTHREADS, want_pass=rc.want_pass or rc.summary)
    exp_st = DemuxStats()
    try:
        with H.bdx.HipClassifier(cfg, want_pass=rc.want_pass) as hc:
            for which in ("main", "edge"):
                seq, off, longest = rc.batch(which)
                n = len(off) - 1
                what = f"{name} {which} batch ({n} reads, longest {longest}, {rc.kw}, rate {rc.rate}, {rc.n_bc} barcodes)"
                exp = oc.classify(seq, off)
                got = hc.classify(seq, off)
                launches = hc.last_launches
                fuzz.assert_same(got, {k: v for k, v in exp.items() if k in got}, f"{what} [{hc.kernel_path}] {launches}")
                assert np.array_equal(hc.counts, oc.counts), f"{what}: counters"
                listed, handed = hc.last_list_reads, hc.last_mid_reads
                check_list_launch(launches, name, listed, n, f"{what} [{hc.kernel_path}]")
                div = rc.mid_div if which == "main" else rc.edge_mid_div
                if div:
                    assert 0 <= handed <= listed // div, f"{what}: {handed} of {listed} listed reads handed on"
                if rc.summary:
                    exp_st.add_pass_outputs(exp, float(cfg.min_delta))
                    got_st = DemuxStats()
                    got_st.add_device_tables(hc.stats_tables(), cfg)
                    for f in STATS_FIELDS:
                        assert getattr(got_st, f) == getattr(exp_st, f), f"{what}: statistics table {f}"
    finally:
        _set_knobs(monkeypatch, {})


@pytest.mark.parametrize("x", KL.PAIRS_EXTRAS, ids=lambda x: x.key)
def test_pairs_extra_case_equals_the_oracle(x, monkeypatch):
    """Further argument states and entry routes of pairs forms that have their recipe: the dual C4-shaped configs with and
    without carried passes, and a KB 8 and a KB 9 cell behind a wave tier, with no tier and with a pairs tier.  The whole-batch
    routes (Middle::all, Front::pairs in front) keep check_launches as it is; the others walk a list (check_list_launch)."""
    cfg = x.config()
    _set_knobs(monkeypatch, x.env)
    oc = H.orc.OracleClassifier(cfg, nthreads=NTHREADS, want_pass=x.want_pass)
    try:
        with H.bdx.HipClassifier(cfg, want_pass=x.want_pass) as hc:
            for which in ("main", "edge"):
                seq, off, longest = x.batch(which)
                n = len(off) - 1
                what = f"{x.key} {x.target} {which} batch ({n} reads, longest {longest}, {x.env})"
                exp = oc.classify(seq, off)
                got = hc.classify(seq, off)
                launches = hc.last_launches
                fuzz.assert_same(got, exp, f"{what} [{hc.kernel_path}] {launches}")
                assert np.array_equal(hc.counts, oc.counts), f"{what}: counters"
                if x.whole:
                    check_launches(launches, x.target, n, f"{what} [{hc.kernel_path}]")
                else:
                    listed = hc.last_list_reads  # (the list of the tier in front, a wave tier's or a pairs tier's)
                    ks = KL.code_object_kernels()
                    assert all(ln["kernel"] in ks for ln in launches), f"{what}: {launches}"
                    hits = [ln for ln in launches if ln["kernel"] == x.target and ln["list"]]
                    assert len(hits) == 1 and listed >= 2 * 16 * hits[0]["units"] > 0, f"{what} [{hc.kernel_path}]: {listed} listed reads, {launches}"
    finally:
        _set_knobs(monkeypatch, {})


def check_cell_launches(launches, target, n_reads, what):
    """Every launched name is in the code object.  A fused-filter target is the call's full-budget launch (its last fused
    launch) and its only launch over the whole batch, not a list launch, under check_launches' geometry: two or more tiles per workgroup, the
    last one ragged.  An exact-kernel target runs over the whole batch, not as a list launch, a thread per read: reads == n,
    three or more whole workgroups and a ragged one."""
    if KL.parse(target)[0] == "bdx_bitpar_kernel":
        fused = [ln for ln in launches if ln["family"] == "bitpar"]
        assert fused and fused[-1]["kernel"] == target and not fused[-1]["list"], f"{what}: {target} is not the full-budget launch: {launches}"
        assert sum(ln["kernel"] == target and not ln["list"] for ln in launches) == 1, f"{what}: {target} ran over the whole batch more than once: {launches}"
        return check_launches(launches, target, n_reads, what)
    ks = KL.code_object_kernels()
    for ln in launches:
        assert ln["kernel"] in ks, f"{what}: launched {ln['kernel']} is not in the code object"
    whole = [ln for ln in launches if ln["kernel"] == target and not ln["list"]]
    assert whole, f"{what}: {target} did not run over the whole batch: {launches}"
    for ln in whole:
        assert ln["reads"] == n_reads and ln["threads"] == ln["tile"], f"{what}: {ln}"
        assert ln["blocks"] == -(-n_reads // ln["tile"]) >= 4 and n_reads % ln["tile"] == 1, f"{what}: the last workgroup is not ragged: {ln}"


@pytest.mark.parametrize("name", CELL_CASES)
def test_cell_instantiation_equals_the_oracle(name, monkeypatch):
    rc = KL.recipe(name)
    cfg = rc.config()
    _set_knobs(monkeypatch, rc.env)
    oc = H.orc.OracleClassifier(cfg, nthreads=NTHREADS, want_pass=rc.want_pass)
    try:
        with H.bdx.HipClassifier(cfg, filter=rc.filter, want_pass=rc.want_pass) as hc:
            for which in ("main", "edge"):
                seq, off, longest = rc.batch(which)
                n = len(off) - 1
                what = f"{name} {which} batch ({n} reads, longest {longest}, {rc.env})"
                exp = oc.classify(seq, off)
                got = hc.classify(seq, off)
                launches = hc.last_launches
                fuzz.assert_same(got, exp, f"{what} [{hc.kernel_path}] {launches}")
                assert np.array_equal(hc.counts, oc.counts), f"{what}: counters"
                check_cell_launches(launches, name, n, what)
    finally:
        _set_knobs(monkeypatch, {})
