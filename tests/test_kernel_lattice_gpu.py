"""One case per classify instantiation that has a recipe (kernel_lattice.py): on one context, a main batch and an edge
batch built for the instantiation's cell.  Each call must launch exactly that kernel over the whole batch, at two or more
tiles per resident wave with a ragged last tile; the kernel must answer most reads itself; and verdicts, per-pass outputs
(doubles by bit pattern) and counters must equal the oracle bit for bit.  The autouse poison and refused-window fixtures
of conftest.py watch the hand-over of the split forms.  The fused filter's instantiations run as the full-budget launch
of a known-score call, the exact kernel's behind the filter of a split call (or alone): there the whole batch is a thread
per read, three whole workgroups and a ragged one."""
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
