"""The library launches what the per-call planner decides: a dozen call shapes of tests/call_cases.py's kind at their smallest
real size — a few thousand synthetic reads with BDX_CU_COUNT=2, so that the tile thresholds sit at ~1 000 reads — among them a
sequence on one context (313 bases, then 150) and a call that wants the per-pass positions, and the headline shape at the
device's own compute-unit count, the fused kernel under a forced grid (BDX_GRID below and above its tile count) and a config
outside the filters' domain (the generic kernel alone).  For every call bdx_kernel_path and every line of bdx_last_launches (family, blocks, threads,
tile, list flag and the template arguments the plan decides) equal what tests/call_host.cpp, built and run here with the same
switches and n_cu, predicts from csrc/bdx_call.cpp alone, and bdx_band_launches advances by the count the plan states; the
verdicts equal the oracle."""
import ctypes
import os

import numpy as np
import pytest

import call_cases as CC
import fuzz
import helpers as H
import kernel_lattice as KL
import plan_cases as PC
from biodemux_jl_amd import synth

pytestmark = pytest.mark.gpu

NTHREADS = min(16, os.cpu_count() or 1)
KNOBS = {"BDX_CU_COUNT": "n_cu", "BDX_WAVE_RW": "wave_rw", "BDX_NO_WAVE": "no_wave", "BDX_NO_TIER": "no_tier", "BDX_GRID": "grid"}
B1 = synth.make_barcodes(96, 24, seed=20260515)
B4A, B4B = synth.make_barcodes(24, 24, seed=1), synth.make_barcodes(16, 24, seed=2)


def _cfg(bcs, bcs2=None, **kw):
    ids = dict(bc_seqs=bcs, bc_lengths_no_N=[len(b) for b in bcs], ids=["a%d" % i for i in range(len(bcs))])
    if bcs2:
        ids.update(is_dual=True, bc_seqs2=bcs2, bc_lengths_no_N2=[len(b) for b in bcs2], ids2=["b%d" % i for i in range(len(bcs2))])
    return H.bdx.DemuxConfig(**ids, **kw)


# name -> (DemuxConfig switches, second barcode set?, developer switches, want_pass, [(n_reads, read_len)], what the path must hold)
SHAPES = {
    "headline_device_cus": (dict(max_error_rate=0.1), False, {}, False, [(65536, 150)], "wave > "),
    "tile16_below_1024": (dict(max_error_rate=0.1), False, {"BDX_CU_COUNT": "2"}, False, [(1023, 150)], "wave > "),
    "tile32_at_1024": (dict(max_error_rate=0.1), False, {"BDX_CU_COUNT": "2"}, False, [(1024, 150)], "wave > "),
    "forced_rw16": (dict(max_error_rate=0.1), False, {"BDX_CU_COUNT": "2", "BDX_WAVE_RW": "16"}, False, [(3001, 150)], "wave > "),
    "no_wave_dense": (dict(max_error_rate=0.1), False, {"BDX_CU_COUNT": "2", "BDX_NO_WAVE": "1"}, False, [(3001, 150)], "qgram+bitpar+verify"),
    "tiered_trim5": (dict(max_error_rate=0.2, min_delta=0.1, trim_side=5), False, {"BDX_CU_COUNT": "2"}, False, [(3001, 150)], "tier1:wave(end)"),
    "tiered_trim5_pass_start": (dict(max_error_rate=0.2, min_delta=0.1, trim_side=5), False, {"BDX_CU_COUNT": "2"}, True, [(3001, 150)], "tier1:wave(aln)"),
    "trim3": (dict(max_error_rate=0.2, trim_side=3), False, {"BDX_CU_COUNT": "2"}, False, [(3001, 150)], "wave(end)"),
    "dual_carry": (dict(max_error_rate=0.2, trim_side=5, trim_side2=3), True, {"BDX_CU_COUNT": "2"}, False, [(3001, 150)], "pairs(end)"),
    "tiered_pairs_list": (dict(max_error_rate=0.2), False, {"BDX_CU_COUNT": "2"}, False, [(3001, 150)], "tier1:wave > pairs"),
    "pairs_tier": (dict(max_error_rate=0.25, min_delta=0.15, indel=2), False, {"BDX_CU_COUNT": "2"}, False, [(3001, 150)], "tier1:pairs(diag)"),
    "hamming_wave_split": (dict(max_error_rate=0.1, matching_algorithm="hamming"), False, {"BDX_CU_COUNT": "2"}, False, [(3001, 150)], "wave+verify"),
    "seq_313_then_150": (dict(max_error_rate=0.13), False, {"BDX_CU_COUNT": "2", "BDX_NO_WAVE": "1", "BDX_NO_TIER": "1"}, False, [(2001, 313), (3001, 150)],
                         "bitpar+verify"),
    # the fused kernel's forced grid: three workgroups; more than there are tiles: one per tile
    "grid_3": (dict(max_error_rate=0.1), False, {"BDX_CU_COUNT": "2", "BDX_NO_WAVE": "1", "BDX_GRID": "3"}, False, [(3001, 150)], "qgram+bitpar+verify"),
    "grid_1000_clamped": (dict(max_error_rate=0.1), False, {"BDX_CU_COUNT": "2", "BDX_NO_WAVE": "1", "BDX_GRID": "1000"}, False, [(3001, 150)],
                          "qgram+bitpar+verify"),
    # a match that scores is outside every filter's cost domain: the generic kernel alone, a thread per read
    "generic_alone": (dict(max_error_rate=0.2, match=-1, mismatch=2, indel=3), False, {"BDX_CU_COUNT": "2"}, False, [(3001, 150)], "generic"),
}
ALG = {"semiglobal": PC.SEMIGLOBAL, "hamming": PC.HAMMING, "exact": PC.EXACT}


@pytest.fixture(scope="module", autouse=True)
def _need_library():
    assert os.path.exists(H.bdx.LIB_PATH), "HIP extension missing: run __graft_entry__.build()"


def _device_cus():
    """The compute units of device 0 as bdx_create reads them: hipDeviceGetAttribute of the HIP runtime the library itself is
    linked against (reached through the library's handle), hipDeviceAttributeMultiprocessorCount = 63 in hip_runtime_api.h.
    No second runtime is brought up in this process for it."""
    cus = ctypes.c_int(0)
    assert H.bdx.load_library().hipDeviceGetAttribute(ctypes.byref(cus), 63, 0) == 0
    assert 1 <= cus.value <= 1024, cus.value
    return cus.value


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("call_gpu")
    return CC.build_driver(d), d


def _predicted(driver, name, kw, dual, env, want_pass, calls):
    tune = {KNOBS[k]: int(v) for k, v in env.items()}
    if "n_cu" not in tune:
        tune["n_cu"] = _device_cus()
    passes = [PC.one_pass(B4A if dual else B1, trim=kw.get("trim_side") or 0)] + ([PC.one_pass(B4B, trim=kw.get("trim_side2") or 0)] if dual else [])
    wanted = 0x3FF if want_pass else 0xF
    case = CC.CallCase(name, None, [CC.call(n, L, wanted=wanted) for n, L in calls], passes=passes, rate=kw["max_error_rate"], min_delta=kw.get("min_delta", 0.0),
                       costs=(kw.get("match", 0), kw.get("mismatch", 1), kw.get("indel", 1)), algorithm=ALG[kw.get("matching_algorithm", "semiglobal")], tune=tune)
    exe, d = driver
    return CC.run_driver(exe, d, cases=[case], launches=True)[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_library_launches_the_planned_call(name, driver, monkeypatch):
    kw, dual, env, want_pass, calls, path_holds = SHAPES[name]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = _cfg(B4A, B4B, **kw) if dual else _cfg(B1, **kw)
    oc = H.orc.OracleClassifier(cfg, nthreads=NTHREADS, want_pass=want_pass)
    with H.bdx.HipClassifier(cfg, want_pass=want_pass) as hc:
        # (the context exists: the device's compute units can be asked of the runtime it runs on)
        want = _predicted(driver, name, kw, dual, env, want_pass, calls)
        for c, (n, L) in enumerate(calls):
            second = dict(second=(B4B, L - 50, L - 24)) if dual else {}
            seq, off, _ = synth.make_reads(B4A if dual else B1, n, L, seed=77 + c, **second)
            assert int((off[1:] - off[:-1]).max()) == L
            band_before = hc.band_launches
            got = hc.classify(seq, off)
            launches = hc.last_launches
            what = f"{name} call {c} [{hc.kernel_path}] {launches}"
            planned_path = want.path(c) if want.i("c%d.filtered" % c) else "generic"
            assert hc.kernel_path == planned_path and path_holds in hc.kernel_path, f"{what}: planned {planned_path}"
            planned = want.launches(c)
            assert [ln["family"] for ln in launches] == [p["family"] for p in planned], f"{what}: planned {planned}"
            for ln, p in zip(launches, planned):
                assert (ln["blocks"], ln["threads"], ln["tile"], int(ln["list"])) == (p["blocks"], p["threads"], p["tile"], p["list"]), f"{what}: planned {p}"
                a = KL.parse(ln["kernel"])[1]
                if p["family"] == "bitpar":
                    assert (a["R"], int(a["SEED"]), int(a["DIAG"]), a["NW"], a["WL"]) == p["args"], f"{what}: planned {p}"
                elif p["family"] == "generic":
                    assert a["BS"] == p["args"][0], f"{what}: planned {p}"
                else:
                    assert (a["RW"], int(a["SPLIT"]), a["KEND"], int(a["WINM"])) == p["args"][:4] and (a["KB"] > 0) == (p["family"] == "pairs"), f"{what}: planned {p}"
            # the diagonal-band DP of the exact kernel: counted where its launch is made, by what the plan states
            assert hc.band_launches - band_before == want.band_launches(c), f"{what}: planned {want.band('band_t1', c)} {want.band('band_exact', c)}"
            if "BDX_GRID" in env:  # as forced, but never more workgroups than tiles
                fused = [ln for ln in launches if ln["family"] == "bitpar"]
                assert fused and all(ln["blocks"] == min(int(env["BDX_GRID"]), -(-n // ln["tile"])) for ln in fused), what
            fuzz.assert_same(got, oc.classify(seq, off), what)
            assert np.array_equal(hc.counts, oc.counts), f"{what}: counters"
        info = hc.launch_info()
        if want.i("c%d.filtered" % (len(calls) - 1)):
            assert info["reads_per_block"] == want.fused(len(calls) - 1)["reads_per_block"] and info["lds_bytes_per_block"] == want.fused(len(calls) - 1)["lds"]
        else:
            assert (info["blocks"], info["reads_per_block"]) == (planned[0]["blocks"], planned[0]["tile"]) and len(planned) == 1
