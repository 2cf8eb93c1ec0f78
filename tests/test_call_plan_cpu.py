"""The per-call planner (csrc/bdx_call.cpp) as host-only code: the stand-alone driver tests/call_host.cpp plans the call
shapes of tests/call_cases.py on the CPU.  Every predicate holds (the case sits on the intended side of its threshold), two
runs agree, a call never changes what the create-time planner produced, and every reported value equals
tests/golden/call_plans.json — recorded from size_* / plan_call / call_path of the commit before the call planner was split
out of bdx_abi.cpp, run on the CPU over a stub of the HIP runtime, every sequence on one context.  One step differs by design:
there the parent handed a dense request the slot-mode geometry the call before had left in the shared plan; the
golden file holds the parent's value with that history and on a fresh context, and the latter is asserted.  The launch lines
(c<i>.launch<j>: the grid, block size, tile and list flag of every classify kernel) were recorded from the commit before the
planner took the grids over from the launchers, whose formulas that commit's driver restated.  The same driver then runs under
ASan / UBSan (no Python process loads sanitised code)."""
import json

import pytest

import call_cases as CC
from test_sanitizers import ENV, SAN


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    d = tmp_path_factory.mktemp("call")
    return CC.run_driver(CC.build_driver(d), d, launches=True), d


@pytest.fixture(scope="module")
def golden():
    with open(CC.GOLDEN) as f:
        return json.load(f)


def test_call_cases_are_many_and_named_once():
    names = [c.name for c in CC.CASES]
    assert len(set(names)) == len(names) >= 100
    assert len(CC.SEQUENCES) >= 4


@pytest.mark.parametrize("case", CC.CASES, ids=lambda c: c.name)
def test_call_case_sits_on_its_side(reports, case):
    assert case.pred(reports[0][case.name]) is True


def test_call_planner_is_deterministic(reports, tmp_path):
    first, d = reports
    again = CC.run_driver(str(d / "call_host"), tmp_path, launches=True)
    assert {k: v.flat() for k, v in again.items()} == {k: v.flat() for k, v in first.items()}


@pytest.mark.parametrize("case", CC.CASES, ids=lambda c: c.name)
def test_a_call_never_changes_the_create_time_plans(reports, case):
    r = reports[0][case.name]
    assert r["digest.before"] == r["digest.after"] and len(r["digest.before"][0]) == 16


def test_the_recorded_exception_is_the_one_named_here(golden):
    ex = golden["history_dependent"]
    assert [(e["case"], e["call"]) for e in ex] == list(CC.FRESH_INSTEAD) and all(e["asserted"] == "parent_fresh" for e in ex)
    for e in ex:
        pre = "c%d." % e["call"]
        assert e["parent_history"] == {k: v for k, v in golden["cases"][e["case"]].items() if k.startswith(pre)}
        fresh = golden["cases"][CC.FRESH_INSTEAD[(e["case"], e["call"])]]
        assert e["parent_fresh"] == {pre + k[3:]: v for k, v in fresh.items() if k.startswith("c0.")}
        assert e["parent_fresh"] != e["parent_history"]


@pytest.mark.parametrize("case", CC.CASES, ids=lambda c: c.name)
def test_call_plan_equals_the_golden_file(reports, golden, case):
    assert sorted(golden["cases"]) == sorted(c.name for c in CC.CASES)
    want = dict(golden["cases"][case.name])
    for e in golden["history_dependent"]:
        if e["case"] == case.name:
            want.update(e[e["asserted"]])
    assert reports[0][case.name].flat() == want


def test_call_planner_under_asan_ubsan(tmp_path):
    exe = CC.build_driver(tmp_path, flags=SAN)
    got = CC.run_driver(exe, tmp_path, env=ENV, launches=True)
    assert len(got) == len(CC.CASES)
