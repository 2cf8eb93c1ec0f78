"""The create-time planner (csrc/bdx_plan.cpp) as host-only code: the stand-alone driver tests/plan_host.cpp plans the
named configs of tests/plan_cases.py on the CPU.  Every predicate holds (the case reaches its branch), two runs agree, and
every scalar, table offset and table digest equals tests/golden/plan_tables.json — recorded from bdx_create of the commit
before the planner was split out of bdx_abi.cpp, run on the CPU over a stub of the HIP runtime.  The same driver then runs
under ASan / UBSan with exact-size barcode buffers (no Python process loads sanitised code)."""
import json

import pytest

import plan_cases as PC
from test_sanitizers import ENV, SAN


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan")
    return PC.run_driver(PC.build_driver(d), d), d


def test_plan_cases_are_many_and_named_once():
    names = [c.name for c in PC.CASES]
    assert len(set(names)) == len(names) >= 40


@pytest.mark.parametrize("case", PC.CASES, ids=lambda c: c.name)
def test_plan_case_reaches_its_branch(reports, case):
    assert case.pred(reports[0][case.name]) is True


def test_planner_is_deterministic(reports, tmp_path):
    first, d = reports
    again = PC.run_driver(str(d / "plan_host"), tmp_path)
    assert {k: v.flat() for k, v in again.items()} == {k: v.flat() for k, v in first.items()}


def test_plan_equals_the_golden_tables(reports):
    with open(PC.GOLDEN) as f:
        golden = json.load(f)
    want = [c.name for c in PC.CASES if c.golden]
    assert sorted(golden) == sorted(want)
    for name in want:
        got = json.loads(json.dumps(reports[0][name].flat()))
        assert got["scalars"] == golden[name]["scalars"], name
        assert got["blobs"] == golden[name]["blobs"], name


def test_planner_under_asan_ubsan(tmp_path):
    exe = PC.build_driver(tmp_path, flags=SAN)
    got = PC.run_driver(exe, tmp_path, env=ENV)
    assert len(got) == len(PC.CASES)
