"""The per-call planner (csrc/bdx_call.cpp) as host-only code: the stand-alone driver tests/call_host.cpp plans the call
shapes of tests/call_cases.py on the CPU.  Every predicate holds (the case sits on the intended side of its threshold), two
runs agree, a call never changes what the create-time planner produced, and every reported value equals
tests/golden/call_plans.json — recorded from size_* / plan_call / call_path of the commit before the call planner was split
out of bdx_abi.cpp, run on the CPU over a stub of the HIP runtime, every sequence on one context.  One step differs by design:
there the parent handed a dense request the slot-mode geometry the call before had left in the shared plan; the
golden file holds the parent's value with that history and on a fresh context, and the latter is asserted.  The launch lines
(c<i>.launch<j>: the grid, block size, tile and list flag of every classify kernel) were recorded from the commit before the
planner took the grids over from the launchers, whose formulas that commit's driver restated.  The same driver then runs under
ASan / UBSan (no Python process loads sanitised code).  The band fields (c<i>.band_t1 / .band_exact) were recorded before the
planner held them, from that commit's band_cfg formula (enqueue, bdx_abi.cpp) in a scratch copy of this driver fed from that
commit's plans.  The last four arguments of the `generic` launch lines (reg_rows, clean, uniform_m, band_roll: what the ladder of
bdx_launch_generic spells the instantiation from) were added later from the create-time plan, and so were the arguments of the
`wave` and `pairs` launch lines behind RW SPLIT KEND WINM (q track_from span_cap slot gen pairs_kb nw groups: what the dispatch
ladders of bdx_wave_kernel.h read); every other value of the file is as it was recorded.

The same driver answers for the two other host-only pieces of a call: the read length of a batch (bdx_batch_len), held against
the rule written out below over its whole input lattice, and the turn of the scratch halves (BdxScratchTurn), held against
event sequences."""
import itertools
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


def test_band_fields_are_reported_for_every_exact_launch(reports):
    seen = set()
    for case in CC.CASES:
        r = reports[0][case.name]
        for c in range(len(case.calls)):
            if r.i("c%d.rc" % c) != 0 or not r.i("c%d.filtered" % c):
                assert r.band("band_exact", c) is None and r.band_launches(c) == 0
                continue
            p, t1, ex = r.plan(c), r.band("band_t1", c), r.band("band_exact", c)
            assert (t1 is not None) == bool(p["t1_exact"]) and ex is not None
            for b, dense in ((t1, 0), (ex, p["dense_w"] if p["exact"] != "known" else 0)):
                if b is not None:
                    assert b["dense_w"] == dense and 0 <= b["launches"] <= sum(k >= 0 for k in (b["kb0"], b["kb1"])) <= p["npass"]
            if p["exact"] == "known":  # no hand-over of windows: the config's own fields
                assert ex == dict(dense_w=0, m=0, kb0=-1, kb1=-1, lb0=0, lb1=0, launches=0)
            seen.add((t1 or ex)["launches"])
    assert {0, 1, 2} <= seen  # no band, one pass, both passes of a dual config


# ---- the read length of a batch ---------------------------------------------------------------------------------------------
LENGTH_ROWS = list(itertools.product((0, 1, 212), (0, 1, 150), (0, -5, 100, 313), (1, 0), (1, 0), (0, 1, 150)))


def length_rule(window_len, host_len, hint, stats, filt, measured):
    """The rule, written out (not the function under test): (measure, longest, planned)."""
    known = window_len if window_len > 0 else host_len if host_len > 0 else None
    measure = (bool(stats) and known is None) or (bool(filt) and window_len <= 0 and hint <= 0 and known is None)
    longest = known if known is not None else measured if measure else None  # the statistics tables: longest + max_m + 2 rows
    if not filt:
        planned = 0  # with the filter off, no length is planned
    elif window_len > 0:
        planned = window_len
    elif hint > 0:
        planned = hint  # also when the host entry knows the true longest read
    else:
        planned = max(longest, 1)
    return int(measure), -1 if longest is None else longest, planned


def test_length_rule_over_its_lattice(reports):
    assert len(LENGTH_ROWS) == 3 * 3 * 4 * 2 * 2 * 3
    got = CC.run_lengths(str(reports[1] / "call_host"), reports[1], LENGTH_ROWS)
    want = [length_rule(*row) for row in LENGTH_ROWS]
    for row, g, w in zip(LENGTH_ROWS, got, want):
        assert g == w, (row, g, w)
    # the lattice reaches every branch: measured for the statistics alone, for the plan alone, for both; all three sources of the plan
    assert {(0, 0, 100, 1, 1, 150), (0, 0, 0, 0, 1, 150), (0, 0, -5, 1, 1, 0)} <= {r for r, w in zip(LENGTH_ROWS, want) if w[0]}
    assert {w[2] for r, w in zip(LENGTH_ROWS, want) if r[4]} == {1, 100, 150, 212, 313} and {w[2] for r, w in zip(LENGTH_ROWS, want) if not r[4]} == {0}


# ---- the scratch halves -------------------------------------------------------------------------------------------------------
# (events, per event: memset needed (None: the event begins no call), the half the next call takes, the other one)
SCRATCH = [
    (("call", "call"), [(1, 1, 0), (0, 0, 1)]),  # the first call clears its half, its last launch the second call's
    (("call", "fail", "call"), [(1, 1, 0), (0, 1, 0), (1, 0, 1)]),  # the failed call took the clean half and did not turn: the next clears it again
    (("call", "stream", "call"), [(1, 1, 0), (None, 1, 0), (1, 0, 1)]),
    (("copy",), [(0, 1, 0)]),  # the copy kernel cleared this call's half
    (("copy", "call"), [(0, 1, 0), (0, 0, 1)]),  # ... and the next call is judged by the clean flag alone: clean
    (("copy", "stream", "call"), [(0, 1, 0), (None, 1, 0), (1, 0, 1)]),  # ... not clean: no credit is left over
    (("call", "plain", "call"), [(1, 1, 0), (None, 1, 0), (0, 0, 1)]),  # an unfiltered call changes nothing
    (("plain", "call", "plain", "plain", "call"), [(None, 0, 1), (1, 1, 0), (None, 1, 0), (None, 1, 0), (0, 0, 1)]),
    (("fail", "fail", "call", "call"), [(1, 0, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1)]),
]


def test_scratch_turn_sequences(reports):
    got = CC.run_scratch(str(reports[1] / "call_host"), reports[1], [s for s, _ in SCRATCH])
    for (events, want), g in zip(SCRATCH, got):
        assert g == want, (events, g)
        # other() after a finished call is the half that call used
        mine = 0
        for ev, (_, now, other) in zip(events, g):
            if ev in ("call", "copy"):
                assert other == mine and now == 1 - mine, events
            else:
                assert now == mine, events
            mine = now


def test_call_planner_under_asan_ubsan(tmp_path):
    exe = CC.build_driver(tmp_path, flags=SAN)
    got = CC.run_driver(exe, tmp_path, env=ENV, launches=True)
    assert len(got) == len(CC.CASES)
    assert CC.run_lengths(exe, tmp_path, LENGTH_ROWS, env=ENV) == [length_rule(*row) for row in LENGTH_ROWS]
    assert CC.run_scratch(exe, tmp_path, [s for s, _ in SCRATCH], env=ENV) == [w for _, w in SCRATCH]
