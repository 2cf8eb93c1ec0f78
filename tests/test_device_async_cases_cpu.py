"""The cases of tests/async_cases.py (the device entry point as hosts drive it), checked on the CPU before anything is enqueued on a device (tests/async_cases.py):
every schedule holds the six sizes in its stated order; the kernel_path written down for every call is what the per-call planner
decides (tests/call_host.cpp: csrc/bdx_plan.cpp + csrc/bdx_call.cpp alone) for the schedule run once and run again on the same
context, at 7 compute units and at 256; and the oracle alone shows that every batch exercises the verdicts a wrong launch would
get wrong: at least 30 % matched reads, at least one unknown read and, for configs with min_delta > 0, at least one ambiguous
read.

One batch of every schedule holds a single read.  One read cannot be 30 % matched AND unknown: that batch must be a match (it
carries an intact barcode), the other conditions hold for the batches from 33 reads on."""
import os

import pytest

import async_cases as AC

NTHREADS = min(16, os.cpu_count() or 1)


def test_schedules_hold_the_sizes_in_their_stated_order():
    assert AC.SIZES == (1, 33, 700, 4097, 9000, 20011)
    assert [AC.SIZES[b] for b in AC.SCHEDULES["growth"]] == [33, 1, 4097, 700, 20011, 9000]
    assert [AC.SIZES[b] for b in AC.SCHEDULES["no_growth"]] == [20011, 1, 9000, 33, 4097, 700]
    for c in AC.CASES:
        for s, order in AC.SCHEDULES.items():
            calls = c.calls(s)
            assert 6 <= len(calls) <= 8 and [k.size for k in calls] == [AC.SIZES[b] for b in order], (c.name, s)
            assert all(k.path for k in calls) and all(k.path for k in c.calls(s, again=True)), (c.name, s)
            for k in calls:
                seq, off = AC.make_batch(c, k)
                lens = off[1:] - off[:-1]
                assert len(off) == k.size + 1 and off[-1] == len(seq) and lens.min() >= k.min_len and lens.max() <= k.max_len, (c.name, s, k.size)
                assert lens.max() <= c.hint_for(s, k), (c.name, s, k.size)  # the hint in force covers the batch
        # the growth schedule's running maximum rises twice after the first call (a buffer is released and allocated anew while the
        # previous call may still run); the other one's never does
        for s, rises in (("growth", 2), ("no_growth", 0)):
            sizes = [k.size for k in c.calls(s)]
            assert sum(sizes[i] > max(sizes[:i]) for i in range(1, 6)) == rises
    assert sorted({c.family for c in AC.CASES}) == list(range(1, 11))
    # rising read lengths (family 10): every call of either schedule brings a new maximum
    for name in ("summary_single", "summary_dual"):
        for s in AC.SCHEDULES:
            hi = [k.max_len for k in AC.BY_NAME[name].calls(s)]
            assert hi == sorted(set(hi)), (name, s)
    # alternating families: both directions of every flip occur in both schedules
    for name in ("trim5_alternating", "kend_then_pass_start", "window60_hints", "filtered_and_not"):
        for s in AC.SCHEDULES:
            paths = [k.path for k in AC.BY_NAME[name].calls(s)]
            flips = {(a, b) for a, b in zip(paths, paths[1:]) if a != b}
            assert len(flips) >= 2 and any((b, a) in flips for a, b in flips), (name, s, paths)


def test_the_written_paths_are_what_the_planner_decides(tmp_path):
    got = AC.predicted_paths(tmp_path)
    for c in AC.CASES:
        for s in AC.SCHEDULES:
            want = [k.path for k in c.calls(s)] + [k.path for k in c.calls(s, again=True)]
            for n_cu in (7, 256):
                assert got[(c.name, s, n_cu)] == want, (c.name, s, n_cu)


@pytest.mark.parametrize("name", [c.name for c in AC.CASES])
def test_every_batch_has_matched_unknown_and_ambiguous_reads(name):
    c = AC.BY_NAME[name]
    seen = set()
    for s in AC.SCHEDULES:
        for k in c.calls(s):
            if k.key in seen:
                continue
            seen.add(k.key)
            total, matched, unknown, ambiguous = (int(v) for v in AC.expected(c, k, NTHREADS)[1][:4])
            what = f"{name} {s} {k.size} reads of {k.min_len}..{k.max_len}: {matched} matched, {unknown} unknown, {ambiguous} ambiguous"
            assert total == k.size, what
            if k.size == 1:
                assert matched == 1, what
                continue
            assert matched * 10 >= total * 3, what
            assert unknown >= 1, what
            if c.min_delta > 0:
                assert ambiguous >= 1, what
