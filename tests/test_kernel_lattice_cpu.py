"""Bookkeeping of the instantiation lattice (no GPU; needs the built library): every classify instantiation in the code
object has exactly one recipe, UNREACHABLE entry or PENDING pattern, and every recipe's target follows from the planner's
rules as kernel_lattice.py restates them — a recipe that drifts off its cell fails here, before it runs on a GPU.  The
fused filter's, the exact kernel's, window mode's, the general forms' and the pairs mode's recipes are held against the
planner itself (tests/call_host.cpp), and the oracle alone shows that their batches are not vacuous."""
import os

import pytest

import kernel_lattice as KL
from biodemux_jl_amd import hipabi

# (the bookkeeping reads the built library's code object: a missing library is a failure, not a skip)
assert os.path.exists(hipabi.LIB_PATH), "HIP extension missing: run __graft_entry__.build()"


def test_parse_round_trips_every_classify_instantiation():
    names = KL.classify_kernels()
    assert len(names) >= 300, len(names)
    for n in names:
        fam, args = KL.parse(n)
        assert KL.spell(fam, args) == n
    assert KL.parse("bdx_copy_kernel") is None and KL.parse("pack_kernel") is None
    assert KL.parse("bdx_wave_kernel<32, 20, 5, 8, false, 0, 0, false, 0, false, false>")[1] == dict(
        RW=32, TF=20, NV=5, Q=8, SPLIT=False, KB=0, NW=0, MG=False, KEND=0, GEN=False, WINM=False)


def test_the_instantiation_list_is_the_pinned_one():
    """The built library holds exactly the classify instantiations of tests/kernel_names.txt (one name per line, sorted):
    a kernel that drops out of the build, or one that joins it, shows here instead of as one parametrised case fewer."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "kernel_names.txt")) as f:
        pinned = f.read().split("\n")[:-1]
    built = KL.classify_kernels()
    missing = sorted(set(pinned) - set(built))
    extra = sorted(set(built) - set(pinned))
    assert not missing and not extra, "missing from the build:\n  " + "\n  ".join(missing) + "\nnot in kernel_names.txt:\n  " + "\n  ".join(extra)
    assert built == pinned


def test_every_instantiation_is_accounted_for():
    for n in KL.classify_kernels():
        has = [KL.recipe(n) is not None, n in KL.UNREACHABLE, KL.pending_reason(n) is not None]
        assert sum(has) == 1, f"{n}: recipe / UNREACHABLE / PENDING = {has}: give it exactly one"
    ks = KL.code_object_kernels()
    for why, names in KL.PENDING.items():
        for n in names:
            assert n in ks, f"PENDING ({why}) names {n}, which the code object does not hold"
    for n, why in KL.UNREACHABLE.items():
        assert n in ks, f"UNREACHABLE names {n}, which the code object does not hold"
        assert "bdx_plan.cpp" in why or "bdx_call.cpp" in why or "bdx_abi.cpp" in why or ".hip" in why, f"{n}: the reason must cite the planner condition: {why}"


def test_the_headline_cell_has_a_recipe():
    assert KL.recipe("bdx_wave_kernel<32, 20, 5, 8, false, 0, 0, false, 0, false, false>") is not None


WAVE_CASES = [n for n in KL.classify_kernels() if isinstance(KL.recipe(n), KL.Recipe)]
CELL_CASES = [n for n in KL.classify_kernels() if isinstance(KL.recipe(n), KL.CellRecipe)]


def test_the_fused_filter_and_the_exact_kernel_are_all_pinned():
    """Every fused-filter and exact-kernel instantiation of the build has a recipe; none is listed as unreachable."""
    fused = [n for n in KL.classify_kernels() if n.startswith("bdx_bitpar_kernel<")]
    exact = [n for n in KL.classify_kernels() if n.startswith("bdx_generic_kernel<")]
    assert (len(fused), len(exact)) == (34, 12)
    assert all(n in CELL_CASES for n in fused)
    assert all(n in CELL_CASES for n in exact) and not KL.UNREACHABLE
    assert len(CELL_CASES) == 46


def test_all_wave_instantiations_have_a_recipe_or_a_proven_unreachable_entry():
    """All 346 wave instantiations have a recipe or a proven UNREACHABLE entry, and PENDING is empty: the 180 single-pass
    whole-range forms, the 18 window-mode forms, the 72 general forms and the 76 pairs forms."""
    wave = [n for n in KL.classify_kernels() if n.startswith("bdx_wave_kernel<")]
    assert len(wave) == 346 and KL.PENDING == {}
    assert all((KL.recipe(n) is not None) != (n in KL.UNREACHABLE) for n in wave)
    assert (len(WAVE_CASES), len(WIN_CASES), len(GEN_CASES), len(PAIRS_CASES)) == (180, 18, 72, 76)
    assert sorted(WAVE_CASES + WIN_CASES + GEN_CASES + PAIRS_CASES + [n for n in KL.UNREACHABLE if n in wave]) == wave


@pytest.fixture(scope="module")
def cell_plans(tmp_path_factory):
    """Every cell recipe through the per-call planner (tests/call_host.cpp), one driver run: `seq` = the main and the edge batch
    in the order the GPU case makes them, on one context; `above` / `below` = one read length beyond either end of the cell on
    a fresh context; `plain` = without the forced switch, every read length of the sweep."""
    import call_cases as CC

    d = tmp_path_factory.mktemp("cells")
    cases = []
    for i, name in enumerate(CELL_CASES):
        rc = KL.recipe(name)
        cases.append(rc.case("seq%d" % i, [(rc.n_main, rc.main_len), (rc.n_edge, rc.edge_len)]))
        cases.append(rc.case("above%d" % i, [(rc.n_edge, rc.edge_len + 1)]))
        if rc.low > 1:
            cases.append(rc.case("below%d" % i, [(rc.n_edge, rc.low - 1)]))
        if rc.forced_why:
            cases.append(rc.case("plain%d" % i, [(rc.n_edge, L) for L in _sweep_lengths(rc)], force=False))
    return CC.run_driver(CC.build_driver(d), d, cases=cases, launches=True)


def _sweep_lengths(rc):
    """The read lengths over which a forced recipe's cell is looked for without the switch: every length up to FUSED_MAX_LEN;
    the two-intact-pieces index stands up to 312 bases."""
    return range(1, 401) if KL.parse(rc.target)[1]["DIAG"] else range(1, KL.FUSED_MAX_LEN + 1)


@pytest.mark.parametrize("name", CELL_CASES)
def test_cell_recipe_lands_in_its_cell(name, cell_plans):
    """The planner itself (bdx_plan.cpp + bdx_call.cpp through the driver) puts both batches of the recipe in the target cell,
    the target running over the whole batch: the fused filter as the full-budget launch with two or more tiles per workgroup
    and a ragged last one, the exact kernel on three whole workgroups and a ragged one.  One base beyond either end of the cell
    plans to another kernel, unless the recipe states what ends the cell; a switch is forced only where no read length reaches
    the cell without it."""
    rc = KL.recipe(name)
    i = CELL_CASES.index(name)
    fam, a = KL.parse(name)
    seq = cell_plans["seq%d" % i]
    for c, n in enumerate((rc.n_main, rc.n_edge)):
        assert seq.i("c%d.rc" % c) == 0
        launches = KL.planned_launches(seq, c)
        assert KL.whole_batch_target(launches, name), (c, launches)
        for ln in launches:
            if ln["kernel"] == name and not ln["list"]:
                tiles = -(-n // ln["tile"])
                if fam == "bdx_bitpar_kernel":
                    assert ln["tile"] == a["R"] and n % a["R"] == 1 and tiles >= 2 * ln["blocks"] > 0, ln
                else:
                    assert ln["tile"] == a["BS"] and n % a["BS"] == 1 and ln["blocks"] == tiles >= 4, ln
    above = KL.whole_batch_target(KL.planned_launches(cell_plans["above%d" % i]), name)
    assert above == (rc.end_why is not None), f"{rc.edge_len} is not the longest read of the cell / the recipe states no end"
    assert rc.low == 1 or not KL.whole_batch_target(KL.planned_launches(cell_plans["below%d" % i]), name), f"{rc.low} is not the shortest read of the cell"
    assert rc.main_len == min(max(rc.low, rc.max_m + 40), rc.edge_len)
    if rc.forced_why:
        assert set(rc.env) == {"BDX_CU_COUNT", "BDX_BITPAR_R"} and "bdx_call.cpp" in rc.forced_why
        plain = cell_plans["plain%d" % i]
        reached = [L for c, L in enumerate(_sweep_lengths(rc)) if KL.whole_batch_target(KL.planned_launches(plain, c), name)]
        assert not reached, f"forced, yet reachable plainly at {reached[:4]} bases"
    else:
        assert rc.env == {"BDX_CU_COUNT": "1"}


@pytest.mark.parametrize("name", CELL_CASES)
def test_cell_recipe_is_not_vacuous(name):
    """By the oracle alone: the edge batch holds at least four reads of every kind and its longest read is the cell's; at
    least a third of the main batch is assigned; every kind planted at the budget has assigned reads and every kind planted one
    operation beyond it (or with one intact piece) has unassigned ones."""
    import helpers as H

    rc = KL.recipe(name)
    oc = H.orc.OracleClassifier(rc.config(), nthreads=min(16, os.cpu_count() or 1), want_pass=False)
    seq, off, longest = rc.batch("main")
    assert len(off) - 1 == rc.n_main and longest == rc.main_len
    assigned = oc.classify(seq, off)["bc1"] > 0
    assert 3 * int(assigned.sum()) >= rc.n_main, f"{int(assigned.sum())} of {rc.n_main} reads of the main batch are assigned"
    seq, off, kinds = rc.edge_batch()
    lens = off[1:] - off[:-1]
    assert len(lens) == rc.n_edge and int(lens.max()) == rc.edge_len
    assert (lens == 0).any() and (lens < rc.min_m).any() and (seq == ord("N")).any()
    assert kinds[-1] == "ragged_last" and set(kinds) == set(rc.kinds) | {"ragged_last"}
    assigned = oc.classify(seq, off)["bc1"] > 0
    for kind in rc.kinds + ("ragged_last",):
        of_kind = [i for i, k in enumerate(kinds) if k == kind]
        assert len(of_kind) >= (1 if kind == "ragged_last" else 4), (kind, len(of_kind))
        if KL.at_kb(kind):
            assert assigned[of_kind].any(), f"no {kind} read is assigned"
        if kind in KL.AT_KB1:
            assert not assigned[of_kind].all(), f"every {kind} read is assigned"


WIN_CASES = [n for n in KL.classify_kernels() if isinstance(KL.recipe(n), KL.WinRecipe)]


def test_wave_name_spells_the_headline_and_pairs_name_a_pairs_form():
    """The two ladders over a launch line's arguments, on lines written out by hand (the order of tests/call_host.cpp)."""
    #            rw split kend winm q tf span slot gen kb nw groups
    assert KL.wave_name((32, 0, 0, 0, 8, 21, 4864, 0, 0, 0, 0, 0)) == "bdx_wave_kernel<32, 20, 5, 8, false, 0, 0, false, 0, false, false>"
    assert KL.wave_name((16, 1, 0, 0, 7, 12, 5136, 0, 1, 0, 0, 0)) == "bdx_wave_kernel<16, 12, 10, 7, true, 0, 0, false, 0, true, false>"
    assert KL.wave_name((8, 0, 2, 0, 6, 10, 1024, 0, 0, 0, 0, 0)) == "bdx_wave_kernel<8, 0, 5, 6, false, 0, 0, false, 2, true, false>"
    assert KL.wave_name((32, 0, 0, 1, 8, 21, 3088, 96, 1, 0, 0, 0)) == "bdx_wave_kernel<32, 20, 3, 8, false, 0, 0, false, 0, true, true>"
    assert KL.wave_name((32, 0, 0, 1, 8, 21, 3600, 112, 1, 0, 0, 0)) == "bdx_wave_kernel<32, 20, 7, 8, false, 0, 0, false, 0, true, true>"
    assert KL.wave_name((16, 0, 0, 1, 8, 21, 4112, 256, 1, 0, 0, 0)) == "bdx_wave_kernel<16, 20, 4, 8, false, 0, 0, false, 0, true, true>"
    assert KL.wave_name((16, 0, 0, 1, 8, 21, 4368, 272, 1, 0, 0, 0)) is None and KL.wave_name((32, 0, 0, 1, 8, 21, 7696, 240, 1, 0, 0, 0)) is None
    assert KL.pairs_name((16, 0, 0, 0, 4, 19, 784, 48, 0, 4, 3, 1)) == "bdx_wave_kernel<16, 12, 3, 4, false, 4, 3, false, 0, true, false>"
    assert KL.pairs_name((16, 0, 2, 0, 4, 19, 3104, 192, 0, 3, 2, 1)) == "bdx_wave_kernel<16, 12, 6, 4, false, 3, 2, false, 2, true, false>"
    assert KL.pairs_name((16, 1, 0, 0, 4, 19, 784, 48, 0, 9, 1, 1)) == "bdx_wave_kernel<16, 12, 3, 4, true, 9, 2, false, 0, true, false>"
    assert KL.pairs_name((16, 0, 0, 0, 4, 19, 784, 48, 0, 4, 4, 2)) == "bdx_wave_kernel<16, 12, 3, 4, false, 4, 4, true, 0, true, false>"
    for n in (KL.wave_name((32, 0, 0, 1, 8, 21, 3088, 96, 1, 0, 0, 0)), KL.pairs_name((16, 1, 0, 0, 4, 19, 784, 48, 0, 9, 1, 1))):
        assert n in KL.code_object_kernels()


def test_window_recipes_cover_every_style_in_every_cell():
    from biodemux_jl_amd import parse_dynamic_range

    assert len(WIN_CASES) == 18
    seen = {(rc.rw, rc.nv, rc.style) for rc in map(KL.recipe, WIN_CASES)}
    assert seen == {(rw, nv, s) for rw, nv in KL.WIN_CELLS for s in KL.WIN_STYLES}
    for rc in map(KL.recipe, WIN_CASES):  # from the start, from the end, and the start from the end with the end from the start
        r = rc.range()
        assert r == parse_dynamic_range(rc.range_str())
        assert (r.start_from_end, r.end_from_end) == {"start": (False, False), "end": (True, True), "mix": (True, False)}[rc.style]
        first, last = rc.window(rc.main_len)
        assert last - first + 1 == rc.w and 2 * rc.w <= rc.main_len == rc.hint


def _one_column_out(rc, cfg, seq, off, kinds, window):
    """By the oracle with per-pass outputs: a barcode from the window's first column or to its last is found without an edit
    (nearly always: N and a second barcode aside), one moved a single column out of the window is not — such reads hold an exact
    copy only by chance, a share of 1 - exp(-window x barcodes / 4^m) (a quarter allowed on top for the few reads), and fewer
    than the reads with the barcode inside.  Only reads whose window leaves that column free count, and only configs where
    chance stays below a half (7-nt barcodes in windows of 300 columns and more say nothing).  This is what tells a window that
    is off by one from a right one."""
    import math
    import helpers as H
    import numpy as np

    got = H.orc.OracleClassifier(cfg, nthreads=min(16, os.cpu_count() or 1), want_pass=True).classify(seq, off)
    exact = (got["bc1"] > 0) & (got["pass_score"][:, 0] == 0.0)
    lens = off[1:] - off[:-1]
    room = {"win_before1": lambda n, f, l: f > 1, "win_after1": lambda n, f, l: l < n}
    inside = np.array([k in ("win_first", "win_last") for k in kinds])
    assert exact[inside].mean() >= 0.9, exact[inside].mean()
    for kind, free in room.items():
        idx = [i for i, k in enumerate(kinds) if k == kind and lens[i] >= rc.m and free(int(lens[i]), *window(int(lens[i])))
               and window(int(lens[i]))[1] - window(int(lens[i]))[0] + 1 >= rc.m]
        f, l = window(int(lens[0]))
        chance = 1.0 - math.exp(-(l - f + 1) * len(cfg.bc_seqs) / 4.0 ** rc.m)
        if idx and chance <= 0.5:
            assert len(idx) >= 4 and exact[idx].mean() <= chance + 0.25 < exact[inside].mean(), (kind, len(idx), exact[idx].mean(), chance)
    return got


def _whole_batch_wave(report, c, name):
    """The call's launches hold `name` as a wave launch over the whole batch; returns that launch (None: planned elsewhere)."""
    if report.i("c%d.rc" % c) != 0 or not report.i("c%d.filtered" % c):
        return None
    hits = [ln for ln in KL.planned_launches(report, c) if ln["family"] == "wave" and ln["kernel"] == name and not ln["list"]]
    return hits[0] if hits else None


@pytest.fixture(scope="module")
def win_plans(tmp_path_factory):
    """Every window recipe through the per-call planner, one driver run: `seq` = the main and the edge batch on one context;
    `ends` = the planned read lengths one beyond either end of the cell and far beyond it; `wide` / `narrow` = the same
    config with the window one column wider than the cell's widest / narrower than its narrowest."""
    import call_cases as CC

    d = tmp_path_factory.mktemp("win")
    cases = []
    for i, name in enumerate(WIN_CASES):
        rc = KL.recipe(name)
        cases.append(rc.case("seq%d" % i, [(rc.n_main, rc.main_len), (rc.n_edge, rc.edge_len)]))
        cases.append(rc.case("ends%d" % i, [(rc.n_edge, rc.low - 1), (rc.n_edge, rc.low), (rc.n_edge, rc.high or 10 * rc.main_len),
                                            (rc.n_edge, (rc.high or 10 * rc.main_len) + 1)]))
        cases.append(rc.case("wide%d" % i, [(rc.n_edge, 2 * rc.w + 3)], w=rc.w + 1))
        if rc.w_lo > 1:
            cases.append(rc.case("narrow%d" % i, [(rc.n_edge, 2 * rc.w_lo - 1)], w=rc.w_lo - 1))
    return CC.run_driver(CC.build_driver(d), d, cases=cases, launches=True)


@pytest.mark.parametrize("name", WIN_CASES)
def test_window_recipe_lands_in_its_cell(name, win_plans):
    """The planner itself puts both batches in the target cell as the call's only wave launch, over the whole batch, two or
    more tiles per resident wave and a ragged last one; one base of planned read length beyond either end of the cell plans
    elsewhere (or the recipe states what ends it, and ten times the length still plans to the target); one window column
    beyond either end of WIN_CELLS plans elsewhere.  No switch is forced."""
    rc = KL.recipe(name)
    i = WIN_CASES.index(name)
    fam, a = KL.parse(name)
    assert rc.env == {"BDX_CU_COUNT": "1"} and rc.forced_why is None
    seq = win_plans["seq%d" % i]
    for c, n in enumerate((rc.n_main, rc.n_edge)):
        ln = _whole_batch_wave(seq, c, name)
        assert ln is not None, (c, KL.planned_launches(seq, c))
        assert seq.plan(c)["front"] == "wave_win" and seq.tiles("wfront", c)["slot"] == (rc.w + 30) & ~15
        waves = ln["blocks"] * ln["threads"] // 64
        assert ln["tile"] == a["RW"] and n % a["RW"] == 1 and -(-n // a["RW"]) >= 2 * waves > 0, ln
    ends = win_plans["ends%d" % i]
    assert _whole_batch_wave(ends, 0, name) is None, f"{rc.low} is not the shortest planned read of the cell"
    assert _whole_batch_wave(ends, 1, name) is not None and _whole_batch_wave(ends, 2, name) is not None
    assert (_whole_batch_wave(ends, 3, name) is not None) == (rc.end_why is not None), "the recipe states no end / a wrong one"
    assert (rc.high is None) == (rc.end_why is not None) and (rc.end_why is None or "bdx_call.cpp" in rc.end_why)
    assert _whole_batch_wave(win_plans["wide%d" % i], 0, name) is None, f"{rc.w} columns are not the widest window of the cell"
    assert rc.w_lo == 1 or _whole_batch_wave(win_plans["narrow%d" % i], 0, name) is None, f"{rc.w_lo} columns are not the narrowest window of the cell"


@pytest.mark.parametrize("name", WIN_CASES)
def test_window_recipe_is_not_vacuous(name):
    """By the oracle alone: at least half of the main batch is assigned.  The edge batch holds at least four reads of every
    kind; reads of no bases, shorter than a barcode, shorter than the window, longer than twice the planned length, with N; the
    window's first byte takes every 16-byte phase of the batch; barcodes at the window's first and last column are assigned,
    barcodes wholly outside it and copies one beyond the budget are not all; and at most an eighth of the reads have a window
    that does not fit the planned slot at its phase (those the kernel hands on by design)."""
    import helpers as H

    rc = KL.recipe(name)
    oc = H.orc.OracleClassifier(rc.config(), nthreads=min(16, os.cpu_count() or 1), want_pass=False)
    seq, off, planned = rc.batch("main")
    assert len(off) - 1 == rc.n_main and planned == rc.main_len and int((off[1:] - off[:-1]).max()) == planned
    assigned = oc.classify(seq, off)["bc1"] > 0
    assert 2 * int(assigned.sum()) >= rc.n_main, f"{int(assigned.sum())} of {rc.n_main} reads of the main batch are assigned"
    seq, off, kinds = rc.edge_batch()
    lens = off[1:] - off[:-1]
    assert len(lens) == rc.n_edge and int(lens[0]) == rc.edge_len
    assert (lens == 0).any() and ((lens > 0) & (lens < rc.m)).any() and (lens > 2 * rc.edge_len).any() and (seq == ord("N")).any()
    assert ((lens >= rc.m) & (lens < rc.w)).any() and len(set(lens.tolist())) >= 20
    # (the host entry uploads whole reads, so that the window kernel sees them: batches of 512 bases per read and more go up as
    # windows alone, classify_host_windows in bdx_host.cpp)
    assert int(off[-1]) < 512 * rc.n_edge and rc.main_len < 512
    wins = [rc.window(int(n)) if n > 0 else (1, 0) for n in lens]
    slot = (rc.w + 30) & ~15
    phases = {int(off[i] + f - 1) & 15 for i, (f, l) in enumerate(wins) if l >= f}
    assert phases == set(range(16)), sorted(phases)
    too_wide = sum(1 for i, (f, l) in enumerate(wins) if l >= f and (int(off[i] + f - 1) & 15) + (l - f + 1) > slot)
    assert too_wide <= rc.n_edge // 8, too_wide
    if rc.style != "end":  # (a window counted from the end alone is never empty)
        assert sum(1 for n, (f, l) in zip(lens, wins) if n > 0 and l < f) >= 4
    full = oc.classify(seq, off)
    assigned = full["bc1"] > 0
    assert set(kinds) == set(rc.kinds)
    for kind in rc.kinds:
        of_kind = [i for i, k in enumerate(kinds) if k == kind]
        assert len(of_kind) >= 4, (kind, len(of_kind))
        if kind in ("win_first", "win_last", "sub_kb", "straddle16", "N_out"):
            assert assigned[of_kind].any(), f"no {kind} read is assigned"
        if kind in ("win_outside", "sub_kb1", "none", "short", "empty", "before_start"):
            assert not assigned[of_kind].all(), f"every {kind} read is assigned"
    _one_column_out(rc, rc.config(), seq, off, kinds, rc.window)
    # long_ends: a window bound counted from the end must be counted from the read's own end.  Cut to the planned length, such a
    # read has the window a kernel that counted from the planned length would give it: the verdict must differ
    import numpy as np

    ends = [i for i, k in enumerate(kinds) if k == "long_ends"]
    assert all(rc.edge_len + rc.m <= lens[i] <= rc.edge_len + rc.m + 8 for i in ends)
    cut = np.concatenate([seq[off[i]: off[i] + rc.edge_len] for i in ends])
    cut_off = np.arange(len(ends) + 1, dtype=np.int64) * rc.edge_len
    wrong = oc.classify(cut, cut_off)["bc1"]
    differ = sum(int(wrong[j] != full["bc1"][i]) for j, i in enumerate(ends))
    if rc.style == "start":
        assert differ == 0 and assigned[ends].all()
    else:
        assert 4 * differ >= 3 * len(ends), (differ, len(ends))
        assert assigned[ends].mean() >= 0.75 if rc.style == "end" else assigned[ends].mean() <= 0.5, assigned[ends].mean()


GEN_CASES = [n for n in KL.classify_kernels() if isinstance(KL.recipe(n), KL.GenRecipe)]


@pytest.fixture(scope="module")
def gen_plans(tmp_path_factory):
    """Every general-form recipe through the per-call planner, one driver run: `seq` = the main and the edge batch on one
    context; `ends` = the longest read one base beyond either end of the cell; `plain` = without BDX_WAVE_RW, every read length."""
    import call_cases as CC

    d = tmp_path_factory.mktemp("gen")
    cases = []
    for i, name in enumerate(GEN_CASES):
        rc = KL.recipe(name)
        cases.append(rc.case("seq%d" % i, [(rc.n_main, rc.main_len), (rc.n_edge, rc.edge_len)]))
        cases.append(rc.case("ends%d" % i, [(rc.n_edge, rc.high + 1), (rc.n_edge, max(rc.low - 1, 1))]))
        if rc.forced_why:
            cases.append(rc.case("plain%d" % i, [(rc.n_edge, L) for L in range(1, KL.MAX_LEN + 1)], force=False))
    return CC.run_driver(CC.build_driver(d), d, cases=cases, launches=True)


@pytest.mark.parametrize("name", GEN_CASES)
def test_general_recipe_lands_in_its_cell(name, gen_plans):
    """The planner itself puts both batches in the target cell as a wave launch over the whole batch (the front stage of a
    known-score call, the filter of a split one), two or more tiles per resident wave and a ragged last one, in the argument
    state the recipe names: passes, ranges and scan_gpr as the plan states them.  One base beyond either end of the cell plans
    elsewhere; BDX_WAVE_RW is forced only where no read length reaches the cell without it."""
    rc = KL.recipe(name)
    i = GEN_CASES.index(name)
    fam, a = KL.parse(name)
    seq = gen_plans["seq%d" % i]
    which = "wfull" if rc.split else "wfront"
    for c, (n, L) in enumerate(((rc.n_main, rc.main_len), (rc.n_edge, rc.edge_len))):
        ln = _whole_batch_wave(seq, c, name)
        assert ln is not None, (c, KL.planned_launches(seq, c))
        waves = ln["blocks"] * ln["threads"] // 64
        assert ln["tile"] == a["RW"] and n % a["RW"] == 1 and n >= 512 and -(-n // a["RW"]) >= 2 * waves > 0, ln
        p, t = seq.plan(c), seq.tiles(which, c)
        assert p["npass"] == (2 if rc.dual else 1) and p["split"] == int(rc.split) and t["winm"] == 0 and rc.low <= L <= rc.high
        assert (p["full"] == "wave_split") == rc.split and (rc.split or p["front"] == "wave")
        if rc.state == "ranged_scan":  # (the window is about half the read: 76..80 columns of 150 bases)
            assert t["scan_gpr"] > 0 and 2 * rc.w > L >= rc.scan_low > 0, (t, rc.w)
        elif not rc.dual:
            assert t["scan_gpr"] == 0
        gen = [x["args"][8] for x in seq.launches(c) if x["family"] == "wave"]
        assert gen == [1], gen
    ends = gen_plans["ends%d" % i]
    assert _whole_batch_wave(ends, 0, name) is None, f"{rc.high} is not the longest read of the cell"
    assert rc.low == 1 or _whole_batch_wave(ends, 1, name) is None, f"{rc.low} is not the shortest read of the cell"
    if rc.forced_why:
        assert rc.env == {"BDX_CU_COUNT": "1", "BDX_WAVE_RW": str(a["RW"])} and "bdx_call.cpp" in rc.forced_why
        plain = gen_plans["plain%d" % i]
        reached = [c + 1 for c in range(KL.MAX_LEN) if _whole_batch_wave(plain, c, name) is not None]
        assert not reached, f"forced, yet reachable plainly at {reached[:4]} bases"
    else:
        assert rc.env == {"BDX_CU_COUNT": "1"}


def test_general_recipes_spread_the_argument_states():
    """All 72 general forms have a recipe; every argument state runs at every RW and both NV of the non-split and of the split
    kernel (the split one takes only ranged configs: bdx_launch_wave, bdx_wave.hip); few cells force the tile size."""
    assert len(GEN_CASES) == 72
    rcs = [KL.recipe(n) for n in GEN_CASES]
    for split in (False, True):
        seen = {(rc.rw, rc.nv, rc.state) for rc in rcs if rc.split == split}
        assert seen == {(rw, nv, s) for rw in (32, 16, 8) for nv in (5, 10) for s in KL.GEN_STATES[split]}, split
    assert "dual_whole" not in KL.GEN_STATES[True] and sum(rc.forced_why is not None for rc in rcs) == 8
    # the non-split target answers all but a quarter of a batch itself, but for the two 1272-base cells that state their own share
    assert sorted((rc.target, rc.list_div) for rc in rcs if not rc.split and rc.list_div != 4) == [
        ("bdx_wave_kernel<8, 0, 10, 6, false, 0, 0, false, 0, true, false>", 2), ("bdx_wave_kernel<8, 12, 10, 7, false, 0, 0, false, 0, true, false>", 1.5)]
    for rc in rcs:
        r1, r2 = rc.range_strs()
        assert (r1 is None) == (rc.state == "dual_whole") and (r2 is not None) == (rc.state == "dual_ranged")


@pytest.mark.parametrize("name", GEN_CASES)
def test_general_recipe_is_not_vacuous(name):
    """By the oracle alone: at least a quarter of the main batch is assigned.  The edge batch holds at least four reads of
    every kind, its longest read is the cell's, and it has reads of no bases, shorter than a barcode and with N; barcodes at the
    window's first and last column are assigned, barcodes wholly outside a window that leaves room outside and copies one beyond
    the budget are not all; dual configs: reads with both barcodes are assigned, reads with pass 2's alone are not."""
    import helpers as H

    rc = KL.recipe(name)
    oc = H.orc.OracleClassifier(rc.config(), nthreads=min(16, os.cpu_count() or 1), want_pass=False)
    seq, off, longest = rc.batch("main")
    assert len(off) - 1 == rc.n_main and longest == rc.main_len
    assigned = oc.classify(seq, off)["bc1"] > 0
    assert 4 * int(assigned.sum()) >= rc.n_main, f"{int(assigned.sum())} of {rc.n_main} reads of the main batch are assigned"
    seq, off, kinds = rc.edge_batch()
    lens = off[1:] - off[:-1]
    assert len(lens) == rc.n_edge and int(lens.max()) == rc.edge_len == int(lens[0])
    assert (lens == 0).any() and ((lens > 0) & (lens < rc.m)).any() and (seq == ord("N")).any() and len(set(lens.tolist())) >= 20
    if rc.state == "ranged_flat":  # reads shorter than the window's first column
        assert sum(1 for n in lens if 0 < n <= KL.GEN_K) >= 4
    if rc.state == "dual_ranged":  # windows counted from the end on reads of several lengths within one tile
        per_tile = [len(set(lens[t: t + rc.rw].tolist())) for t in range(0, rc.n_edge - 1, rc.rw)]
        assert 4 * sum(k >= 3 for k in per_tile) >= len(per_tile), per_tile
    got = oc.classify(seq, off)
    assigned = got["bc1"] > 0
    assert set(kinds) == set(rc.kinds)
    for kind in rc.kinds:
        of_kind = [i for i, k in enumerate(kinds) if k == kind]
        assert len(of_kind) >= 4, (kind, len(of_kind))
        if kind in ("win_first", "win_last", "sub_kb", "straddle16", "both") and (kind == "both" or not rc.dual):
            assert assigned[of_kind].any(), f"no {kind} read is assigned"
        if kind in ("sub_kb1", "none", "short", "empty", "before_start", "p2_only") or (kind == "win_outside" and rc.state != "dual_whole"):
            assert not assigned[of_kind].all(), f"every {kind} read is assigned"
    if not rc.dual:
        _one_column_out(rc, rc.config(), seq, off, kinds, rc.window)


PAIRS_CASES = [n for n in KL.classify_kernels() if isinstance(KL.recipe(n), KL.PairsRecipe)]


def _pairs_list_launch(report, c, name):
    """The call's launches hold `name` as a pairs launch over tier 1's list behind a wave launch over the whole batch."""
    if report.i("c%d.rc" % c) != 0 or not report.i("c%d.filtered" % c):
        return None
    ls = KL.planned_launches(report, c)
    hits = [ln for ln in ls if ln["family"] == "pairs" and ln["kernel"] == name and ln["list"]]
    return hits[0] if hits and ls[0]["family"] == "wave" and not ls[0]["list"] else None


@pytest.fixture(scope="module")
def pairs_plans(tmp_path_factory):
    import call_cases as CC

    d = tmp_path_factory.mktemp("pairs")
    cases = []
    for i, name in enumerate(PAIRS_CASES):
        rc = KL.recipe(name)
        cases.append(rc.case("seq%d" % i, [(rc.n_main, rc.main_len), (rc.n_edge, rc.edge_len)]))
        cases.append(rc.case("ends%d" % i, [(rc.n_edge, rc.high + 1), (rc.n_edge, max(rc.low - 1, 1)), (rc.n_edge, rc.low)]))
        cases.append(rc.case("cpr%d" % i, [(rc.n_edge, L) for L in range(max(rc.low, rc.m), rc.edge_len + 1)]))
    return CC.run_driver(CC.build_driver(d), d, cases=cases, launches=True)


@pytest.mark.parametrize("name", PAIRS_CASES)
def test_pairs_recipe_lands_in_its_cell(name, pairs_plans):
    """The planner itself puts both batches in the target cell: tier 1 over the whole batch, then the target over tier 1's list
    (a list launch).  The shortest and the longest read of the cell plan to the target, one base beyond either end plans
    elsewhere (NV 3 begins at one base).  No switch is forced; the forms with a summary are planned with statistics."""
    rc = KL.recipe(name)
    i = PAIRS_CASES.index(name)
    assert rc.env == {"BDX_CU_COUNT": "1"} and rc.forced_why is None
    seq = pairs_plans["seq%d" % i]
    for c in range(2):
        ln = _pairs_list_launch(seq, c, name)
        assert ln is not None, (c, KL.planned_launches(seq, c))
        assert ln["tile"] == 16 and seq.plan(c)["middle"] in ("list", "end", "split") and seq.plan(c)["tier_len"] > 0, seq.plan(c)
    ends = pairs_plans["ends%d" % i]
    assert _pairs_list_launch(ends, 0, name) is None, f"{rc.high} is not the longest read of the cell"
    assert rc.low == 1 or _pairs_list_launch(ends, 1, name) is None, f"{rc.low} is not the shortest read of the cell"
    assert _pairs_list_launch(ends, 2, name) is not None
    # the edge batch has reads on both sides of a step of cpr (the 16-diagonal chunks scanned per read) and of a slot step, as
    # the planner's wmid line states them for every read length of the cell
    import numpy as np

    sweep = pairs_plans["cpr%d" % i]
    lo = max(rc.low, rc.m)
    tiles = [sweep.tiles("wmid", c) for c in range(rc.edge_len + 1 - lo)]
    lens = set(np.diff(rc.edge_batch()[1]).tolist())
    for key in ("cpr", "slot"):
        steps = [lo + c for c in range(1, len(tiles)) if tiles[c][key] != tiles[c - 1][key]]
        assert steps and any(s in lens and s - 1 in lens for s in steps), (key, steps)


@pytest.fixture(scope="module")
def extra_plans(tmp_path_factory):
    import call_cases as CC

    d = tmp_path_factory.mktemp("extras")
    cases = [x.case(x.key) for x in KL.PAIRS_EXTRAS]
    cases += [x.case(x.key + "_plain") for x in KL.PAIRS_EXTRAS if x.forced_why]
    for c, x in zip(cases[len(KL.PAIRS_EXTRAS):], [x for x in KL.PAIRS_EXTRAS if x.forced_why]):
        c.tune = dict(n_cu=1)
    return CC.run_driver(CC.build_driver(d), d, cases=cases, launches=True)


@pytest.mark.parametrize("x", KL.PAIRS_EXTRAS, ids=lambda x: x.key)
def test_pairs_extra_case_plans_its_state_and_route(x, extra_plans):
    """The planner itself gives each extra case its argument state and entry route, on both calls of the context: the dual
    C4-shaped configs launch the KEND form over tier 1's list with carried passes exactly where min_delta = 0 and the caller wants
    the verdict alone; the KB 8 / KB 9 cells run behind a wave tier (Middle::split), with no tier (Middle::all, over the whole
    batch) and with a pairs tier (Front::pairs: KB 8 in front over the whole batch, KB 9 over its list).  BDX_NO_TIER is forced
    only for the KB 9 cell's Middle::all, which the same config does not plan without it."""
    r = extra_plans[x.key]
    for c in range(2):
        p = r.plan(c)
        hits = [ln for ln in KL.planned_launches(r, c) if ln["family"] == "pairs" and ln["kernel"] == x.target]
        assert len(hits) == 1 and bool(hits[0]["list"]) == (not x.whole), (p, KL.planned_launches(r, c))
        assert p["carry"] == x.carry and p["npass"] == (2 if x.dual else 1)
        want = {"split": (("wave", "wave_split", "wave_end"), ("list", "split", "end")), "all": (("none",), ("all",)), "front": (("pairs",), ("split",))}[x.route]
        assert p["front"] in want[0] and p["middle"] in want[1], p
        if x.whole:
            assert x.n % 16 == 1 and -(-x.n // 16) >= 2 * hits[0]["blocks"] * hits[0]["threads"] // 64
    assert (x.env != {"BDX_CU_COUNT": "1"}) == (x.forced_why is not None)
    if x.forced_why:
        assert "bdx_call.cpp" in x.forced_why and extra_plans[x.key + "_plain"].plan(0)["middle"] != "all"


def test_pairs_extra_cases_are_the_ones_named():
    keys = [x.key for x in KL.PAIRS_EXTRAS]
    assert len(keys) == len(set(keys)) == 14
    dual = sorted((KL.parse(x.target)[1]["KEND"], x.delta > 0, x.carry) for x in KL.PAIRS_EXTRAS if x.dual)
    # (carried passes need min_delta = 0 and a caller that wants the verdict alone: the KEND 3 case wants per-pass outputs)
    assert dual == sorted((k, d, int(not d and k < 3)) for k in range(4) for d in (False, True))
    assert all(KL.parse(x.target)[1] == dict(KL.parse(x.target)[1], NV=3, KB=4, NW=2) for x in KL.PAIRS_EXTRAS if x.dual)
    assert {(KL.parse(x.target)[1]["KB"], x.route) for x in KL.PAIRS_EXTRAS if not x.dual} == {(kb, r) for kb in (8, 9) for r in ("split", "all", "front")}
    for x in KL.PAIRS_EXTRAS:
        assert x.target in KL.code_object_kernels() and KL.recipe(x.target) is not None


@pytest.mark.parametrize("x", KL.PAIRS_EXTRAS, ids=lambda x: x.key)
def test_pairs_extra_case_is_not_vacuous(x):
    """By the oracle alone: a quarter and more of the main batch is assigned and a tenth is not; dual edge batches have reads with
    both barcodes (some assigned) and with pass 2's alone (not all assigned)."""
    import helpers as H

    oc = H.orc.OracleClassifier(x.config(), nthreads=min(16, os.cpu_count() or 1), want_pass=False)
    seq, off, _ = x.batch("main")
    assigned = oc.classify(seq, off)["bc1"] > 0
    assert 0.25 <= assigned.mean() <= 0.9, assigned.mean()
    if x.dual:
        seq, off, kinds = KL.win_edge_reads(x.barcodes(), 4, lambda n: (1, n), x.len, x.n, 8500 + len(x.key), KL.GEN_DUAL_KINDS, k_front=1,
                                            spread=x.len - x.m, second=(x.barcodes(1), lambda n: (1, n)))
        assert (seq == x.batch("edge")[0]).all()
        assigned = oc.classify(seq, off)["bc1"] > 0
        both, p2 = [i for i, k in enumerate(kinds) if k == "both"], [i for i, k in enumerate(kinds) if k == "p2_only"]
        assert len(both) >= 4 and len(p2) >= 4 and assigned[both].any() and not assigned[p2].all()


def test_pairs_recipes_cover_the_lattice():
    """Every (NV, KB, NW, KEND, SPLIT, MG) cell of the pairs lattice once; barcode numbers of 64 and more (a third mask word)
    in every NW 3 / 4 cell; the KEND 3 cells compare the statistics tables (NW 2) or the per-pass outputs (NW 3 / 4)."""
    assert len(PAIRS_CASES) == 76
    rcs = [KL.recipe(n) for n in PAIRS_CASES]
    assert len({(rc.nv, rc.kb, rc.nw, rc.kend, rc.split, rc.mg) for rc in rcs}) == 76
    for rc in rcs:
        assert (rc.n_bc > 64) == (rc.nw >= 3) and (rc.n_bc > 128) == rc.mg
        assert (rc.summary, rc.want_pass) == ((rc.nw == 2, rc.nw != 2) if rc.kend == 3 else (False, False))
        assert (rc.mid_div == 4) == (not rc.split and not rc.mg)
        overflows = rc.mid_div == 4 and (rc.kb, rc.nv) == (4, 6) and rc.nw >= 3  # (the cells whose flag queue runs over at the cell's longest reads)
        assert rc.edge_mid_div == rc.mid_div and (rc.edge_len < rc.high) == overflows == (rc.edge_why is not None)
        assert rc.edge_why is None or "bdx_call.cpp" in rc.edge_why


@pytest.mark.parametrize("name", PAIRS_CASES)
def test_pairs_recipe_is_not_vacuous(name):
    """By the oracle alone.  Main batch: at least a quarter of the reads are assigned at a distance above tier 1's cap (m / q - 1
    = 2 for 24 nt) — the reads only the pairs mode can settle — and at least a quarter carry no barcode.  Edge batch: four or
    more reads of every kind, the longest read is the cell's, lengths on both sides of a slot step (1 and 2 mod 16), reads with
    exactly two intact pieces are assigned and reads with one intact piece are not all (unit costs)."""
    import helpers as H

    rc = KL.recipe(name)
    oc = H.orc.OracleClassifier(rc.config(), nthreads=min(16, os.cpu_count() or 1), want_pass=True)
    seq, off, longest = rc.batch("main")
    got = oc.classify(seq, off)
    assigned = got["bc1"] > 0
    import numpy as np

    beyond = assigned & (np.rint(got["pass_score"][:, 0] * rc.m) > 2)  # (the score is the cost over the barcode's length)
    assert 4 * int(beyond.sum()) >= rc.n_main, f"{int(beyond.sum())} of {rc.n_main} reads are assigned beyond tier 1's cap"
    assert 4 * int((~assigned).sum()) >= rc.n_main, f"{int((~assigned).sum())} of {rc.n_main} reads are unassigned"
    seq, off, kinds = rc.edge_batch()
    lens = off[1:] - off[:-1]
    assert len(lens) == rc.n_edge and int(lens.max()) == rc.edge_len == int(lens[0])
    assert (lens % 16 == 1).any() and (lens % 16 == 2).any() and (lens == 0).any()
    assigned = oc.classify(seq, off)["bc1"] > 0
    for kind in rc.kinds:
        of_kind = [i for i, k in enumerate(kinds) if k == kind]
        assert len(of_kind) >= 4, (kind, len(of_kind))
        if "indel" not in rc.kw and "matching_algorithm" not in rc.kw:
            if kind in ("diag_adjacent", "diag_first_last", "sub_kb", "col1", "cut_front"):  # (col1: a barcode at the slot's first column)
                assert assigned[of_kind].any(), f"no {kind} read is assigned"
            if kind in ("diag_one_piece", "sub_kb1"):
                assert not assigned[of_kind].all(), f"every {kind} read is assigned"
        if "indel" in rc.kw:  # the same-diagonal variants: as many indels as the budget pays for are assigned, budget + 1 not always
            if kind in ("sd_gmax", "sub_kb", "col1"):
                assert assigned[of_kind].any(), f"no {kind} read is assigned"
            if kind == "sub_kb1":
                assert not assigned[of_kind].all(), f"every {kind} read is assigned"
    if rc.nw >= 3:
        # a third (fourth) mask word is in use: of the main batch's reads that only the pairs mode can settle, at least half the
        # even share carry a barcode number of 65 and more (97 and more)
        nums = got["bc1"][beyond]
        assert (nums > 64).mean() >= 0.5 * (rc.n_bc - 64) / rc.n_bc, (nums > 64).mean()
        if rc.nw == 4:
            assert (nums > 96).mean() >= 0.5 * (rc.n_bc - 96) / rc.n_bc, (nums > 96).mean()


def test_the_rolling_band_takes_64_lanes_by_the_barcode_count(tmp_path):
    """The step the recipe of bdx_generic_kernel<64, 0, true, false> sits on, by the planner itself: the lane count of the
    rolling band follows plan_generic's `fixed` term (staged barcode bytes, per-barcode words, histogram) as much as its cells.
    The recipe's own set at its own rate plans 64 lanes; one budget less (rate 0.43), ten barcodes fewer, or no trace-back (no
    trimming) plan 128 lanes; four barcodes (what a sweep over length and rate alone would use) never leave 128 lanes."""
    import call_cases as CC
    import plan_cases as PC

    rc = KL.recipe("bdx_generic_kernel<64, 0, true, false>")
    bcs = rc.barcodes()
    assert (len(bcs), rc.rate, rc.kw["trim_side"]) == (250, 0.44, 5) and not KL.UNREACHABLE
    shapes = {"own": (bcs, 0.44, 5), "rate043": (bcs, 0.43, 5), "b240": (bcs[:240], 0.44, 5), "no_trim": (bcs, 0.44, 0), "b4": (bcs[:4], 0.44, 5)}
    cases = [CC.CallCase(k, None, [CC.call(rc.n_edge, rc.edge_len, wanted=KL.WANT_ALL)], passes=[PC.one_pass(b, trim=t)], rate=r, tune=dict(n_cu=1))
             for k, (b, r, t) in shapes.items()]
    got = CC.run_driver(CC.build_driver(tmp_path), tmp_path, cases=cases, launches=True)
    lanes = {k: {KL.generic_name(ln["args"]) for ln in got[k].launches() if ln["family"] == "generic"} for k in shapes}
    assert lanes["own"] == {"bdx_generic_kernel<64, 0, true, false>"}
    for k in ("rate043", "b240", "no_trim", "b4"):
        assert lanes[k] == {"bdx_generic_kernel<128, 0, true, false>"}, (k, lanes[k])


@pytest.mark.parametrize("name", WAVE_CASES)
def test_recipe_lands_in_its_cell(name):
    """The rules (form from the config, geometry from size_wave of bdx_call.cpp) put both batches of the recipe in the target cell; the
    edge batch's longest read is the longest that stays there and the main batch's the shortest that holds a barcode with
    flanks; both batches end in a ragged tile and walk at least two tiles per resident wave of the one CU.  BDX_WAVE_RW is
    forced only where no read length reaches the cell with the planner's own choice."""
    rc = KL.recipe(name)
    fam, a = KL.parse(name)
    assert KL.wave_form_of(rc.form["kw"], rc.want_pass)["form"] == KL.wave_form(name), "the config lands in another form"
    assert rc.predict(rc.n_main, rc.main_len) == name, (rc.env, rc.main_len)
    assert rc.predict(rc.n_edge, rc.edge_len) == name, (rc.env, rc.edge_len)
    assert rc.predict(rc.n_edge, rc.edge_len + 1) != name, f"{rc.edge_len} is not the longest read of the cell"
    assert rc.low == 1 or rc.predict(rc.n_edge, rc.low - 1) != name, f"{rc.low} is not the shortest read of the cell"
    assert rc.main_len == min(max(rc.low, rc.m + 40), rc.edge_len)
    plain = KL.Recipe(name, KL.wave_form(name), rc.m, rc.min_hamming, rc.n_bc, rc.rw, rc.nv)
    if "BDX_WAVE_RW" in rc.env:
        assert rc.forced_why, name
        plain.env = {"BDX_CU_COUNT": "1"}
        assert not [L for L in range(1, KL.MAX_LEN + 1) if plain.predict(rc.n_edge, L) == name], "forced, yet reachable plainly"
    else:
        assert rc.forced_why is None and rc.env == {"BDX_CU_COUNT": "1"}
    for n in (rc.n_main, rc.n_edge):
        assert n % a["RW"] == 1 and n >= 512
        assert -(-n // a["RW"]) >= 2 * 16
    sp = KL.wave_seed_plan([rc.m] * rc.n_bc, KL.RATE)
    assert sp["chance"] <= 6.0 and sp["expected"] <= 7.0 and 3 * sp["expected"] <= rc.n_bc, sp
    seq, off, longest = rc.batch("edge")
    lens = off[1:] - off[:-1]
    assert len(lens) == rc.n_edge and int(lens.max()) == rc.edge_len == longest
    assert (lens == 0).any() and (lens < rc.m).any() and (seq == ord("N")).any()


def test_size_wave_restated_equals_the_call_planner(tmp_path):
    """Over the lattice's own grid — every recipe's config, both batch sizes, one CU, the forced tile size where the recipe
    forces one, the read lengths at and beside both ends of its cell — kernel_lattice.size_wave returns what the per-call
    planner (csrc/bdx_call.cpp, through tests/call_host.cpp) returns: tile, workgroup shape, grid and span, or no wave plan."""
    import call_cases as CC
    import plan_cases as PC

    grid = {}
    for name in WAVE_CASES:
        rc = KL.recipe(name)
        key = (tuple(sorted(rc.form["kw"].items())), rc.want_pass, rc.m, rc.n_bc, rc.env.get("BDX_WAVE_RW", "0"))
        grid.setdefault(key, (rc, set()))[1].update((n, L) for n in (rc.n_main, rc.n_edge)
                                                    for L in (max(rc.low - 1, 1), rc.low, rc.main_len, rc.edge_len, rc.edge_len + 1))
    assert len(grid) >= 20
    cases, expect = [], {}
    for i, (key, (rc, shapes)) in enumerate(sorted(grid.items(), key=lambda kv: kv[0])):
        kw = dict(key[0])
        costs = (kw.get("match", 0), kw.get("mismatch", 1), kw.get("indel", 1))
        tune = dict(n_cu=1, **({"wave_rw": int(key[4])} if key[4] != "0" else {}))
        shapes = sorted(shapes)
        cases.append(CC.CallCase("lattice%d" % i, None, [CC.call(n, L, wanted=CC.PASS_START if rc.want_pass else 0) for n, L in shapes],
                                 passes=[PC.one_pass(rc.barcodes(), trim=kw.get("trim_side") or 0)], rate=KL.RATE, costs=costs, tune=tune))
        sp = KL.wave_seed_plan([rc.m] * rc.n_bc, KL.RATE)
        expect["lattice%d" % i] = [KL.size_wave(sp, rc.derived["kend"], rc.cand_words, L, n, 1, int(key[4])) for n, L in shapes]
    got = CC.run_driver(CC.build_driver(tmp_path), tmp_path, cases=cases)
    checked = 0
    for name, want in expect.items():
        r = got[name]
        for c, g in enumerate(want):
            p = r.plan(c)
            which = "wfull" if p["full"] == "wave_split" else "wfront" if p["front"] in ("wave", "wave_end") else None
            if g is None:
                assert which is None, (name, c)
                continue
            assert which is not None, (name, c, g)
            t = r.tiles(which, c)
            assert dict(rw=t["rw"], waves=t["waves"], blocks=t["blocks"], span=t["span_cap"]) == g, (name, c)
            checked += 1
    assert checked >= 100
