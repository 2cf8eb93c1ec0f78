"""Bookkeeping of the instantiation lattice (no GPU; needs the built library): every classify instantiation in the code
object has exactly one recipe, UNREACHABLE entry or PENDING pattern, and every recipe's target follows from the planner's
rules as kernel_lattice.py restates them — a recipe that drifts off its cell fails here, before it runs on a GPU.  The
fused filter's and the exact kernel's recipes are held against the planner itself (tests/call_host.cpp), and the oracle
alone shows that their batches are not vacuous."""
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
    assert len(WAVE_CASES) == 180 and len(CELL_CASES) == 46


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
