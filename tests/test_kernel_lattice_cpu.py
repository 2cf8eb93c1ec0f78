"""Bookkeeping of the instantiation lattice (no GPU; needs the built library): every classify instantiation in the code
object has exactly one recipe, UNREACHABLE entry or PENDING pattern, and every recipe's target follows from the planner's
rules as kernel_lattice.py restates them — a recipe that drifts off its cell fails here, before it runs on a GPU."""
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


@pytest.mark.parametrize("name", [n for n in KL.classify_kernels() if KL.recipe(n) is not None])
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
    for name in KL.classify_kernels():
        rc = KL.recipe(name)
        if rc is not None:
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
