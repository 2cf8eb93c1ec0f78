"""The builders of offset_cases.py, checked without a GPU (needs the built library for the lattice's recipes): every fetch site
still has its recipe and the planner itself (tests/call_host.cpp) plans that recipe to its site; the bases put the 2^31 / 2^32
boundary where they say; every alias of every base lies inside the arena; and, by the oracle alone, the decoys and the planted
ends are not vacuous: a truncated offset or a leaking granule mask WOULD change what the kernels answer."""
import os

import numpy as np
import pytest

import helpers as H
import kernel_lattice as KL
import offset_cases as OC

NTHREADS = min(16, os.cpu_count() or 1)
assert os.path.exists(H.bdx.LIB_PATH), "HIP extension missing: run __graft_entry__.build()"


def test_every_site_still_has_its_recipe():
    assert len(OC.SITES) == 14 and len(set(OC.NAMES)) == 14
    for site, (name, why) in OC.SITES.items():
        obj = OC.get(name)
        assert obj is not None, f"{site}: kernel_lattice.py has no recipe {name} any more"
        assert OC.target(name) in KL.code_object_kernels(), f"{site}: {OC.target(name)} is not in the code object"
        for which in ("main", "edge"):
            seq, off, _ = obj.batch(which)
            assert off[0] == 0 and off[-1] == len(seq) and len(off) >= 2
    assert set(OC.HOSTILE_NAMES) <= set(OC.NAMES)
    assert sorted(s for v in OC.SHIFTS.values() for s in v) == list(range(16)) and all(2 <= len(v) <= 3 for v in OC.SHIFTS.values())


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    import call_cases as CC

    d = tmp_path_factory.mktemp("offset_sites")
    cases = [OC.driver_case(name, "s%d" % i) for i, name in enumerate(OC.NAMES)]
    return CC.run_driver(CC.build_driver(d), d, cases=cases, launches=True)


@pytest.mark.parametrize("site", list(OC.SITES))
def test_recipe_plans_to_its_site(site, plans):
    """Both calls of the recipe (main, then edge, on one context) as the planner plans them: the target instantiation in the
    role the site is named for."""
    name = OC.SITES[site][0]
    obj, target = OC.get(name), OC.target(name)
    r = plans["s%d" % OC.NAMES.index(name)]
    for c, which in enumerate(("main", "edge")):
        assert r.i("c%d.rc" % c) == 0
        launches = KL.planned_launches(r, c)
        raw = r.launches(c)
        what = f"{site} {which}: {launches}"
        filtered = bool(r.i("c%d.filtered" % c))
        plan = r.plan(c) if filtered else {}
        hits = [ln for ln in launches if ln["kernel"] == target]
        assert hits, what
        if site == "wave_contiguous":
            assert plan["front"] == "wave" and launches[0]["kernel"] == target and not launches[0]["list"], what
        elif site == "wave_split":
            assert plan["full"] == "wave_split" and plan["windows"] == 1 and plan["exact"] in ("split", "split_list"), plan
            assert not hits[0]["list"] and launches[-1]["family"] == "generic", what
        elif site == "wave_scattered":
            assert plan["middle"] == "all" and hits[0]["family"] == "pairs" and not hits[0]["list"] and launches[0] is hits[0], what
        elif site == "wave_carry":
            assert plan["carry"] == 1 and plan["middle"] == "end" and hits[0]["family"] == "pairs" and hits[0]["list"], (plan, what)
        elif site == "window":
            assert plan["front"] == "wave_win" and launches[0]["kernel"] == target and r.tiles("wfront", c)["winm"] == 1, what
        elif site == "pairs_list":
            assert plan["middle"] == "list" and hits[0]["family"] == "pairs" and hits[0]["list"] and launches[0]["family"] == "wave", what
        elif site == "fused_dense":
            assert KL.whole_batch_target(launches, target) and r.fused(c)["slot_bytes"] == 0, what
        elif site == "fused_list":
            assert plan["front"] == "bitpar" and any(ln["family"] == "bitpar" and ln["list"] for ln in launches), what
            assert KL.whole_batch_target(launches, target), what
        elif site in ("exact_staged", "exact_band", "exact_roll", "exact_unstaged"):
            assert KL.whole_batch_target(launches, target), what
            dense = [ln for ln in raw if ln["family"] == "generic" and not ln["list"]][0]
            bs, reg, clean, um, roll = dense["args"]
            band = r.band("band_exact", c)
            seq, off, _ = obj.batch(which)
            if site == "exact_staged":  # CLEAN register DP without the band; the main batch's workgroups all fit the stage
                assert (reg, clean, roll) == (32, 1, 0) and band["launches"] == 0, (dense, band)
                stage = OC.exact_stage_bytes(obj.barcodes(), bs)
                if which == "main":
                    assert max(OC.workgroup_spans(off, bs)) + 15 + 16 <= stage
            elif site == "exact_band":
                assert band["launches"] >= 1 and band["m"] == 24 and clean == 1, band
            elif site == "exact_roll":
                assert roll == 1 and reg == 0 and bs in (64, 128), dense
            else:  # whatever the pointer's phase, two or more workgroups of the edge batch hold more bytes than the stage
                assert (reg, clean, roll) == (0, 0, 0), dense
                stage = OC.exact_stage_bytes(obj.barcodes(), bs, dp_rows=max(len(x) for x in obj.barcodes()) + 1)
                assert 1024 <= stage < 32 * 1024
                if which == "edge":
                    assert sum(s + 16 > stage for s in OC.workgroup_spans(off, bs)) >= 2, OC.workgroup_spans(off, bs)
        else:
            assert site in ("exact_alone", "exact_alone_m1")
            assert not filtered and [ln["kernel"] for ln in launches] == [target] and not launches[0]["list"], what
    if site == "exact_alone_m1":
        assert obj.kw["match"] == -1


@pytest.mark.parametrize("name", OC.NAMES)
def test_bases_cross_where_they_say(name):
    obj = OC.get(name)
    for which in ("main", "edge"):
        seq, off, _ = obj.batch(which)
        k = OC.crossing_read(off)
        assert 0 < k < len(off) - 1 and off[k + 1] - off[k] >= 16
        b = OC.bases(off)
        assert list(b) == list(OC.BASE_LABELS)
        assert off[k] + b["at_2p31"] == OC.P31 and off[k] + b["at_2p32"] == OC.P32
        assert off[k] + b["in_2p31"] + 7 == OC.P31 and off[k] + b["in_2p32"] + 7 == OC.P32 and off[k + 1] + b["in_2p32"] > OC.P32
        assert b["beyond_2p32"] > OC.P32 and b["beyond_2p32"] % 16 == 3 and b["small"] == 5
        total = len(seq)
        for label, base in b.items():
            assert base > 0
            runs = OC.alias_runs(base, total)
            for a, lo, hi in runs:
                # inside the arena: [origin - 2^31, origin + 2^32 + 16 MiB), clear of the batch itself
                assert -OC.P31 <= a and a + (hi - lo) + 16 <= OC.P32 and 0 <= lo < hi <= total
                assert a + (hi - lo) <= base or a >= base + total
            assert base + total + 16 + OC.SURROUND <= OC.ARENA_BYTES - OC.P31 - 16
            # the reads from the crossing on have an alias; a base whose offsets fit 31 bits has none
            covered = np.zeros(total, dtype=bool)
            for a, lo, hi in runs:
                covered[lo:hi] = True
            if label == "small":
                assert not runs
            elif label == "beyond_2p32":
                assert covered.all()
            else:
                at = int(off[k]) + (7 if label.startswith("in_") else 0)
                assert covered[at:].all() and (label.endswith("2p32") or not covered[:at].any())


def test_alias_runs_by_hand():
    assert OC.alias_runs(5, 100) == []
    assert OC.alias_runs(OC.P32 + 83, 10) == [(83, 0, 10)]
    # crossing 2^31 at byte 4: sign extension alone moves the bytes from there on
    assert OC.alias_runs(OC.P31 - 4, 10) == [(-OC.P31, 4, 10)]
    # crossing 2^32 at byte 4: both extensions move the bytes from there on, sign extension those in front as well
    assert OC.alias_runs(OC.P32 - 4, 10) == [(-4, 0, 4), (0, 4, 10)]


@pytest.mark.parametrize("name", OC.NAMES)
def test_decoy_differs_from_the_batch_on_half_of_the_reads(name):
    """By the oracle alone: under the batch's own offsets the decoy's verdicts differ from the batch's on at least half of the
    reads, so reads fetched from an alias window cannot come out right by accident."""
    obj = OC.get(name)
    oc = H.orc.OracleClassifier(obj.config(), nthreads=NTHREADS, want_pass=False)
    for which in ("main", "edge"):
        seq, off, _ = obj.batch(which)
        dec = OC.decoy(name, off)
        assert dec.shape == seq.shape and dec.dtype == np.uint8
        differ = OC.verdicts_differ(oc.classify(seq, off), oc.classify(dec, off))
        assert differ.mean() >= 0.5, f"{name} {which}: the decoy differs on {differ.mean():.2f} of the reads"


@pytest.mark.parametrize("name", OC.HOSTILE_NAMES)
def test_planted_ends_would_show_a_leak(name):
    """By the oracle alone: every planted end answers differently (verdict or pass_score) once the read is extended by the c
    bytes that lie just outside the batch; the surroundings are what hostile() says; every variant has a planted end."""
    obj = OC.get(name)
    oc = H.orc.OracleClassifier(obj.config(), nthreads=NTHREADS, want_pass=True)
    bcs = OC._plain_barcodes(obj)
    for variant in OC.hostile_variants(name):
        for c in OC.PLANT_CUTS:
            seq, off, before, after, plants = OC.hostile(name, variant, c)
            n = len(off) - 1
            assert len(before) == len(after) == OC.SURROUND and off[-1] == len(seq)
            assert before[-c:].tobytes().decode() == bcs[1][:c] and after[:c].tobytes().decode() == bcs[2][-c:]
            assert bcs[0] * 8 in before[:-c].tobytes().decode() and bcs[0] * 8 in after[c:].tobytes().decode()
            assert plants, (name, variant)
            lens = np.diff(off)
            assert (lens[0] == 0) == (variant in ("first_empty", "both_empty")) and (lens[-1] == 0) == (variant in ("last_empty", "both_empty"))
            assert n == {"one_read": 1, "tile": OC.tile_reads(name), "tile_plus1": OC.tile_reads(name) + 1}.get(variant, n)
            for plant in plants:
                alone, extended = OC.plant_pair(seq, off, before, after, plant, c)
                assert len(extended) == len(alone) + c
                a = oc.classify(alone, np.array([0, len(alone)], dtype=np.int64))
                e = oc.classify(extended, np.array([0, len(extended)], dtype=np.int64))
                seen = bool(OC.verdicts_differ(a, e)[0]) or a["pass_score"].view(np.uint64).tolist() != e["pass_score"].view(np.uint64).tolist()
                assert seen, f"{name} {variant} c={c} {plant}: a leak of the outside bytes would not be seen"
    # both ends are planted wherever the config looks at the whole read
    if not hasattr(obj, "window"):
        assert len(OC.hostile(name, "full", 1)[4]) == 2


def test_host_route_shapes():
    """The host routes' batches lie on the intended side of the 2 MiB of the staged route (bdx_classify_host) and far below the
    96 MiB of the pipelined one."""
    seq, off, _ = OC.get(OC.HEADLINE).batch("main")
    assert len(seq) + 8 * len(off) <= 2 << 20
    seq, off = OC.plain_route_batch()
    assert (2 << 20) < len(seq) + 8 * len(off) < (96 << 20) and len(off) == 20002
    cfg, seq, off = OC.window_route_case()
    assert len(seq) >= 512 * (len(off) - 1) and len(seq) + 8 * len(off) > (2 << 20)
