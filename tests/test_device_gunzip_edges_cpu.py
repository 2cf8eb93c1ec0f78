"""The device inflate's decoder (csrc/bdx_inflate_core.h as plain C++) on streams zlib's encoder never writes: the members
of tests/inflate_edge_cases.py.  Every member reaches the edge it is named for (read from its bytes), the host build gives
zlib's bytes for every good one and the status of its fault for every bad one, one shared state serves them all in any
order, and 1 500 seeded random dynamic blocks — none of which the writer may throw away — inflate to what zlib makes of
them.  tests/test_device_gunzip_edges_gpu.py holds the device to the same members."""
import gzip
import os

import numpy as np
import pytest

import helpers as H
import inflate_cases as IC
import inflate_edge_cases as EC

GOOD, BAD = EC.good_edge_members(), EC.bad_edge_members()


def _name(x):
    return x.name if hasattr(x, "name") else x[0].name


@pytest.fixture(scope="module")
def decode():
    return IC.host_decoder()


def test_the_lists_hold_every_kind_of_case():
    names = [m.name for m in GOOD]
    for prefix, least in (("ll_depth_", 4), ("d_depth_", 3), ("cl1", 4), ("cl_same", 1), ("only_eob", 2), ("overlap_lattice", 2),
                          ("literals_", 6), ("match_", 3), ("largest_group", 1), ("far_matches", 1), ("headers_at", 1), ("stored_", 2),
                          ("body_end_", 16), ("dynamic_200", 1), ("libdeflate_", 14), ("nl_", 2), ("every_cl", 1), ("deep_tables", 1),
                          ("shallow_probe", 1), ("no_distance", 1), ("one_distance", 1)):
        assert sum(n.startswith(prefix) for n in names) >= least, prefix
    by_status = {st: sum(s == st for _, s in BAD) for st in (1, 4, 5, 6, 7, 9)}
    assert by_status == {1: 1, 4: 14, 5: 6, 6: 1, 7: 3, 9: 8}
    assert all(m.plen <= IC.MEMBER_MAX for m in GOOD) and all(m.plen <= IC.MEMBER_MAX for m, _ in BAD)


@pytest.mark.parametrize("m", GOOD, ids=_name)
def test_member_reaches_the_edge_it_is_named_for(m):
    assert EC.predicate(m)


def test_edges_that_members_reach_together():
    for what, ok in EC.set_predicates().items():
        assert ok, what


@pytest.mark.parametrize("m", GOOD, ids=_name)
def test_good_edge_member_inflates_to_zlibs_bytes(decode, m):
    st, got = decode(m.comp, m.plen, fresh=True)  # (-1: a byte beside the slot was touched)
    assert st == 0, IC.STATUS.get(st, st)
    assert got == gzip.decompress(m.comp) == m.plain


@pytest.mark.parametrize("case", BAD, ids=_name)
def test_bad_edge_member_is_refused_for_its_fault(decode, case):
    m, want = case
    with pytest.raises(Exception):  # noqa: B017 - zlib.error, EOFError or gzip.BadGzipFile
        gzip.decompress(m.comp)
    st, _ = decode(m.comp, m.plen, fresh=True)
    assert st != -1, "a byte beside the slot was touched"
    assert st == want, (IC.STATUS.get(st, st), IC.STATUS[want])


def test_one_shared_state_for_the_edge_members(decode):
    """tables of every shape after one another in one InfShared, as a persistent workgroup has them"""
    members = list(GOOD) + [m for m, _ in BAD] + list(IC.good_members()[:6])
    alone = [decode(m.comp, m.plen, fresh=True) for m in members]
    for seed in (7, 8):
        decode(b"x", 0, fresh=True)
        for k in np.random.default_rng(seed).permutation(len(members)):
            st, got = decode(members[k].comp, members[k].plen)
            assert st == alone[k][0] and st != -1 and (st != 0 or got == alone[k][1]), members[k].name


def test_random_dynamic_blocks_are_held_to_zlib(decode):
    """zlib accepted every one of them, with the writer's own bytes, when the list was built: a discard is a writer bug"""
    members, discarded = EC.random_members()
    assert discarded == () and len(members) == 1500
    decode(b"x", 0, fresh=True)
    deep = crossed = 0
    for m in members:  # one state for all of them, in turn
        st, got = decode(m.comp, m.plen)
        assert st == 0 and got == m.plain, m.name
    for m in members[:300]:  # what the generator reaches, from the bytes of a sample
        B = EC.anatomy(m.comp)[0][-1]
        deep += B.ll_max > 12 or B.d_max > 12
        crossed += any(EC.crossing(B, s) for s in (16, 17, 18))
    assert deep > 30 and crossed > 30


def test_coverage_listing_is_the_one_committed(decode):
    lines = EC.listing(decode)
    with open(os.path.join(H.ROOT, "profiles", "inflate_case_coverage.txt")) as f:
        assert f.read().splitlines() == lines
    assert not any(line.endswith("WRONG") for line in lines)
