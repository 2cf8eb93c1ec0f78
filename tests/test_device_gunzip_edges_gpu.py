"""Device gunzip (csrc/bdx_inflate.hip) on the MI355X on streams zlib's encoder never writes: the members of
tests/inflate_edge_cases.py — 15-bit codes and the deepest sub-tables, code-length runs across the two alphabets,
HLIT / HDIST / HCLEN at their ends, blocks without a distance code, headers at every bit offset, token groups of 127, 128
and 129, the largest group, libdeflate's members — good ones and refused ones, and workgroups steered to decode tables
of every shape after one another.  What only the device has is what is under test: the parallel table fill, the parallel
placing of bytes an earlier group stored, the unaligned 8-byte refill next to the body's end and InfShared reused by a
persistent workgroup.  The verdicts come from zlib and from the decoder's plain C++ build (test_device_gunzip_edges_cpu.py,
and under ASan / UBSan in test_device_gunzip_sanitize.py), never from the device."""
import pytest

import inflate_cases as IC
import inflate_edge_cases as EC
import test_device_gunzip_gpu as G
from test_device_gunzip_gpu import _classifier, _inflate, _need_gpu, hc  # noqa: F401 - fixtures

pytestmark = pytest.mark.gpu

GOOD, BAD = EC.good_edge_members(), EC.bad_edge_members()


def _check(members, rc, status, slots, intact, err, want=None):
    """slots, statuses and canaries of one call against zlib's bytes and the expected statuses (0 for a good member)"""
    want = [0 if m.plain is not None else None for m in members] if want is None else want
    assert intact, "a byte outside the slots was written"
    assert status.tolist() == want, [(m.name, s, w) for m, s, w in zip(members, status.tolist(), want) if s != w][:10]
    for m, s in zip(members, slots):
        assert m.plain is None or s == m.plain, m.name
    assert (rc == 0) == (not any(want)), err


def test_every_good_edge_member_in_one_call(hc, monkeypatch):
    members = list(GOOD)
    assert len(members) >= 70
    res = _inflate(hc, members)
    _check(members, *res)
    monkeypatch.setattr(G, "LEAD", 0)  # the compressed input at the start of its tensor: other alignments of every 8-byte load
    res0 = _inflate(hc, members)
    _check(members, *res0)
    assert res0[2] == res[2]


def test_bad_edge_members_among_good_ones(hc):
    """Every bad member has passed the decoder's plain C++ build under ASan / UBSan (test_device_gunzip_sanitize.py): it is
    refused without a byte read outside it or written outside its slot.  Here the device gives that build's status, which
    is the one the fault has in bdx_inflate_core.h's table."""
    decode = IC.host_decoder()
    members, want = [], []
    for k, (m, st) in enumerate(BAD):
        members += [GOOD[(5 * k) % len(GOOD)], m]
        want += [0, st]
        assert decode(m.comp, m.plen, fresh=True)[0] == st, m.name
    rc, status, slots, intact, err = _inflate(hc, members)
    _check(members, rc, status, slots, intact, err, want)
    assert "member 1 " in err and IC.STATUS[want[1]] in err
    _check(list(GOOD), *_inflate(hc, list(GOOD)))  # the context is fine afterwards


def test_workgroups_steered_through_tables_of_every_shape(monkeypatch):
    """BDX_CU_COUNT=1: a grid of 16 workgroups, so members m and m + 16 share a workgroup and its InfShared.  Each workgroup
    decodes in turn a member with the deepest tables, a shallow one whose codes sit where the deep one had links, a refused
    one, a stored-only one and a libdeflate member."""
    monkeypatch.setenv("BDX_CU_COUNT", "1")
    grid = 16
    by = {m.name: m for m in GOOD}
    deep = [m for m in GOOD if m.name in ("deep_tables", "ll_depth_15", "d_depth_15", "ll_subtables_of_four_sizes", "nl_286_nd_30_hclen_19",
                                          "every_cl_symbol_cl_lengths_to_7", "dynamic_200_code_sets")]
    shallow = [by["shallow_probe"], by["ll_depth_9"], by["d_depth_6"], by["only_eob_one_bit_code_final"], by["no_distance_code"],
               by["one_distance_code_of_one_bit"]]
    stored = [by["stored_len_65535"], by["stored_3000_empty_then_text"]] + [m for m in IC.good_members() if m.name.startswith("random_")]
    fixtures = [m for m in GOOD if m.name.startswith("libdeflate_")]
    assert len(deep) == 7 and len(stored) == 5 and len(fixtures) >= 14
    rows = [deep, shallow, [m for m, _ in BAD], stored, fixtures]
    members = [row[(w + r) % len(row)] for r, row in enumerate(rows) for w in range(grid)]
    for w in range(grid):  # behind the member with the fullest tables, the one whose codes are proven to sit where it had links
        if members[w].name == "deep_tables":
            members[grid + w] = by["shallow_probe"]
    assert sum(a.name == "deep_tables" and b.name == "shallow_probe" for a, b in zip(members[:grid], members[grid:])) >= 2
    status_of = {m.name: st for m, st in BAD}
    want = [status_of.get(m.name, 0) for m in members]
    assert len(members) == 5 * grid > 3 * grid and sum(bool(w) for w in want) == grid
    steered = _classifier()  # (its grid: min(members, 16 workgroups per compute unit x 1 unit))
    try:
        first = _inflate(steered, members)
        _check(members, *first, want=want)
        second = _inflate(steered, members)
        _check(members, *second, want=want)
        ok = [k for k, w in enumerate(want) if not w]
        assert [second[2][k] for k in ok] == [first[2][k] for k in ok]
    finally:
        steered.close()


def test_random_dynamic_blocks_on_the_device(hc):
    """the first 300 cases of the seeded generator: their bytes are zlib's, fixed when the list was built"""
    members, discarded = EC.random_members()
    assert discarded == ()
    members = list(members[:300])
    _check(members, *_inflate(hc, members))
