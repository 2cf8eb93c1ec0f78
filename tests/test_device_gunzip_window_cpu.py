"""The windowed stream inflate without a GPU: csrc/bdx_inflate_window_core.h as plain C++ (tests/inflate_window_host.cpp),
with zlib as the arbiter.  Every cut of the small files and of the small good and bad members; cuts at the edges the
format has, derived from the files' bytes; matches whose source lies in the windows before; a member over hundreds of
windows held to its trailer; no progress, BDX_E_SPACE and the dead object; the seeded corpus under random window
schedules; and the same with every workgroup starting from a filled state on grids of 1 and 16.
The module takes about 110 s on one core (the stream inflate's fuzz module: 95 s); half of it is the corpus under its two
schedules and the slice at nine launch settings, a quarter every cut of the small files."""
import numpy as np
import pytest

import inflate_cases as IC
import inflate_edge_cases as EC
import inflate_stream_cases as SC
import inflate_stream_fuzz as FZ
import inflate_window_cases as WC

FILLS, GRIDS = (0x00, 0xFF, 0xA5), (1, 16, 0)
REFUSED_CAP = 1 << 20  # what a refused file is given to get to its fault
SMALL = 1500


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    h = WC.Host(tmp_path_factory.mktemp("infw_host"))
    yield h
    h.set_launch(-1, 0)


def _cap(want):
    return len(want) if want is not None else REFUSED_CAP


def _derived():
    return dict((c.name, (c, plain)) for c, plain in SC.derived_cases())


def test_the_chain_keeps_the_lds_bound(host):
    assert host.shared_bytes <= 20 * 1024


# ---- every cut ----
def _every_cut_files():
    files = list(SC.small_files()) + [(n, d) for n, d in SC.arbiter_cases() if len(d) <= SMALL]
    assert len(files) > 100 and any(SC.arbiter(d) is None for _, d in files) and any(SC.arbiter(d) is not None for _, d in files)
    return files


def test_every_cut_gets_zlibs_verdict(host):
    """[0, c) with last = 0, then what is left with last = 1 (a window without progress is offered again, longer)"""
    cuts = 0
    for name, data in _every_cut_files():
        want = SC.arbiter(data)
        for c in range(len(data) + 1):
            rc, got, member, at, wins = host.run(data, [c], 64, _cap(want))
            assert WC.verdict_ok(want, rc, got, member, at, len(data)), (name, c, rc, member, at)
            assert wins >= 2 or c >= len(data) or c == 0 or rc != 0, (name, c, wins)
            cuts += 1
    assert cuts > 50000


def test_a_single_bad_member_is_refused_as_the_whole_file_build_refuses_it(host):
    """status, member and the compressed byte, at every cut"""
    alone = {m.name for m in IC.bad_members()} | {m.name for m, _ in EC.bad_edge_members()}
    seen = 0
    for name, data in SC.arbiter_cases():
        if name not in alone or len(data) > SMALL:
            continue
        assert SC.arbiter(data) is None, name
        ref = host.whole(data, 64, REFUSED_CAP)
        assert 1 <= ref[0] <= 11, (name, ref)
        for c in range(len(data) + 1):
            rc, _, member, at, _ = host.run(data, [c], 64, REFUSED_CAP)
            assert (rc, member, at) == ref, (name, c, (rc, member, at), ref)
        seen += 1
    assert seen >= 20, seen


# ---- the named edges ----
EDGES = ("on a block's first bit", "on a block's last bit", "inside a dynamic header", "inside LEN/NLEN", "inside the trailer",
         "right behind the trailer", "between two members", "inside the next header")


def test_cuts_at_the_edges_of_the_format(host):
    reached = {}
    for name, (case, plain) in _derived().items():
        if len(case.data) > 300000:
            continue
        for edge, cuts in WC.edge_cuts(case).items():
            cuts = sorted(set(cuts))
            if len(cuts) > 64:  # (a long file: a spread of them)
                cuts = cuts[:: len(cuts) // 64 + 1]
            for c in cuts:
                rc, got, _, _, _ = host.run(case.data, [c], 64, len(plain))
                assert rc == 0 and got == plain, (name, edge, c, rc)
            reached[edge] = reached.get(edge, 0) + len(cuts)
    for edge in EDGES:
        assert reached.get(edge, 0) >= 8, (edge, reached)
    assert reached["inside the trailer"] >= 8 * 8


def test_the_trailer_cut_at_each_of_its_bytes_carries_the_crc_to_the_next_window(host):
    case, plain = _derived()["every_block_type"]
    off, body, _ = case.members[-1]
    end = off + len(body)
    assert end + 8 == len(case.data)
    for i in range(0, 8):
        w = host.open()
        rc, used, plen, got, _, _, clean = w.feed(case.data[:end + i], 0, 64, len(plain))
        st = w.state()
        assert rc == 0 and got == plain and clean and st["where"] == WC.TRAILER and st["member_n"] == len(plain), (i, rc, st)
        assert used in (end - 1, end) and st["member"] == 0
        rc, used2, plen, got, _, _, _ = w.feed(case.data[used:], 1, 64, 0)
        assert rc == 0 and plen == 0 and used2 == len(case.data) - used and w.state()["member"] == 1
        w.close()
        bad = bytearray(case.data)
        bad[end + 5] ^= 0x10  # ISIZE
        w = host.open()
        rc, used, _, _, _, _, _ = w.feed(bytes(bad[:end + i]), 0, 64, len(plain))
        assert rc == 0
        rc, _, _, _, member, at, _ = w.feed(bytes(bad[used:]), 1, 64, 0)
        assert (rc, member, at) == (11, 0, 0)
        w.close()


def test_a_cut_inside_fname_and_right_behind_a_trailer(host):
    case, plain = _derived()["every_block_type"]
    data, cuts = WC.with_fname(case)
    assert SC.arbiter(data) == plain and len(cuts) >= 12
    for c in cuts:
        w = host.open()
        rc, used, plen, _, _, _, _ = w.feed(data[:c], 0, 64, 0)
        assert (rc, used, plen) == (0, 0, 0) and w.state()["where"] == WC.BETWEEN, c  # the header runs off: not a refusal
        rc, used, plen, got, _, _, _ = w.feed(data, 1, 64, len(plain))
        assert rc == 0 and got == plain and used == len(data)
        w.close()
    two = case.data + data  # a second member with a name: cut right behind the first trailer, and inside the second name
    for c in [len(case.data), len(case.data) + 1, len(case.data) + 2] + [len(case.data) + k for k in cuts]:
        w = host.open()
        rc, used, plen, got, _, _, _ = w.feed(two[:c], 0, 64, len(plain))
        assert rc == 0 and got == plain and used == len(case.data) and w.state()["where"] == WC.BETWEEN, c
        assert w.state()["member"] == 1
        rc, used, plen, got, _, _, _ = w.feed(two[len(case.data):], 1, 64, len(plain))
        assert rc == 0 and got == plain
        w.close()


def test_trailing_bytes_are_ignored_wherever_the_cut_falls(host):
    case, plain = _derived()["every_block_type"]
    for tail in (b"\0" * 9, b"\x1f", b"junk!", b"\x1fjunk and more of it, longer than a header" * 3):
        data = case.data + tail
        assert SC.arbiter(data) == plain
        for c in range(len(case.data) - 2, len(data) + 1):
            rc, got, _, _, _ = host.run(data, [c], 64, len(plain))
            assert rc == 0 and got == plain, (tail, c, rc)
    w = host.open()  # behind the first byte that is no header, nothing is looked at again
    rc, used, _, got, _, _, _ = w.feed(case.data + b"ju", 0, 64, len(plain))
    assert rc == 0 and got == plain and used == len(case.data) + 2 and w.state()["where"] == WC.IGNORE
    rc, used, plen, _, _, _, _ = w.feed(SC.HDR + b"\xff" * 40, 0, 64, 0)
    assert (rc, used, plen) == (0, 50, 0)
    rc, used, plen, _, _, _, _ = w.feed(b"", 1, 64, 0)
    assert (rc, used, plen) == (0, 0, 0)
    w.close()


def test_the_last_window(host):
    case, plain = _derived()["every_block_type"]
    w = host.open()  # zero bytes between members: a good end of the file
    assert w.feed(case.data, 0, 64, len(plain))[:3] == (0, len(case.data), len(plain))
    assert w.state()["where"] == WC.BETWEEN
    assert w.feed(b"", 1, 64, 0)[:3] == (0, 0, 0)
    w.close()
    w = host.open()  # ending inside a member: input exhausted, at the byte the next block begins in
    cut = len(case.data) - 30
    rc, used, plen, _, _, _, _ = w.feed(case.data[:cut], 0, 64, len(plain))
    assert rc == 0 and 0 < used <= cut and w.state()["where"] == WC.INSIDE
    rc, _, _, _, member, at, _ = w.feed(b"", 1, 64, 0)
    assert (rc, member, at) == (9, 0, used)
    assert w.feed(case.data[used:], 1, 64, len(plain))[0] == WC.STATE  # dead, whatever it is given
    assert w.feed(b"", 0, 64, 0)[0] == WC.STATE
    w.close()
    w = host.open()  # an empty file is no gzip file
    rc, _, _, _, member, at, _ = w.feed(b"", 1, 64, 0)
    assert (rc, member, at) == (1, 0, 0)
    w.close()


def test_between_the_members_of_many_members(host):
    g = FZ.many_members()
    ends = [off + len(body) + 8 for off, body, _ in g.case.members]
    for chunk in (64, 4096):
        for cuts in (ends[::37], [e + 1 for e in ends[5::41]], [e - 3 for e in ends[3::43]], [e + 7 for e in ends[1::47]]):
            w = host.open()
            rc, text, log, _, _ = WC.feed_cuts(w, g.data, cuts, chunk, len(g.plain))
            assert rc == 0 and text == g.plain and len(log) >= 20, (chunk, rc, len(log))
            assert w.state()["member"] == 1100
            w.close()


# ---- the history ----
def test_matches_whose_source_lies_in_the_windows_before(host):
    """length 258 at distance 32 768 and distance 1 into the window before; distance 32 768 again with the source three
    windows back, the history shifted through windows of 100, 1 and 0 plain bytes"""
    data, plain, marks = WC.history_file()
    cuts, lens = WC.history_cuts()
    for chunk in (64, 4096):
        w = host.open()
        rc, text, log, _, _ = WC.feed_cuts(w, data, cuts, chunk, len(plain))
        assert rc == 0 and text == plain
        assert [x[3] for x in log] == lens, log
        assert all(x[2] > 0 for x in log)  # (the window of 0 plain bytes consumes its empty stored block)
        w.close()
    for c in range(marks["far"] - 2, marks["tail"] + 3):
        rc, got, _, _, _ = host.run(data, [c], 64, len(plain))
        assert rc == 0 and got == plain, c


def test_a_distance_beyond_the_members_first_byte_is_refused_from_the_carried_size(host):
    for dist, want_rc in ((300, 0), (301, 6)):
        t = SC.Stream()
        t.stored(t.text(300))
        cut = t.byte()
        EC.fixed_block(t.w, [(10, dist)], True)  # (written past Stream.fixed, which would not build the one too far)
        body = t.w.bytes()
        plain = t.plain + (t.plain[:10] if dist == 300 else b"\0" * 10)
        data = SC.HDR + body + IC.trailer(plain)
        assert (SC.arbiter(data) is None) == (want_rc != 0)
        w = host.open()
        rc, used, plen, _, _, _, _ = w.feed(data[:cut], 0, 64, 400)
        assert rc == 0 and plen == 300 and w.state()["member_n"] == 300
        rc, _, _, got, member, at, _ = w.feed(data[used:], 1, 64, 400)
        assert rc == want_rc and (rc or got == plain[300:]), (dist, rc)
        if rc:
            assert (member, at) == (0, 0)
        w.close()


# ---- a member over many windows ----
def test_a_member_over_hundreds_of_windows_is_held_to_its_trailer(host):
    g = FZ.memlevel1(6)
    sizes = [1024] * (len(g.data) // 1024 + 1)
    rc, got, _, _, wins = host.run(g.data, sizes, 64, len(g.plain))
    assert rc == 0 and got == g.plain and wins >= 5 and wins >= len(g.data) // 1100
    for at_byte, why in ((-8, 10), (-4, 11), (len(g.data) // 2, None)):
        bad = bytearray(g.data)
        bad[at_byte] ^= 0x40
        bad = bytes(bad)
        assert SC.arbiter(bad) is None
        rc, _, member, at, wins = host.run(bad, sizes, 64, REFUSED_CAP)
        assert 1 <= rc <= 11 and member == 0 and wins >= 5, (at_byte, rc)
        if why:
            assert (rc, at) == (why, 0)  # known at its end only: the windows before gave their text


def test_a_window_smaller_than_a_block_makes_no_progress(host):
    case, plain = _derived()["zlib_level_6"]
    first = SC.file_blocks(case)[0][0]
    assert first.btype == 2 and first.end // 8 > 4096
    w = host.open()
    for n in (0, 1, 9, 11, 17):  # (a header is taken with the 8 bytes a trailer needs behind it)
        assert w.feed(case.data[:n], 0, 64, 0)[:3] == (0, 0, 0), n
        assert w.state() == dict(where=WC.BETWEEN, bit=0, member=0, member_n=0, comp_abs=0, plain_abs=0)
    assert w.feed(case.data[:64], 0, 64, 0)[:3] == (0, 10, 0)  # the header alone: consumed, no text yet
    st = w.state()
    assert st == dict(where=WC.INSIDE, bit=0, member=0, member_n=0, comp_abs=10, plain_abs=0)
    for n in (0, 1, 64, 1024, 4096):
        assert w.feed(case.data[10:10 + n], 0, 64, 0)[:3] == (0, 0, 0), n
        assert w.state() == st
    n = first.end // 8 + 1
    rc, used, plen, got, _, _, _ = w.feed(case.data[10:n], 0, 64, len(plain))
    used += 10
    assert rc == 0 and used == first.end // 8 and plen == first.nbytes and got == plain[:plen]
    st = w.state()
    assert (st["where"], st["bit"], st["comp_abs"], st["plain_abs"]) == (WC.INSIDE, first.end % 8, used, plen)
    assert w.feed(case.data[used:used + 5], 0, 64, 0)[:3] == (0, 0, 0)  # inside a member too
    assert w.state() == st
    w.close()
    rc, got, _, _, wins = host.run(case.data, [100] * 50, 0, len(plain))  # doubled until a block fits, again and again
    blocks = SC.file_blocks(case)[0]
    doublings = sum(int(np.log2((b.end - b.bit) // 8 / 100)) for b in blocks)  # 100 bytes, 200, ... hold none of a block
    assert doublings >= 20 and rc == 0 and got == plain and wins >= doublings, (wins, doublings)


def test_space_then_the_same_call_with_the_room_it_asked_for(host):
    data, plain, marks = WC.history_file()
    a, b = marks["far"], marks["far2"]
    ref = host.open()
    assert ref.feed(data[:a], 0, 64, 40000)[:3] == (0, a, 40000)
    want = ref.feed(data[a:b + 1], 0, 64, 1000)
    assert want[0] == 0 and want[2] == 263 + 100 + 1
    w = host.open()
    assert w.feed(data[:a], 0, 64, 40000)[:3] == (0, a, 40000)
    before = w.state()
    for cap in (0, 1, want[2] - 1):
        rc, used, plen, _, _, _, clean = w.feed(data[a:b + 1], 0, 64, cap)
        assert (rc, used, plen) == (WC.SPACE, 0, want[2]) and clean and w.state() == before, cap
    assert w.feed(data[a:b + 1], 0, 64, want[2]) == want and w.state() == ref.state()
    rest_a, rest_b = ref.feed(data[a + want[1]:], 1, 64, 1000), w.feed(data[a + want[1]:], 1, 64, 1000)
    assert rest_a == rest_b and rest_a[0] == 0 and plain.endswith(rest_a[3])
    ref.close()
    w.close()


# ---- the corpus under seeded window schedules ----
def _under_schedules(host, name, data, want, k, chunks, seg_room=4):
    out = []
    for j, chunk in enumerate(chunks):
        sizes = WC.schedule(WC.SEED + 2 * k + j, len(data))
        rc, got, member, at, wins = host.run(data, sizes, chunk, _cap(want), seg_room)
        if want is None and rc == WC.SPACE:
            rc, got, member, at, wins = host.run(data, sizes, chunk, 1 << 26, seg_room)
        assert WC.verdict_ok(want, rc, got, member, at, len(data)), (name, chunk, sizes[:8], rc, member, at)
        out.append((rc, got, member, at, wins))
    return out


def test_good_files_under_two_schedules_each(host):
    files = FZ.good_files() + FZ.named()
    assert len(files) >= 300
    windows = 0
    for k, g in enumerate(files):
        windows += sum(r[4] for r in _under_schedules(host, g.name, g.data, g.plain, k, (64, FZ.ODD[k % len(FZ.ODD)])))
    assert windows > 4 * len(files)


def test_mutants_under_two_schedules_each(host):
    ms = FZ.mutants()
    assert len(ms) >= 1500
    accepted = sum(m.want is not None for m in ms)
    assert 0.03 * len(ms) <= accepted <= 0.97 * len(ms), accepted  # (zlib alone says so)
    for k, m in enumerate(ms):
        _under_schedules(host, m.name, m.data, m.want, 10000 + k, (64, FZ.ODD[k % len(FZ.ODD)]))


# ---- how the device starts a workgroup ----
def _slice(host):
    seen = []
    for k, (name, data, want, _) in enumerate(FZ.slice_files()):
        seen += _under_schedules(host, name, data, want, 20000 + k, (64,))
    data, plain, _ = WC.history_file()
    cuts, _ = WC.history_cuts()
    w = host.open()
    seen.append(WC.feed_cuts(w, data, cuts, 64, len(plain)))
    w.close()
    g = FZ.many_members()
    seen.append(host.run(g.data, [4096] * 40, 0, len(g.plain), seg_room=1024))
    assert len(seen) >= 402
    return seen


@pytest.fixture(scope="module")
def baseline(host):
    host.set_launch(-1, 0)
    return _slice(host)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("fill", FILLS, ids=["fill_%02x" % f for f in FILLS])
def test_results_do_not_depend_on_what_the_lds_held_or_on_the_grid(host, baseline, fill, grid):
    host.set_launch(fill, grid)
    try:
        seen = _slice(host)
    finally:
        host.set_launch(-1, 0)
    assert len(seen) == len(baseline)
    for k, (a, b) in enumerate(zip(seen, baseline)):
        assert a == b, (k, a[0], b[0])


# ---- the keyword and the entries of the library, without a device ----
@pytest.mark.parametrize("kw, needle", [
    (dict(_gunzip="device-window", _io="native"), "_io='device'"),
    (dict(_gunzip="device-window"), "_io='device'"),
    (dict(_gunzip="device-window", _io="device", _gunzip_window=1023), "_gunzip_window must be an int of 1024"),
    (dict(_gunzip="device-window", _io="device", _gunzip_window=(1 << 28) + 1), "_gunzip_window must be"),
    (dict(_gunzip="device-window", _io="device", _gunzip_window=4096.0), "_gunzip_window must be"),
    (dict(_gunzip="device-window", _io="device", _gunzip_window="4096"), "_gunzip_window must be"),
    (dict(_gunzip="device-window", _io="device", _gunzip_window=True), "_gunzip_window must be"),
    (dict(_gunzip="device-stream", _io="device", _gunzip_window=4096), "_gunzip='device-window'"),
    (dict(_gunzip="window"), "^_gunzip must be .*'device-stream' or 'device-window'"),
])
def test_the_keyword_is_validated_before_the_output_directory_exists(tmp_path, kw, needle):
    import helpers as H

    out = tmp_path / "never_made"
    with pytest.raises(ValueError, match=needle):
        H.bdx.execute_demultiplexing(str(tmp_path / "no.fastq.gz"), str(tmp_path / "no.csv"), str(out), **kw)
    assert not out.exists()


def test_a_gz_input_that_is_no_gzip_file_is_refused_before_the_output_directory(tmp_path):
    import helpers as H

    fq = tmp_path / "plain_inside.fastq.gz"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    out = tmp_path / "never_made"
    with pytest.raises(ValueError, match=r"device-window.*plain_inside\.fastq\.gz.*gzip header"):
        H.bdx.execute_demultiplexing(str(fq), str(tmp_path / "no.csv"), str(out), _io="device", _gunzip="device-window", _gunzip_window=4096)
    assert not out.exists()


def test_the_entries_check_their_arguments_without_a_device():
    import ctypes as C

    import helpers as H
    from biodemux_jl_amd import deviceio

    lib = H.bdx.load_library()
    w, used, plen = C.c_void_p(), C.c_int64(7), C.c_int64(7)
    assert lib.bdx_fq_inflate_window_open(None, 0, C.byref(w)) == -1 and not w.value
    assert b"ctx is NULL" in lib.bdx_last_error(None)
    assert lib.bdx_fq_inflate_window_feed(None, None, 0, 1, None, 0, C.byref(used), C.byref(plen), None) == -1
    assert lib.bdx_fq_inflate_window_close(None) == 0
    assert deviceio.WINDOW_MIN == 1024 and deviceio.WINDOW_MAX == 1 << 28 and deviceio.window_bytes(deviceio.WINDOW_BYTES) == deviceio.WINDOW_BYTES
