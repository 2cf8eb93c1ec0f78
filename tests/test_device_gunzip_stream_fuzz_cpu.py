"""The stream inflate (csrc/bdx_inflate_stream_core.h as plain C++, tests/inflate_stream_host.cpp) over the seeded corpus
of tests/inflate_stream_fuzz.py, with zlib as the arbiter: good files at five chunk sizes each, odd ones among them;
bit-flipped and truncated files, accepted exactly when zlib accepts them; the same runs with every workgroup starting
from an LDS full of some byte and a grid of 1 or 16 workgroups, which is how the device starts them; and with the
32-bit view rebased every 2^17 bytes instead of every 2^30."""
import functools

import pytest

import inflate_stream_cases as SC
import inflate_stream_fuzz as FZ

FILLS, GRIDS = (0x00, 0xFF, 0xA5), (1, 16, 0)
REFUSED_CAP = 70000  # what a refused file is given to get to its fault


@pytest.fixture(scope="module")
def inflate(tmp_path_factory):
    f = SC.build_host(tmp_path_factory.mktemp("infs_fuzz_host"))
    yield f
    f.set_launch(-1, 0)


@pytest.fixture(scope="module")
def inflate_small_rebase(tmp_path_factory):
    return SC.build_host(tmp_path_factory.mktemp("infs_fuzz_rebase"), flags=("-DINFS_REBASE=(1u<<17)",), name="libinfs_host_rebase17.so")


def _good(inflate, g, chunks=None):
    """a good file at its chunk sizes -> [(rc, text, plain_len, info)], each held to zlib's text"""
    out = []
    for chunk in chunks or g.chunks:
        rc, got, plen, info, _, _, clean = inflate(g.data, chunk, len(g.plain))
        assert rc == 0 and plen == len(g.plain) and got == g.plain and clean, (g.name, chunk, rc)
        assert info[2] + info[3] + info[4] == info[1] - 1, (g.name, chunk, info)
        out.append((rc, got, plen, info))
    return out


def _mutant(inflate, m, chunks=None):
    """-> [(rc, text, plain_len, member, at)]: accepted with zlib's bytes exactly when zlib accepts"""
    out = []
    for chunk in chunks or m.chunks:
        rc, got, plen, _, member, at, clean = inflate(m.data, chunk, len(m.want) if m.want is not None else REFUSED_CAP)
        if m.want is None:  # (a refused file may need more room than it was given: then its size is all it says)
            assert 1 <= rc <= 11 or (rc == SC.SPACE and plen > REFUSED_CAP), (m.name, chunk, rc)
            if rc == SC.SPACE:
                rc, got, plen, _, member, at, clean = inflate(m.data, chunk, plen)
            assert 1 <= rc <= 11 and 0 <= at <= len(m.data) and member >= 0 and clean, (m.name, chunk, rc, at, member)
        else:
            assert rc == 0 and got == m.want and clean, (m.name, chunk, rc)
        out.append((rc, got, plen if rc == 0 else None, member, at))
    return out


# ---- good files ----
def test_good_files_at_five_chunk_sizes_each(inflate):
    files = FZ.good_files() + FZ.named()
    assert len(files) >= 300
    sizes = set()
    for g in files:
        assert len(g.chunks) == 5 or g in FZ.named()
        sizes.update(g.chunks)
        _good(inflate, g)
    assert {64, 0} <= sizes and sizes & set(FZ.ODD) and any(c % 2 and c > 300 for c in sizes)


def test_counters_of_the_files_whose_blocks_are_known(inflate):
    files = FZ.known(FZ.good_files() + FZ.named())
    assert {g.name.split("_")[0] for g in files} == {"pigz", "blocks", "memlevel1", "many"}
    for g in files:
        for chunk, (_, _, _, info) in zip(g.chunks, _good(inflate, g)):
            assert info == SC.expected_info(g.case, chunk), (g.name, chunk)


def test_the_named_files_are_what_they_are_named_for():
    for level in (6, 1):
        g = FZ.memlevel1(level)
        blocks = SC.file_blocks(g.case)[0]
        assert len(blocks) > 200 and sum(b.btype == 2 for b in blocks) > 200, (g.name, len(blocks))
        assert len(SC.chain(g.case, 64)[0]) > 250 and len(SC.chain(g.case, 256)[0]) > 250
    g = FZ.many_members()
    assert len(g.case.members) == 1100 and len(g.data) < 1 << 17
    for chunk in (0, 4096):  # more segments than the first room: the chain runs twice
        segs, info = SC.chain(g.case, chunk)
        assert len(segs) > 2 * info[1] + 1024, (chunk, len(segs), info[1])
    segs, info = SC.chain(g.case, 64)
    assert len(segs) <= 2 * info[1] + 1024  # (and once here)


def test_many_members_with_the_first_room_of_the_device(inflate):
    g = FZ.many_members()
    for chunk in g.chunks:
        n_chunks = -(-len(g.data) // (chunk or SC.DEFAULT_CHUNK))
        rc, got, plen, info, _, _, clean = inflate(g.data, chunk, len(g.plain), seg_room=2 * n_chunks + 1024)
        assert rc == 0 and got == g.plain and clean and info == SC.expected_info(g.case, chunk), (chunk, rc)


# ---- mutants ----
def test_mutants_get_zlibs_verdict(inflate):
    ms = FZ.mutants()
    assert len(ms) >= 1500
    accepted = sum(m.want is not None for m in ms)
    assert 0.03 * len(ms) <= accepted <= 0.97 * len(ms), accepted  # (zlib alone says so)
    assert any("/cut" in m.name for m in ms) and any("/flip" in m.name for m in ms)
    for m in ms:
        assert m.chunks[0] == 64 and m.chunks[2] == 0 and 64 < m.chunks[1]
        _mutant(inflate, m)


# ---- how the device starts a workgroup ----
@functools.lru_cache(maxsize=1)
def _arbiter_verdicts():
    return tuple(SC.arbiter(data) for _, data in SC.arbiter_cases())


def _everything(inflate):
    """every derived case, every arbiter case and the fixed slice of the corpus -> all that a caller sees of them"""
    seen = []
    for case, plain in SC.derived_cases():
        for chunk in SC.CHUNKS:
            seen.append(inflate(case.data, chunk, len(plain))[:6])
            assert seen[-1][:3] == (0, plain, len(plain)), (case.name, chunk)
    for (name, data), want in zip(SC.arbiter_cases(), _arbiter_verdicts()):
        for chunk in (64, 0):
            seen.append(inflate(data, chunk, len(want) if want is not None else REFUSED_CAP)[:6])
            assert (seen[-1][0] == 0 and seen[-1][1] == want) if want is not None else 1 <= seen[-1][0] <= 11, (name, chunk)
    good, bad = FZ.fixed_slice()
    assert len(good) >= 100 and len(bad) >= 300
    for g in good:
        seen += _good(inflate, g, FZ.slice_chunks(g))
    for m in bad:
        seen += _mutant(inflate, m, (64,))
    return seen


@pytest.fixture(scope="module")
def baseline(inflate):
    inflate.set_launch(-1, 0)
    return _everything(inflate)


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("fill", FILLS, ids=["fill_%02x" % f for f in FILLS])
def test_results_do_not_depend_on_what_the_lds_held_or_on_the_grid(inflate, baseline, fill, grid):
    """rc, text, plain_len, info, member and at: identical to the run on one zeroed, carried state (and so zlib's)"""
    inflate.set_launch(fill, grid)
    try:
        seen = _everything(inflate)
    finally:
        inflate.set_launch(-1, 0)
    assert len(seen) == len(baseline)
    for k, (a, b) in enumerate(zip(seen, baseline)):
        assert a == b, (k, a[0], b[0])


def test_a_grid_of_16_gives_every_workgroup_a_second_item():
    for g in (FZ.memlevel1(6), FZ.memlevel1(1)):
        for chunk in g.chunks:
            segs, info = SC.chain(g.case, chunk)
            assert info[1] > 2 * 16 and len(segs) > 2 * 16, (g.name, chunk)


def test_the_named_files_with_filled_lds_and_small_grids(inflate):
    try:
        for fill in FILLS:
            for grid in GRIDS:
                inflate.set_launch(fill, grid)
                for g in FZ.named():
                    for chunk, (_, _, _, info) in zip(g.chunks, _good(inflate, g)):
                        assert info == SC.expected_info(g.case, chunk), (g.name, chunk, fill, grid)
    finally:
        inflate.set_launch(-1, 0)


# ---- the rebased view ----
def test_rebase_every_128_kib_changes_nothing(inflate_small_rebase, baseline):
    seen = _everything(inflate_small_rebase)
    assert len(seen) == len(baseline)
    for k, (a, b) in enumerate(zip(seen, baseline)):
        assert a == b, (k, a[0], b[0])
    # read from the files: a segment of more than 2^17 plain bytes (lim, plen clipped; the CRC in pieces), a file of more
    # than 2^17 compressed bytes (the limit of a view clipped)
    cases = dict((c.name, c) for c, _ in SC.derived_cases())
    assert max(g.n for g in SC.chain(cases["zlib_level_6"], 0)[0]) > 1 << 17
    assert len(cases["zlib_random"].data) > 1 << 17


# ---- what the corpus reaches, read from the files' bytes ----
def test_the_corpus_reaches_what_it_is_written_for():
    flush_marker = False
    for g in FZ.known(FZ.good_files()):
        if not g.name.startswith("pigz"):
            continue
        for blocks in SC.file_blocks(g.case):
            for a, b in zip(blocks, blocks[1:]):
                flush_marker |= a.btype == 0 and a.nbytes == 0 and b.btype == 2  # a sync flush: an empty stored block
    assert flush_marker
    assert max(SC.expected_info(g.case, c)[2] for g in FZ.named() for c in g.chunks) > 200  # confirmed guesses
    seen, discarded = set(), 0
    for g in FZ.known(FZ.good_files()):
        if g.name.startswith("blocks"):
            for chunk in g.chunks:
                seen |= SC.features(g.case, chunk)
                discarded += SC.expected_info(g.case, chunk)[3] > 0
    for what in ("distance 32768 into an earlier segment", "source straddles 3 earlier segments", "candidate discarded",
                 "block start on a chunk's first bit", "block start on a chunk's last bit", "segment of 0 bytes"):
        assert what in seen, what
    assert discarded > 0
