"""The stream inflate for ordinary .gz input without a GPU: csrc/bdx_inflate_stream_core.h as plain C++
(tests/inflate_stream_host.cpp) over every case of tests/inflate_stream_cases.py at chunk sizes 64, 4096 and the default,
with the `info` counters held to what the cases module derives from the files' bytes; the keyword, the entries of the
library and their argument checks."""
import ctypes as C
import os

import pytest

import helpers as H
import inflate_stream_cases as SC
from biodemux_jl_amd import hipabi

BDX_E_INVALID = -1


# ---- keyword validation: before any file or device is touched ----
@pytest.mark.parametrize("kw, needle", [
    (dict(_gunzip="device-stream", _io="native"), "_io='device'"),
    (dict(_gunzip="device-stream", _io="auto"), "_io='device'"),
    (dict(_gunzip="device-stream"), "_io='device'"),
    (dict(_gunzip="stream"), "^_gunzip must be"),
])
def test_gunzip_stream_keyword_is_validated_first(tmp_path, kw, needle):
    out = tmp_path / "never_made"
    with pytest.raises(ValueError, match=needle):
        H.bdx.execute_demultiplexing(str(tmp_path / "no.fastq.gz"), str(tmp_path / "no.csv"), str(out), **kw)
    assert not out.exists()


def test_a_gz_input_that_is_no_gzip_file_is_refused_before_the_output_directory(tmp_path):
    fq = tmp_path / "plain_inside.fastq.gz"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    out = tmp_path / "never_made"
    with pytest.raises(ValueError, match=r"plain_inside\.fastq\.gz.*gzip header"):
        H.bdx.execute_demultiplexing(str(fq), str(tmp_path / "no.csv"), str(out), _io="device", _gunzip="device-stream")
    assert not out.exists()


# ---- the entries of the library ----
def test_new_entries_are_part_of_the_abi():
    lib = H.bdx.load_library()
    header = open(os.path.join(H.ROOT, "include", "biodemux_hip.h")).read()
    for name in ("bdx_fq_inflate_stream_chunk", "bdx_fq_inflate_stream_device"):
        assert name in hipabi.ABI_SYMBOLS and hasattr(lib, name) and name + "(" in header
    assert "#define BDX_E_SPACE (-5)" in header
    assert 64 <= lib.bdx_fq_inflate_stream_chunk() <= 1 << 24  # without a context, without a device
    assert lib.bdx_fq_inflate_member_max() == 65536  # (the tagged decoder keeps its limit)


def test_arguments_are_checked_before_anything_else():
    """without a device: a wrong argument is named before the missing context is"""
    lib = H.bdx.load_library()
    plen = C.c_int64(-1)
    for args, needle in [
        ((None, -1, 0, None, 0, C.byref(plen), None), "negative"),
        ((None, 100, 0, None, -1, C.byref(plen), None), "negative"),
        ((None, 100, 63, None, 0, C.byref(plen), None), "chunk_bytes"),
        ((None, 100, (1 << 24) + 1, None, 0, C.byref(plen), None), "chunk_bytes"),
        ((None, 100, -64, None, 0, C.byref(plen), None), "chunk_bytes"),
        ((None, 100, 64, None, 0, None, None), "plain_len is NULL"),
        ((None, 100, 64, None, 0, C.byref(plen), None), "ctx is NULL"),
        ((None, 100, 1 << 24, None, 0, C.byref(plen), None), "ctx is NULL"),
    ]:
        rc = lib.bdx_fq_inflate_stream_device(None, *args)
        assert rc == BDX_E_INVALID and needle in lib.bdx_last_error(None).decode(), (args, lib.bdx_last_error(None))


# ---- the core as plain C++ ----
@pytest.fixture(scope="module")
def inflate(tmp_path_factory):
    f = SC.build_host(tmp_path_factory.mktemp("infs_host"))
    assert f.chunk_default == SC.DEFAULT_CHUNK == H.bdx.load_library().bdx_fq_inflate_stream_chunk()
    return f


@pytest.mark.parametrize("k", range(len(SC.derived_cases())), ids=[c.name for c, _ in SC.derived_cases()])
def test_case_inflates_to_its_text_with_the_derived_counters(inflate, k):
    case, plain = SC.derived_cases()[k]
    for chunk in SC.CHUNKS:
        rc, got, plen, info, _, _, clean = inflate(case.data, chunk, len(plain))
        assert rc == 0 and plen == len(plain) and got == plain and clean, (case.name, chunk, rc)
        assert info == SC.expected_info(case, chunk), (case.name, chunk)
        assert info[2] + info[3] + info[4] == info[1] - 1
        assert inflate(case.data, chunk, len(plain), seg_room=1 << 16)[1:4] == (got, plen, info)  # (the chain run once, not twice)


def test_the_cases_reach_every_edge_they_are_written_for():
    seen = {}
    for case, _ in SC.derived_cases():
        for chunk in SC.CHUNKS:
            for f in SC.features(case, chunk):
                seen.setdefault(f, set()).add(chunk)
    for what, chunks in SC.WANTED.items():
        assert set(chunks) <= seen.get(what, set()), (what, chunks, seen.get(what))


def test_zlib_streams_confirm_every_dynamic_block_start_and_discard_nothing(inflate):
    for case, plain in SC.derived_cases():
        if case.name not in SC.ZLIB_CASES:
            continue
        for chunk in SC.CHUNKS:
            c8 = 8 * (chunk or SC.DEFAULT_CHUNK)
            first = {}
            for b in SC.file_blocks(case)[0]:
                first.setdefault(b.bit // c8, b)
            dynamic = sum(1 for k, b in first.items() if k >= 1 and b.btype == 2)
            info = inflate(case.data, chunk, len(plain))[3]
            assert info[2] == dynamic and info[3] == 0, (case.name, chunk, info)
    assert all(SC.expected_info(c, 4096)[2] for c, _ in SC.derived_cases() if c.name in SC.ZLIB_CASES[:3])  # (guesses there are)


def test_zlib_is_the_arbiter(inflate):
    """every good and bad member of the two case modules, alone and behind a good member; flipped CRC and ISIZE;
    trailing bytes as zlib's gzread takes them"""
    cases = SC.arbiter_cases()
    assert len(cases) > 250
    verdicts = {}
    for name, data in cases:
        want = SC.arbiter(data)
        for chunk in (64, 4096, 0) if len(data) > 4096 else (64, 0):
            rc, got, plen, _, member, at, clean = inflate(data, chunk, len(want) if want is not None else 70000)
            if want is None:
                assert 1 <= rc <= 11 and 0 <= at <= len(data) and member >= 0, (name, chunk, rc)
            else:
                assert rc == 0 and got == want and clean, (name, chunk, rc)
            verdicts[name] = rc
    assert sum(1 for v in verdicts.values() if v) > 50 and sum(1 for v in verdicts.values() if not v) > 100  # (both kinds, many)
    assert verdicts["flipped_crc"] == 10 and verdicts["flipped_isize"] == 11 and verdicts["flipped_crc_first_member"] == 10
    assert verdicts["reach_back_first_segment"] == 6 and verdicts["reach_back_later_segment"] == 6  # distance too far
    assert verdicts["trailing_zeros"] == verdicts["trailing_junk"] == verdicts["trailing_one_byte"] == 0
    assert verdicts["trailing_junk_with_magic"] and verdicts["trailing_magic_alone"]
    assert {v for n, v in verdicts.items() if n.startswith("lead+") and v} >= {2, 3, 4, 5, 6, 9, 10, 11}
    assert verdicts["trailing_magic_alone"] == 1  # (a second header that is cut short: bad header)


def test_every_prefix_of_the_small_files(inflate):
    files = SC.small_files()
    assert len(files) >= 2
    accepted = 0
    for name, data in files:
        for cut in range(len(data)):
            want = SC.arbiter(data[:cut])
            rc, got = inflate(data[:cut], 64, 4000)[:2]
            assert (rc == 0 and got == want) if want is not None else 1 <= rc <= 11, (name, cut, rc)
            accepted += want is not None
    assert accepted > 0  # (a cut right behind a member of a file of several leaves a good file)


def test_capacity(inflate):
    for case, plain in SC.derived_cases()[:6]:
        n = len(plain)
        assert inflate(case.data, 64, n)[:3] == (0, plain, n)
        rc, got, plen, _, _, _, clean = inflate(case.data, 64, n - 1)
        assert rc == SC.SPACE and plen == n and got is None and clean  # the size needed; the buffer keeps its fill
        assert inflate(case.data, 4096, 0)[:3] == (SC.SPACE, None, n)
