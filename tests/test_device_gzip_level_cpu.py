"""Level 2 of the device gzip encoder, the parts that need no GPU: the _gzip_level keyword's validation, the pure
entries, and both levels of the chunk encoder compiled as plain C++ (tests/deflate2_core_host.cpp) — level 1 held to the
existing host build's bytes, level 2 to zlib's inflate, to the run-length coding of its header, to the named edges of
tests/deflate2_cases.py, and to a smaller total than level 1 on FASTQ text."""
import ctypes as C
import gzip
import zlib

import numpy as np
import pytest

import deflate2_cases as D2
import deflate_cases as DC
import helpers as H
from biodemux_jl_amd import hipabi, nativeio


# ---- keyword validation: before any file or device is touched ----
@pytest.mark.parametrize("kw, needle", [
    (dict(_io="device", _gzip="device", _gzip_level=3), "_gzip_level must be 1 or 2"),
    (dict(_io="device", _gzip="device", _gzip_level=0), "_gzip_level must be 1 or 2"),
    (dict(_io="device", _gzip="device", _gzip_level="2"), "_gzip_level must be 1 or 2"),
    (dict(_io="device", _gzip="device", _gzip_level=True), "_gzip_level must be 1 or 2"),
    (dict(_io="device", _gzip="host", _gzip_level=2), "needs _gzip='device'"),
    (dict(_gzip_level=2), "needs _gzip='device'"),
    (dict(_gzip="device", _gzip_level=2), "_io='device'"),
])
def test_gzip_level_keyword_is_validated_first(tmp_path, kw, needle):
    out = tmp_path / "never_made"
    with pytest.raises(ValueError, match=needle):
        H.bdx.execute_demultiplexing(str(tmp_path / "no.fastq"), str(tmp_path / "no.csv"), str(out), gzip_output=True, **kw)
    assert not out.exists()


# ---- the pure entries of the library ----
def test_level_entries_are_part_of_the_abi():
    lib = H.bdx.load_library()
    hdr = open(H.ROOT + "/include/biodemux_hip.h").read()
    for name in ("bdx_fq_deflate_levels", "bdx_fq_deflate_level_device"):
        assert name in hipabi.ABI_SYMBOLS and hasattr(lib, name) and name + "(" in hdr
    assert lib.bdx_fq_deflate_levels() == 2
    assert lib.bdx_fq_deflate_level_device.argtypes[1] is C.c_int32 and len(lib.bdx_fq_deflate_level_device.argtypes) == 8


@pytest.mark.parametrize("level", [0, 3, -1, 1 << 30])
def test_a_level_that_does_not_exist_is_refused_without_a_context(level):
    lib = H.bdx.load_library()
    cb = np.array([100, 0, 7], dtype=np.int64)
    zb = np.full(3, -7, dtype=np.int64)
    rc = lib.bdx_fq_deflate_level_device(None, level, None, cb.ctypes.data, 3, None, 1 << 20, zb.ctypes.data)
    assert rc == -1  # BDX_E_INVALID
    assert b"deflate level %d" % level in lib.bdx_last_error(None) and b"1 .. 2" in lib.bdx_last_error(None)
    assert list(zb) == [0, 0, 0]


# ---- both levels as plain C++ ----
@pytest.fixture(scope="module")
def enc():
    e = D2.host_encoder()
    assert e.chunk == H.bdx.load_library().bdx_fq_deflate_chunk()
    return e


@pytest.mark.parametrize("case", DC.CASES, ids=repr)
def test_level_1_through_the_level_entry_is_the_existing_host_build(enc, case):
    want = DC.host_encoder().raw(case.data, fresh=True)
    assert enc.raw(case.data, 1, fresh=True) == want
    enc.raw(DC.text(700, "dirty"), 2)  # level 1 after level 2 on the same shared state
    assert enc.raw(case.data, 1) == want


def test_host_build_refuses_other_levels(enc):
    assert enc.raw(b"abc", 0) is None and enc.raw(b"abc", 3) is None


def _check_members(data, comp):
    members = DC.split_members(comp)  # the 'D','X' tags walk to the block's end
    assert len(members) == -(-len(data) // DC.CH)
    for k, m in enumerate(members):
        chunk = data[k * DC.CH:(k + 1) * DC.CH]
        z = zlib.decompressobj(-15)
        assert z.decompress(m[20:-8]) == chunk and z.eof and not z.unused_data
        assert int.from_bytes(m[-8:-4], "little") == zlib.crc32(chunk) and int.from_bytes(m[-4:], "little") == len(chunk)
        assert len(m) <= len(chunk) + 33
    assert gzip.decompress(comp) == data
    return members


@pytest.mark.parametrize("case", D2.CASES, ids=repr)
def test_level_2_case_is_valid_and_reaches_its_edge(enc, case):
    comp = enc(case.data, fresh=True)
    dyn = enc.last_dynamic_bytes()
    cl = enc.last_cl_lengths()
    members = _check_members(case.data, comp)
    x = D2.View(enc, case.data, comp)  # (anatomy: complete codes, zero padding, CRC-32, ISIZE, the tag)
    assert b"".join(a["data"] for a in x.A) == case.data
    for a, h in zip(x.A, x.H):
        if a["btype"] == 2:
            assert h["lengths"] == a["ll_lengths"] + a["d_lengths"]
            assert h["symbols"] == D2.expected_header_symbols(h["lengths"]), "the header's run-length coding"
    assert case.pred(x), case.why
    if x.A[-1]["btype"] == 2:
        assert dyn == len(members[-1]) - 28 and cl == x.H[-1]["cl_lengths"]
    else:  # stored for a reason
        assert dyn >= x.A[-1]["n"] + 5 or dyn > DC.TAB_BYTES
    if case.tries is not None:
        assert dyn == case.dynamic_bytes and case.tries <= DC.SEARCH_CAP
    assert enc(case.data) == comp, "the same bytes from a Dfl2Shared that other chunks and dfl2_host_records have used"


@pytest.mark.parametrize("case", DC.CASES, ids=repr)
def test_level_2_is_valid_on_the_level_1_cases(enc, case):
    comp = enc(case.data, fresh=True)
    _check_members(case.data, comp)
    for m in DC.split_members(comp):
        a, h = DC.anatomy(m), D2.header_anatomy(m)
        if a["btype"] == 2:
            assert h["symbols"] == D2.expected_header_symbols(a["ll_lengths"] + a["d_lengths"])
    assert enc(case.data) == comp


def test_parallel_inflate_of_the_reader_takes_a_level_2_chain(enc, tmp_path):
    nativeio.build()
    text = D2.fastq_varied(600)
    comp = enc(text, fresh=True)
    assert len(DC.split_members(comp)) > 5
    path = tmp_path / "l2.fastq.gz"
    path.write_bytes(comp)
    assert gzip.open(path).read() == text
    f = nativeio.FastqFile(str(path), 4)  # bdx_fq_open
    try:
        assert C.c_int32(nativeio._load().bdx_fq_parallel_inflate(f.h)).value == 1
    finally:
        f.close()


@pytest.mark.parametrize("mix", ["persistent", "scan_257"])
def test_one_shared_state_over_a_mix_of_chunks_and_levels(enc, mix):
    """one Dfl2Shared for all chunks, as in a persistent workgroup: every class equals its encoding by a fresh one"""
    texts = DC.persistent_mix(2 * 24 + 3, 24) if mix == "persistent" else DC.scan_mix(int(mix[5:]))
    enc(b"x", fresh=True)
    shared = [enc.raw(t) for t in texts]
    alone = [enc.raw(t, fresh=True) for t in texts]
    assert shared == alone
    for t, c in zip(texts, shared):
        assert gzip.decompress(c) == t
    if mix == "persistent":
        kinds = {(len(t) == DC.CH, DC.anatomy(c)["btype"]) for t, c in zip(texts, shared)}
        assert kinds == {(False, 0), (False, 2), (True, 0), (True, 2)}  # small and full, stored and dynamic
        levels = [1 + (i * 7 // 3) % 2 for i in range(len(texts))]
        mixed = [enc.raw(t, lv) for t, lv in zip(texts, levels)]
        assert mixed == [shared[i] if lv == 2 else DC.host_encoder().raw(texts[i], fresh=True) for i, lv in enumerate(levels)]


# ---- ratio: level 2 is smaller than level 1 and than Huffman coding alone; the rest is reported ----
@pytest.mark.parametrize("recipe", ["varied_quality", "constant_quality"])
def test_level_2_is_smaller_than_level_1_on_fastq(enc, recipe):
    text = (D2.fastq_varied if recipe == "varied_quality" else D2.fastq_constant)(600)
    l1, l2 = len(enc(text, 1)), len(enc(text, 2))
    huff = D2.zlib_per_chunk(text, 6, zlib.Z_HUFFMAN_ONLY)
    print("%s, %d B: level 1 %.3fx, level 2 %.3fx, Huffman-only %.3fx; zlib per chunk: %s" % (
        recipe, len(text), len(text) / l1, len(text) / l2, len(text) / huff,
        ", ".join("level %d %.3fx" % (lv, len(text) / D2.zlib_per_chunk(text, lv)) for lv in range(1, 10))))
    assert l2 < l1
    assert l2 < huff
