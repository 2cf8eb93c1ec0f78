"""Device gunzip, the parts that need no GPU: the _gunzip keyword's validation, the new entries of the C-ABI and their
table checks, the member-table reader of csrc/bdx_io.cpp, and the decoder itself (csrc/bdx_inflate_core.h) compiled as
plain C++ and held to the members of tests/inflate_cases.py, the ones the GPU tests hold the device to."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import inflate_cases as IC
import helpers as H
from biodemux_jl_amd import hipabi, nativeio

MAX = 65536
BDX_E_INVALID = -1


# ---- keyword validation: before any file or device is touched ----
@pytest.mark.parametrize("kw, needle", [
    (dict(_gunzip="zstd"), "_gunzip must be"),
    (dict(_gunzip="device", _io="native"), "_io='device'"),
    (dict(_gunzip="device", _io="auto"), "_io='device'"),
    (dict(_gunzip="device"), "_io='device'"),
])
def test_gunzip_keyword_is_validated_first(tmp_path, kw, needle):
    out = tmp_path / "never_made"
    with pytest.raises(ValueError, match=needle):
        H.bdx.execute_demultiplexing(str(tmp_path / "no.fastq.gz"), str(tmp_path / "no.csv"), str(out), **kw)
    assert not out.exists()


# ---- the entries of the library ----
def test_new_entries_are_part_of_the_abi():
    lib = H.bdx.load_library()
    header = open(os.path.join(H.ROOT, "include", "biodemux_hip.h")).read()
    for name in ("bdx_fq_inflate_member_max", "bdx_fq_inflate_device"):
        assert name in hipabi.ABI_SYMBOLS and hasattr(lib, name) and name + "(" in header
    assert lib.bdx_abi_version() == 1
    assert lib.bdx_fq_inflate_member_max() == MAX == IC.MEMBER_MAX


def _call(tables, n=None, out_cap=1 << 20, ctx=None):
    lib = H.bdx.load_library()
    coff, clen, poff, plen = (np.asarray(a, dtype=t) for a, t in zip(tables, (np.int64, np.int32, np.int64, np.int32)))
    n = len(coff) if n is None else n
    rc = lib.bdx_fq_inflate_device(ctx, None, coff.ctypes.data, clen.ctypes.data, poff.ctypes.data, plen.ctypes.data, n, None, out_cap, None)
    return rc, lib.bdx_last_error(ctx).decode()


def test_tables_are_validated_before_anything_else():
    """without a device: a wrong table is named before the missing context is"""
    ok = ([0, 100], [100, 50], [0, 4000], [4000, MAX])
    for tables, cap, needle in [
        (([0, -1], [100, 50], [0, 4000], [4000, 10]), 1 << 20, "member 1: a negative"),
        (([0, 100], [100, -50], [0, 4000], [4000, 10]), 1 << 20, "member 1: a negative"),
        (([0, 100], [100, 50], [-1, 4000], [4000, 10]), 1 << 20, "member 0: a negative"),
        (([0, 100], [100, 50], [0, 4000], [-4000, 10]), 1 << 20, "member 0: a negative"),
        (([0, 100], [100, 50], [0, 4000], [4000, MAX + 1]), 1 << 20, "bdx_fq_inflate_member_max"),
        (ok, 4000 + MAX - 1, "member 1: its slot"),
        (([0], [100], [2 ** 62], [MAX]), 2 ** 62 + MAX - 1, "member 0: its slot"),
    ]:
        rc, err = _call(tables, out_cap=cap)
        assert rc == BDX_E_INVALID and needle in err, (tables, err)
    rc, err = _call(ok, n=-1)
    assert rc == BDX_E_INVALID and "negative" in err
    for tables, n in ((ok, None), (([], [], [], []), 0)):  # fine tables: now the NULL context is what is wrong
        rc, err = _call(tables, n=n, out_cap=4000 + MAX)
        assert rc == BDX_E_INVALID and "ctx is NULL" in err


# ---- the member-table reader (bdx_fq_members_*) ----
@pytest.fixture(scope="module", autouse=True)
def _io_lib():
    nativeio.build()


def _table(path):
    g = nativeio.GzMembers(str(path), MAX)
    try:
        return g.eligible, g.reason, g.comp_off.tolist(), g.comp_len.tolist(), g.isize.tolist(), g.plain_off.tolist(), g.size
    finally:
        g.close()


def test_member_table_of_a_chain(tmp_path):
    members = list(IC.good_members())
    members.insert(3, IC.zmember("end_marker_inside", b"", tag="BC"))
    members.append(IC.zmember("end_marker", b"", tag="BC"))
    blob = IC.chain(members)
    assert gzip.decompress(blob) == b"".join(m.plain for m in members)
    p = tmp_path / "chain.fastq.gz"
    p.write_bytes(blob)
    ok, why, coff, clen, isize, poff, size = _table(p)
    assert ok and why == "" and size == len(blob)
    assert clen == [len(m.comp) for m in members] and isize == [m.plen for m in members]
    assert coff == np.cumsum([0] + clen[:-1]).tolist() and poff == np.cumsum([0] + isize).tolist()
    f = nativeio.FastqFile(str(p), 4)
    try:
        assert f.parallel_inflate
    finally:
        f.close()


def test_member_table_of_the_raw_block_writer(tmp_path):
    L = nativeio._load()
    L.bdx_fq_write_blocks_raw.restype = C.c_int32
    L.bdx_fq_write_blocks_raw.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.c_int32]
    members = IC.encoder_members()
    blob = IC.chain(members)
    path = str(tmp_path / "raw.fastq.gz")
    data = np.frombuffer(blob, dtype=np.uint8).copy()
    cb = np.array([len(blob)], dtype=np.int64)
    assert L.bdx_fq_write_blocks_raw(data.ctypes.data, cb.ctypes.data, 1, (C.c_char_p * 1)(path.encode()), 2) == 0
    ok, why, coff, clen, isize, _, _ = _table(path)
    assert ok and clen == [len(m.comp) for m in members] and isize == [m.plen for m in members]


def test_member_table_refuses_what_the_device_cannot_take(tmp_path):
    text = IC.fastq_text(200000, 3)
    plain_gz = tmp_path / "ordinary.fastq.gz"
    with gzip.open(plain_gz, "wb") as f:
        f.write(text)
    ok, why, coff, *_ = _table(plain_gz)
    assert not ok and coff == [] and "member 0" in why and "no size tag" in why
    # the host writers' 4 MiB members: tagged, but far above the decoder's member size
    big = tmp_path / "host_writer.fastq.gz"
    L = nativeio._load()
    L.bdx_fq_write_blocks.restype = C.c_int32
    L.bdx_fq_write_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.c_int32, C.c_int32]
    data = np.frombuffer(text, dtype=np.uint8).copy()
    cb = np.array([len(text)], dtype=np.int64)
    assert L.bdx_fq_write_blocks(data.ctypes.data, cb.ctypes.data, 1, (C.c_char_p * 1)(str(big).encode()), 1, 2) == 0
    assert gzip.open(big).read() == text
    ok, why, coff, *_ = _table(big)
    assert not ok and coff == [] and "inflates to 200000 bytes" in why and str(MAX) in why
    # a chain whose last tag overshoots the file's end; and one with an untagged member behind two tagged ones
    good = [IC.zmember("a", text[:3000]), IC.zmember("b", text[3000:9000]), IC.zmember("c", text[9000:9100])]
    cut = tmp_path / "cut.fastq.gz"
    cut.write_bytes(IC.chain(good)[:-1])
    ok, why, coff, clen, *_ = _table(cut)
    assert not ok and len(coff) == 2 and "member 2" in why and "past the end" in why
    mixed = tmp_path / "mixed.fastq.gz"
    mixed.write_bytes(IC.chain(good[:2]) + gzip.compress(text[9000:9100]))
    ok, why, coff, *_ = _table(mixed)
    assert not ok and len(coff) == 2 and "member 2" in why and "no size tag" in why
    empty = tmp_path / "empty.fastq.gz"
    empty.write_bytes(b"")
    assert _table(empty)[:3] == (True, "", [])


# ---- the decoder as plain C++ (tests/inflate_core_host.cpp) ----
@pytest.fixture(scope="module")
def decode():
    d = IC.host_decoder()
    assert d.shared_bytes * 8 <= 160 * 1024, "at least 8 decoders per compute unit"
    return d


@pytest.mark.parametrize("m", IC.good_members(), ids=lambda m: m.name)
def test_good_member_inflates_to_its_input(decode, m):
    st, got = decode(m.comp, m.plen, fresh=True)  # (-1: a byte beside the slot was touched)
    assert st == 0 and got == m.plain


@pytest.mark.parametrize("m", IC.bad_members(), ids=lambda m: m.name)
def test_bad_member_is_refused_inside_its_slot(decode, m):
    st, _ = decode(m.comp, m.plen, fresh=True)
    assert st > 0, IC.STATUS.get(st)
    expect = {"crc_bit": 10, "btype_3": 2, "stored_nlen": 3, "distance_before_start": 6, "isize_small": 7, "isize_large": 8,
              "truncated_9": 9, "oversubscribed_code_lengths": 4}
    assert st == expect.get(m.name, st), IC.STATUS.get(st)


def test_isize_of_the_table_against_the_trailer(decode):
    """the slot's size comes from a table: a stream that fills it exactly but states another ISIZE is refused too"""
    m = IC.good_members()[5]
    lied = m.comp[:-4] + (m.plen + 7).to_bytes(4, "little")
    assert decode(lied, m.plen)[0] == 11
    assert decode(m.comp, m.plen + 1)[0] == 8 and decode(m.comp, m.plen - 1)[0] == 7
    assert decode(m.comp[:17], m.plen)[0] == 1 and decode(b"", 0)[0] == 1


def test_every_prefix_and_many_bit_flips_stay_inside_the_slot(decode):
    """no input faults or writes beside its slot: -1 is the harness's word for a touched canary"""
    m = IC.zmember("t", IC.fastq_text(700, 41))
    for cut in range(len(m.comp)):
        st, _ = decode(m.comp[:cut], m.plen)
        assert st > 0, cut
    rng = np.random.default_rng(42)
    refused = 0
    for src in (m, IC.zmember("f", IC.fastq_text(900, 43), strategy=IC.zlib.Z_FIXED), IC.good_members()[-1]):
        for _ in range(300):
            b = bytearray(src.comp)
            for pos in rng.integers(12, len(b), int(rng.integers(1, 4))):
                b[pos] ^= 1 << int(rng.integers(0, 8))
            st, got = decode(bytes(b), src.plen)
            assert st >= 0
            try:
                same = gzip.decompress(bytes(b)) == src.plain
            except Exception:  # noqa: BLE001
                same = False
            assert (st == 0) == same  # zlib is the arbiter
            refused += st > 0
    assert refused > 800


def test_one_shared_state_for_many_members(decode):
    members = IC.good_members() + IC.bad_members()
    alone = [decode(m.comp, m.plen, fresh=True) for m in members]
    decode(b"x", 0, fresh=True)
    order = np.random.default_rng(7).permutation(len(members))
    for k in order:
        st, got = decode(members[k].comp, members[k].plen)
        assert st == alone[k][0] and (st != 0 or got == alone[k][1]), members[k].name
