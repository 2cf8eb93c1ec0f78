"""Device gzip, the parts that need no GPU: the _gzip keyword's validation, the pure size functions of
csrc/bdx_deflate.hip, the raw block writer of csrc/bdx_io.cpp, and the chunk encoder itself (csrc/bdx_deflate_core.h)
compiled as plain C++ and held to the checks the GPU tests hold the device to."""
import ctypes as C
import gzip
import os
import zlib

import numpy as np
import pytest

import deflate_cases as DC
import helpers as H
from biodemux_jl_amd import hipabi, nativeio


# ---- keyword validation: before any file or device is touched ----
@pytest.mark.parametrize("kw, needle", [
    (dict(_gzip="zstd"), "_gzip must be"),
    (dict(_gzip="device", _io="native"), "_io='device'"),
    (dict(_gzip="device", _io="auto"), "_io='device'"),
    (dict(_gzip="device"), "_io='device'"),
])
def test_gzip_keyword_is_validated_first(tmp_path, kw, needle):
    out = tmp_path / "never_made"
    with pytest.raises(ValueError, match=needle):
        H.bdx.execute_demultiplexing(str(tmp_path / "no.fastq"), str(tmp_path / "no.csv"), str(out), gzip_output=True, **kw)
    assert not out.exists()


# ---- the pure entries of the library ----
def test_new_entries_are_part_of_the_abi():
    lib = H.bdx.load_library()
    for name in ("bdx_fq_deflate_chunk", "bdx_fq_deflate_bound", "bdx_fq_deflate_device"):
        assert name in hipabi.ABI_SYMBOLS and hasattr(lib, name)
    assert lib.bdx_abi_version() == 1


def test_deflate_chunk_range():
    assert 4096 <= H.bdx.load_library().bdx_fq_deflate_chunk() <= 65535


def _bound(sizes):
    a = np.asarray(sizes, dtype=np.int64)
    return int(H.bdx.load_library().bdx_fq_deflate_bound(a.ctypes.data if len(a) else None, len(a)))


def test_deflate_bound_without_a_device():
    ch = H.bdx.load_library().bdx_fq_deflate_chunk()
    rng = np.random.default_rng(4)
    cases = [[1], [ch - 1, ch, ch + 1], [0, 3, 0, 2 * ch + 1, 0], [10 * ch], [2 ** 33 + 5]]
    cases += [list(rng.integers(0, 5 * ch, 40)) for _ in range(5)]
    for sizes in cases:
        need = sum(int(n) + 33 * -(-int(n) // ch) for n in sizes if n > 0)
        got = _bound(sizes)
        assert need <= got <= need + 64 * len(sizes), sizes
    assert _bound([]) == 0 and _bound([0]) == 0 and _bound([0] * 9) == 0
    assert _bound([5, -1, 5]) < 0


# ---- bdx_fq_write_blocks_raw ----
def _members(data: bytes, piece: int) -> bytes:
    """`data` as a chain of 'D','X'-tagged gzip members of `piece` bytes each, the way deflate_gz_members makes them"""
    out = []
    for o in range(0, len(data), piece):
        part = data[o:o + piece]
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = z.compress(part) + z.flush()
        total = 20 + len(body) + 8
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x08\0DX\x04\0" + total.to_bytes(4, "little") + body
                   + zlib.crc32(part).to_bytes(4, "little") + (len(part) & 0xFFFFFFFF).to_bytes(4, "little"))
    return b"".join(out)


def _raw(buf: bytes, sizes, paths, threads=4):
    L = nativeio._load()
    L.bdx_fq_write_blocks_raw.restype = C.c_int32
    L.bdx_fq_write_blocks_raw.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.c_int32]
    L.bdx_io_last_error.restype = C.c_char_p
    cb = np.asarray(sizes, dtype=np.int64)
    arr = (C.c_char_p * len(paths))(*[p.encode() if p else None for p in paths])
    data = np.frombuffer(buf + b"\0", dtype=np.uint8)
    return L.bdx_fq_write_blocks_raw(data.ctypes.data, cb.ctypes.data, len(cb), arr, threads), L


def test_write_blocks_raw_appends_verbatim(tmp_path):
    nativeio.build()
    rec = b"".join(b"@r%d\nACGTACGTAC\n+\nIIIIIIIIII\n" % i for i in range(4000))
    blocks = [_members(rec, 30000), b"", _members(rec[:290], 100), b"", b"not gzip at all"]
    paths = [str(tmp_path / "a.fastq.gz"), None, str(tmp_path / "b.fastq.gz"), str(tmp_path / "empty.fastq.gz"),
             str(tmp_path / "c.fastq.gz")]
    for times in (1, 2):  # the second call appends
        rc, L = _raw(b"".join(blocks), [len(b) for b in blocks], paths)
        assert rc == 0, L.bdx_io_last_error()
        for b, p in zip(blocks, paths):
            if b:
                assert open(p, "rb").read() == b * times
        assert sorted(os.listdir(tmp_path)) == ["a.fastq.gz", "b.fastq.gz", "c.fastq.gz"]
    assert gzip.open(paths[0]).read() == rec * 2
    f = nativeio.FastqFile(paths[0], 4)  # the tagged chain reads back through the parallel inflate
    try:
        assert C.c_int32(nativeio._load().bdx_fq_parallel_inflate(f.h)).value == 1
    finally:
        f.close()


def test_write_blocks_raw_refuses_a_block_without_a_path(tmp_path):
    nativeio.build()
    rc, L = _raw(b"abcdef", [3, 3], [str(tmp_path / "x.gz"), None])
    assert rc != 0 and b"no path" in L.bdx_io_last_error()
    rc, L = _raw(b"abc", [3, -1], [str(tmp_path / "y.gz"), None])
    assert rc != 0


# ---- the chunk encoder as plain C++ (tests/deflate_core_host.cpp) ----
@pytest.fixture(scope="module")
def host_encode(tmp_path_factory):
    encode = DC.build_host_encoder(tmp_path_factory.mktemp("dfl"))
    assert encode.chunk == H.bdx.load_library().bdx_fq_deflate_chunk()
    return encode


def test_host_encoder_sizes_and_edge_inputs(host_encode):
    ch = host_encode.chunk
    rng = np.random.default_rng(8)
    alphabet = np.frombuffer(b"ACGTN\n@+FFFF:,I#0123 ", dtype=np.uint8)
    for n in (1, 2, 3, 4, 5, 258, 259, ch - 1, ch, ch + 1, 2 * ch + 1):
        host_encode(rng.choice(alphabet, n).tobytes())
    assert len(host_encode(b"G" * ch)) < 1024
    assert len(host_encode(rng.integers(0, 256, ch, dtype=np.uint8).tobytes())) <= ch + 33  # one stored block
    host_encode(b"aaababbbaa")  # no 3-gram twice: no distance code at all
    host_encode(b"ab" * 40)     # one distance code


@pytest.mark.parametrize("k", [22, 21])
def test_host_encoder_limits_code_lengths(host_encode, k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    data = np.repeat(np.arange(65, 65 + k, dtype=np.uint8), f)  # an unrestricted Huffman tree is k - 1 > 15 deep
    assert len(host_encode(data.tobytes())) < 2048
    mixed = np.random.default_rng(11).permutation(data).tobytes()
    assert len(host_encode(mixed)) < len(mixed) // 2


def test_host_encoder_beats_huffman_only_on_fastq(host_encode):
    rng = np.random.default_rng(20)
    qsym = np.frombuffer(b"F:,#FFFF::0123456789-", dtype=np.uint8)[:16]
    p = np.array([40, 15, 8, 2, 6, 6, 5, 4, 3, 3, 2, 2, 1, 1, 1, 1], dtype=np.float64)
    out = []
    for _ in range(600):
        x, y = rng.integers(1000, 32000, 2)
        out.append(b"@A00123:45:HXXXXXXX:1:1101:%d:%d 1:N:0:ACGT\n" % (x, y))
        out.append(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 150).tobytes() + b"\n+\n")
        out.append(rng.choice(qsym, 150, p=p / p.sum()).tobytes() + b"\n")
    text = b"".join(out)
    z = zlib.compressobj(6, zlib.DEFLATED, 31, 8, zlib.Z_HUFFMAN_ONLY)
    assert len(host_encode(text)) < len(z.compress(text) + z.flush())
    assert host_encode(text) == host_encode(text)


# ---- the named cases of tests/deflate_cases.py: the host build reaches every edge the GPU tests hold the device to ----
@pytest.mark.parametrize("case", DC.CASES, ids=repr)
def test_case_reaches_its_edge_on_the_host_build(host_encode, case):
    comp = host_encode(case.data, fresh=True)  # (gunzips to the input, one member per chunk)
    dyn = host_encode.last_dynamic_bytes()
    members = DC.split_members(comp)
    A = [DC.anatomy(m) for m in members]
    assert b"".join(a["data"] for a in A) == case.data
    assert all((p - d) // DC.SUB < p // DC.SUB for a in A for t in a["tokens"] if len(t) == 3 for (_, d, p) in [t]), \
        "a candidate from the match's own sub-block: the table was consulted after this sub-block's inserts"
    assert case.pred(A), (case.why, [(a["btype"], a["tokens"][-3:]) for a in A])
    if A[-1]["btype"] == 2:
        assert dyn == len(members[-1]) - 28
    else:  # stored for a reason
        assert dyn >= A[-1]["n"] + 5 or dyn > DC.TAB_BYTES
    if case.tries is not None:
        assert dyn == case.dynamic_bytes and case.tries <= DC.SEARCH_CAP
    assert host_encode(case.data) == comp, "the same bytes from a DflShared that another chunk has used"


@pytest.mark.parametrize("mix", ["persistent", "scan_257", "scan_768"])
def test_host_encoder_leaks_no_state_between_chunks(host_encode, mix):
    """one DflShared for all chunks, as in a persistent workgroup: every class equals its encoding by a fresh one"""
    texts = DC.persistent_mix(2 * 32 + 3, 32) if mix == "persistent" else DC.scan_mix(int(mix[5:]))
    if mix == "persistent":
        sizes = [len(t) for t in texts]
        assert sizes.count(DC.CH) >= 4 and min(sizes) <= 40
    host_encode(b"x", fresh=True)
    shared = [host_encode(t) for t in texts]
    alone = [host_encode(t, fresh=True) for t in texts]
    assert shared == alone
    if mix == "persistent":
        kinds = {(len(t) == DC.CH, DC.anatomy(c)["btype"]) for t, c in zip(texts, shared)}
        assert kinds == {(False, 0), (False, 2), (True, 0), (True, 2)}  # small and full, stored and dynamic
