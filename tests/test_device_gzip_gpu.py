"""Device gzip (csrc/bdx_deflate.hip) on the MI355X: every class block bdx_fq_deflate_device returns is a chain of
size-tagged gzip members that any reader inflates to the input, the bytes are the same on every run, and
execute_demultiplexing(..., _io="device", _gzip="device") writes files that gunzip to what _io="native" writes."""
import ctypes as C
import functools
import gzip
import os
import zlib

import numpy as np
import pytest

import helpers as H
from biodemux_jl_amd import nativeio, synth

pytestmark = pytest.mark.gpu

run_nat = functools.partial(H.bdx.execute_demultiplexing, _io="native")
run_dev = functools.partial(H.bdx.execute_demultiplexing, _io="device")
run_dgz = functools.partial(H.bdx.execute_demultiplexing, _io="device", _gzip="device")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    nativeio.build()


@pytest.fixture(scope="module")
def hc():
    cfg = H.bdx.DemuxConfig(bc_seqs=["ACGTACGT"], bc_lengths_no_N=[8], ids=["a"])
    c = H.bdx.HipClassifier(cfg)
    yield c
    c.close()


def _chunk() -> int:
    return int(H.bdx.load_library().bdx_fq_deflate_chunk())


def _deflate(hc, blocks, lead=0, out_cap=None, canary=0):
    """bdx_fq_deflate_device over `blocks` (bytes per class, placed back to back `lead` bytes into a device buffer);
    returns (rc, compressed bytes per class, the `canary` bytes after out_cap)"""
    import torch

    lib = hc.lib
    cb = np.array([len(b) for b in blocks], dtype=np.int64)
    bound = int(lib.bdx_fq_deflate_bound(cb.ctypes.data, len(cb)))
    cap = bound if out_cap is None else out_cap
    host = np.frombuffer(b"\0" * lead + b"".join(blocks), dtype=np.uint8)  # no pad byte: the input ends the tensor
    d_in = torch.from_numpy(host.copy()).to("cuda:0") if len(host) else torch.zeros(1, dtype=torch.uint8, device="cuda:0")
    d_out = torch.full((max(cap + canary, 1),), 0xC5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    zb = np.full(len(cb), -7, dtype=np.int64)
    rc = lib.bdx_fq_deflate_device(hc.h, d_in.data_ptr() + lead, cb.ctypes.data, len(cb), d_out.data_ptr(), cap, zb.ctypes.data)
    out = d_out.cpu().numpy().tobytes()
    if rc != 0:
        return rc, None, out[cap:cap + canary]
    assert int(zb.sum()) <= bound
    parts, pos = [], 0
    for z in zb:
        parts.append(out[pos:pos + int(z)])
        pos += int(z)
    return rc, parts, out[cap:cap + canary]


def _walk(block: bytes):
    """member sizes by the 'D','X' tags; must land on the block's end"""
    sizes, p = [], 0
    while p < len(block):
        assert block[p:p + 4] == b"\x1f\x8b\x08\x04" and block[p + 9] == 255, "FEXTRA gzip header with OS = 255"
        assert block[p + 10:p + 16] == b"\x08\x00DX\x04\x00"
        s = int.from_bytes(block[p + 16:p + 20], "little")
        assert s >= 28
        sizes.append(s)
        p += s
    assert p == len(block)
    return sizes


def _check_blocks(blocks, parts):
    ch = _chunk()
    assert len(parts) == len(blocks)
    for plain, comp in zip(blocks, parts):
        if not plain:
            assert comp == b""
            continue
        assert gzip.decompress(comp) == plain  # (every member's CRC-32 and ISIZE)
        assert len(_walk(comp)) == -(-len(plain) // ch)


def _text(n, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.frombuffer(b"ACGTN\n@+FFFF:,I#0123 ", dtype=np.uint8), size=n).tobytes()


def _sizes():
    ch = _chunk()
    return [1, 2, 3, 258, 259, ch - 1, ch, ch + 1, 2 * ch + 1]


@pytest.mark.parametrize("n", [1, 2, 3, 258, 259, "CH-1", "CH", "CH+1", "2CH+1"])
def test_sizes_single_class(hc, n):
    ch = _chunk()
    n = {"CH-1": ch - 1, "CH": ch, "CH+1": ch + 1, "2CH+1": 2 * ch + 1}.get(n, n)
    blocks = [_text(n, n)]
    rc, parts, _ = _deflate(hc, blocks)
    assert rc == 0
    _check_blocks(blocks, parts)


def test_sizes_nine_classes_between_empty_ones_at_odd_offsets(hc):
    blocks = []
    for n in _sizes():
        blocks += [_text(n, 100 + n), b""]
    blocks = [b""] + blocks
    rc, parts, _ = _deflate(hc, blocks, lead=3)
    assert rc == 0
    _check_blocks(blocks, parts)


def test_one_repeated_byte(hc):
    blocks = [b"G" * _chunk()]
    rc, parts, _ = _deflate(hc, blocks)
    assert rc == 0
    _check_blocks(blocks, parts)
    assert len(parts[0]) < 1024  # matches of 258, a code of two or three symbols


def test_random_bytes_fall_back_to_stored(hc):
    ch = _chunk()
    blocks = [np.random.default_rng(3).integers(0, 256, ch, dtype=np.uint8).tobytes()]
    rc, parts, _ = _deflate(hc, blocks)
    assert rc == 0
    _check_blocks(blocks, parts)
    assert len(parts[0]) <= ch + 33


def test_two_letters_without_a_repeated_triple(hc):
    s = b"aaababbbaa"  # de Bruijn B(2, 3) with its wrap: the eight 3-grams, each once (the longest such text there is)
    assert len({s[i:i + 3] for i in range(len(s) - 2)}) == len(s) - 2
    rc, parts, _ = _deflate(hc, [s])
    assert rc == 0
    _check_blocks([s], parts)


def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f


@pytest.mark.parametrize("k", [22, 21])  # 22: the 46 367 bytes of the issue; 21: 28 656 bytes, the whole histogram in ONE chunk
@pytest.mark.parametrize("order", ["shuffled", "sorted"])
def test_length_limited_codes(hc, k, order):
    """byte counts 1, 1, 2, 3, 5, ...: an unrestricted Huffman tree over them is k - 1 > 15 levels deep"""
    counts = _fib(k)
    assert sum(counts) == {22: 46367, 21: 28656}[k]
    data = np.repeat(np.arange(65, 65 + k, dtype=np.uint8), counts)
    if k == 21:
        assert len(data) <= _chunk()
    if order == "shuffled":
        data = np.random.default_rng(11).permutation(data)
    blocks = [data.tobytes()]
    rc, parts, _ = _deflate(hc, blocks)
    assert rc == 0
    _check_blocks(blocks, parts)
    assert len(parts[0]) < len(blocks[0])


@functools.lru_cache(maxsize=1)
def _fastq_text(records=600, seed=20):
    rng = np.random.default_rng(seed)
    qsym = np.frombuffer(b"F:,#FFFF::0123456789-", dtype=np.uint8)[:16]
    p = np.array([40, 15, 8, 2, 6, 6, 5, 4, 3, 3, 2, 2, 1, 1, 1, 1], dtype=np.float64)
    out = []
    for _ in range(records):
        x, y = rng.integers(1000, 32000, 2)
        out.append(b"@A00123:45:HXXXXXXX:1:1101:%d:%d 1:N:0:ACGT\n" % (x, y))
        out.append(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 150).tobytes() + b"\n+\n")
        out.append(rng.choice(qsym, 150, p=p / p.sum()).tobytes() + b"\n")
    return b"".join(out)


def test_fastq_beats_huffman_only(hc):
    text = _fastq_text()
    rc, parts, _ = _deflate(hc, [text])
    assert rc == 0
    _check_blocks([text], parts)
    z = zlib.compressobj(6, zlib.DEFLATED, 31, 8, zlib.Z_HUFFMAN_ONLY)
    huff = len(z.compress(text) + z.flush())
    print(f"fastq {len(text)} B: device {len(parts[0])} B ({len(text) / len(parts[0]):.2f}x), zlib Huffman-only {huff} B "
          f"({len(text) / huff:.2f}x), level 1 {len(zlib.compress(text, 1))} B, level 6 {len(zlib.compress(text, 6))} B")
    assert len(parts[0]) < huff


def test_same_bytes_on_every_run_and_in_every_context(hc):
    text = _fastq_text()
    a = _deflate(hc, [text])[1]
    b = _deflate(hc, [text], lead=5)[1]
    cfg = H.bdx.DemuxConfig(bc_seqs=["TTGCA"], bc_lengths_no_N=[5], ids=["z"])
    with H.bdx.HipClassifier(cfg) as other:
        c = _deflate(other, [text])[1]
    assert a == b == c


def test_out_cap_below_the_bound_is_refused(hc):
    blocks = [_text(5000, 1), b"", _text(70000, 2)]
    cb = np.array([len(b) for b in blocks], dtype=np.int64)
    bound = int(hc.lib.bdx_fq_deflate_bound(cb.ctypes.data, len(cb)))
    rc, parts, canary = _deflate(hc, blocks, out_cap=bound - 1, canary=4096)
    assert rc != 0 and parts is None
    assert b"bdx_fq_deflate_bound" in hc.lib.bdx_last_error(hc.h)
    assert canary == b"\xC5" * 4096
    rc, parts, canary = _deflate(hc, blocks, out_cap=bound, canary=4096)  # exactly the bound is enough, and respected
    assert rc == 0 and canary == b"\xC5" * 4096
    _check_blocks(blocks, parts)


# ---- end to end: _io="device", _gzip="device" against _io="native" ----
def _fastq(path, seqs):
    blob = b"".join(b"@r%d some header\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n" for i, s in enumerate(seqs))
    open(path, "wb").write(blob)


def _same_gunzipped(a, b, times=1):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb and fa
    for f in fa:
        assert f.endswith(".gz"), f
        assert gzip.open(os.path.join(b, f)).read() == gzip.open(os.path.join(a, f)).read() * times, f


def _single_case(tmp_path, n=700, lo=0, hi=90, seed=5):
    bcs = synth.make_barcodes(6, 12, seed=seed, min_hamming=4)
    seq, off, _ = synth.make_ragged_reads(bcs, n, lo, hi, seed=seed)
    seqs = [seq[off[i]:off[i + 1]].tobytes() for i in range(n)]
    bc = tmp_path / "bc.csv"
    bc.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"b{i},{b},{'B' * len(b)}\n" for i, b in enumerate(bcs)))
    fq = str(tmp_path / "reads.fastq")
    _fastq(fq, seqs)
    return fq, str(bc)


@pytest.mark.parametrize("batch", [128, 37])
def test_device_gzip_equals_native(tmp_path, batch):
    fq, bc = _single_case(tmp_path)
    kw = dict(max_error_rate=0.2, trim_side=5, gzip_output=True, _batch_reads=batch)
    tm = {}
    a = run_nat(fq, bc, str(tmp_path / "nat"), **kw)
    b = run_dgz(fq, bc, str(tmp_path / "dev"), _timings=tm, **kw)
    _same_gunzipped(str(tmp_path / "nat"), str(tmp_path / "dev"))
    assert vars(a) == vars(b)
    assert tm["deflate_s"] > 0 and 0 < tm["compressed_bytes"] < tm["plain_bytes"]
    out = tmp_path / "dev"
    name = max(os.listdir(out), key=lambda f: os.path.getsize(out / f))
    f = nativeio.FastqFile(str(out / name), 4)
    try:
        assert C.c_int32(nativeio._load().bdx_fq_parallel_inflate(f.h)).value == 1
    finally:
        f.close()


def test_device_gzip_dual_many_tiny_members(tmp_path):
    b1 = synth.make_barcodes(24, 24, seed=1)
    b2 = synth.make_barcodes(16, 24, seed=2)
    seq, off, _ = synth.make_reads(b1, 6000, 150, seed=77, plant_lo=0, plant_hi=40, second=(b2, 100, 126))
    fq = str(tmp_path / "dual.fastq")
    _fastq(fq, [seq[off[i]:off[i + 1]].tobytes() for i in range(6000)])
    f1, f2 = tmp_path / "b1.csv", tmp_path / "b2.csv"
    f1.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"x{i},{b},{'B' * len(b)}\n" for i, b in enumerate(b1)))
    f2.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"y{i},{b},{'B' * len(b)}\n" for i, b in enumerate(b2)))
    kw = dict(barcode_file2=str(f2), max_error_rate=0.2, trim_side=5, trim_side2=3, _batch_reads=2500, gzip_output=True)
    a = run_nat(fq, str(f1), str(tmp_path / "nat"), **kw)
    b = run_dgz(fq, str(f1), str(tmp_path / "dev"), **kw)
    _same_gunzipped(str(tmp_path / "nat"), str(tmp_path / "dev"))
    assert vars(a) == vars(b)
    assert len(os.listdir(tmp_path / "dev")) > 100 and a.matched_reads > 0


def test_device_gzip_paired_classify_both(tmp_path):
    bcs = synth.make_barcodes(5, 12, seed=6, min_hamming=4)
    seq, off, _ = synth.make_reads(bcs, 500, 60, seed=6)
    bc = tmp_path / "bc.tsv"
    bc.write_text("ID\tFull_seq\tFull_annotation\n" + "".join(f"b{i}\t{b}\t{'B' * len(b)}\n" for i, b in enumerate(bcs)))
    f1, f2 = str(tmp_path / "x_R1.fastq"), str(tmp_path / "x_R2.fastq")
    _fastq(f1, [seq[off[i]:off[i + 1]].tobytes() for i in range(500)])
    _fastq(f2, [b"ACGT" * 10 for _ in range(430)])
    kw = dict(classify_both=True, trim_side=3, _batch_reads=128, gzip_output=True)
    a = run_nat(f1, f2, str(bc), str(tmp_path / "nat"), **kw)
    b = run_dgz(f1, f2, str(bc), str(tmp_path / "dev"), **kw)
    _same_gunzipped(str(tmp_path / "nat"), str(tmp_path / "dev"))
    assert vars(a) == vars(b) and a.total_reads == 430


def test_device_gzip_appends_like_the_reference(tmp_path):
    fq, bc = _single_case(tmp_path)
    kw = dict(max_error_rate=0.2, trim_side=5, gzip_output=True, _batch_reads=128)
    run_nat(fq, bc, str(tmp_path / "nat"), **kw)
    run_dgz(fq, bc, str(tmp_path / "dev"), **kw)
    run_dgz(fq, bc, str(tmp_path / "dev"), **kw)
    _same_gunzipped(str(tmp_path / "nat"), str(tmp_path / "dev"), times=2)


def test_host_gzip_stays_the_default(tmp_path):
    fq, bc = _single_case(tmp_path)
    kw = dict(max_error_rate=0.2, trim_side=5, gzip_output=True, _batch_reads=128)
    tm = {}
    a = run_nat(fq, bc, str(tmp_path / "nat"), **kw)
    b = run_dev(fq, bc, str(tmp_path / "dev"), _gzip="host", _timings=tm, **kw)
    _same_gunzipped(str(tmp_path / "nat"), str(tmp_path / "dev"))
    assert vars(a) == vars(b) and "deflate_s" not in tm
    # inert without gzip output: plain files, byte for byte
    run_nat(fq, bc, str(tmp_path / "nat_plain"), max_error_rate=0.2, trim_side=5, _batch_reads=128)
    run_dgz(fq, bc, str(tmp_path / "dev_plain"), max_error_rate=0.2, trim_side=5, _batch_reads=128)
    for f in sorted(os.listdir(tmp_path / "nat_plain")):
        assert open(tmp_path / "nat_plain" / f, "rb").read() == open(tmp_path / "dev_plain" / f, "rb").read(), f
