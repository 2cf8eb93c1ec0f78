"""The launch paths of the stream inflate (csrc/bdx_inflate_stream.hip) on the MI355X that its case tests do not reach:
persistent grids narrow enough (BDX_CU_COUNT 1 and 7) that every workgroup of the scan, decode and rest kernels takes a
second and a third item on the LDS state the item before left; a file with more chunks than the real grid is wide; the
chain kernel run a second time with a regrown segment list; many calls on one context, refusals, BDX_E_SPACE and the
tagged inflate among them; the fixed slice of the seeded corpus (tests/inflate_stream_fuzz.py), the very files the
stand-alone sanitizer driver runs; and execute_demultiplexing(..., _gunzip="device-stream") against _gunzip="host" on
pigz-like input, with device gzip output, at the edges of the resident text and on both sides of the capacity guess.
zlib says what every file gives; the counters are the ones tests/inflate_stream_cases.py derives from the files' bytes."""
import contextlib
import gzip
import os
import zlib

import numpy as np
import pytest

import helpers as H
import inflate_cases as IC
import inflate_stream_cases as SC
import inflate_stream_fuzz as FZ
from biodemux_jl_amd import nativeio, synth
from test_device_gunzip_gpu import _inflate as _tagged
from test_device_gunzip_stream_gpu import BDX_E_INVALID, _case, _records, _stream, run_host, run_stream

pytestmark = pytest.mark.gpu

REFUSED_CAP = 70000


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    nativeio.build()


@contextlib.contextmanager
def _context(monkeypatch=None, cus=None):
    """a context of its own; cus: one that takes the device to have that many compute units (a grid of 16 * cus)"""
    cfg = H.bdx.DemuxConfig(bc_seqs=["ACGTACGT"], bc_lengths_no_N=[8], ids=["a"])
    if cus:
        monkeypatch.setenv("BDX_CU_COUNT", str(cus))
    c = H.bdx.HipClassifier(cfg)
    if cus:
        monkeypatch.delenv("BDX_CU_COUNT")
    try:
        yield c
    finally:
        c.close()


@pytest.fixture(scope="module")
def hc():
    with _context() as c:
        yield c


def _derived(name):
    return next(FZ.Good(c.name, c.data, plain, c, SC.CHUNKS) for c, plain in SC.derived_cases() if c.name == name)


def _arbiter_case(name):
    return dict(SC.arbiter_cases())[name]


def _good(hc, g, chunk, counters=True):
    rc, got, plen, info, err, intact = _stream(hc, g.data, chunk, len(g.plain))
    assert rc == 0 and intact, (g.name, chunk, err)
    assert plen == len(g.plain) and got == g.plain, (g.name, chunk)
    assert info[2] + info[3] + info[4] == info[1] - 1, (g.name, chunk, info)
    if counters:
        assert info == SC.expected_info(g.case, chunk), (g.name, chunk)
    return rc, got, plen, info


# ---- second laps ----
LAP_CHUNKS = (64, 256, 129)


def _lap_files():
    return [FZ.memlevel1(6), FZ.memlevel1(1), FZ.many_members(), _derived("every_block_type"), _derived("bgzf_chain")] + \
        [g for g in FZ.known(FZ.good_files()) if g.name.startswith("pigz")][:3]


@pytest.mark.parametrize("cus", [1, 7])
def test_every_workgroup_takes_more_than_one_item(monkeypatch, cus):
    grid = 16 * cus
    files = _lap_files()
    assert len(files) == 8
    laps = {}
    for g in files:
        for chunk in LAP_CHUNKS:
            segs, info = SC.chain(g.case, chunk)
            laps[g.name, chunk] = info[1] > 2 * grid and len(segs) > 2 * grid  # scan, decode and rest: at least two items each
    if cus == 1:
        for g in files[:3]:
            assert all(laps[g.name, chunk] for chunk in LAP_CHUNKS), g.name
    assert sum(laps.values()) >= 9, laps
    with _context(monkeypatch, cus) as c:
        for g in files:
            for chunk in LAP_CHUNKS:
                _good(c, g, chunk)


def test_a_lap_at_the_real_width(hc):
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    need = 64 * (16 * cus + 64)
    n = 4 * need
    g = FZ.memlevel1(6, n)
    while len(g.data) <= need:
        n *= 2
        g = FZ.memlevel1(6, n)
    assert -(-len(g.data) // 64) > 16 * cus  # more chunks than the scan's grid is wide
    rc, got, plen, info = _good(hc, g, 64, counters=False)
    assert info[0:2] == [1, -(-len(g.data) // 64)]
    assert info[2] > 500  # (small dynamic blocks: guesses that hold, by the hundred)


# ---- the chain run twice ----
def test_the_chain_runs_again_with_the_room_it_asked_for():
    g = FZ.many_members()
    tiny = _derived("tiny").data
    assert len(tiny) == 25 and SC.arbiter(tiny) == b"hello"
    with _context() as c:
        for chunk in (0, 4096):
            segs, info = SC.chain(g.case, chunk)
            assert len(segs) > 2 * info[1] + 1024, (chunk, len(segs))
            for _ in range(2):  # the list grows, a small file is content with it, the list is large enough already
                rc, got, plen, info = _good(c, g, chunk)
                assert info[0] == 1100
                rc, got, _, _, err, intact = _stream(c, tiny, chunk, 5)
                assert (rc, got, intact) == (0, b"hello", True), err


# ---- one context, many calls ----
def test_one_context_many_calls():
    l1, rnd = FZ.memlevel1(1), _derived("zlib_random")
    tiny, bad = _derived("tiny"), _arbiter_case("flipped_crc")
    assert SC.arbiter(bad) is None
    members = list(IC.good_members())

    def stream(c, data, chunk, cap):  # (bdx_last_error is the last FAILED call's text, errno's way: it counts when rc != 0)
        r = _stream(c, data, chunk, cap)
        return r[:4] + (r[4] if r[0] else "",) + r[5:]

    calls = [
        ("memlevel1_l1", lambda c: stream(c, l1.data, 64, len(l1.plain))),
        ("tiny", lambda c: stream(c, tiny.data, 0, len(tiny.plain))),
        ("flipped_crc", lambda c: stream(c, bad, 64, REFUSED_CAP)),
        ("no space", lambda c: stream(c, l1.data, 64, len(l1.plain) - 1)),
        ("tagged", lambda c: _tagged(c, members)),
        ("zlib_random", lambda c: stream(c, rnd.data, 0, len(rnd.plain))),
        ("memlevel1_l1 again", lambda c: stream(c, l1.data, 64, len(l1.plain))),
    ]
    with _context() as one:
        seen = [call(one) for _, call in calls]
    assert seen[0][:3] == (0, l1.plain, len(l1.plain)) and seen[0][3] == SC.expected_info(l1.case, 64) and seen[0][5]
    assert seen[1][:2] == (0, tiny.plain)
    assert seen[2][0] == BDX_E_INVALID and "CRC mismatch" in seen[2][4] and seen[2][5]
    assert seen[3][0] == SC.SPACE and seen[3][2] == len(l1.plain) and seen[3][5]
    rc, status, slots, intact, err = seen[4]
    assert rc == 0 and intact and not status.any() and slots == [m.plain for m in members], err  # its own reference
    assert seen[5][:3] == (0, rnd.plain, len(rnd.plain)) and seen[5][3] == SC.expected_info(rnd.case, 0) and seen[5][5]
    assert seen[6] == seen[0]
    for (name, call), got in zip(calls, seen):  # what the same call gives on a fresh context
        with _context() as fresh:
            want = call(fresh)
        if name == "tagged":
            assert want[0] == got[0] and want[1].tolist() == got[1].tolist() and want[2:4] == got[2:4], name
        else:
            assert want == got, name


# ---- the fixed slice of the corpus ----
def test_the_slice_is_the_one_the_sanitizer_driver_runs():
    files = FZ.slice_files()
    good, bad = FZ.fixed_slice()
    assert [f[0] for f in files] == [g.name for g in good] + [m.name for m in bad]
    assert all(name.split("/")[0].endswith(FZ.TAG) for name, _, _, _ in files)  # the seed is in every name
    assert len(good) == 100 and len(bad) == 300 and all(f[3] == (64,) for f in files[100:])


@pytest.mark.parametrize("part", range(4))
def test_fuzz_slice(hc, part):
    files = FZ.slice_files()
    follow = _derived("every_block_type")
    refused = accepted = 0
    for k, (name, data, want, chunks) in enumerate(files[part::4]):
        for chunk in chunks:
            cap = len(want) if want is not None else REFUSED_CAP
            rc, got, plen, info, err, intact = _stream(hc, data, chunk, cap)
            if want is None and rc == SC.SPACE:  # (its blocks are fine and long: its fault is in its bytes)
                assert plen > cap and intact, (name, chunk)
                rc, got, plen, info, err, intact = _stream(hc, data, chunk, plen)
            assert intact, (name, chunk)
            if want is None:
                assert rc == BDX_E_INVALID and "is refused: " in err, (name, chunk, rc, err)
                refused += 1
            else:
                assert rc == 0 and got == want, (name, chunk, err)
                assert info[2] + info[3] + info[4] == info[1] - 1, (name, chunk, info)
                accepted += 1
        if k % 50 == 49:
            _good(hc, follow, 64)
    assert refused >= 40 and accepted >= 75
    _good(hc, follow, 64)  # the context is fine afterwards


# ---- end to end ----
def _gunzipped(directory):
    out = {}
    for f in sorted(os.listdir(directory)):
        raw = open(os.path.join(directory, f), "rb").read()
        out[f] = gzip.decompress(raw) if f.endswith(".gz") else raw
    return out


def _pigz_like_gz(blob, cut, every=20000):
    """two members at memLevel 1, a sync flush every `every` bytes"""
    out = b""
    for part in (blob[:cut], blob[cut:]):
        z = zlib.compressobj(6, zlib.DEFLATED, 31, 1)
        out += b"".join(z.compress(part[p:p + every]) + z.flush(zlib.Z_SYNC_FLUSH) for p in range(0, len(part), every)) + z.flush()
    assert gzip.decompress(out) == blob
    return out


def test_flushed_two_member_input_and_every_gzip_output(tmp_path):
    blob, bc = _case(tmp_path)
    fq = str(tmp_path / "reads.fastq.gz")
    open(fq, "wb").write(_pigz_like_gz(blob, len(blob) // 2 + 7))
    kw = dict(max_error_rate=0.2, trim_side=5, _batch_reads=700)
    a = run_host(fq, bc, str(tmp_path / "host"), **kw)
    want = _gunzipped(str(tmp_path / "host"))
    assert a.total_reads == 3000 and want and all(f.endswith(".gz") for f in want)
    for tag, extra in (("writers", {}), ("device", dict(_gzip="device")), ("device2", dict(_gzip="device", _gzip_level=2))):
        tm = {}
        b = run_stream(fq, bc, str(tmp_path / tag), _timings=tm, **extra, **kw)
        assert vars(a) == vars(b), tag
        assert _gunzipped(str(tmp_path / tag)) == want, tag
        assert tm["stream_members"] == 2 and tm["plain_in_bytes"] == len(blob)


def _both(tmp_path, inputs, bc, **kw):
    """host leg and stream leg: both refuse, or both give the same stats and files -> the stats, the stream leg's timings"""
    tm, got = {}, []
    for tag, run in (("host", run_host), ("stream", run_stream)):
        try:
            got.append(vars(run(*inputs, bc, str(tmp_path / tag), gzip_output=False, **(dict(_timings=tm) if tag == "stream" else {}), **kw)))
        except Exception:  # noqa: BLE001 - refused, by whichever layer
            got.append(None)
    assert got[0] == got[1], got
    if isinstance(got[0], dict):
        assert _gunzipped(str(tmp_path / "host")) == _gunzipped(str(tmp_path / "stream"))
    return got[0], tm


def test_resident_text_edges(tmp_path):
    blob, bc = _case(tmp_path, n=300)
    for name, text, kw, reads in (
            ("empty", b"", {}, 0),
            ("no_final_newline", blob[:-1], {}, 300),
            ("one_long_read", _records([b"ACGT" * 50000]) + blob, dict(_batch_reads=1), 301)):  # longer than the first window
        d = tmp_path / name
        d.mkdir()
        fq = str(d / "reads.fastq.gz")
        open(fq, "wb").write(gzip.compress(text, 6))
        stats, _ = _both(d, (fq,), bc, max_error_rate=0.2, **kw)
        if isinstance(stats, dict):
            assert stats["total_reads"] == reads, name
        else:
            assert name == "empty", (name, stats)  # (only a file without a read may be refused, by both legs alike)


def test_paired_both_gz_with_unequal_record_counts(tmp_path):
    bcs = synth.make_barcodes(5, 12, seed=6, min_hamming=4)
    seq, off, _ = synth.make_reads(bcs, 500, 60, seed=6)
    bc = tmp_path / "bc.csv"
    bc.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"b{i},{b},{'B' * len(b)}\n" for i, b in enumerate(bcs)))
    f1, f2 = str(tmp_path / "x_R1.fastq.gz"), str(tmp_path / "x_R2.fastq.gz")
    open(f1, "wb").write(gzip.compress(_records([seq[off[i]:off[i + 1]].tobytes() for i in range(500)]), 6))
    open(f2, "wb").write(_pigz_like_gz(_records([b"ACGT" * 10 for _ in range(430)]), 9000, every=3000))
    stats, _ = _both(tmp_path, (f1, f2), str(bc), classify_both=True, trim_side=3, _batch_reads=128)
    assert isinstance(stats, dict) and stats["total_reads"] == 430


def test_both_sides_of_the_capacity_guess(tmp_path):
    """_ResidentText.prepare guesses four times the compressed size: a text that deflates better needs the second call"""
    rng = np.random.default_rng(11)
    bcs = synth.make_barcodes(4, 12, seed=8, min_hamming=4)
    bc = tmp_path / "bc.csv"
    bc.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"b{i},{b},{'B' * len(b)}\n" for i, b in enumerate(bcs)))
    seq, off, _ = synth.make_reads(bcs, 40, 80, seed=8)
    few = [seq[off[i]:off[i + 1]].tobytes() for i in range(40)]
    dense = b"".join(b"@r\n" + few[i % 40] + b"\n+\n" + b"I" * 80 + b"\n" for i in range(2000))  # repeated reads, one quality
    seq, off, _ = synth.make_reads(bcs, 2000, 80, seed=9)
    quals = rng.integers(33, 127, (2000, 80), dtype=np.uint8)
    quals[quals == ord("@")] = ord("A")
    loose = b"".join(b"@r%d\n" % i + seq[off[i]:off[i + 1]].tobytes() + b"\n+\n" + quals[i].tobytes() + b"\n" for i in range(2000))
    for name, text, more in (("dense", dense, True), ("loose", loose, False)):
        d = tmp_path / name
        d.mkdir()
        fq = str(d / "reads.fastq.gz")
        open(fq, "wb").write(gzip.compress(text, 6))
        stats, tm = _both(d, (fq,), str(bc), max_error_rate=0.2)
        assert isinstance(stats, dict) and stats["total_reads"] == 2000
        assert tm["plain_in_bytes"] == len(text) and tm["compressed_in_bytes"] == os.path.getsize(fq)
        assert (tm["plain_in_bytes"] > 4 * tm["compressed_in_bytes"]) == more, (name, tm["plain_in_bytes"], tm["compressed_in_bytes"])
        assert tm["plain_in_bytes"] != 4 * tm["compressed_in_bytes"]
