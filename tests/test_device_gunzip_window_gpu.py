"""The windowed stream inflate (bdx_fq_inflate_window_*, csrc/bdx_inflate_window_core.h) on the MI355X, at chunk 64 and
windows of 256 bytes to 4 KiB on files of at most a few hundred KB: a cut goes wrong at these sizes exactly as at 256 MiB.
zlib says what every file gives; a refusal is the one the plain C++ build (tests/inflate_window_host.cpp) gives under the
same schedule.  Then execute_demultiplexing(..., _io="device", _gunzip="device-window") against _gunzip="host".

The reference's demo2 files are one deflate block of some 5.4 KB each (31 392 bytes of text): a window cannot stop inside a
block, so they go through in a few windows that double (no progress, then longer) and their whole text appears at once.
They are held to the host inflate and the golden outputs; that a run takes at least 10 windows and keeps less than half of
its text is asserted on the synthetic file, whose blocks are small."""
import ctypes as C
import functools
import gzip
import os
import re
import zlib

import numpy as np
import pytest

import helpers as H
import inflate_cases as IC
import inflate_stream_cases as SC
import inflate_stream_fuzz as FZ
import inflate_window_cases as WC
from biodemux_jl_amd import deviceio, nativeio, synth
from biodemux_jl_amd.hipabi import BdxError

pytestmark = pytest.mark.gpu

run_host = functools.partial(H.bdx.execute_demultiplexing, _io="device", _gunzip="host")
run_stream = functools.partial(H.bdx.execute_demultiplexing, _io="device", _gunzip="device-stream")
run_window = functools.partial(H.bdx.execute_demultiplexing, _io="device", _gunzip="device-window")
CANARY, GUARD, LEAD = 0xC5, 64, 3
BDX_E_INVALID, BDX_E_STATE = -1, -3
REFUSED_CAP = 1 << 19


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    nativeio.build()


def _classifier():
    return H.bdx.HipClassifier(H.bdx.DemuxConfig(bc_seqs=["ACGTACGT"], bc_lengths_no_N=[8], ids=["a"]))


@pytest.fixture(scope="module")
def hc():
    c = _classifier()
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return WC.Host(tmp_path_factory.mktemp("infw_host_gpu"))


class GpuWindow:
    """a window object of the library with HostWindow's feed: the compressed bytes LEAD bytes into a tensor that ends with
    their last byte, d_out[0, cap) between two guards; a refusal comes back as the core's status, member and byte"""

    def __init__(self, hc, chunk=64):
        self.hc, self.w = hc, C.c_void_p()
        assert hc.lib.bdx_fq_inflate_window_open(hc.h, chunk, C.byref(self.w)) == 0, hc.lib.bdx_last_error(hc.h)
        self.info = None

    def feed(self, data: bytes, last: int, chunk: int, cap: int):
        import torch

        hc = self.hc
        d_comp = torch.from_numpy(np.frombuffer(b"\0" * LEAD + data, dtype=np.uint8).copy()).to("cuda:0")
        d_out = torch.full((cap + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        used, plen, info = C.c_int64(-1), C.c_int64(-1), np.full(8, -1, dtype=np.int64)
        rc = hc.lib.bdx_fq_inflate_window_feed(self.w, d_comp.data_ptr() + LEAD, len(data), last, d_out.data_ptr() + GUARD, cap, C.byref(used),
                                               C.byref(plen), info.ctypes.data)
        self.info = info.tolist()
        out = d_out.cpu().numpy()
        n = plen.value if rc == 0 else 0
        keep = np.ones(len(out), dtype=bool)
        keep[GUARD:GUARD + (cap if rc == BDX_E_INVALID else n)] = False  # (a refused window leaves d_out[0, cap) unspecified)
        clean = bool((out[keep] == CANARY).all())
        member = at = -1
        if rc == BDX_E_INVALID:
            err = hc.lib.bdx_last_error(hc.h).decode()
            m = re.search(r"gzip member (\d+) \(near compressed byte (\d+)\) is refused: (.+) \(status (\d+)\)", err)
            assert m and m.group(3) in set(IC.STATUS.values()) - {"ok"}, err
            rc, member, at = int(m.group(4)), int(m.group(1)), int(m.group(2))
        return rc, used.value, plen.value, out[GUARD:GUARD + n].tobytes(), member, at, clean

    def close(self):
        if self.w:
            assert self.hc.lib.bdx_fq_inflate_window_close(self.w) == 0
        self.w = None


def _cap(want):
    return len(want) if want is not None else REFUSED_CAP


# ---- the fixed slice ----
@pytest.mark.parametrize("part", range(4))
def test_the_fixed_slice_under_a_seeded_schedule(hc, host, part):
    files = FZ.slice_files()
    assert len(files) >= 400
    refused = 0
    for k, (name, data, want, _) in list(enumerate(files))[part::4]:
        sizes = WC.schedule(WC.SEED + 30000 + k, len(data), lo=64, hi=4096)
        w = GpuWindow(hc)
        got = WC.run_schedule(w, data, sizes, 64, _cap(want))
        w.close()
        assert WC.verdict_ok(want, got[0], got[1], got[2], got[3], len(data)), (name, got[0], got[2:])
        if want is None:
            h = host.open()
            assert got == WC.run_schedule(h, data, sizes, 64, _cap(want)), name  # status, member, byte, windows
            h.close()
            refused += 1
    assert refused >= 20


# ---- the named edges ----
def test_matches_whose_source_lies_in_the_windows_before(hc):
    data, plain, marks = WC.history_file()
    cuts, lens = WC.history_cuts()
    w = GpuWindow(hc)
    rc, text, log, _, _ = WC.feed_cuts(w, data, cuts, 64, len(plain))
    w.close()
    assert rc == 0 and text == plain and [x[3] for x in log] == lens, log


def test_the_trailer_cuts_no_progress_and_space(hc, host):
    case, plain = dict((c.name, (c, p)) for c, p in SC.derived_cases())["every_block_type"]
    off, body, _ = case.members[-1]
    end = off + len(body)
    for i in range(9):  # inside the trailer at each of its bytes, and right behind it
        w = GpuWindow(hc)
        rc, used, plen, got, _, _, clean = w.feed(case.data[:end + i], 0, 64, len(plain))
        assert rc == 0 and got == plain and clean and used == (end + 8 if i == 8 else used) and used >= end - 1, (i, rc, used)
        rc, used2, plen, _, _, _, clean = w.feed(case.data[used:], 1, 64, 0)
        assert (rc, used2, plen, clean) == (0, len(case.data) - used, 0, True), i
        w.close()
    bad = bytearray(case.data)
    bad[end + 1] ^= 2  # the CRC, found by the window that holds the trailer alone
    w = GpuWindow(hc)
    rc, used, _, got, _, _, _ = w.feed(bytes(bad[:end + 3]), 0, 64, len(plain))
    assert rc == 0 and got == plain
    rc, _, _, _, member, at, _ = w.feed(bytes(bad[used:]), 1, 64, 0)
    assert (rc, member, at) == (10, 0, 0)
    assert w.feed(b"", 1, 64, 0)[0] == BDX_E_STATE  # dead
    w.close()
    # no progress, then longer; BDX_E_SPACE, then the room it asked for: what the plain C++ build gives, call by call
    data, hplain, marks = WC.history_file()
    a, b = marks["far"], marks["far2"]
    w, h = GpuWindow(hc), host.open()
    for piece, last, cap in ((data[:5], 0, 0), (data[:17], 0, 0), (data[:a], 0, 39999), (data[:a], 0, 40000), (data[a:a + 3], 0, 10),
                             (data[a:b + 1], 0, 0), (data[a:b + 1], 0, 363), (data[a:b + 1], 0, 364)):
        x, y = w.feed(piece, last, 64, cap), h.feed(piece, last, 64, cap)
        assert x[:6] == y[:6] and x[6], (len(piece), cap, x[:3], y[:3])
    assert x[0] == 0 and x[2] == 364
    rest = data[a + x[1]:]
    x, y = w.feed(rest, 1, 64, 1000), h.feed(rest, 1, 64, 1000)
    assert x[:6] == y[:6] and x[0] == 0 and hplain.endswith(x[3])
    w.close()
    h.close()


# ---- long files ----
def test_a_member_over_many_windows_of_1_kib(hc):
    g = FZ.memlevel1(6)
    w = GpuWindow(hc)
    rc, text, _, _, wins = WC.run_schedule(w, g.data, [1024] * (len(g.data) // 1024 + 1), 64, len(g.plain))
    w.close()
    assert rc == 0 and text == g.plain and wins >= len(g.data) // 1100 >= 20, wins


def test_many_members_in_windows_of_4_kib_at_the_default_chunk(hc):
    g = FZ.many_members()
    w = GpuWindow(hc, chunk=0)
    members = 0
    pos, text = 0, []
    while True:  # (the chain runs twice inside a window: more segments than its first room)
        piece = g.data[pos:pos + 4096]
        last = int(pos + len(piece) == len(g.data))
        rc, used, plen, got, _, _, clean = w.feed(piece, last, 0, len(g.plain))
        assert rc == 0 and clean and (used or last), pos
        members += w.info[0]
        text.append(got)
        pos += used
        if last:
            break
    w.close()
    assert b"".join(text) == g.plain and members == 1100


# ---- two objects on one context ----
def test_two_objects_interleaved_and_a_dead_one_beside_a_live_one(hc):
    a, b = FZ.memlevel1(6), FZ.memlevel1(1)
    bad = bytearray(b.data)
    bad[len(bad) // 2] ^= 0x20
    bad = bytes(bad)
    assert SC.arbiter(bad) is None
    for second, want in ((b.data, b.plain), (bad, None)):
        wa, wb = GpuWindow(hc), GpuWindow(hc)
        pa = pb = 0
        ta, tb, rb = [], [], 0
        while pa < len(a.data) or (pb < len(second) and rb == 0):
            if pa < len(a.data):
                piece = a.data[pa:pa + 3000]
                rc, used, _, got, _, _, clean = wa.feed(piece, int(pa + len(piece) == len(a.data)), 64, len(a.plain))
                assert rc == 0 and clean and used > 0
                ta.append(got)
                pa += used
            if pb < len(second) and rb == 0:
                piece = second[pb:pb + 2500]
                rb, used, _, got, member, _, clean = wb.feed(piece, int(pb + len(piece) == len(second)), 64, len(b.plain) + 70000)
                assert clean and (rb or used > 0)
                tb.append(got)
                pb += used
        assert b"".join(ta) == a.plain
        if want is None:
            assert 1 <= rb <= 11 and member == 0 and wb.feed(b"", 1, 64, 0)[0] == BDX_E_STATE
        else:
            assert rb == 0 and b"".join(tb) == want
        wa.close()
        wb.close()


def test_an_object_opened_on_one_stream_is_fed_on_another(hc):
    """as the pipeline does: open on the context's own stream, then the context is given a fresh non-blocking stream
    that nothing orders behind the first.  open has finished the carried state before it returns."""
    rt = deviceio._Runtime(hc.lib)
    g = FZ.memlevel1(1)
    for _ in range(8):
        w = GpuWindow(hc)
        s = rt.stream()
        hc.set_stream(s)
        try:
            rc, text, _, _, wins = WC.run_schedule(w, g.data, [8192] * 3, 64, len(g.plain))
            w.close()
        finally:
            hc.set_stream(None)
            rt.hipStreamDestroy(s)
        assert rc == 0 and text == g.plain and wins >= 4


# ---- narrow grids ----
def test_a_grid_of_16_takes_several_items_a_workgroup(monkeypatch):
    monkeypatch.setenv("BDX_CU_COUNT", "1")
    c = _classifier()
    try:
        g = FZ.memlevel1(6)
        assert len(SC.chain(g.case, 64)[0]) > 8 * 16  # segments of the whole file: a window of a quarter has more than 2 * 16
        w = GpuWindow(c)
        quarter = len(g.data) // 4 + 1
        rc, text, _, _, wins = WC.run_schedule(w, g.data, [quarter] * 4, 64, len(g.plain))
        w.close()
        assert rc == 0 and text == g.plain and 4 <= wins <= 6
        data, plain, _ = WC.history_file()
        w = GpuWindow(c)
        rc, text, log, _, _ = WC.feed_cuts(w, data, WC.history_cuts()[0], 64, len(plain))
        w.close()
        assert rc == 0 and text == plain
    finally:
        c.close()


# ---- end to end ----
def _same_dirs(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb and fa
    for f in fa:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f


@pytest.mark.parametrize("window, batch", [(1024, 37), (1024, 128), (4096, 37), (4096, 128)])
def test_demo2_gz_fixtures_equal_the_host_inflate_and_the_golden_outputs(tmp_path, monkeypatch, window, batch):
    monkeypatch.setattr(deviceio, "STREAM_CHUNK", 64)
    seen = []

    def run(*a, **kw):
        tm = {}
        out = run_window(*a, _gunzip_window=window, _batch_reads=batch, _timings=tm, **kw)
        seen.append(tm)
        return out

    assert H.scenario_demo2(run, str(tmp_path / "window")) == 76  # (byte-identical to results/demo2)
    assert H.scenario_demo2(run_host, str(tmp_path / "host")) == 76
    _same_dirs(str(tmp_path / "window"), str(tmp_path / "host"))
    for tm in seen:  # two inputs a run, each one block: the header, then windows that double up to the block
        assert tm["stream_windows"] >= 2 * 2 and tm["stream_members"] == 2 and tm["stream_window_bytes"] == window
        assert tm["plain_in_bytes"] == 2 * 31392


def _records(seqs):
    return b"".join(b"@r%d some header\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n" for i, s in enumerate(seqs))


def _small_blocks(blob: bytes, level=6) -> bytes:
    """one gzip member of many small dynamic blocks (memLevel 1)"""
    z = zlib.compressobj(level, zlib.DEFLATED, 31, 1)
    return z.compress(blob) + z.flush()


@functools.lru_cache(maxsize=None)
def _ragged(n=700, seed=5, lo=100, hi=500):
    bcs = synth.make_barcodes(6, 12, seed=seed, min_hamming=4)
    seq, off, _ = synth.make_ragged_reads(bcs, n, lo, hi, seed=seed)
    blob = _records([seq[off[i]:off[i + 1]].tobytes() for i in range(n)])
    table = "ID,Full_seq,Full_annotation\n" + "".join(f"b{i},{b},{'B' * len(b)}\n" for i, b in enumerate(bcs))
    return blob, table


def _case(tmp_path, **kw):
    blob, table = _ragged(**kw)
    bc = tmp_path / "bc.csv"
    bc.write_text(table)
    return blob, str(bc)


@pytest.mark.parametrize("window, batch", [(1024, 37), (1024, 128), (4096, 37), (4096, 128)])
def test_700_ragged_reads_in_one_member(tmp_path, monkeypatch, window, batch):
    blob, bc = _case(tmp_path)
    fq = str(tmp_path / "reads.fastq.gz")
    open(fq, "wb").write(_small_blocks(blob))
    assert SC.arbiter(open(fq, "rb").read()) == blob
    monkeypatch.setattr(deviceio, "STREAM_CHUNK", 64)
    kw = dict(max_error_rate=0.2, trim_side=5, gzip_output=False, _batch_reads=batch)
    tw = {}
    a = run_host(fq, bc, str(tmp_path / "host"), **kw)
    b = run_window(fq, bc, str(tmp_path / "window"), _gunzip_window=window, _timings=tw, **kw)
    _same_dirs(str(tmp_path / "host"), str(tmp_path / "window"))
    assert vars(a) == vars(b) and a.total_reads == 700 and tw["batches"] >= 700 // batch
    assert tw["stream_windows"] >= 10 and tw["stream_text_peak_bytes"] < len(blob) // 2, (tw["stream_windows"], tw["stream_text_peak_bytes"], len(blob))
    assert tw["compressed_in_bytes"] == os.path.getsize(fq) and tw["plain_in_bytes"] == len(blob) and tw["stream_members"] == 1
    assert tw["stream_window_bytes"] == window and tw["inflate_s"] > 0


def test_modes_untouched_and_a_plain_input(tmp_path, monkeypatch):
    blob, bc = _case(tmp_path)
    fq, plain = str(tmp_path / "reads.fastq.gz"), str(tmp_path / "plain.fastq")
    open(fq, "wb").write(gzip.compress(blob, 6))
    open(plain, "wb").write(blob)
    monkeypatch.setattr(deviceio, "STREAM_CHUNK", 64)
    kw = dict(max_error_rate=0.2, trim_side=5, gzip_output=False, _batch_reads=128)
    ts, th, tp = {}, {}, {}
    a = run_host(fq, bc, str(tmp_path / "host"), _timings=th, **kw)
    b = run_stream(fq, bc, str(tmp_path / "stream"), _timings=ts, **kw)
    c = run_window(fq, bc, str(tmp_path / "window"), _gunzip_window=4096, **kw)
    d = run_window(plain, bc, str(tmp_path / "plain_out"), _timings=tp, output_prefix="reads", **kw)  # inert
    for other in ("stream", "window", "plain_out"):
        _same_dirs(str(tmp_path / "host"), str(tmp_path / other))
    assert vars(a) == vars(b) == vars(c) == vars(d)
    assert "stream_windows" not in ts and "stream_windows" not in th and "inflate_s" not in th and "inflate_s" not in tp
    assert ts["stream_members"] == 1 and ts["plain_in_bytes"] == len(blob)


def test_paired_inputs_and_gzip_output(tmp_path, monkeypatch):
    bcs = synth.make_barcodes(5, 12, seed=6, min_hamming=4)
    seq, off, _ = synth.make_reads(bcs, 500, 60, seed=6)
    bc = tmp_path / "bc.csv"
    bc.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"b{i},{b},{'B' * len(b)}\n" for i, b in enumerate(bcs)))
    r1 = _records([seq[off[i]:off[i + 1]].tobytes() for i in range(500)])
    r2 = _records([b"ACGT" * 10 for _ in range(430)])
    monkeypatch.setattr(deviceio, "STREAM_CHUNK", 64)
    kw = dict(classify_both=True, trim_side=3, _batch_reads=128, gzip_output=False)
    for tag, second in (("plain", ("x_R2.fastq", r2)), ("gz", ("x_R2.fastq.gz", _small_blocks(r2, 1)))):
        d = tmp_path / tag
        d.mkdir()
        f1, f2 = str(d / "x_R1.fastq.gz"), str(d / second[0])
        open(f1, "wb").write(_small_blocks(r1))
        open(f2, "wb").write(second[1])
        a = run_host(f1, f2, str(bc), str(d / "host"), **kw)
        b = run_window(f1, f2, str(bc), str(d / "window"), _gunzip_window=1024, **kw)
        _same_dirs(str(d / "host"), str(d / "window"))
        assert vars(a) == vars(b) and a.total_reads == 430  # (different record counts: the shorter file ends the run)
    # .gz in -> _gzip="device" out: the files gunzip to the same bytes
    d = tmp_path / "gzout"
    d.mkdir()
    f1 = str(d / "reads.fastq.gz")
    open(f1, "wb").write(_small_blocks(r1))
    kw = dict(trim_side=3, _batch_reads=128, gzip_output=True)
    a = run_host(f1, str(bc), str(d / "host"), **kw)
    b = run_window(f1, str(bc), str(d / "window"), _gunzip_window=1024, _gzip="device", _gzip_level=2, **kw)
    assert vars(a) == vars(b)
    fa = sorted(os.listdir(d / "host"))
    assert fa == sorted(os.listdir(d / "window")) and fa
    for f in fa:
        assert gzip.open(d / "host" / f).read() == gzip.open(d / "window" / f).read(), f


def test_a_record_longer_than_a_windows_text(tmp_path, monkeypatch):
    blob, bc = _case(tmp_path, n=60)
    long_read = bytes(np.random.default_rng(3).choice(np.frombuffer(b"ACGT", dtype=np.uint8), 150000))
    blob = blob[:len(blob) // 2 + 3]
    blob = blob[:blob.rindex(b"\n@r") + 1] + _records([long_read]) + _ragged(n=60)[0]
    fq = str(tmp_path / "reads.fastq.gz")
    open(fq, "wb").write(_small_blocks(blob))
    monkeypatch.setattr(deviceio, "STREAM_CHUNK", 64)
    kw = dict(max_error_rate=0.2, gzip_output=False, _batch_reads=37)
    tw = {}
    a = run_host(fq, bc, str(tmp_path / "host"), **kw)
    b = run_window(fq, bc, str(tmp_path / "window"), _gunzip_window=1024, _timings=tw, **kw)
    _same_dirs(str(tmp_path / "host"), str(tmp_path / "window"))
    assert vars(a) == vars(b) and tw["stream_windows"] >= 10 and tw["plain_in_bytes"] == len(blob)


def test_a_refusal_in_the_third_member_names_the_file_the_member_and_the_reason(tmp_path, monkeypatch):
    blob, bc = _case(tmp_path)
    third = len(blob) // 3
    cut = [blob.index(b"\n@r", third) + 1, blob.index(b"\n@r", 2 * third) + 1]
    parts = [_small_blocks(p) for p in (blob[:cut[0]], blob[cut[0]:cut[1]], blob[cut[1]:])]
    bad = bytearray(parts[2])
    bad[-8] ^= 1  # the third member's CRC
    fq = str(tmp_path / "bad_crc.fastq.gz")
    open(fq, "wb").write(parts[0] + parts[1] + bytes(bad))
    monkeypatch.setattr(deviceio, "STREAM_CHUNK", 64)
    out = tmp_path / "out"
    with pytest.raises(BdxError, match=r"bad_crc\.fastq\.gz: .*gzip member 2 \(near compressed byte %d\).*CRC mismatch" % (len(parts[0]) + len(parts[1]))):
        run_window(fq, bc, str(out), max_error_rate=0.2, gzip_output=False, _gunzip_window=1024, _batch_reads=37)
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) > 0  # known at the member's end only: earlier text was written
