"""The opt-in FASTQ checks on the MI355X: bdx_fq_check_device and bdx_fq_check_pair_device against the restatement of
tests/fastq_check_cases.py on every case (which tests/test_fastq_check_cpu.py holds to the host library), texts at five
offsets inside larger buffers, every refusal and a correct call after it; _check=True through _io="device" in every input
mode and through _io="device-deal": the goldens unchanged, the failing texts of the CPU tests with the messages of
_io="native".

Nothing here provokes a fault: every "bad" input is well-formed memory with wrong bytes in it, every text lies at least
64 bytes inside its device buffer, and the tampered line tables point at most a few bytes behind the text, into that padding."""
import ctypes as C
import functools
import gzip
import os

import numpy as np
import pytest

import fastq_cases as FC
import fastq_check_cases as CC
import helpers as H
import test_fastq_check_cpu as CPU
from biodemux_jl_amd import hipabi, nativeio

pytestmark = pytest.mark.gpu

PAD = 64
FRONTS = (0, 1, 5, 15, 16)
run_dev = functools.partial(H.bdx.execute_demultiplexing, _io="device")
run_nat = functools.partial(H.bdx.execute_demultiplexing, _io="native")
run_deal = functools.partial(H.bdx.execute_demultiplexing, _io="device-deal", devices=[0, 0])


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    nativeio.build()


@pytest.fixture(scope="module")
def hc():
    cfg = H.bdx.DemuxConfig(bc_seqs=["ACGTACGT"], bc_lengths_no_N=[8], ids=["a"])
    with H.bdx.HipClassifier(cfg) as ctx:
        yield ctx


def _dev(arr):
    import torch

    t = torch.from_numpy(np.array(arr, copy=True)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _err(ctx):
    return ctx.lib.bdx_last_error(ctx.h).decode()


class Text:
    """a text PAD + `front` bytes into a device buffer whose other bytes are a canary pattern"""

    def __init__(self, text, front=0):
        t = FC._u8(text)
        self.n, self.lead = len(t), PAD + front
        self.host = np.concatenate([self.canary(self.lead), t, self.canary(PAD)])
        self.buf = _dev(self.host)
        self.ptr = self.buf.data_ptr() + self.lead

    @staticmethod
    def canary(n):
        return ((np.arange(n, dtype=np.int64) * 31 + 7) % 251).astype(np.uint8)

    def untouched(self):
        return np.array_equal(self.buf.cpu().numpy(), self.host)


class Table:
    """a line table on the device; `shift`: entries in front of it, so that its address is no multiple of 16"""

    def __init__(self, off, ln, shift=0):
        self.off = _dev(np.concatenate([np.zeros(shift, np.int64), np.asarray(off, dtype=np.int64)]))
        self.len = _dev(np.concatenate([np.zeros(shift, np.int32), np.asarray(ln, dtype=np.int32)]))
        self.shift = shift

    def at(self, record):
        return self.off.data_ptr() + 8 * (self.shift + 4 * record), self.len.data_ptr() + 4 * (self.shift + 4 * record)


def _check(ctx, d, tb, start, count, rules):
    bad, broken = C.c_int64(-7), C.c_int32(-7)
    o, l = tb.at(start)
    rc = ctx.lib.bdx_fq_check_device(ctx.h, d.ptr, d.n, o, l, count, rules, C.byref(bad), C.byref(broken))
    assert rc == 0, _err(ctx)
    return bad.value, broken.value


def _check_pair(ctx, d1, tb1, d2, tb2, start, count):
    bad = C.c_int64(-7)
    (o1, l1), (o2, l2) = tb1.at(start), tb2.at(start)
    rc = ctx.lib.bdx_fq_check_pair_device(ctx.h, d1.ptr, d1.n, o1, l1, d2.ptr, d2.n, o2, l2, count, C.byref(bad))
    assert rc == 0, _err(ctx)
    return bad.value


# ---- the two entries against the restatement ----
@pytest.mark.parametrize("c", CC.check_cases(), ids=lambda c: c.name)
def test_check_equals_the_restatement(hc, c):
    """every rules mask, every failing record (walk), both table alignments (16-byte loads or not), five text offsets"""
    masks = CC.ref_masks(c.text, c.off, c.len, c.n)
    for front in FRONTS:
        d = Text(c.text, front)
        for shift in (0, 1) if front in (0, 5) else (0,):
            tb = Table(c.off, c.len, shift)
            assert (tb.at(0)[0] % 16 == 0) == (shift == 0)
            for rules in CC.MASKS:
                got = CC.walk(lambda s, k: _check(hc, d, tb, s, k, rules), c.n)
                assert got == CC.expected_walk(masks, rules), (front, shift, rules)
        assert d.untouched()


def test_check_of_the_big_cases(hc):
    for c in CC.big_check_cases():
        masks = CC.ref_masks(c.text, c.off, c.len, c.n)
        d, tb = Text(c.text, 5), Table(c.off, c.len)
        for rules in (7, 1, 6):
            got = CC.walk(lambda s, k: _check(hc, d, tb, s, k, rules), c.n)
            assert got == CC.expected_walk(masks, rules), (c.name, rules)
        tb = Table(c.off, c.len, 1)
        assert _check(hc, d, tb, 0, c.n, 7) == CC.ref_check(c.text, c.off, c.len, c.n, 7), c.name
        assert d.untouched()


@pytest.mark.parametrize("c", CC.name_cases(), ids=lambda c: c.name)
def test_pair_check_equals_the_restatement(hc, c):
    want = np.flatnonzero(CC.ref_pair_flags(c.text1, c.off1, c.len1, c.text2, c.off2, c.len2, c.n)).tolist()
    tb1, tb2 = Table(c.off1, c.len1), Table(c.off2, c.len2, 3)
    for f1, f2 in zip(FRONTS, FRONTS[::-1]) if c.n <= 4096 else ((5, 16),):
        d1, d2 = Text(c.text1, f1), Text(c.text2, f2)
        got = CC.walk(lambda s, k: (_check_pair(hc, d1, tb1, d2, tb2, s, k), 0), c.n)
        assert [i for i, _ in got] == want, (f1, f2)
        # the pair rule is symmetric
        assert _check_pair(hc, d2, tb2, d1, tb1, 0, c.n) == (want[0] if want else -1)
        assert d1.untouched() and d2.untouched()


def test_device_equals_host_library(hc, tmp_path):
    """each device step has the contract of a host function of bdx_io.cpp: the same calls on both"""
    for c in (CC.check_cases()[-1], CC.check_cases()[5]):
        f = FC.host_open(tmp_path / ("%s.fastq" % c.name), c.text)
        try:
            d, tb = Text(c.text), Table(c.off, c.len)
            for rules in CC.MASKS:
                assert _check(hc, d, tb, 0, c.n, rules) == f.check(c.off, c.len, c.n, rules, 4)
        finally:
            f.close()
    c = next(c for c in CC.name_cases() if c.name == "suffixes")
    f1, f2 = FC.host_open(tmp_path / "a.fastq", c.text1), FC.host_open(tmp_path / "b.fastq", c.text2)
    try:
        d1, d2, tb1, tb2 = Text(c.text1), Text(c.text2), Table(c.off1, c.len1), Table(c.off2, c.len2)
        for s in range(c.n):
            assert _check_pair(hc, d1, tb1, d2, tb2, s, c.n - s) == f1.check_pair(c.off1[4 * s:], c.len1[4 * s:], f2, c.off2[4 * s:], c.len2[4 * s:], c.n - s, 2)
    finally:
        f1.close()
        f2.close()


# ---- refusals ----
def test_refusals_and_a_correct_call_after_each(hc):
    c = next(c for c in CC.check_cases() if c.name == "breaks_7")
    d, tb = Text(c.text), Table(c.off, c.len)
    o, l = tb.at(0)
    lib, h = hc.lib, hc.h
    want = CC.ref_check(c.text, c.off, c.len, c.n, 7)
    assert want == (4, 7)

    def refused(rc, message):
        assert rc == -1 and message in _err(hc), (rc, _err(hc))
        assert _check(hc, d, tb, 0, c.n, 7) == want and _check_pair(hc, d, tb, d, tb, 0, c.n) == -1

    bad, broken = C.c_int64(5), C.c_int32(5)
    args = (C.byref(bad), C.byref(broken))
    refused(lib.bdx_fq_check_device(h, d.ptr, d.n, o, l, c.n, 7, None, C.byref(broken)), "first_bad / broken is NULL")
    refused(lib.bdx_fq_check_device(h, d.ptr, d.n, o, l, c.n, 7, C.byref(bad), None), "first_bad / broken is NULL")
    for ptrs in ((None, o, l), (d.ptr, None, l), (d.ptr, o, None)):
        refused(lib.bdx_fq_check_device(h, ptrs[0], d.n, ptrs[1], ptrs[2], c.n, 7, *args), "NULL device pointer")
        assert (bad.value, broken.value) == (-1, 0)
    refused(lib.bdx_fq_check_device(h, d.ptr, -1, o, l, c.n, 7, *args), "n / text_len is negative")
    refused(lib.bdx_fq_check_device(h, d.ptr, d.n, o, l, -1, 7, *args), "n / text_len is negative")
    for rules in (0, 8, 15, -1, 1 << 30):
        refused(lib.bdx_fq_check_device(h, d.ptr, d.n, o, l, c.n, rules, *args), "rules must be a mask of 1, 2 and 4")
    refused(lib.bdx_fq_check_device(h, d.ptr, d.n, o, l, 1 << 32, 7, *args), "more than 2^32 - 1 records")
    assert lib.bdx_fq_check_device(h, d.ptr, d.n, o, l, 0, 7, *args) == 0 and (bad.value, broken.value) == (-1, 0)
    assert lib.bdx_fq_check_device(h, None, 0, None, None, 0, 7, *args) == 0
    # a line outside its text: each of the four lines in turn; the text is cut short by a byte, or a line reaches a byte
    # beyond it, or a length is negative (everything the kernel could read lies inside the buffer's padding)
    for k in range(4):
        off, ln = c.off.copy(), c.len.copy()
        ln[4 * 2 + k] += len(c.text) - int(off[4 * 2 + k] + ln[4 * 2 + k]) + 1
        t = Table(off, ln)
        refused(lib.bdx_fq_check_device(h, d.ptr, d.n, *t.at(0), c.n, 7, *args), "a line of the line table lies outside the text")
        assert (bad.value, broken.value) == (-1, 0)
        ln = c.len.copy()
        ln[4 * 3 + k] = -1
        t = Table(c.off, ln)
        refused(lib.bdx_fq_check_device(h, d.ptr, d.n, *t.at(0), c.n, 7, *args), "a line of the line table lies outside the text")
    off = c.off.copy()
    off[0] = -1
    t = Table(off, c.len)
    refused(lib.bdx_fq_check_device(h, d.ptr, d.n, *t.at(0), c.n, 7, *args), "a line of the line table lies outside the text")
    assert lib.bdx_fq_check_device(h, d.ptr, d.n - 1, o, l, c.n, 7, *args) == 0  # (without the last "\n": every line is still inside)
    refused(lib.bdx_fq_check_device(h, d.ptr, d.n - 2, o, l, c.n, 7, *args), "a line of the line table lies outside the text")
    # the pair entry
    pa = (d.ptr, d.n, o, l)
    refused(lib.bdx_fq_check_pair_device(h, *pa, *pa, c.n, None), "first_bad is NULL")
    for k in range(8):
        if k % 4 == 1:
            continue
        both = list(pa + pa)
        both[k] = None
        refused(lib.bdx_fq_check_pair_device(h, *both, c.n, C.byref(bad)), "NULL device pointer")
        assert bad.value == -1
    refused(lib.bdx_fq_check_pair_device(h, d.ptr, -1, o, l, *pa, c.n, C.byref(bad)), "n / text_len is negative")
    refused(lib.bdx_fq_check_pair_device(h, *pa, d.ptr, -1, o, l, c.n, C.byref(bad)), "n / text_len is negative")
    refused(lib.bdx_fq_check_pair_device(h, *pa, *pa, -1, C.byref(bad)), "n / text_len is negative")
    refused(lib.bdx_fq_check_pair_device(h, *pa, *pa, 1 << 32, C.byref(bad)), "more than 2^32 - 1 records")
    assert lib.bdx_fq_check_pair_device(h, *pa, *pa, 0, C.byref(bad)) == 0 and bad.value == -1
    ln = c.len.copy()
    ln[4 * 5] = len(c.text) - int(c.off[4 * 5]) + 1  # a header line that reaches one byte beyond the text
    t = Table(c.off, ln)
    refused(lib.bdx_fq_check_pair_device(h, d.ptr, d.n, *t.at(0), *pa, c.n, C.byref(bad)), "a line of the line table lies outside the text")
    refused(lib.bdx_fq_check_pair_device(h, *pa, d.ptr, d.n, *t.at(0), c.n, C.byref(bad)), "a line of the line table lies outside the text")
    assert d.untouched()


# ---- the pipelines ----
def test_goldens_through_the_device_pipeline_with_the_checks_on(tmp_path):
    """plain and gzip input, paired and not: the reference's goldens, which is what _check=False gives"""
    tm = {}
    run = functools.partial(run_dev, _check=True, _timings=tm)
    assert H.scenario_demo1_R1(run, str(tmp_path / "a")) == 24
    assert tm["checked_records"] > 0 and 0 <= tm["check_s"] <= tm["device_s"]
    assert H.scenario_demo1_R2(run, str(tmp_path / "b")) == 24
    assert H.scenario_demo2(run, str(tmp_path / "c")) == 76  # gz in, classify_both
    os.mkdir(str(tmp_path / "d"))
    H.scenario_dual_trim(run, str(tmp_path / "d"))
    tm.clear()
    H.scenario_demo1_R1(functools.partial(run_dev, _timings=tm), str(tmp_path / "e"))
    assert "check_s" not in tm and "checked_records" not in tm


@pytest.mark.parametrize("name", list(CPU.failing_inputs()))
def test_device_pipeline_fails_like_the_native_one(tmp_path, name):
    fastqs, bc, msg, before, t1, t2 = CPU.write_inputs(tmp_path, name)
    kw = dict(max_error_rate=0.2, _batch_reads=4, **(dict(classify_both=True) if t2 is not None else {}))
    trees = {}
    for io, run in (("native", run_nat), ("device", run_dev)):
        out = str(tmp_path / io)
        with pytest.raises(hipabi.BdxError) as e:
            run(*fastqs, bc, out, _check=True, **kw)
        assert str(e.value) == msg, io
        trees[io] = CPU.tree(out)
    assert trees["device"] == trees["native"]
    assert sum(v.count(b"\n") for v in trees["device"].values()) == 4 * before * len(fastqs)


@pytest.mark.parametrize("mode", ["host", "device", "device-stream", "device-window"])
def test_gzip_input_modes_fail_with_the_same_message(tmp_path, mode):
    """one failing text through every input class of the device pipeline: the offset is the plain text's"""
    fastqs, bc, msg, before, t1, _ = CPU.write_inputs(tmp_path, "length")
    gz = str(tmp_path / "x_R1.fastq.gz")
    if mode == "device":  # (a chain of size-tagged members: what the device encoder writes)
        none = str(tmp_path / "none.csv")
        open(none, "w").write("ID,Full_seq,Full_annotation\nc,CCCCCCCCCCCCCCCCCCCC,BBBBBBBBBBBBBBBBBBBB\n")
        run_dev(fastqs[0], none, str(tmp_path / "made"), max_error_rate=0.0, _gzip="device", gzip_output=True, output_prefix="m")
        made = sorted(os.listdir(str(tmp_path / "made")))
        assert len(made) == 1, made  # (every read in one file: the barcode matches nothing of this text)
        os.replace(os.path.join(str(tmp_path / "made"), made[0]), gz)
        assert gzip.open(gz).read() == t1
    else:
        with gzip.open(gz, "wb") as fh:
            fh.write(t1)
    out = str(tmp_path / "out")
    with pytest.raises(hipabi.BdxError) as e:
        run_dev(gz, bc, out, _check=True, _gunzip=mode, max_error_rate=0.2, _batch_reads=4, gzip_output=False)
    assert str(e.value) == msg.replace(fastqs[0], gz)
    assert sum(v.count(b"\n") for v in CPU.tree(out).values()) == 4 * before


def _deal_text(n, bad=None):
    recs = CPU._records(n)
    if bad is not None:
        recs[bad] = (recs[bad][0], recs[bad][1], b"-", recs[bad][3])
    return CPU._text(recs), CPU._offset(recs, bad or 0)


def test_device_deal_reports_the_absolute_byte_offset(tmp_path):
    """spans of 256 bytes: a bad record whose first line starts in the second span; the spans in front of it are written"""
    text, at = _deal_text(40, bad=8)
    assert 256 <= at < 512
    fq, bc = str(tmp_path / "r.fastq"), str(tmp_path / "bc.csv")
    open(fq, "wb").write(text)
    open(bc, "w").write(CPU.BARCODES)
    out = str(tmp_path / "out")
    with pytest.raises(hipabi.BdxError) as e:
        run_deal(fq, bc, out, _check=True, _span_bytes=256, max_error_rate=0.2)
    assert str(e.value) == "%s: the record at byte %d of the text: the third line does not begin with '+'" % (fq, at)
    first_span = sum(1 for k in range(40) if CPU._offset(CPU._records(40), k) < 256)
    assert sum(v.count(b"\n") for v in CPU.tree(out).values()) == 4 * first_span


def test_device_deal_of_a_clean_text_writes_the_same_files(tmp_path):
    text, _ = _deal_text(200)
    fq, bc = str(tmp_path / "r.fastq"), str(tmp_path / "bc.csv")
    open(fq, "wb").write(text)
    open(bc, "w").write(CPU.BARCODES)
    tm = {}
    a = run_deal(fq, bc, str(tmp_path / "on"), _check=True, _span_bytes=1024, max_error_rate=0.2, _timings=tm)
    b = run_deal(fq, bc, str(tmp_path / "off"), _span_bytes=1024, max_error_rate=0.2)
    assert CPU.tree(str(tmp_path / "on")) == CPU.tree(str(tmp_path / "off")) and a.total_reads == b.total_reads == 200
    assert tm["checked_records"] == 200 and tm["check_s"] >= 0
