"""_io="device-deal" on the MI355X: bdx_fq_count_lines_device and bdx_fq_index_span_device against the numpy restatement
of tests/fastq_span_cases.py (which tests/test_device_deal_cpu.py holds to the host library), and the dealt pipeline end
to end against _io="device".

No call here can touch memory outside its buffers: every text lies inside a larger device buffer (64 bytes on both sides
at the least), the line tables have 64 entries of canary behind the room the call is told of."""
import ctypes as C
import functools
import gzip
import os
import threading

import numpy as np
import pytest

import fastq_cases as FC
import fastq_span_cases as SP
import helpers as H
from biodemux_jl_amd import nativeio, synth

pytestmark = pytest.mark.gpu

PAD, CANARY = 64, 64
E_SPACE = -5
FRONTS = (0, 1, 5, 15, 16)

run_dev = functools.partial(H.bdx.execute_demultiplexing, _io="device")
run_deal = functools.partial(H.bdx.execute_demultiplexing, _io="device-deal")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    nativeio.build()


def _ctx():
    cfg = H.bdx.DemuxConfig(bc_seqs=["ACGTACGT"], bc_lengths_no_N=[8], ids=["a"])
    return H.bdx.HipClassifier(cfg)


@pytest.fixture(scope="module")
def hc():
    """one context for the cases of this file: every call meets the scratch buffers the call before it left"""
    with _ctx() as ctx:
        yield ctx


def _err(ctx):
    return ctx.lib.bdx_last_error(ctx.h).decode()


class Text:
    """a text `front` bytes into a device buffer, newlines on both sides: a look outside it shows as a line"""

    def __init__(self, text, front=PAD):
        import torch

        t = SP._u8(text)
        self.n = len(t)
        host = np.concatenate([np.full(front, SP.NL, np.uint8), t, np.full(PAD, SP.NL, np.uint8)])
        self.buf = torch.from_numpy(host).to("cuda:0")
        torch.cuda.synchronize()
        self.ptr = self.buf.data_ptr() + front


class Tables:
    """line tables with room for `max_reads` records and CANARY entries of a pattern behind it"""

    def __init__(self, max_reads):
        import torch

        self.room = 4 * max_reads
        self.off = torch.full((self.room + CANARY,), -77, dtype=torch.int64, device="cuda:0")
        self.len = torch.full((self.room + CANARY,), -77, dtype=torch.int32, device="cuda:0")

    def untouched_from(self, k):
        return bool((self.off[k:] == -77).all()) and bool((self.len[k:] == -77).all())


def _count(ctx, ptr, n):
    out = C.c_int64(-1)
    ctx._check(ctx.lib.bdx_fq_count_lines_device(ctx.h, ptr, n, C.byref(out)))
    return out.value


def _index_span(ctx, ptr, text_len, span_len, phase, starts_line, final, max_reads, tb):
    """-> (rc, n_records, complete, off, len); the canaries are checked here"""
    import torch

    n, complete = C.c_int64(-1), C.c_int32(-1)
    tb.off.fill_(-77)
    tb.len.fill_(-77)
    torch.cuda.synchronize()  # (the entry runs on the context's stream, not on torch's)
    rc = ctx.lib.bdx_fq_index_span_device(ctx.h, ptr, text_len, span_len, phase, starts_line, final, max_reads,
                                          tb.off.data_ptr(), tb.len.data_ptr(), C.byref(n), C.byref(complete))
    assert tb.untouched_from(min(4 * max_reads, tb.room)), "a line table was written behind its room"
    if rc != 0 or not complete.value:
        return rc, n.value, complete.value, None, None
    k = 4 * n.value
    assert tb.untouched_from(k), "a line table was written behind the records"
    return rc, n.value, 1, tb.off[:k].cpu().numpy(), tb.len[:k].cpu().numpy()


def _device_span(ctx, d, tb, text, S, k, tail, max_reads):
    w, span_len, phase, starts_line, final = SP.span_args(text, S, k, tail)
    assert _count(ctx, d.ptr + k * S, span_len) == int(np.count_nonzero(w[:span_len] == SP.NL))
    rc, n, complete, off, ln = _index_span(ctx, d.ptr + k * S, len(w), span_len, phase, starts_line, final, max_reads, tb)
    assert rc == 0, _err(ctx)
    return n, complete, off, ln


def _same(got, exp):
    return got[0] == exp[0] and got[1] == exp[1] and (not exp[1] or (np.array_equal(got[2], exp[2]) and np.array_equal(got[3], exp[3])))


# ---- the two entries against the restatement ----
@pytest.mark.parametrize("c", SP.span_texts(), ids=lambda c: c.name)
def test_spans_equal_the_restatement(hc, c):
    """every span of the text at every span size and buffer offset, offered with a growing tail: each call's records,
    `complete` and tables; the newline count of every span; both alignments of the text pointer"""
    max_reads = len(c.text) // 4 + 4
    tb = Tables(max_reads)
    for front in FRONTS:
        d = Text(c.text, front=front)
        for S in SP.SPANS:
            def index(text, S, k, tail):
                got = _device_span(hc, d, tb, text, S, k, tail, max_reads)
                exp = SP.ref_span_index(text, S, k, tail)
                assert _same(got, exp), (c.name, front, S, k, tail, got[:2], exp[:2])
                return got

            SP.walk_spans(c.text, S, index=index)
    assert _count(hc, d.ptr, 0) == 0


def test_partition_property_against_the_whole_index(hc):
    """the spans' tables, shifted and concatenated, are bdx_fq_index_device's table of the whole text (final = 1)"""
    import torch

    for c in SP.span_texts():
        if not c.text:
            continue
        max_reads = len(c.text) // 4 + 4
        tb = Tables(max_reads)
        d = Text(c.text, front=16)
        woff = torch.empty(4 * max_reads, dtype=torch.int64, device="cuda:0")
        wlen = torch.empty(4 * max_reads, dtype=torch.int32, device="cuda:0")
        n, nxt = C.c_int64(-1), C.c_int64(-1)
        hc._check(hc.lib.bdx_fq_index_device(hc.h, d.ptr, d.n, 1, max_reads, woff.data_ptr(), wlen.data_ptr(), C.byref(n), C.byref(nxt)))
        for S in SP.SPANS + (len(c.text),) + ((1,) if len(c.text) <= 150 else ()):
            off, ln, per_span = SP.walk_spans(c.text, S, index=lambda t, S, k, tail: _device_span(hc, d, tb, t, S, k, tail, max_reads))
            assert sum(per_span) == n.value, (c.name, S)
            assert np.array_equal(off, woff[:4 * n.value].cpu().numpy()) and np.array_equal(ln, wlen[:4 * n.value].cpu().numpy()), (c.name, S)


def test_short_tail_then_a_longer_one(hc):
    c = next(c for c in SP.span_texts() if c.name == "line_longer_than_two_spans")
    d, tb = Text(c.text), Tables(64)
    k = 2  # the span in which the record with the long lines starts
    exp = SP.ref_span_index(c.text, 16, k, 16)
    assert exp[0] == 1 and exp[1] == 0
    assert _device_span(hc, d, tb, c.text, 16, k, 16, 64)[:2] == (1, 0)
    exp = SP.ref_span_index(c.text, 16, k, 256)
    assert exp[1] == 1 and _same(_device_span(hc, d, tb, c.text, 16, k, 256, 64), exp)


def test_max_reads_one_too_small(hc):
    c = next(c for c in SP.span_texts() if c.name == "all_phase_pairs")
    d = Text(c.text)
    w, span_len, phase, starts_line, final = SP.span_args(c.text, 100, 1, 64)
    exp = SP.ref_window_index(w, span_len, phase, starts_line, final)
    need = exp[0]
    assert need >= 5
    tb = Tables(need)
    rc, n, _, _, _ = _index_span(hc, d.ptr + 100, len(w), span_len, phase, starts_line, final, need - 1, tb)
    assert rc == E_SPACE and n == need and "%d records start in the span, the line table holds %d" % (need, need - 1) in _err(hc)
    assert tb.untouched_from(0), "nothing is written when the table is too small"
    got = _index_span(hc, d.ptr + 100, len(w), span_len, phase, starts_line, final, need, tb)
    assert got[0] == 0 and _same(got[1:], exp)


def test_eight_mib_span_of_four_byte_records(hc):
    """2^21 records of four empty lines in one span; the window (the span and a tail of long lines) takes more than 1024
    tiles, so the one-workgroup scan of the tiles' counts carries"""
    t, span = SP.big_text()
    assert FC.tiles(len(t)) > FC.FQ_SCAN_BLOCK and FC.tiles(span) == 512
    d = Text(t, front=16)
    assert _count(hc, d.ptr, span) == span
    assert _count(hc, d.ptr, len(t)) == int(np.count_nonzero(t == SP.NL)) > span
    assert _count(hc, d.ptr + 3, len(t) - 3) == int(np.count_nonzero(t == SP.NL)) - 3  # the unaligned form
    exp = SP.ref_window_index(t, span, 0, 1, 1)
    assert exp[0] == span // 4
    tb = Tables(exp[0])
    got = _index_span(hc, d.ptr, len(t), span, 0, 1, 1, exp[0], tb)
    assert got[0] == 0 and _same(got[1:], exp)
    # the same window one byte on: phase 1, and the last record of the span reaches into the tail
    exp = SP.ref_window_index(t[1:], span, 1, 1, 1)
    got = _index_span(hc, d.ptr + 1, len(t) - 1, span, 1, 1, 1, exp[0], tb)
    assert got[0] == 0 and _same(got[1:], exp) and exp[2][-1] >= span


def test_refusals_and_a_correct_call_afterwards(hc):
    c = next(c for c in SP.span_texts() if c.name == "all_phase_pairs")
    d, tb = Text(c.text), Tables(64)
    n, complete, cnt = C.c_int64(7), C.c_int32(7), C.c_int64(7)
    lib, h = hc.lib, hc.h

    def call(ptr=d.ptr, text_len=200, span_len=100, phase=0, max_reads=64, off=tb.off.data_ptr(), ln=tb.len.data_ptr(),
             pn=C.byref(n), pc=C.byref(complete)):
        return lib.bdx_fq_index_span_device(h, ptr, text_len, span_len, phase, 1, 0, max_reads, off, ln, pn, pc)

    for kw, needle in ((dict(text_len=-1), "negative"), (dict(span_len=-1), "negative"), (dict(max_reads=-1), "negative"),
                       (dict(max_reads=2 ** 40 + 1), "max_reads is too large"),
                       (dict(span_len=201), "span_len (201) is larger than text_len (200)"), (dict(phase=4), "phase must be 0 .. 3 (got 4)"),
                       (dict(phase=-1), "phase must be 0 .. 3 (got -1)"), (dict(ptr=None), "NULL device pointer"),
                       (dict(off=None), "NULL device pointer"), (dict(ln=None), "NULL device pointer"),
                       (dict(pn=None), "n_records / complete is NULL"), (dict(pc=None), "n_records / complete is NULL")):
        assert call(**kw) != 0 and needle in _err(hc), (kw, _err(hc))
        assert tb.untouched_from(0)
    assert lib.bdx_fq_count_lines_device(h, d.ptr, -1, C.byref(cnt)) != 0 and "len is negative" in _err(hc)
    assert lib.bdx_fq_count_lines_device(h, None, 10, C.byref(cnt)) != 0 and "NULL device pointer" in _err(hc)
    assert lib.bdx_fq_count_lines_device(h, d.ptr, 10, None) != 0 and "n_newlines is NULL" in _err(hc)
    assert call(text_len=0, span_len=0, ptr=None, off=None, ln=None) == 0 and (n.value, complete.value) == (0, 1)
    exp = SP.ref_span_index(c.text, 100, 2, 64)
    assert _same(_device_span(hc, d, tb, c.text, 100, 2, 64, 64), exp) and exp[0] > 0


# ---- end to end ----
def _same_tree(a, b, plain):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb and fa
    for f in fa:
        if f.startswith("summary."):  # (run times differ)
            continue
        if plain:
            assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f
        else:
            assert H._read_maybe_gz(os.path.join(a, f)) == H._read_maybe_gz(os.path.join(b, f)), f


def _fastq(path, seqs, crlf=False, tail=b"", gz=False):
    nl = b"\r\n" if crlf else b"\n"
    blob = b"".join(b"@r%d some header" % i + nl + s + nl + b"+" + nl + b"I" * len(s) + nl for i, s in enumerate(seqs)) + tail
    with (gzip.open if gz else open)(path, "wb") as f:
        f.write(blob)
    return len(blob)


def _barcodes(path, bcs, tag):
    path.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"{tag}{i},{b},{'B' * len(b)}\n" for i, b in enumerate(bcs)))
    return str(path)


CASES = ("plain", "crlf", "truncated", "blankline", "no_final_newline", "gz_in_gz_out", "gzip_device_1", "gzip_device_2", "dual_trim",
         "summary")
N_READS, SPAN = 700, 1000


_MADE = {}


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """case name -> its input files and keywords, and its tree and result through _io="device": made once per case,
    shared by the tests and never changed"""
    def get(case):
        if case not in _MADE:
            _MADE[case] = _make_case(case, tmp_path_factory.mktemp("deal_" + case))
        return _MADE[case]

    yield get
    _MADE.clear()


def _make_case(case, P):
    kw = dict(max_error_rate=0.2, trim_side=5, _batch_reads=128)
    if case == "dual_trim":
        b1, b2 = synth.make_barcodes(24, 24, seed=1), synth.make_barcodes(16, 24, seed=2)
        seq, off, _ = synth.make_reads(b1, N_READS, 150, seed=77, plant_lo=0, plant_hi=40, second=(b2, 100, 126))
        bc = _barcodes(P / "b1.csv", b1, "x")
        kw.update(barcode_file2=_barcodes(P / "b2.csv", b2, "y"), trim_side2=3)
    else:
        bcs = synth.make_barcodes(6, 12, seed=5, min_hamming=4)
        seq, off, _ = synth.make_ragged_reads(bcs, N_READS, 100, 190, seed=5)
        bc = _barcodes(P / "bc.csv", bcs, "b")
    seqs = [seq[off[i]:off[i + 1]].tobytes() for i in range(N_READS)]
    tail = {"truncated": b"@last\nACGTAC", "blankline": b"\n", "no_final_newline": b"@x\nACGT\n+\nIIII"}.get(case, b"")
    gz_in = case == "gz_in_gz_out"
    fq = str(P / ("reads.fastq.gz" if gz_in else "reads.fastq"))
    size = _fastq(fq, seqs, crlf=case == "crlf", tail=tail, gz=gz_in)
    if case in ("gz_in_gz_out", "gzip_device_1", "gzip_device_2"):
        kw["gzip_output"] = True
    if case.startswith("gzip_device"):
        kw.update(_gzip="device", _gzip_level=int(case[-1]))
    if case == "summary":
        kw.update(summary=True, summary_format="json")
    ref = run_dev(fq, bc, str(P / "ref"), **kw)
    return fq, bc, kw, size, str(P / "ref"), ref


@pytest.mark.parametrize("devices", [None, [0, 0], [0, 0, 0]], ids=["one", "two", "three"])
@pytest.mark.parametrize("case", CASES)
def test_dealt_equals_device_io(tmp_path, cases, case, devices):
    fq, bc, kw, size, ref_dir, ref = cases(case)
    tm = {}
    got = run_deal(fq, bc, str(tmp_path / "deal"), devices=devices, _span_bytes=SPAN, _timings=tm, **kw)
    _same_tree(ref_dir, str(tmp_path / "deal"), plain=not kw.get("gzip_output"))
    assert vars(got) == vars(ref)  # counters and the report tables
    assert tm["spans"] == -(-size // SPAN) > 200 and tm["span_bytes"] == SPAN
    assert len(tm["spans_per_device"]) == len(devices or [0]) and sum(tm["spans_per_device"]) == tm["spans"]
    assert tm["devices"] == (devices or [0])


def test_gzip_members_do_not_depend_on_the_contexts(tmp_path, cases):
    fq, bc, kw, _, _, _ = cases("gzip_device_1")
    for name, devices in (("a", None), ("b", [0, 0, 0])):
        run_deal(fq, bc, str(tmp_path / name), devices=devices, _span_bytes=SPAN, **kw)
    _same_tree(str(tmp_path / "a"), str(tmp_path / "b"), plain=True)


def test_spans_without_a_record_start(tmp_path):
    bcs = synth.make_barcodes(6, 12, seed=5, min_hamming=4)
    seq, off, _ = synth.make_reads(bcs, 60, 300, seed=8)
    seqs = [seq[off[i]:off[i + 1]].tobytes() for i in range(60)]
    fq, bc = str(tmp_path / "long.fastq"), _barcodes(tmp_path / "bc.csv", bcs, "b")
    size = _fastq(fq, seqs)
    text = open(fq, "rb").read()
    assert len(SP._spans_without_record_start(text, 64)) > 60 and any(n == 0 for n in SP.walk_spans(text, 64)[2])
    kw = dict(max_error_rate=0.2, trim_side=3)
    ref = run_dev(fq, bc, str(tmp_path / "ref"), **kw)
    for name, devices in (("one", None), ("three", [0, 0, 0])):
        tm = {}
        got = run_deal(fq, bc, str(tmp_path / name), devices=devices, _span_bytes=64, _timings=tm, **kw)
        _same_tree(str(tmp_path / "ref"), str(tmp_path / name), plain=True)
        assert vars(got) == vars(ref) and got.total_reads == 60
        assert tm["spans"] == -(-size // 64) == sum(tm["spans_per_device"]) and tm["batches"] < tm["spans"]


def test_default_span_and_an_empty_input(tmp_path, cases):
    fq, bc, kw, size, ref_dir, ref = cases("plain")
    tm = {}
    got = run_deal(fq, bc, str(tmp_path / "d"), devices=[0, 0], _timings=tm, **kw)
    _same_tree(ref_dir, str(tmp_path / "d"), plain=True)
    assert vars(got) == vars(ref) and tm["span_bytes"] == 65536 and tm["spans"] == -(-size // 65536)
    empty = tmp_path / "empty.fastq"
    empty.write_bytes(b"")
    tm = {}
    assert run_deal(str(empty), bc, str(tmp_path / "e"), devices=[0, 0], _timings=tm, **kw).total_reads == 0
    assert tm["spans"] == 0 and tm["spans_per_device"] == [0, 0]


# ---- errors ----
def _in_thread(fn, timeout=120):
    result = {}

    def run():
        try:
            fn()
            result["ok"] = True
        except BaseException as e:  # noqa: BLE001
            result["err"] = e

    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(timeout)
    assert not t.is_alive(), "the dealt pipeline hangs on an error"
    return result


def _deal_threads():
    return [t.name for t in threading.enumerate() if t.name.startswith("bdx-deal")]


def test_writer_error_reaches_the_caller_and_leaves_no_thread(tmp_path, cases):
    """a directory stands where the busiest output file goes (open() gives EISDIR on the host; nothing is wrong on the
    device) while most spans are still to come"""
    fq, bc, kw, _, ref_dir, _ = cases("plain")
    busiest = max(os.listdir(ref_dir), key=lambda f: os.path.getsize(os.path.join(ref_dir, f)))
    (tmp_path / "o1" / busiest).mkdir(parents=True)
    r = _in_thread(lambda: run_deal(fq, bc, str(tmp_path / "o1"), devices=[0, 0, 0], _span_bytes=SPAN, **kw))
    assert isinstance(r.get("err"), OSError), r
    assert not _deal_threads()
    r = _in_thread(lambda: run_deal(fq, bc, str(tmp_path / "o2"), devices=[0, 0], _span_bytes=SPAN, **kw))  # and goes on working
    assert r.get("ok"), r
    _same_tree(ref_dir, str(tmp_path / "o2"), plain=True)


def test_a_device_that_does_not_exist_closes_context_0(tmp_path, cases, monkeypatch):
    from biodemux_jl_amd import core, hipabi

    opened = []
    real = hipabi.HipClassifier

    class Spy(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            opened.append(self)

    fq, bc, kw, _, _, _ = cases("plain")
    monkeypatch.setattr(core, "HipClassifier", Spy)
    with pytest.raises(hipabi.BdxError, match="out of range"):
        run_deal(fq, bc, str(tmp_path / "o"), devices=[0, 99], _span_bytes=SPAN, **kw)
    monkeypatch.undo()
    assert len(opened) == 1 and opened[0].h is None and not _deal_threads()
