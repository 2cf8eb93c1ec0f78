"""csrc/bdx_fastq.hip on the MI355X, at its edges: the line index, the pack, the stable radix partition and the gather
against the plain references of tests/fastq_cases.py (which tests/test_device_io_cases_cpu.py holds to the host library)
on every named text and gather case; one case large enough that every scan of the pipeline carries across its
one-workgroup stage; scratch reuse on one context; and every documented refusal of the three entries.

No call here can touch memory outside its buffers, lost checks included: every text lies inside a larger device buffer
(64 bytes of padding on both sides at the least), d_out and d_seq are larger than any total the call can reach, and the
tampered line tables point at most one byte outside the text."""
import ctypes as C

import numpy as np
import pytest

import fastq_cases as FC
import helpers as H
from biodemux_jl_amd import nativeio

pytestmark = pytest.mark.gpu

PAD = 64       # bytes around every text on the device
CANARY = 256   # bytes of d_out behind the expected total


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


def _dev(arr):
    import torch

    t = torch.from_numpy(np.array(arr, copy=True)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _empty(n, dtype):
    import torch

    return torch.empty(max(int(n), 1), dtype=dtype, device="cuda:0")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _err(ctx):
    return ctx.lib.bdx_last_error(ctx.h).decode()


class Text:
    """a text `front` bytes into a device buffer, `pad` bytes on both sides holding `fill`"""

    def __init__(self, text, front=PAD, fill=ord("!")):
        t = FC._u8(text)
        self.n = len(t)
        self.buf = _dev(np.concatenate([np.full(front, fill, np.uint8), t, np.full(PAD, fill, np.uint8)]))
        self.ptr = self.buf.data_ptr() + front


# ---- index ----
def _index(ctx, d, final, max_reads):
    import torch

    off = _empty(4 * max_reads, torch.int64)
    ln = _empty(4 * max_reads, torch.int32)
    n, nxt = C.c_int64(-1), C.c_int64(-1)
    ctx._check(ctx.lib.bdx_fq_index_device(ctx.h, d.ptr, d.n, final, max_reads, off.data_ptr(), ln.data_ptr(), C.byref(n), C.byref(nxt)))
    k = 4 * n.value
    return n.value, nxt.value, off[:k].cpu().numpy(), ln[:k].cpu().numpy()


def _same_index(got, exp):
    return got[0] == exp[0] and got[1] == exp[1] and np.array_equal(got[2], exp[2]) and np.array_equal(got[3], exp[3])


@pytest.mark.parametrize("t", FC.index_texts(), ids=lambda t: t.name)
def test_index_equals_reference(hc, t):
    """both instantiations (a 16-byte aligned text pointer or not), an aligned pointer that is not the allocation's base,
    final and not, five kinds of cap; the bytes around the text are newlines, so a look outside it shows as a line"""
    caps = FC.caps_for(t.text)
    exp = {(final, cap): FC.ref_index(t.text, final, cap) for final in (0, 1) for cap in caps.values()}
    for front in (0, 1, 5, 15, 16):
        d = Text(t.text, front=front, fill=FC.NL)
        assert (d.ptr % 16 == 0) == (front % 16 == 0)
        for final in (0, 1):
            for label, cap in caps.items():
                got = _index(hc, d, final, cap)
                assert _same_index(got, exp[final, cap]), (front, final, label, cap, got[:2], exp[final, cap][:2])


# ---- pack ----
def _pack(ctx, d, off, ln, n, seq_cap=None):
    import torch

    d_off, d_len = _dev(np.asarray(off, dtype=np.int64)), _dev(np.asarray(ln, dtype=np.int32))
    seq = _empty(d.n + PAD, torch.uint8)
    so = _empty(n + 1, torch.int64)
    total = C.c_int64(-1)
    rc = ctx.lib.bdx_fq_pack_device(ctx.h, d.ptr, d.n, d_off.data_ptr(), d_len.data_ptr(), n, seq.data_ptr(),
                                    d.n + PAD if seq_cap is None else seq_cap, so.data_ptr(), C.byref(total))
    return rc, total.value, seq, so


@pytest.mark.parametrize("c", FC.gather_cases(), ids=lambda c: c.name)
def test_pack_equals_reference(hc, c):
    seq, so = FC.ref_pack(c.text, c.off, c.len, c.n)
    rc, total, d_seq, d_so = _pack(hc, Text(c.text), c.off, c.len, c.n)
    assert rc == 0, _err(hc)
    assert total == len(seq) and np.array_equal(d_so[:c.n + 1].cpu().numpy(), so)
    assert d_seq[:total].cpu().numpy().tobytes() == seq.tobytes()


# ---- gather ----
def _canary(n):
    return ((np.arange(n, dtype=np.int64) * 31 + 7) % 251).astype(np.uint8)


class Tables:
    def __init__(self, c, off=None, ln=None, bc1=None, bc2=None):
        self.off = _dev(np.asarray(c.off if off is None else off, dtype=np.int64))
        self.len = _dev(np.asarray(c.len if ln is None else ln, dtype=np.int32))
        self.bc1 = _dev(np.asarray(c.bc1 if bc1 is None else bc1, dtype=np.int32))
        self.bc2 = _dev(np.asarray(c.bc2 if bc2 is None else bc2, dtype=np.int32))
        self.ks = None if c.keep_start is None else _dev(c.keep_start)
        self.ke = None if c.keep_end is None else _dev(c.keep_end)


def _gather(ctx, d, tb, c, room, out_cap=None, stride=None, n_classes=None):
    """-> (rc, class_bytes, all of d_out): d_out holds `room` bytes of a canary pattern before the call"""
    ncl = c.n_classes if n_classes is None else n_classes
    out = _dev(_canary(room))
    class_bytes = np.full(ncl, -1, np.int64)
    rc = ctx.lib.bdx_fq_gather_device(ctx.h, d.ptr, d.n, tb.off.data_ptr(), tb.len.data_ptr(), c.n, tb.bc1.data_ptr(), tb.bc2.data_ptr(),
                                      c.stride if stride is None else stride, ncl, _ptr(tb.ks), _ptr(tb.ke), c.trim, out.data_ptr(),
                                      room if out_cap is None else out_cap, class_bytes.ctypes.data)
    return rc, class_bytes, out.cpu().numpy()


def _reference(c):
    return FC.ref_gather(c.text, c.off, c.len, c.bc1, c.bc2, c.stride, c.n_classes, c.keep_start, c.keep_end, c.trim)


def _gather_equals_reference(ctx, c, exp=None):
    exp, exp_bytes = exp or _reference(c)
    total = len(exp)
    rc, class_bytes, out = _gather(ctx, Text(c.text), Tables(c), c, total + CANARY)
    assert rc == 0, _err(ctx)
    assert np.array_equal(class_bytes, exp_bytes)
    if not np.array_equal(out[:total], exp):
        k = int(np.flatnonzero(out[:total] != exp)[0])
        raise AssertionError("%s: d_out differs from byte %d of %d on: %r, expected %r" % (
            c.name, k, total, out[k:k + 40].tobytes(), exp[k:k + 40].tobytes()))
    assert np.array_equal(out[total:], _canary(total + CANARY)[total:]), "d_out was written behind the blocks"
    return out


@pytest.mark.parametrize("c", FC.gather_cases(), ids=lambda c: c.name)
def test_gather_equals_reference(hc, c):
    _gather_equals_reference(hc, c)


def test_large_case_carries_across_every_scan(tmp_path):
    """more than FQ_SCAN_BLOCK tiles of text, and more than FQ_SCAN_BLOCK partials in the pack scan, the gather's byte scan
    and the partition's histogram scan: the carry loop of the one-workgroup scan runs in all four"""
    import torch

    c = FC.large_case()
    assert c.ok and len(c.text) > 16 << 20 and FC.tiles(len(c.text)) > FC.FQ_SCAN_BLOCK
    assert FC.scan_partials(c.n) > FC.FQ_SCAN_BLOCK, "pack scan and byte scan"
    assert FC.scan_partials(FC.hist_items(c.n)) > FC.FQ_SCAN_BLOCK, "histogram scan"
    f = FC.host_open(tmp_path / "in.fastq", c.text)
    try:
        hn, hoff, hln = f.next_batch(c.n + 5, 4)
        hoff, hln = hoff[:4 * hn], hln[:4 * hn]
        hseq, hso = f.pack(hoff, hln, hn, 4)
        hout, hbytes = FC.host_gather(tmp_path / "out", f, c)
        assert hn == c.n and f.cursor == len(c.text)
    finally:
        f.close()
    hout = np.frombuffer(hout, dtype=np.uint8)
    with _ctx() as ctx:
        d = Text(c.text, front=16)
        n, nxt, off, ln = _index(ctx, d, 1, c.n + 5)
        assert (n, nxt) == (hn, len(c.text)) and np.array_equal(off, hoff) and np.array_equal(ln, hln)
        assert _same_index(_index(ctx, d, 0, c.n - 3), (c.n - 3, int(hoff[4 * (c.n - 3)]), hoff[:4 * (c.n - 3)], hln[:4 * (c.n - 3)]))
        rc, total, d_seq, d_so = _pack(ctx, d, off, ln, n)
        assert rc == 0, _err(ctx)
        assert total == len(hseq) and np.array_equal(d_so[:n + 1].cpu().numpy(), hso)
        assert np.array_equal(d_seq[:total].cpu().numpy(), hseq)
        del d_seq, d_so
        room = len(hout) + CANARY
        rc, class_bytes, out = _gather(ctx, d, Tables(c, off=off, ln=ln), c, room)
        assert rc == 0, _err(ctx)
        assert np.array_equal(class_bytes, hbytes) and (hbytes > 0).all()
        assert np.array_equal(out[:len(hout)], hout)
        assert np.array_equal(out[len(hout):], _canary(room)[len(hout):])
        # a few thousand records by plain slicing: where a stable sort by class puts each, and what is written there
        cls = FC.ref_classes(c.bc1, c.bc2, c.stride, c.n_classes)
        a, sl, ql = FC.ref_slices(c.len, c.n, c.keep_start, c.keep_end, c.trim)
        nbytes = c.len[0::4].astype(np.int64) + sl + c.len[2::4] + ql + 4
        order = np.argsort(cls, kind="stable")
        pos = np.empty(c.n, np.int64)
        pos[order] = np.cumsum(nbytes[order]) - nbytes[order]
        text = c.text.tobytes()
        for i in np.random.default_rng(5).integers(0, c.n, 4000).tolist() + [0, c.n - 1]:
            rec = FC.ref_record(text, c.off, c.len, i, c.keep_start, c.keep_end, c.trim)
            assert len(rec) == nbytes[i] and out[pos[i]:pos[i] + len(rec)].tobytes() == rec, i
        # the same context, its scratch sized for a million records, on small cases
        del out
        torch.cuda.empty_cache()
        for name in ("n1_one_class", "classes_257"):
            _gather_equals_reference(ctx, FC.gather_case(name))


def test_one_context_large_then_one_record_then_other_classes():
    """scratch of an earlier call (more records, more classes, more passes) must not show in a later one"""
    with _ctx() as ctx:
        for name in ("n1025_top_byte", "n1_one_class", "classes_257", "n1025_own_class", "n1_top_byte", "n257_two_alternating"):
            _gather_equals_reference(ctx, FC.gather_case(name))


# ---- refusals ----
def _base():
    return FC.gather_case("n65_two_alternating")


def test_class_out_of_range_is_refused(hc):
    c = _base()
    d, exp = Text(c.text), _reference(c)
    room = len(exp[0]) + CANARY
    last = (c.n_classes - 2) // c.stride  # the largest bc1
    for what, i, b1, b2, stride, ncl in (
            ("bc1 too large", 17, last + 1, 1, c.stride, c.n_classes),
            ("bc2 > stride on the last bc1", 64, last, c.stride + 1, c.stride, c.n_classes),
            ("bc1 = INT32_MAX, large stride: beyond an int32 product", 0, FC.INT32_MAX, 1, FC.INT32_MAX, c.n_classes)):
        bc1, bc2 = c.bc1.copy(), c.bc2.copy()
        bc1[i], bc2[i] = b1, b2
        with pytest.raises(ValueError):
            FC.ref_classes(bc1, bc2, stride, ncl)
        rc, _, out = _gather(hc, d, Tables(c, bc1=bc1, bc2=bc2), c, room, stride=stride, n_classes=ncl)
        assert rc != 0 and "class index out of range" in _err(hc), what
        assert np.array_equal(out, _canary(room)), what
        if stride == c.stride:  # the largest valid values in the same place are taken
            bc1[i], bc2[i] = last, c.stride
            assert _gather(hc, d, Tables(c, bc1=bc1, bc2=bc2), c, room)[0] == 0, _err(hc)
        _gather_equals_reference(hc, c, exp)


def test_blocks_larger_than_out_cap_are_refused(hc):
    c = _base()
    exp, exp_bytes = _reference(c)
    total = len(exp)
    rc, class_bytes, out = _gather(hc, Text(c.text), Tables(c), c, total + CANARY, out_cap=total - 1)
    assert rc != 0 and "d_out holds %d" % (total - 1) in _err(hc) and "need %d" % total in _err(hc)
    assert np.array_equal(class_bytes, exp_bytes), "class_bytes is filled all the same"
    assert np.array_equal(out, _canary(total + CANARY)), "nothing was written"
    rc, class_bytes, out = _gather(hc, Text(c.text), Tables(c), c, total + CANARY, out_cap=total)  # exactly enough
    assert rc == 0 and np.array_equal(out[:total], exp) and np.array_equal(out[total:], _canary(total + CANARY)[total:])


TAMPERINGS = ("len = -1", "off = -1", "off + len = text_len + 1", "off = text_len + 1, len = 0")


def _tamper(c, how, k):
    """line k of the table: at most one byte outside the text, which lies PAD bytes inside its device buffer"""
    off, ln = c.off.copy(), c.len.copy()
    size = len(c.text)
    if how == "len = -1":
        ln[k] = -1
    elif how == "off = -1":
        off[k] = -1
    elif how == "off + len = text_len + 1":
        off[k] = size + 1 - int(ln[k])
    else:
        off[k], ln[k] = size + 1, 0
    assert -1 <= off[k] and off[k] + max(int(ln[k]), 0) <= size + 1 and PAD >= 1
    return off, ln


@pytest.mark.parametrize("how", TAMPERINGS)
def test_line_outside_the_text_is_refused_by_gather(hc, how):
    c = _base()
    d, exp = Text(c.text), _reference(c)
    room = len(c.text) + 4 + CANARY  # (a tampered table still needs at most text_len + 4)
    for line in range(4):
        off, ln = _tamper(c, how, 4 * 23 + line)
        rc, _, out = _gather(hc, d, Tables(c, off=off, ln=ln), c, room)
        assert rc != 0 and "lies outside the text" in _err(hc), (how, line)
        assert np.array_equal(out[len(c.text) + 4:], _canary(room)[len(c.text) + 4:])
    _gather_equals_reference(hc, c, exp)


@pytest.mark.parametrize("how", TAMPERINGS)
def test_sequence_line_outside_the_text_is_refused_by_pack(hc, how):
    c = _base()
    d = Text(c.text)
    off, ln = _tamper(c, how, 4 * 23 + 1)
    rc, _, _, _ = _pack(hc, d, off, ln, c.n)
    assert rc != 0 and "lies outside the text" in _err(hc), how
    seq, so = FC.ref_pack(c.text, c.off, c.len, c.n)
    rc, total, d_seq, d_so = _pack(hc, d, c.off, c.len, c.n)
    assert rc == 0 and total == len(seq) and np.array_equal(d_so[:c.n + 1].cpu().numpy(), so)
    assert np.array_equal(d_seq[:total].cpu().numpy(), seq)


def test_bad_scalar_arguments_are_refused_before_any_pointer_is_used(hc):
    class_bytes = np.full(8, -1, np.int64)

    def call(n=1, stride=1, n_classes=8, cb=class_bytes.ctypes.data, text_len=10, out_cap=100):
        return hc.lib.bdx_fq_gather_device(hc.h, None, text_len, None, None, n, None, None, stride, n_classes, None, None, 0, None, out_cap, cb)

    for kw, needle in ((dict(n=-1), "negative"), (dict(n=2 ** 32), "2^32 - 1"), (dict(n_classes=1), "n_classes must be >= 2"),
                       (dict(stride=0), "stride >= 1"), (dict(cb=None), "class_bytes is NULL"), (dict(text_len=-1), "negative"),
                       (dict(out_cap=-1), "negative"), (dict(), "NULL device pointer")):
        assert call(**kw) != 0 and needle in _err(hc), (kw, _err(hc))
    class_bytes[:] = 7
    assert call(n=0) == 0 and not class_bytes.any(), "n = 0: no record, every class 0 bytes"
    _gather_equals_reference(hc, _base())
