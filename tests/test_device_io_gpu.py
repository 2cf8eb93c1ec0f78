"""The device FASTQ pipeline on the MI355X: every device step equals its host partner of csrc/bdx_io.cpp (index, pack),
the reference goldens come out byte-exact through _io="device", and _io="device" writes the same files, counters and
reports as _io="native" with the same HIP classifier."""
import ctypes as C
import functools
import gzip
import os
import threading

import numpy as np
import pytest

import helpers as H
from biodemux_jl_amd import nativeio, synth

pytestmark = pytest.mark.gpu

run_dev = functools.partial(H.bdx.execute_demultiplexing, _io="device")
run_nat = functools.partial(H.bdx.execute_demultiplexing, _io="native")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    nativeio.build()


# ---- the device steps against their host partners ----
def _dev(arr):
    import torch

    t = torch.from_numpy(np.array(arr, copy=True)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _empty(n, dtype):
    import torch

    return torch.empty(max(int(n), 1), dtype=dtype, device="cuda:0")


def _ctx():
    cfg = H.bdx.DemuxConfig(bc_seqs=["ACGTACGT"], bc_lengths_no_N=[8], ids=["a"])
    return H.bdx.HipClassifier(cfg)


def _index_dev(hc, text: bytes, final: int, max_reads: int, offset: int = 0):
    """bdx_fq_index_device over text (placed `offset` bytes into a device buffer: unaligned starts too)"""
    import torch

    buf = _dev(np.frombuffer(b"\0" * offset + text + b"\0", dtype=np.uint8))
    off = _empty(4 * max_reads, torch.int64)
    ln = _empty(4 * max_reads, torch.int32)
    n, nxt = C.c_int64(), C.c_int64()
    hc._check(hc.lib.bdx_fq_index_device(hc.h, buf.data_ptr() + offset, len(text), final, max_reads, off.data_ptr(),
                                         ln.data_ptr(), C.byref(n), C.byref(nxt)))
    k = 4 * n.value
    return n.value, nxt.value, off[:k].cpu().numpy(), ln[:k].cpu().numpy(), (buf, off, ln)


def _index_host(tmp_path, text: bytes, max_reads: int):
    p = tmp_path / "t.fastq"
    p.write_bytes(text)
    f = nativeio.FastqFile(str(p))
    try:
        n, off, ln = f.next_batch(max_reads, 4)
        return n, f.cursor, off[:4 * n].copy(), ln[:4 * n].copy()
    finally:
        f.close()


def _expect_not_final(tmp_path, text: bytes, max_reads: int):
    """final == 0: the complete records only — the host index of the text, cut after the last whole record"""
    nl = [i for i, b in enumerate(text) if b == 10]
    k = min(len(nl), 4 * max_reads)
    k -= k % 4
    n, _, off, ln = _index_host(tmp_path, text, max(max_reads, 1))
    return k // 4, (nl[k - 1] + 1 if k else 0), off[:k], ln[:k]


def _texts():
    rng = np.random.default_rng(3)
    long_reads = b"".join(b"@long%d\n" % i + bytes(rng.choice(list(b"ACGT"), 10000)) + b"\n+\n" + b"F" * 10000 + b"\n"
                          for i in range(5))
    plain = b"".join(b"@r%d x\nACGTACGTAA\n+\nIIIIIIIIII\n" % i for i in range(300))
    return {
        "plain": plain,
        "crlf": plain.replace(b"\n", b"\r\n"),
        "no_final_newline": plain + b"@x\nACGT\n+\nIIII",
        "truncated": plain + b"@last\nACGTAC",
        "blank_trailing_line": plain + b"\n",
        "zero_length_lines": b"@a\n\n+\n\n@b\r\n\r\n+\r\n\r\n" + plain + b"\n\n\n",
        "cr_only_lines": b"@a\r\n\r\nACGT\n\r\n" * 9,
        "long_reads": long_reads,
        "empty_text": b"",
        "only_newlines": b"\n" * 37,
    }


@pytest.mark.parametrize("name", list(_texts()))
def test_index_equals_host_index(tmp_path, name):
    text = _texts()[name]
    with _ctx() as hc:
        for max_reads in (1, 3, 7, 100000):
            for offset in (0, 5):
                if not text:
                    continue
                got = _index_dev(hc, text, 1, max_reads, offset)[:4]
                exp = _index_host(tmp_path, text, max_reads)
                assert got[0] == exp[0] and got[1] == exp[1], (max_reads, offset, got[:2], exp[:2])
                assert np.array_equal(got[2], exp[2]) and np.array_equal(got[3], exp[3]), (max_reads, offset)
                got = _index_dev(hc, text, 0, max_reads, offset)[:4]
                exp = _expect_not_final(tmp_path, text, max_reads)
                assert got[0] == exp[0] and got[1] == exp[1], ("final=0", max_reads, offset, got[:2], exp[:2])
                assert np.array_equal(got[2], exp[2]) and np.array_equal(got[3], exp[3]), ("final=0", max_reads)
        assert _index_dev(hc, b"", 1, 10)[:2] == (0, 0)


def test_index_of_windows_that_cut_a_record(tmp_path):
    text = _texts()["crlf"] + _texts()["long_reads"]
    rng = np.random.default_rng(11)
    cuts = sorted(set(int(c) for c in rng.integers(1, len(text), 40))) + [len(text) - 1, len(text)]
    with _ctx() as hc:
        for cut in cuts:
            w = text[:cut]
            got = _index_dev(hc, w, 1, 100000)[:4]  # final: the window is all there is (a truncated file)
            exp = _index_host(tmp_path, w, 100000)
            assert got[:2] == exp[:2] and np.array_equal(got[2], exp[2]) and np.array_equal(got[3], exp[3]), cut
            got = _index_dev(hc, w, 0, 100000)[:4]  # more text follows: whole records only
            exp = _expect_not_final(tmp_path, w, 100000)
            assert got[:2] == exp[:2] and np.array_equal(got[2], exp[2]) and np.array_equal(got[3], exp[3]), cut


@pytest.mark.parametrize("name", ["plain", "crlf", "truncated", "zero_length_lines", "long_reads"])
def test_pack_equals_host_pack(tmp_path, name):
    import torch

    text = _texts()[name]
    with _ctx() as hc:
        n, _, _, _, (buf, off, ln) = _index_dev(hc, text, 1, 100000)
        seq = _empty(len(text) + 1, torch.uint8)
        so = _empty(n + 1, torch.int64)
        total = C.c_int64()
        hc._check(hc.lib.bdx_fq_pack_device(hc.h, buf.data_ptr(), len(text), off.data_ptr(), ln.data_ptr(), n, seq.data_ptr(),
                                            seq.numel(), so.data_ptr(), C.byref(total)))
        p = tmp_path / "p.fastq"
        p.write_bytes(text)
        f = nativeio.FastqFile(str(p))
        try:
            hn, hoff, hln = f.next_batch(100000, 4)
            hseq, hso = f.pack(hoff, hln, hn, 4)
        finally:
            f.close()
        assert n == hn and total.value == len(hseq)
        assert np.array_equal(so.cpu().numpy(), hso)
        assert seq[:total.value].cpu().numpy().tobytes() == hseq.tobytes()
        # a d_seq too small is refused, not overrun
        if total.value:
            rc = hc.lib.bdx_fq_pack_device(hc.h, buf.data_ptr(), len(text), off.data_ptr(), ln.data_ptr(), n, seq.data_ptr(),
                                           total.value - 1, so.data_ptr(), None)
            assert rc != 0 and b"d_seq holds" in hc.lib.bdx_last_error(hc.h)


# ---- goldens and the file contract through _io="device" ----
def test_goldens_through_device_io(tmp_path):
    assert H.scenario_demo1_R1(run_dev, str(tmp_path / "a")) == 24
    assert H.scenario_demo1_R2(run_dev, str(tmp_path / "b")) == 24
    assert H.scenario_demo2(run_dev, str(tmp_path / "c")) == 76  # gz in, paired, classify_both, revcomp


@pytest.mark.parametrize("scenario", H.SCENARIOS_SMALL, ids=[s.__name__ for s in H.SCENARIOS_SMALL])
def test_reference_scenarios_through_device_io(tmp_path, scenario):
    scenario(run_dev, str(tmp_path))


def _same_tree(a, b, skip_reports=False):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb
    for f in fa:
        if skip_reports and f.startswith("summary."):  # (run times differ)
            continue
        assert H._read_maybe_gz(os.path.join(a, f)) == H._read_maybe_gz(os.path.join(b, f)), f


def _fastq(path, seqs, crlf=False, tail=b"", gz=False, quals=None):
    nl = b"\r\n" if crlf else b"\n"
    quals = quals or [b"I" * len(s) for s in seqs]
    blob = b"".join(b"@r%d some header" % i + nl + s + nl + b"+" + nl + q + nl for i, (s, q) in enumerate(zip(seqs, quals))) + tail
    (gzip.open if gz else open)(path, "wb").write(blob)


def _both(tmp_path, args, **kw):
    """the same call through _io="native" and _io="device": same files, counters and summary tables"""
    a = run_nat(*args[:-1], str(tmp_path / "nat"), **kw)
    b = run_dev(*args[:-1], str(tmp_path / "dev"), **kw)
    _same_tree(str(tmp_path / "nat"), str(tmp_path / "dev"), skip_reports=bool(kw.get("summary")))
    assert vars(a) == vars(b)
    return a, b


def _single_case(tmp_path, n=700, lo=0, hi=90, seed=5):
    bcs = synth.make_barcodes(6, 12, seed=seed, min_hamming=4)
    seq, off, _ = synth.make_ragged_reads(bcs, n, lo, hi, seed=seed)
    seqs = [seq[off[i]:off[i + 1]].tobytes() for i in range(n)]
    bc = tmp_path / "bc.csv"
    bc.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"b{i},{b},{'B' * len(b)}\n" for i, b in enumerate(bcs)))
    return seqs, str(bc)


@pytest.mark.parametrize("case", ["plain", "crlf", "truncated", "blankline", "no_final_newline", "gz", "small_batches",
                                  "trim3", "batch1", "batch4000", "summary", "short_quals", "gz_out"])
def test_device_equals_native_io(tmp_path, case):
    seqs, bc = _single_case(tmp_path)
    tail = {"truncated": b"@last\nACGTAC", "blankline": b"\n", "no_final_newline": b"@x\nACGT\n+\nIIII"}.get(case, b"")
    quals = [b"I" * max(0, len(s) - 7) for s in seqs] if case == "short_quals" else None
    fq = str(tmp_path / ("reads.fastq.gz" if case == "gz" else "reads.fastq"))
    _fastq(fq, seqs, crlf=(case == "crlf"), tail=tail, gz=(case == "gz"), quals=quals)
    kw = dict(max_error_rate=0.2, trim_side=3 if case == "trim3" else 5)
    kw["_batch_reads"] = {"small_batches": 37, "batch1": 1, "batch4000": 4000}.get(case, 128)
    if case == "summary":
        kw.update(summary=True, summary_format="json")
    if case == "gz_out":
        kw["gzip_output"] = True
    _both(tmp_path, (fq, bc, None), **kw)
    if case == "gz_out":  # the device writer's members read back through the parallel inflate
        out = tmp_path / "dev"
        name = max(os.listdir(out), key=lambda f: os.path.getsize(out / f))
        f = nativeio.FastqFile(str(out / name), 4)
        try:
            assert C.c_int32(nativeio._load().bdx_fq_parallel_inflate(f.h)).value == 1
        finally:
            f.close()


@pytest.mark.parametrize("trim", [(5, 3), (3, 5)])
def test_device_equals_native_dual_many_classes(tmp_path, trim):
    """24 x 16 barcodes: 386 classes, two passes of the counting sort; both trim sides"""
    b1 = synth.make_barcodes(24, 24, seed=1)
    b2 = synth.make_barcodes(16, 24, seed=2)
    seq, off, _ = synth.make_reads(b1, 6000, 150, seed=77, plant_lo=0, plant_hi=40, second=(b2, 100, 126))
    seqs = [seq[off[i]:off[i + 1]].tobytes() for i in range(6000)]
    fq = str(tmp_path / "dual.fastq")
    _fastq(fq, seqs)
    f1, f2 = tmp_path / "b1.csv", tmp_path / "b2.csv"
    f1.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"x{i},{b},{'B' * len(b)}\n" for i, b in enumerate(b1)))
    f2.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"y{i},{b},{'B' * len(b)}\n" for i, b in enumerate(b2)))
    a, _ = _both(tmp_path, (fq, str(f1), None), barcode_file2=str(f2), max_error_rate=0.2, trim_side=trim[0],
                 trim_side2=trim[1], _batch_reads=2500)
    assert len(os.listdir(tmp_path / "dev")) > 100 and a.matched_reads > 0


@pytest.mark.parametrize("both", [False, True])
def test_device_equals_native_paired(tmp_path, both):
    """R2 shorter than R1: stop at the shorter file; classify_both trims R1 only"""
    bcs = synth.make_barcodes(5, 12, seed=6, min_hamming=4)
    seq, off, _ = synth.make_reads(bcs, 500, 60, seed=6)
    s1 = [seq[off[i]:off[i + 1]].tobytes() for i in range(500)]
    s2 = [b"ACGT" * 10 for _ in range(430)]
    bc = tmp_path / "bc.tsv"
    bc.write_text("ID\tFull_seq\tFull_annotation\n" + "".join(f"b{i}\t{b}\t{'B' * len(b)}\n" for i, b in enumerate(bcs)))
    f1, f2 = str(tmp_path / "x_R1.fastq"), str(tmp_path / "x_R2.fastq")
    _fastq(f1, s1)
    _fastq(f2, s2)
    a, _ = _both(tmp_path, (f1, f2, str(bc), None), classify_both=both, trim_side=3, _batch_reads=128)
    assert a.total_reads == 430


def test_device_equals_native_streamed_gz_pairs(tmp_path):
    seqs, bc = _single_case(tmp_path, n=3000, lo=0, hi=120, seed=7)
    f1, f2 = str(tmp_path / "y_R1.fastq.gz"), str(tmp_path / "y_R2.fastq.gz")
    _fastq(f1, seqs, gz=True, tail=b"@last\nACGTAC")
    _fastq(f2, [b"TTGCA" * 9 for _ in seqs] + [b"ACGT"], gz=True)
    _both(tmp_path, (f1, f2, bc, None), classify_both=True, trim_side=5, _batch_reads=211)


def test_device_c2_shape_two_million_reads(tmp_path):
    n = 2_000_000
    bcs = synth.make_barcodes(96, 24, seed=synth.SEED)
    seq, off, _ = synth.make_reads(bcs, n, 150, seed=synth.SEED)
    rec = np.empty((n, 319), dtype=np.uint8)
    rec[:, 0:5] = np.frombuffer(b"@read", dtype=np.uint8)
    ids = np.arange(n, dtype=np.int64)
    for k in range(9):
        rec[:, 13 - k] = (ids // 10 ** k % 10 + 48).astype(np.uint8)
    rec[:, 14] = 10
    rec[:, 15:165] = seq.reshape(n, 150)
    rec[:, 165:168] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 168:318] = ord("F")
    rec[:, 318] = 10
    fq = str(tmp_path / "c2.fastq")
    rec.tofile(fq)
    del rec, seq, off
    bc = tmp_path / "bc.csv"
    bc.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"bc{i + 1:03d},{b},{'B' * 24}\n" for i, b in enumerate(bcs)))
    tm = {}
    a = run_nat(fq, str(bc), str(tmp_path / "nat"), max_error_rate=0.1)
    b = run_dev(fq, str(bc), str(tmp_path / "dev"), max_error_rate=0.1, _timings=tm)
    _same_tree(str(tmp_path / "nat"), str(tmp_path / "dev"))
    assert vars(a) == vars(b) and b.total_reads == n
    for k in ("upload_s", "device_s", "download_s", "write_s"):
        assert tm[k] > 0, k
    assert tm["batches"] == -(-n // (1 << 19))


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
    assert not t.is_alive(), "the device pipeline hangs on an error"
    return result


def test_device_errors_propagate_instead_of_hanging(tmp_path):
    seqs, bc = _single_case(tmp_path, n=6000, lo=20, hi=60, seed=9)
    good = str(tmp_path / "good.fastq.gz")
    _fastq(good, seqs, gz=True)
    blob = open(good, "rb").read()
    bad = str(tmp_path / "bad.fastq.gz")
    open(bad, "wb").write(blob[:len(blob) // 2] + b"\x00" * 64 + blob[len(blob) // 2 + 64:])
    r = _in_thread(lambda: run_dev(bad, bc, str(tmp_path / "o1"), _batch_reads=100))
    assert isinstance(r.get("err"), OSError), r
    r = _in_thread(lambda: run_dev(good, str(tmp_path / "missing_R2.fastq"), bc, str(tmp_path / "o2"), _batch_reads=100))
    assert isinstance(r.get("err"), OSError), r
    # the writer fails while most batches are still to come: a directory stands where the busiest output file goes
    # (open() gives EISDIR on the host; nothing is wrong on the device)
    ref = tmp_path / "ref"
    run_nat(good, bc, str(ref), _batch_reads=1000)
    busiest = max(os.listdir(ref), key=lambda f: os.path.getsize(ref / f))
    (tmp_path / "o4" / busiest).mkdir(parents=True)
    r = _in_thread(lambda: run_dev(good, bc, str(tmp_path / "o4"), _batch_reads=100))
    assert isinstance(r.get("err"), OSError), r
    # the context is usable afterwards: a good run in the same process
    r = _in_thread(lambda: run_dev(good, bc, str(tmp_path / "o3"), _batch_reads=1000))
    assert r.get("ok"), r


# ---- the short-index retry of the modes that upload a window again, and the _timings keys of every mode ----
def _bgzf_file(path, blob, seed=1):
    """`blob` as a chain of BGZF members of 1 .. 4000 plain bytes and the empty end marker"""
    import inflate_cases as IC

    rng = np.random.default_rng(seed)
    cuts = [0]
    while cuts[-1] < len(blob):
        cuts.append(cuts[-1] + int(rng.integers(1, 4001)))
    with open(path, "wb") as f:
        for a, b in zip(cuts, cuts[1:]):
            f.write(IC.zmember("m", blob[a:b], tag="BC", level=int(rng.integers(0, 10))).comp)
        f.write(IC.zmember("eof", b"", tag="BC").comp)
    assert gzip.open(path).read() == blob


def test_a_record_longer_than_the_window_is_uploaded_again_in_every_mode_that_uploads(tmp_path):
    """Five short reads, then one record of 200 000 bases (400 KB with its qualities).  With _batch_reads=1 a window is
    1 * 330 * 1.05 + 65536 = 65 882 bytes at the start and smaller once the short reads set the average: the index of the
    long record's batch comes back empty and the window is uploaded again at twice the size, three times (132, 264, 528 KB),
    from the calling thread.  The plain file and the host-inflated .gz upload text again; the size-tagged members upload
    the compressed members again and inflate them again: the last of the four uploads alone covers the file from the cursor's
    member on, and the three before it 66, 132 and 264 KB of text each, so more compressed bytes go up than the file has."""
    seqs, bc = _single_case(tmp_path, n=5)
    seqs.append(b"ACGT" * 50000)
    plain = str(tmp_path / "long.fastq")
    _fastq(plain, seqs)
    blob = open(plain, "rb").read()
    ordinary, tagged = str(tmp_path / "ordinary" / "long.fastq.gz"), str(tmp_path / "tagged" / "long.fastq.gz")
    for p in (ordinary, tagged):
        os.mkdir(os.path.dirname(p))
    with gzip.open(ordinary, "wb") as f:
        f.write(blob)
    _bgzf_file(tagged, blob)
    kw = dict(max_error_rate=0.2, trim_side=5, _batch_reads=1)
    for name, fq, more in (("plain", plain, {}), ("host", ordinary, dict(_gunzip="host")), ("members", tagged, dict(_gunzip="device"))):
        nat, dev = str(tmp_path / f"nat_{name}"), str(tmp_path / f"dev_{name}")
        tm = {}
        a = run_nat(fq, bc, nat, **kw)
        b = run_dev(fq, bc, dev, _timings=tm, **kw, **more)
        _same_tree(nat, dev)
        assert vars(a) == vars(b) and a.total_reads == 6, name
    assert tm["compressed_in_bytes"] > os.path.getsize(tagged) and tm["batches"] == 6  # (the members leg ran last)


_T_CALL = {"setup_s", "pre_s", "close_s", "total_s"}  # execute_demultiplexing's own
_T_DEVICE = _T_CALL | {"upload_s", "device_s", "download_s", "write_s", "batches", "wall_s", "threads"}
_T_DEFLATE = {"deflate_s", "plain_bytes", "compressed_bytes", "gzip_level"}
_T_INFLATE = {"inflate_s", "compressed_in_bytes", "plain_in_bytes"}
_T_STREAM = _T_INFLATE | {"stream_members", "stream_chunks", "stream_confirmed", "stream_discarded", "stream_no_candidate",
                          "stream_longest_segment"}
_T_DEAL = _T_CALL | {"devices", "upload_s", "device_s", "phase_wait_s", "download_s", "write_s", "batches", "spans",
                     "spans_per_device", "span_bytes", "wall_s", "threads"}
# mode -> (the input, execute_demultiplexing's arguments, the keys _timings then has: all of them, and no other)
TIMINGS_KEYS = {
    "device": ("plain", dict(_io="device"), _T_DEVICE),
    "device gzip=device": ("plain", dict(_io="device", _gzip="device", gzip_output=True), _T_DEVICE | _T_DEFLATE),
    "gunzip=device": ("tagged", dict(_io="device", _gunzip="device"), _T_DEVICE | _T_INFLATE),
    "gunzip=device-stream": ("ordinary", dict(_io="device", _gunzip="device-stream"), _T_DEVICE | _T_STREAM),
    "gunzip=device-window": ("ordinary", dict(_io="device", _gunzip="device-window"),
                             _T_DEVICE | _T_STREAM | {"stream_windows", "stream_window_bytes", "stream_text_peak_bytes"}),
    "deal": ("plain", dict(_io="device-deal", devices=[0, 0]), _T_DEAL),
    "deal gzip=device": ("plain", dict(_io="device-deal", devices=[0, 0], _gzip="device", gzip_output=True), _T_DEAL | _T_DEFLATE),
}


@pytest.fixture(scope="module")
def timing_inputs(tmp_path_factory):
    """2000 ragged reads three times: plain, one ordinary gzip member, a chain of BGZF members"""
    d = tmp_path_factory.mktemp("timings")
    seqs, bc = _single_case(d, n=2000)
    paths = {k: str(d / k / ("reads.fastq" if k == "plain" else "reads.fastq.gz")) for k in ("plain", "ordinary", "tagged")}
    for p in paths.values():
        os.mkdir(os.path.dirname(p))
    _fastq(paths["plain"], seqs)
    blob = open(paths["plain"], "rb").read()
    with gzip.open(paths["ordinary"], "wb") as f:
        f.write(blob)
    _bgzf_file(paths["tagged"], blob, seed=2)
    return paths, bc


@pytest.mark.parametrize("mode", list(TIMINGS_KEYS))
def test_timings_keys_of_every_device_mode(tmp_path, timing_inputs, mode):
    paths, bc = timing_inputs
    which, kw, keys = TIMINGS_KEYS[mode]
    tm = {}
    stats = H.bdx.execute_demultiplexing(paths[which], bc, str(tmp_path / "out"), max_error_rate=0.2, _batch_reads=700,
                                         _timings=tm, **kw)
    assert stats.total_reads == 2000
    assert set(tm) == keys, (sorted(set(tm) - keys), sorted(keys - set(tm)))
