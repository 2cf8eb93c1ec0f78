"""The stream inflate for ordinary .gz input (csrc/bdx_inflate_stream.hip) on the MI355X: bdx_fq_inflate_stream_device over
the cases of tests/inflate_stream_cases.py — the ones its plain C++ build is held to — with d_out between canaries and
the counters the cases module derives; and execute_demultiplexing(..., _io="device", _gunzip="device-stream") against
_gunzip="host" and the reference's golden outputs.  Bad files are refused here; that they are refused inside their
bounds is what the CPU and sanitizer runs prove."""
import ctypes as C
import functools
import gzip
import os

import numpy as np
import pytest

import helpers as H
import inflate_stream_cases as SC
from biodemux_jl_amd import deviceio, nativeio, synth
from biodemux_jl_amd.hipabi import BdxError

pytestmark = pytest.mark.gpu

run_host = functools.partial(H.bdx.execute_demultiplexing, _io="device", _gunzip="host")
run_stream = functools.partial(H.bdx.execute_demultiplexing, _io="device", _gunzip="device-stream")
CANARY, GUARD = 0xC5, 64
LEAD = 3  # the compressed file starts this far into its tensor
BDX_E_INVALID = -1


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


def _stream(hc, data: bytes, chunk: int, cap: int):
    """bdx_fq_inflate_stream_device: the file LEAD bytes into a tensor that ends with its last byte, d_out[0, cap) between
    two guards.  -> (rc, bytes or None, plain_len, info, error text, everything beside d_out[0, plain_len) untouched)"""
    import torch

    d_comp = torch.from_numpy(np.frombuffer(b"\0" * LEAD + data, dtype=np.uint8).copy()).to("cuda:0")
    d_out = torch.full((cap + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    plen, info = C.c_int64(-1), np.full(8, -1, dtype=np.int64)
    rc = hc.lib.bdx_fq_inflate_stream_device(hc.h, d_comp.data_ptr() + LEAD, len(data), chunk, d_out.data_ptr() + GUARD, cap, C.byref(plen),
                                             info.ctypes.data)
    out = d_out.cpu().numpy()
    used = plen.value if rc == 0 else 0
    keep = np.ones(len(out), dtype=bool)
    if rc != BDX_E_INVALID:  # (a refused file leaves d_out[0, cap) unspecified; the guards stay)
        keep[GUARD:GUARD + used] = False
    else:
        keep[GUARD:GUARD + cap] = False
    got = out[GUARD:GUARD + used].tobytes() if rc == 0 else None
    return rc, got, plen.value, info.tolist(), hc.lib.bdx_last_error(hc.h).decode(), bool((out[keep] == CANARY).all())


@pytest.mark.parametrize("k", range(len(SC.derived_cases())), ids=[c.name for c, _ in SC.derived_cases()])
def test_case_inflates_to_its_text_with_the_derived_counters(hc, k):
    case, plain = SC.derived_cases()[k]
    for chunk in SC.CHUNKS:
        rc, got, plen, info, err, intact = _stream(hc, case.data, chunk, len(plain))
        assert rc == 0 and intact, (case.name, chunk, err)
        assert plen == len(plain) and got == plain, (case.name, chunk)
        assert info == SC.expected_info(case, chunk), (case.name, chunk)


@pytest.mark.parametrize("part", range(4))
def test_zlib_is_the_arbiter(hc, part):
    cases = SC.arbiter_cases()[part::4]
    refused = 0
    for name, data in cases:
        want = SC.arbiter(data)
        for chunk in (64, 0):
            rc, got, _, _, err, intact = _stream(hc, data, chunk, len(want) if want is not None else 70000)
            assert intact, (name, chunk)
            if want is None:
                assert rc == BDX_E_INVALID and "gzip member" in err and "is refused: " in err and "compressed byte" in err, (name, chunk, rc, err)
                assert err.split("is refused: ")[1].split(" (status")[0] in set(SC.IC.STATUS.values()) - {"ok"}, err
            else:
                assert rc == 0 and got == want, (name, chunk, err)
        refused += want is None
    assert 0 < refused < len(cases)


def test_refusals_say_why(hc):
    by_name = dict(SC.arbiter_cases())
    for name, member, why in (("flipped_crc", 0, "CRC mismatch"), ("flipped_isize", 0, "ISIZE mismatch"),
                              ("flipped_crc_first_member", 0, "CRC mismatch"), ("reach_back_first_segment", 1, "distance too far"),
                              ("reach_back_later_segment", 1, "distance too far"), ("trailing_magic_alone", 1, "bad header")):
        for chunk in SC.CHUNKS:
            rc, _, _, _, err, intact = _stream(hc, by_name[name], chunk, 70000)
            assert rc == BDX_E_INVALID and intact and "gzip member %d " % member in err and why in err, (name, chunk, err)
    case, plain = SC.derived_cases()[5]
    assert _stream(hc, case.data, 64, len(plain))[:2] == (0, plain)  # the context is fine afterwards


def test_capacity(hc):
    for case, plain in SC.derived_cases()[:6]:
        n = len(plain)
        rc, got, plen, _, err, intact = _stream(hc, case.data, 64, n)
        assert (rc, got, plen, intact) == (0, plain, n, True), err
        for cap in (n - 1, 0):
            rc, got, plen, _, err, intact = _stream(hc, case.data, 64, cap)
            assert rc == SC.SPACE and plen == n and intact and str(n) in err, (case.name, cap, err)  # d_out keeps its fill


# ---- end to end ----
def test_demo2_gz_fixtures_equal_the_host_inflate_and_the_golden_outputs(tmp_path):
    """the reference's own .fastq.gz fixtures, paired: ordinary gzip files"""
    assert H.scenario_demo2(run_stream, str(tmp_path / "stream")) == 76  # (byte-identical to results/demo2)
    assert H.scenario_demo2(run_host, str(tmp_path / "host")) == 76
    a, b = tmp_path / "stream", tmp_path / "host"
    assert sorted(os.listdir(a)) == sorted(os.listdir(b))
    for f in os.listdir(a):
        assert (a / f).read_bytes() == (b / f).read_bytes(), f


def _records(seqs):
    return b"".join(b"@r%d some header\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n" for i, s in enumerate(seqs))


def _case(tmp_path, n=3000, seed=5):
    bcs = synth.make_barcodes(6, 12, seed=seed, min_hamming=4)
    seq, off, _ = synth.make_ragged_reads(bcs, n, 0, 90, seed=seed)
    blob = _records([seq[off[i]:off[i + 1]].tobytes() for i in range(n)])
    bc = tmp_path / "bc.csv"
    bc.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"b{i},{b},{'B' * len(b)}\n" for i, b in enumerate(bcs)))
    return blob, str(bc)


def _same_dirs(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb and fa
    for f in fa:
        assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), f


@pytest.mark.parametrize("batch, chunk", [(512, 0), (137, 256)])
def test_resident_text_in_many_batches_and_segments(tmp_path, monkeypatch, batch, chunk):
    """one ordinary gzip member (and one of two members); many batches are windows into the resident text"""
    blob, bc = _case(tmp_path)
    fq = str(tmp_path / "reads.fastq.gz")
    half = len(blob) // 2 + 7  # (inside a record)
    open(fq, "wb").write(gzip.compress(blob[:half], 6) + gzip.compress(blob[half:], 1) if chunk else gzip.compress(blob, 6))
    monkeypatch.setattr(deviceio, "STREAM_CHUNK", chunk)
    kw = dict(max_error_rate=0.2, trim_side=5, gzip_output=False, _batch_reads=batch)
    tm, th = {}, {}
    a = run_host(fq, bc, str(tmp_path / "host"), _timings=th, **kw)
    b = run_stream(fq, bc, str(tmp_path / "stream"), _timings=tm, **kw)
    _same_dirs(str(tmp_path / "host"), str(tmp_path / "stream"))
    assert vars(a) == vars(b) and a.total_reads == 3000 and tm["batches"] >= 3000 // batch
    assert tm["inflate_s"] > 0 and tm["compressed_in_bytes"] == os.path.getsize(fq) and tm["plain_in_bytes"] == len(blob)
    assert tm["stream_members"] == (2 if chunk else 1) and tm["stream_chunks"] == -(-os.path.getsize(fq) // (chunk or SC.DEFAULT_CHUNK))
    assert tm["stream_confirmed"] + tm["stream_discarded"] + tm["stream_no_candidate"] == tm["stream_chunks"] - 1
    assert "inflate_s" not in th and "stream_members" not in th
    plain = str(tmp_path / "plain.fastq")  # inert for a plain input
    open(plain, "wb").write(blob)
    tp = {}
    c = run_stream(plain, bc, str(tmp_path / "plain_out"), _timings=tp, output_prefix="reads", **kw)
    assert vars(a) == vars(c) and "inflate_s" not in tp


def test_paired_one_gz_one_plain(tmp_path):
    bcs = synth.make_barcodes(5, 12, seed=6, min_hamming=4)
    seq, off, _ = synth.make_reads(bcs, 500, 60, seed=6)
    bc = tmp_path / "bc.csv"
    bc.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"b{i},{b},{'B' * len(b)}\n" for i, b in enumerate(bcs)))
    f1, f2 = str(tmp_path / "x_R1.fastq.gz"), str(tmp_path / "x_R2.fastq")
    open(f1, "wb").write(gzip.compress(_records([seq[off[i]:off[i + 1]].tobytes() for i in range(500)])))
    open(f2, "wb").write(_records([b"ACGT" * 10 for _ in range(430)]))
    kw = dict(classify_both=True, trim_side=3, _batch_reads=128, gzip_output=False)
    a = run_host(f1, f2, str(bc), str(tmp_path / "host"), **kw)
    b = run_stream(f1, f2, str(bc), str(tmp_path / "stream"), **kw)
    _same_dirs(str(tmp_path / "host"), str(tmp_path / "stream"))
    assert vars(a) == vars(b) and a.total_reads == 430


def test_a_refused_member_names_the_file_and_trailing_bytes_follow_the_host(tmp_path):
    blob, bc = _case(tmp_path, n=400)
    good = gzip.compress(blob, 6)
    bad = str(tmp_path / "bad_crc.fastq.gz")
    open(bad, "wb").write(good[:-8] + bytes([good[-8] ^ 1]) + good[-7:])
    with pytest.raises(BdxError, match=r"bad_crc\.fastq\.gz: .*gzip member 0 .*CRC mismatch"):
        run_stream(bad, bc, str(tmp_path / "out"), max_error_rate=0.2)
    kw = dict(max_error_rate=0.2, gzip_output=False, output_prefix="reads")
    for name, tail in (("zeros", b"\0" * 9), ("junk", b"junk!"), ("magic", b"\x1f\x8bjunk, but long enough for a header")):
        fq = str(tmp_path / (name + ".fastq.gz"))
        open(fq, "wb").write(good + tail)
        verdict = []
        for tag, run in (("host", run_host), ("stream", run_stream)):
            try:
                verdict.append(vars(run(fq, bc, str(tmp_path / (name + "_" + tag)), **kw)))
            except Exception:  # noqa: BLE001 - refused, by whichever layer
                verdict.append(None)
        assert (verdict[0] is None) == (verdict[1] is None), (name, verdict)  # both accept or both refuse
        if verdict[0] is not None:
            assert verdict[0] == verdict[1] and verdict[0]["total_reads"] == 400
            _same_dirs(str(tmp_path / (name + "_host")), str(tmp_path / (name + "_stream")))
