"""Device gunzip (csrc/bdx_inflate.hip) on the MI355X: bdx_fq_inflate_device inflates every good member of
tests/inflate_cases.py into its slot and nothing beside it, refuses the bad ones by name, gives the same bytes in every
context, and execute_demultiplexing(..., _io="device", _gunzip="device") writes what _io="native" writes."""
import functools
import gzip
import os

import numpy as np
import pytest

import helpers as H
import inflate_cases as IC
from biodemux_jl_amd import nativeio, synth
from biodemux_jl_amd.hipabi import BdxError

pytestmark = pytest.mark.gpu

run_nat = functools.partial(H.bdx.execute_demultiplexing, _io="native")
run_dev = functools.partial(H.bdx.execute_demultiplexing, _io="device")
run_gun = functools.partial(H.bdx.execute_demultiplexing, _io="device", _gunzip="device")
CANARY = 0xC5
LEAD = 3  # the compressed input starts this far into its tensor


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    nativeio.build()


def _classifier():
    cfg = H.bdx.DemuxConfig(bc_seqs=["ACGTACGT"], bc_lengths_no_N=[8], ids=["a"])
    return H.bdx.HipClassifier(cfg)


@pytest.fixture(scope="module")
def hc():
    c = _classifier()
    yield c
    c.close()


def _inflate(hc, members):
    """bdx_fq_inflate_device over `members`: slots at odd byte offsets with canaries between them, the compressed bytes
    LEAD bytes into a tensor that ends with the last member's last byte.  -> (rc, status, slots, canaries intact, error)"""
    import torch

    comp = b"".join(m.comp for m in members)
    clen = np.array([len(m.comp) for m in members], dtype=np.int32)
    coff = (np.cumsum(clen, dtype=np.int64) - clen).astype(np.int64)
    plen = np.array([m.plen for m in members], dtype=np.int32)
    gaps = 5 + 2 * (np.arange(len(members) + 1) % 7)  # odd gaps: odd offsets whatever the sizes
    poff = np.zeros(len(members), dtype=np.int64)
    pos = 0
    for k in range(len(members)):
        pos += int(gaps[k])
        poff[k] = pos | 1
        pos = int(poff[k]) + int(plen[k])
    cap = pos + int(gaps[-1])
    d_comp = torch.from_numpy(np.frombuffer(b"\0" * LEAD + comp, dtype=np.uint8).copy()).to("cuda:0")
    d_out = torch.full((cap,), CANARY, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    status = np.full(len(members), -7, dtype=np.int32)
    rc = hc.lib.bdx_fq_inflate_device(hc.h, d_comp.data_ptr() + LEAD, coff.ctypes.data, clen.ctypes.data, poff.ctypes.data,
                                      plen.ctypes.data, len(members), d_out.data_ptr(), cap, status.ctypes.data)
    out = d_out.cpu().numpy()
    keep = np.ones(cap, dtype=bool)
    slots = []
    for o, n in zip(poff, plen):
        keep[int(o):int(o) + int(n)] = False
        slots.append(out[int(o):int(o) + int(n)].tobytes())
    return rc, status, slots, bool((out[keep] == CANARY).all()), hc.lib.bdx_last_error(hc.h).decode()


def test_every_good_member_in_one_call(hc):
    members = list(IC.good_members())
    assert len(members) >= 30
    rc, status, slots, intact, err = _inflate(hc, members)
    assert rc == 0, err
    assert status.tolist() == [0] * len(members) and intact
    for m, s in zip(members, slots):
        assert s == m.plain, m.name
    other = _classifier()  # the same call in a second context: the same bytes
    try:
        rc2, status2, slots2, intact2, _ = _inflate(other, members)
    finally:
        other.close()
    assert rc2 == 0 and intact2 and slots2 == slots and status2.tolist() == status.tolist()


def test_more_members_than_workgroups_and_no_members(hc):
    """a persistent grid: every workgroup decodes many members in turn, big and tiny ones mixed"""
    pool = [m for m in IC.good_members() if len(m.comp) < 2000]
    members = [pool[(7 * k) % len(pool)] for k in range(6000)] + list(IC.good_members())
    rc, status, slots, intact, err = _inflate(hc, members)
    assert rc == 0 and intact and not status.any(), err
    assert all(s == m.plain for m, s in zip(members, slots))
    assert hc.lib.bdx_fq_inflate_device(hc.h, None, None, None, None, None, 0, None, 0, None) == 0


def test_bad_members_among_good_ones(hc):
    good, bad = list(IC.good_members()), list(IC.bad_members())
    members, is_bad = [], []
    for k, m in enumerate(good):
        members.append(m)
        is_bad.append(False)
        if 2 <= k < 2 + len(bad):
            members.append(bad[k - 2])
            is_bad.append(True)
    assert sum(is_bad) == len(bad)
    rc, status, slots, intact, err = _inflate(hc, members)
    assert rc != 0 and intact
    assert [s != 0 for s in status.tolist()] == is_bad, status.tolist()
    for m, s, b in zip(members, slots, is_bad):
        assert b or s == m.plain, m.name
    first = is_bad.index(True)
    assert "member %d " % first in err and IC.STATUS[int(status[first])] in err
    expect = {"crc_bit": 10, "btype_3": 2, "stored_nlen": 3, "distance_before_start": 6, "isize_small": 7, "isize_large": 8,
              "truncated_9": 9, "oversubscribed_code_lengths": 4}
    for m, s in zip(members, status.tolist()):
        assert s == expect.get(m.name, s), (m.name, s)
    rc, status, _, intact, _ = _inflate(hc, good)  # the context is fine afterwards
    assert rc == 0 and intact and not status.any()


# ---- end to end: _io="device", _gunzip="device" against _io="native" on the same inputs ----
def _records(seqs):
    return b"".join(b"@r%d some header\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n" for i, s in enumerate(seqs))


def _bgzf(path, blob, seed, lo=1, hi=4000, end_marker=True):
    """`blob` as a BGZF file: members of lo .. hi plain bytes (boundaries fall inside records), then the empty end marker"""
    rng = np.random.default_rng(seed)
    out, p = [], 0
    while p < len(blob):
        n = int(rng.integers(lo, hi + 1))
        out.append(IC.zmember("m", blob[p:p + n], tag="BC", level=int(rng.integers(0, 10))).comp)
        p += n
    if end_marker:
        out.append(IC.zmember("eof", b"", tag="BC").comp)
    open(path, "wb").write(b"".join(out))
    assert gzip.open(path).read() == blob
    return len(out)


def _barcodes(tmp_path, bcs):
    bc = tmp_path / "bc.csv"
    bc.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"b{i},{b},{'B' * len(b)}\n" for i, b in enumerate(bcs)))
    return str(bc)


def _single_case(tmp_path, n=700, seed=5):
    bcs = synth.make_barcodes(6, 12, seed=seed, min_hamming=4)
    seq, off, _ = synth.make_ragged_reads(bcs, n, 0, 90, seed=seed)
    blob = _records([seq[off[i]:off[i + 1]].tobytes() for i in range(n)])
    fq = str(tmp_path / "reads.fastq.gz")
    assert _bgzf(fq, blob, seed) > 30
    return fq, _barcodes(tmp_path, bcs), blob


def _same_files(a, b, gunzipped):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb and fa
    for f in fa:
        if gunzipped:
            assert f.endswith(".gz") and gzip.open(os.path.join(b, f)).read() == gzip.open(os.path.join(a, f)).read(), f
        else:
            assert open(os.path.join(b, f), "rb").read() == open(os.path.join(a, f), "rb").read(), f


@pytest.mark.parametrize("batch", [128, 37])
def test_device_gunzip_equals_native_on_bgzf(tmp_path, batch):
    fq, bc, blob = _single_case(tmp_path)
    kw = dict(max_error_rate=0.2, trim_side=5, gzip_output=False, _batch_reads=batch)
    tm = {}
    a = run_nat(fq, bc, str(tmp_path / "nat"), **kw)
    b = run_gun(fq, bc, str(tmp_path / "dev"), _timings=tm, **kw)
    _same_files(str(tmp_path / "nat"), str(tmp_path / "dev"), gunzipped=False)
    assert vars(a) == vars(b) and a.total_reads == 700
    assert tm["inflate_s"] > 0 and 0 < tm["compressed_in_bytes"] < tm["plain_in_bytes"]
    assert tm["plain_in_bytes"] >= len(blob)


@pytest.mark.parametrize("batch", [128, 37])
def test_device_gzip_output_read_back_by_device_gunzip(tmp_path, batch):
    """a file first written by _gzip="device" is the input; gzip in -> gzip out, both on the device"""
    fq, bc, _ = _single_case(tmp_path, n=900, seed=9)
    first = tmp_path / "first"
    H.bdx.execute_demultiplexing(fq, bc, str(first), max_error_rate=0.2, gzip_output=True, _io="device", _gzip="device", _batch_reads=300)
    src = str(max(first.iterdir(), key=lambda p: p.stat().st_size))
    assert src.endswith(".gz")
    kw = dict(max_error_rate=0.2, trim_side=3, _batch_reads=batch)  # (gzip output follows the input's suffix)
    a = run_nat(src, bc, str(tmp_path / "nat"), **kw)
    b = run_gun(src, bc, str(tmp_path / "dev"), _gzip="device", **kw)
    _same_files(str(tmp_path / "nat"), str(tmp_path / "dev"), gunzipped=True)
    assert vars(a) == vars(b) and a.total_reads > 50
    c = run_gun(src, bc, str(tmp_path / "dev2"), _gzip="device", gzip_output=True, **kw)
    _same_files(str(tmp_path / "nat"), str(tmp_path / "dev2"), gunzipped=True)
    assert vars(a) == vars(c)


@pytest.mark.parametrize("second_gz", [True, False])
def test_device_gunzip_paired_classify_both(tmp_path, second_gz):
    bcs = synth.make_barcodes(5, 12, seed=6, min_hamming=4)
    seq, off, _ = synth.make_reads(bcs, 500, 60, seed=6)
    bc = _barcodes(tmp_path, bcs)
    f1 = str(tmp_path / "x_R1.fastq.gz")
    f2 = str(tmp_path / ("x_R2.fastq.gz" if second_gz else "x_R2.fastq"))
    _bgzf(f1, _records([seq[off[i]:off[i + 1]].tobytes() for i in range(500)]), 1)
    blob2 = _records([b"ACGT" * 10 for _ in range(430)])
    if second_gz:
        _bgzf(f2, blob2, 2, lo=200, hi=900, end_marker=False)
    else:
        open(f2, "wb").write(blob2)
    kw = dict(classify_both=True, trim_side=3, _batch_reads=128, gzip_output=False)
    tm = {}
    a = run_nat(f1, f2, bc, str(tmp_path / "nat"), **kw)
    b = run_gun(f1, f2, bc, str(tmp_path / "dev"), _timings=tm, **kw)
    _same_files(str(tmp_path / "nat"), str(tmp_path / "dev"), gunzipped=False)
    assert vars(a) == vars(b) and a.total_reads == 430 and tm["inflate_s"] > 0


def test_ordinary_gzip_input_is_refused_before_the_output_directory(tmp_path):
    _, bc, blob = _single_case(tmp_path)
    fq = str(tmp_path / "ordinary.fastq.gz")
    with gzip.open(fq, "wb") as f:
        f.write(blob)
    out = tmp_path / "never_made"
    with pytest.raises(ValueError, match="ordinary.fastq.gz.*no size tag"):
        run_gun(fq, bc, str(out), max_error_rate=0.2)
    assert not out.exists()
    assert run_dev(fq, bc, str(tmp_path / "host"), max_error_rate=0.2).total_reads == 700  # the host inflate takes it


def test_wrong_crc_in_the_third_member_names_it(tmp_path):
    fq, bc, blob = _single_case(tmp_path)
    g = nativeio.GzMembers(fq, IC.MEMBER_MAX)
    try:
        at = int(g.comp_off[2] + g.comp_len[2]) - 8
    finally:
        g.close()
    raw = bytearray(open(fq, "rb").read())
    raw[at] ^= 1
    bad = str(tmp_path / "bad_crc.fastq.gz")
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(BdxError, match=r"bad_crc\.fastq\.gz: gzip member 2 .*CRC mismatch"):
        run_gun(bad, bc, str(tmp_path / "out"), max_error_rate=0.2, _batch_reads=128)


def test_host_gunzip_stays_the_default(tmp_path):
    fq, bc, _ = _single_case(tmp_path)
    kw = dict(max_error_rate=0.2, trim_side=5, gzip_output=False, _batch_reads=128)
    a = run_nat(fq, bc, str(tmp_path / "nat"), **kw)
    for name, extra in (("default", {}), ("host", dict(_gunzip="host"))):
        tm = {}
        b = run_dev(fq, bc, str(tmp_path / name), _timings=tm, **extra, **kw)
        _same_files(str(tmp_path / "nat"), str(tmp_path / name), gunzipped=False)
        assert vars(a) == vars(b) and "inflate_s" not in tm and "compressed_in_bytes" not in tm
    plain = str(tmp_path / "plain.fastq")  # inert for a plain input
    open(plain, "wb").write(gzip.open(fq).read())
    tm = {}
    c = run_gun(plain, bc, str(tmp_path / "plain_dev"), _timings=tm, output_prefix="reads", **kw)
    assert vars(a) == vars(c) and "inflate_s" not in tm
