"""Level 2 of the device gzip encoder on the MI355X, byte for byte: what bdx_fq_deflate_level_device(level 2) writes is
what the plain C++ build of the same text (tests/deflate2_core_host.cpp) writes — on the named edges of
tests/deflate2_cases.py and on the level-1 cases, with more chunks than workgroups, with both levels taking turns on one
context, and with nothing written past the members — and execute_demultiplexing(..., _gzip="device", _gzip_level=2)
writes files that gunzip to what _io="native" writes."""
import functools
import gzip
import os

import numpy as np
import pytest

import deflate2_cases as D2
import deflate_cases as DC
import helpers as H
from biodemux_jl_amd import synth
from test_device_gzip_gpu import _fastq, _need_gpu, _same_gunzipped, hc  # noqa: F401  (fixtures and helpers)

pytestmark = pytest.mark.gpu

LEADS = (0, 3)
BATCHES = 2  # calls per lead
ALL_CASES = D2.CASES + DC.CASES
WG_PER_CU = 3  # DFL2_WG_PER_CU of csrc/bdx_deflate.hip

run_nat = functools.partial(H.bdx.execute_demultiplexing, _io="native")
run_dgz2 = functools.partial(H.bdx.execute_demultiplexing, _io="device", _gzip="device", _gzip_level=2)


def _host(data: bytes, level=2) -> bytes:
    return D2.host_encoder().raw(data, level, fresh=True) if data else b""


def _deflate(hc, level, blocks, lead=0, canary=0):
    """bdx_fq_deflate_level_device over `blocks` (bytes per class, back to back `lead` bytes into a device buffer that
    ends with them); returns (rc, compressed bytes per class, class_cbytes, the `canary` bytes behind the bound)"""
    import torch

    lib = hc.lib
    cb = np.array([len(b) for b in blocks], dtype=np.int64)
    cap = int(lib.bdx_fq_deflate_bound(cb.ctypes.data, len(cb)))
    host = np.frombuffer(b"\0" * lead + b"".join(blocks), dtype=np.uint8)
    d_in = torch.from_numpy(host.copy()).to("cuda:0") if len(host) else torch.zeros(1, dtype=torch.uint8, device="cuda:0")
    d_out = torch.full((max(cap + canary, 1),), 0xC5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    zb = np.full(len(cb), -7, dtype=np.int64)
    rc = lib.bdx_fq_deflate_level_device(hc.h, level, d_in.data_ptr() + lead, cb.ctypes.data, len(cb), d_out.data_ptr(), cap, zb.ctypes.data)
    out = d_out.cpu().numpy().tobytes()
    if rc != 0:
        return rc, None, zb, out
    assert int(zb.sum()) <= cap
    parts, pos = [], 0
    for z in zb:
        parts.append(out[pos:pos + int(z)])
        pos += int(z)
    return rc, parts, zb, out[pos:]


@pytest.fixture(scope="module")
def device_case_bytes(hc):
    """{(case name, lead): the class block the device made at level 2}: every case a class of its own, half a call"""
    got = {}
    for lead in LEADS:
        for b in range(BATCHES):
            cases = ALL_CASES[b::BATCHES]
            rc, parts, _, _ = _deflate(hc, 2, [c.data for c in cases], lead=lead)
            assert rc == 0, hc.lib.bdx_last_error(hc.h)
            for c, part in zip(cases, parts):
                got[(c.name, lead)] = part
    return got


def _where(dev: bytes, host: bytes) -> str:
    """which stage differs, by the anatomy of the first member that does"""
    try:
        for k, (d, h) in enumerate(zip(DC.split_members(dev), DC.split_members(host))):
            if d == h:
                continue
            a, b = DC.anatomy(d), DC.anatomy(h)
            if a["btype"] != b["btype"]:
                return "member %d: device btype %d, host %d (codes / stored rule)" % (k, a["btype"], b["btype"])
            if a["tokens"] != b["tokens"]:
                i = next((i for i, (x, y) in enumerate(zip(a["tokens"], b["tokens"])) if x != y), min(len(a["tokens"]), len(b["tokens"])))
                return "member %d: tokens differ from #%d (hash / find / insert_walk / emit): device %s, host %s" % (
                    k, i, a["tokens"][i:i + 3], b["tokens"][i:i + 3])
            if (a["ll_lengths"], a["d_lengths"]) != (b["ll_lengths"], b["d_lengths"]):
                return "member %d: code lengths differ (rank / codes)" % k
            if D2.header_anatomy(d) != D2.header_anatomy(h):
                return "member %d: same tokens and codes, the header differs (header plan / header)" % k
            return "member %d: same tokens, codes and header, bits differ (pack / member)" % k
        return "member counts differ"
    except AssertionError as e:
        return "the device's block does not parse: %s" % e


@pytest.mark.parametrize("case", ALL_CASES, ids=repr)
def test_level_2_device_bytes_equal_host_build(device_case_bytes, case):
    want = _host(case.data)
    for lead in LEADS:
        dev = device_case_bytes[(case.name, lead)]
        assert dev == want, "lead %d: %s" % (lead, _where(dev, want))


def test_level_2_persistent_workgroups_reuse_their_state(hc):
    import torch

    grid = WG_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count
    n_chunks = 2 * grid + 3
    texts = DC.persistent_mix(n_chunks, grid)
    assert all(1 <= len(t) <= DC.CH for t in texts) and len(texts) == n_chunks  # one chunk per class
    want = [_host(t) for t in texts]
    rc, first, _, _ = _deflate(hc, 2, texts)
    assert rc == 0, hc.lib.bdx_last_error(hc.h)
    wrong = [c for c in range(n_chunks) if first[c] != want[c]]
    assert not wrong, "%d classes differ, the first is chunk %d (iteration %d of workgroup %d): %s" % (
        len(wrong), wrong[0], wrong[0] // grid, wrong[0] % grid, _where(first[wrong[0]], want[wrong[0]]))
    rc, second, _, _ = _deflate(hc, 2, texts)
    assert rc == 0 and second == first


def test_levels_take_turns_on_one_context(hc):
    """level 1, level 2, level 1: the scratch buffers are shared, level 1's bytes are bdx_fq_deflate_device's both times"""
    from test_device_gzip_gpu import _deflate as deflate_old

    texts = [D2.fastq_varied(300), DC.text(5, "turn5"), b"", D2.fastq_constant(250), DC.text(DC.CH + 9, "turnch")]
    rc, old, _ = deflate_old(hc, texts)
    assert rc == 0 and old == [DC.host_encoder().raw(t, fresh=True) if t else b"" for t in texts]
    rc, a, _, _ = _deflate(hc, 1, texts)
    assert rc == 0 and a == old
    rc, b, _, _ = _deflate(hc, 2, texts, lead=1)
    assert rc == 0 and b == [_host(t) for t in texts]
    assert sum(map(len, b)) < sum(map(len, a))
    rc, c, _, _ = _deflate(hc, 1, texts)
    assert rc == 0 and c == old
    assert deflate_old(hc, texts)[1] == old


def test_level_2_compaction_writes_nothing_past_the_members(hc):
    blocks = [DC.text(5000, "l2compact5000"), b"", DC.text(70000, "l2compact70000")]
    rc, parts, zb, rest = _deflate(hc, 2, blocks, canary=4096)
    assert rc == 0, hc.lib.bdx_last_error(hc.h)
    want = [_host(b) for b in blocks]
    assert [int(z) for z in zb] == [len(w) for w in want] and parts == want  # class_cbytes
    assert len(rest) > 4096 and rest == b"\xC5" * len(rest)


@pytest.mark.parametrize("level", [0, 3])
def test_a_bad_level_is_refused_and_the_context_works_on(hc, level):
    blocks = [DC.text(3000, "badlevel")]
    rc, parts, zb, out = _deflate(hc, level, blocks, canary=64)
    assert rc == -1 and parts is None and list(zb) == [0]
    assert b"deflate level %d" % level in hc.lib.bdx_last_error(hc.h)
    assert out == b"\xC5" * len(out)  # nothing launched
    rc, parts, _, _ = _deflate(hc, 2, blocks)
    assert rc == 0 and parts == [_host(blocks[0])]


# ---- end to end ----
def _dual_case(tmp_path, n=3000):
    b1 = synth.make_barcodes(24, 24, seed=1)
    b2 = synth.make_barcodes(16, 24, seed=2)
    seq, off, _ = synth.make_reads(b1, n, 150, seed=78, plant_lo=0, plant_hi=40, second=(b2, 100, 126))
    fq = str(tmp_path / "dual.fastq")
    _fastq(fq, [seq[off[i]:off[i + 1]].tobytes() for i in range(n)])
    f1, f2 = tmp_path / "b1.csv", tmp_path / "b2.csv"
    f1.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"x{i},{b},{'B' * len(b)}\n" for i, b in enumerate(b1)))
    f2.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"y{i},{b},{'B' * len(b)}\n" for i, b in enumerate(b2)))
    return fq, str(f1), str(f2)


def test_pipeline_at_level_2_equals_native(tmp_path):
    fq, f1, f2 = _dual_case(tmp_path)
    kw = dict(barcode_file2=f2, max_error_rate=0.2, trim_side=5, trim_side2=3, _batch_reads=1100, gzip_output=True)
    t1, t2 = {}, {}
    a = run_nat(fq, f1, str(tmp_path / "nat"), **kw)
    b = run_dgz2(fq, f1, str(tmp_path / "dev2"), _timings=t2, **kw)
    _same_gunzipped(str(tmp_path / "nat"), str(tmp_path / "dev2"))
    assert vars(a) == vars(b) and a.matched_reads > 0
    c = H.bdx.execute_demultiplexing(fq, f1, str(tmp_path / "dev1"), _io="device", _gzip="device", _timings=t1, **kw)
    assert vars(a) == vars(c)
    assert (t1["gzip_level"], t2["gzip_level"]) == (1, 2) and t1["plain_bytes"] == t2["plain_bytes"]
    assert 0 < t2["compressed_bytes"] < t1["compressed_bytes"] and t2["deflate_s"] > 0


def test_level_2_output_read_back_by_device_gunzip(tmp_path):
    """the demultiplexing of a file level 2 wrote, inflated on the device, is that of its plain text"""
    bcs = synth.make_barcodes(6, 12, seed=9, min_hamming=4)
    seq, off, _ = synth.make_ragged_reads(bcs, 3000, 0, 90, seed=9)
    fq = str(tmp_path / "reads.fastq")
    _fastq(fq, [seq[off[i]:off[i + 1]].tobytes() for i in range(3000)])
    bc = tmp_path / "bc.csv"
    bc.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"b{i},{b},{'B' * len(b)}\n" for i, b in enumerate(bcs)))
    first = tmp_path / "first"
    run_dgz2(fq, str(bc), str(first), max_error_rate=0.2, gzip_output=True, _batch_reads=1100)
    src = max(first.iterdir(), key=lambda p: p.stat().st_size)
    assert src.name.endswith(".gz") and len(DC.split_members(src.read_bytes())) > 1
    plain = tmp_path / "plain.fastq"
    plain.write_bytes(gzip.open(src).read())
    kw = dict(max_error_rate=0.2, trim_side=3, _batch_reads=500, gzip_output=True)
    a = run_nat(str(plain), str(bc), str(tmp_path / "from_plain"), output_prefix="x", **kw)
    b = run_dgz2(str(src), str(bc), str(tmp_path / "from_gz"), output_prefix="x", _gunzip="device", **kw)
    _same_gunzipped(str(tmp_path / "from_plain"), str(tmp_path / "from_gz"))
    assert vars(a) == vars(b) and a.total_reads > 50


def test_reference_golden_through_level_2(tmp_path):
    """demo1_R1 of the reference's results, byte-exact after gunzip"""
    src = os.path.join(H.REF, "FASTQ_files", "demo1_R1")
    out = str(tmp_path / "out")
    for f in sorted(os.listdir(src)):
        run_dgz2(os.path.join(src, f), os.path.join(H.REF, "reference_files", "demo1.tsv"), out, gzip_output=True)
    ideal = os.path.join(H.REF, "results", "demo1_R1")
    names = sorted(os.listdir(ideal))
    assert len(names) == 24
    for name in names:
        got = [p for p in (os.path.join(out, name), os.path.join(out, name + ".gz")) if os.path.isfile(p)]
        assert len(got) == 1, name
        raw = open(got[0], "rb").read()
        assert raw[:4] == b"\x1f\x8b\x08\x04", "a chain of device members"
        assert gzip.decompress(raw) == H._read_maybe_gz(os.path.join(ideal, name)), name
