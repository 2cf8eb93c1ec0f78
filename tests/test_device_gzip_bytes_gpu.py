"""Device gzip on the MI355X, byte for byte: what bdx_fq_deflate_device writes is what the plain C++ build of the same
encoder text (tests/deflate_core_host.cpp) writes, on the cases of tests/deflate_cases.py — each proven on the CPU
(test_device_gzip_cpu.py) to reach the edge it is named for — with more chunks than workgroups, with runs of one, two
and three members per thread of the scan kernel, and with nothing written past the members.  The reference in every
test is the host build's bytes, compared with == ."""
import numpy as np
import pytest

import deflate_cases as DC
from test_device_gzip_gpu import _deflate, _need_gpu, _walk, hc  # noqa: F401  (fixtures and helpers)

pytestmark = pytest.mark.gpu

LEADS = (0, 3)
BATCHES = 3  # calls per lead: about six calls for all cases


def _host(data: bytes) -> bytes:
    return DC.host_encoder().raw(data, fresh=True) if data else b""


@pytest.fixture(scope="module")
def device_case_bytes(hc):
    """{(case name, lead): the class block the device made}: every case a class of its own, a third of the cases per call"""
    got = {}
    for lead in LEADS:
        for b in range(BATCHES):
            cases = DC.CASES[b::BATCHES]
            rc, parts, _ = _deflate(hc, [c.data for c in cases], lead=lead)
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
                return "member %d: tokens differ from #%d (find / insert_walk / emit): device %s, host %s" % (
                    k, i, a["tokens"][i:i + 3], b["tokens"][i:i + 3])
            if (a["ll_lengths"], a["d_lengths"]) != (b["ll_lengths"], b["d_lengths"]):
                return "member %d: code lengths differ (rank / codes)" % k
            return "member %d: same tokens and codes, bits differ (pack / member)" % k
        return "member counts differ"
    except AssertionError as e:
        return "the device's block does not parse: %s" % e


@pytest.mark.parametrize("case", DC.CASES, ids=repr)
def test_device_bytes_equal_host_build(device_case_bytes, case):
    want = _host(case.data)
    for lead in LEADS:
        dev = device_case_bytes[(case.name, lead)]
        assert dev == want, "lead %d: %s" % (lead, _where(dev, want))


def test_persistent_workgroups_reuse_their_state(hc):
    import torch

    grid = 4 * torch.cuda.get_device_properties(0).multi_processor_count  # 4: DFL_WG_PER_CU of csrc/bdx_deflate.hip
    n_chunks = 2 * grid + 3
    texts = DC.persistent_mix(n_chunks, grid)
    assert all(1 <= len(t) <= DC.CH for t in texts) and len(texts) == n_chunks  # one chunk per class
    assert n_chunks > 2 * grid  # some workgroups encode a third chunk, all a second
    want = [_host(t) for t in texts]
    rc, first, _ = _deflate(hc, texts)
    assert rc == 0, hc.lib.bdx_last_error(hc.h)
    wrong = [c for c in range(n_chunks) if first[c] != want[c]]
    assert not wrong, "%d classes differ, the first is chunk %d (iteration %d of workgroup %d): %s" % (
        len(wrong), wrong[0], wrong[0] // grid, wrong[0] % grid, _where(first[wrong[0]], want[wrong[0]]))
    rc, second, _ = _deflate(hc, texts)
    assert rc == 0 and second == first
    few = [texts[2], texts[n_chunks - 1], texts[1]]  # the scratch buffers are now far larger than three chunks need
    rc, parts, _ = _deflate(hc, few, lead=1)
    assert rc == 0 and parts == [_host(t) for t in few]


@pytest.mark.parametrize("nch", DC.SCAN_NCH)
def test_scan_runs_of_one_two_and_three(hc, nch):
    texts = DC.scan_mix(nch)
    want = [_host(t) for t in texts]
    rc, parts, _ = _deflate(hc, texts)
    assert rc == 0, hc.lib.bdx_last_error(hc.h)
    assert [len(p) for p in parts] == [len(w) for w in want]  # class_cbytes
    assert b"".join(parts) == b"".join(want)
    assert [len(_walk(p)) for p in parts] == [1] * nch


def test_compaction_writes_nothing_past_the_members(hc):
    import torch

    blocks = [DC.text(5000, "compact5000"), b"", DC.text(70000, "compact70000")]
    cb = np.array([len(b) for b in blocks], dtype=np.int64)
    bound = int(hc.lib.bdx_fq_deflate_bound(cb.ctypes.data, len(cb)))
    cap = bound + 4096
    d_in = torch.from_numpy(np.frombuffer(b"".join(blocks), dtype=np.uint8).copy()).to("cuda:0")
    d_out = torch.full((cap,), 0xC5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    zb = np.full(len(cb), -7, dtype=np.int64)
    rc = hc.lib.bdx_fq_deflate_device(hc.h, d_in.data_ptr(), cb.ctypes.data, len(cb), d_out.data_ptr(), cap, zb.ctypes.data)
    assert rc == 0, hc.lib.bdx_last_error(hc.h)
    out = d_out.cpu().numpy().tobytes()
    used = int(zb.sum())
    want = [_host(b) for b in blocks]
    assert [int(z) for z in zb] == [len(w) for w in want] and out[:used] == b"".join(want)
    assert used < bound and out[used:] == b"\xC5" * (cap - used)
