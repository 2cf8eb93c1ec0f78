"""execute_demultiplexing(..., devices=[...]) with the HIP classifier on the MI355X: the batches are dealt over several
device contexts (repeated entries put several contexts on one GPU), and the reference goldens, the counters and the
summary reports (statistics tables summed over the contexts on the host) must be those of a single context."""
import functools
import gzip
import os
import re

import pytest

import helpers as H
from biodemux_jl_amd import nativeio, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    nativeio.build()


class _Dealt:
    """execute_demultiplexing bound to ``devices`` and a small batch size; sums _timings["batches_per_device"] over the calls."""

    def __init__(self, devices, batch_reads):
        self.devices = devices
        self.batch_reads = batch_reads
        self.per_device = [0] * len(devices)

    def __call__(self, *args, **kw):
        t = {}
        stats = H.bdx.execute_demultiplexing(*args, devices=self.devices, _io="native", _batch_reads=self.batch_reads,
                                             _timings=t, **kw)
        assert t["devices"] == list(self.devices)
        assert sum(t["batches_per_device"]) == t["batches"]
        self.per_device = [a + b for a, b in zip(self.per_device, t["batches_per_device"])]
        return stats


_BIG = [H.scenario_demo1_R1, H.scenario_demo1_R2, H.scenario_demo2]  # 240 / 240 / 2400 reads in 24 calls
_SMALL = [H.scenario_dual, H.scenario_dual_trim, H.scenario_hamming, H.scenario_exact, H.scenario_summary_counts,
          H.scenario_summary_distribution_reads]


@pytest.mark.parametrize("scenario", _BIG + _SMALL, ids=[s.__name__ for s in _BIG + _SMALL])
def test_reference_goldens_through_two_contexts(tmp_path, scenario):
    """The reference's integration tests, byte-exact, with every call dealt over two contexts on device 0."""
    run = _Dealt([0, 0], 2 if scenario in _BIG else 1)
    scenario(run, str(tmp_path))
    assert sum(run.per_device) > 0
    if scenario in _BIG:  # (60+ batches per scenario: both contexts take some; the tiny ones may all go to one)
        assert all(b > 0 for b in run.per_device), run.per_device


_VOLATILE = re.compile(r'Date:|Duration:|"date":|"duration":')  # (the wall clock of a run)


def _same_tree(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    assert fa == fb
    for f in fa:
        x, y = H._read_maybe_gz(os.path.join(a, f)), H._read_maybe_gz(os.path.join(b, f))
        if f.startswith("summary."):
            x, y = ([ln for ln in z.split(b"\n") if not _VOLATILE.search(ln.decode())] for z in (x, y))
        assert x == y, f
    return fa


def _dual_case(tmp_path, n=300_000):
    """Dual barcodes, ragged reads; a few much longer reads in one batch, so the contexts size their statistics tables
    differently (height and key0 of the start-position table)."""
    b1 = synth.make_barcodes(24, 24, seed=41)
    b2 = synth.make_barcodes(16, 24, seed=42)
    seq, off, _ = synth.make_ragged_reads(b1, n, 100, 150, seed=43, plant_lo=0, plant_hi=40, second=(b2, 60, 100))
    seqs = [seq[off[i]:off[i + 1]].tobytes() for i in range(n)]
    for i in range(123_456, 123_460):
        seqs[i] = seqs[i] + seqs[i + 100] + seqs[i + 200]
    fq = str(tmp_path / "reads.fastq")
    with open(fq, "wb") as f:
        f.write(b"".join(b"@r%d x\n" % i + s + b"\n+\n" + b"F" * len(s) + b"\n" for i, s in enumerate(seqs)))
    bc1, bc2 = tmp_path / "bc1.csv", tmp_path / "bc2.csv"
    bc1.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"x{i},{b},{'B' * len(b)}\n" for i, b in enumerate(b1)))
    bc2.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"y{i},{b},{'B' * len(b)}\n" for i, b in enumerate(b2)))
    return fq, str(bc1), str(bc2)


def test_three_contexts_equal_one(tmp_path):
    fq, bc1, bc2 = _dual_case(tmp_path)
    kw = dict(barcode_file2=bc2, max_error_rate=0.2, trim_side=5, trim_side2=3, summary=True, _batch_reads=20_000)
    for fmt in ("txt", "json"):  # (one directory pair per run: each compares one run's output)
        one, three = str(tmp_path / f"one_{fmt}"), str(tmp_path / f"three_{fmt}")
        t1, t3 = {}, {}
        s1 = H.bdx.execute_demultiplexing(fq, bc1, one, summary_format=fmt, _io="native", _timings=t1, **kw)
        s3 = H.bdx.execute_demultiplexing(fq, bc1, three, summary_format=fmt, devices=[0, 0, 0], _io="native", _timings=t3, **kw)
        assert vars(s1) == vars(s3)
        assert s1.matched_reads > 0 and s1.bc1_pos_counts and s1.bc2_len_counts
        assert "devices" not in t1 and t3["devices"] == [0, 0, 0]
        assert sum(t3["batches_per_device"]) == t1["batches"] == 15
        assert sum(1 for b in t3["batches_per_device"] if b) >= 2, t3["batches_per_device"]
        names = _same_tree(one, three)
        assert f"summary.{fmt}" in names and len(names) > 50


def test_python_path_with_two_contexts_equals_native(tmp_path):
    """batch k -> context k % N, on the calling thread: the plain statement of the dealing, on the HIP classifier"""
    bcs = synth.make_barcodes(12, 16, seed=44)
    seq, _, _ = synth.make_reads(bcs, 3000, 90, seed=44)
    fq = str(tmp_path / "reads.fastq.gz")
    with gzip.open(fq, "wb") as f:
        f.write(b"".join(b"@q%d\n" % i + s.tobytes() + b"\n+\n" + b"I" * 90 + b"\n" for i, s in enumerate(seq.reshape(3000, 90))))
    bc = tmp_path / "bc.csv"
    bc.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"b{i},{b},{'B' * len(b)}\n" for i, b in enumerate(bcs)))
    kw = dict(max_error_rate=0.2, trim_side=3, summary=True, summary_format="txt", _batch_reads=500, devices=[0, 0])
    t = {}
    a = H.bdx.execute_demultiplexing(fq, str(bc), str(tmp_path / "py"), _io="python", _timings=t, **kw)
    b = H.bdx.execute_demultiplexing(fq, str(bc), str(tmp_path / "nat"), _io="native", **kw)
    assert t["batches_per_device"] == [3, 3]
    _same_tree(str(tmp_path / "py"), str(tmp_path / "nat"))
    assert vars(a) == vars(b)


def test_distinct_gpus(tmp_path):
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("needs two or more GPUs")
    fq, bc1, bc2 = _dual_case(tmp_path, n=100_000)
    kw = dict(barcode_file2=bc2, max_error_rate=0.2, trim_side=5, summary=True, summary_format="json", _batch_reads=10_000)
    t = {}
    s1 = H.bdx.execute_demultiplexing(fq, bc1, str(tmp_path / "one"), _io="native", **kw)
    s2 = H.bdx.execute_demultiplexing(fq, bc1, str(tmp_path / "two"), devices=[0, 1], _io="native", _timings=t, **kw)
    assert vars(s1) == vars(s2)
    assert t["devices"] == [0, 1] and sum(t["batches_per_device"]) == 10
    _same_tree(str(tmp_path / "one"), str(tmp_path / "two"))


def test_a_device_that_does_not_exist_closes_the_open_contexts(tmp_path, monkeypatch):
    """devices=[0, 99]: context 0 opens, device 99 fails; the error reaches the caller and context 0 is closed."""
    from biodemux_jl_amd import core, hipabi

    opened = []
    real = hipabi.HipClassifier

    class Spy(real):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            opened.append(self)

    bc = tmp_path / "bc.csv"
    bc.write_text("ID,Full_seq,Full_annotation\nb0,ACGTACGTAC,BBBBBBBBBB\n")
    fq = tmp_path / "r.fastq"
    fq.write_text("@r\nACGTACGTACGG\n+\nIIIIIIIIIIII\n")
    monkeypatch.setattr(core, "HipClassifier", Spy)
    with pytest.raises(hipabi.BdxError, match="out of range"):
        H.bdx.execute_demultiplexing(str(fq), str(bc), str(tmp_path / "o"), devices=[0, 99], _io="native")
    monkeypatch.undo()
    assert len(opened) == 1 and opened[0].h is None  # closed
    run = functools.partial(H.bdx.execute_demultiplexing, _io="native", devices=[0, 0])
    assert run(str(fq), str(bc), str(tmp_path / "o2")).matched_reads == 1  # and the process goes on working
