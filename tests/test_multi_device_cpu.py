"""execute_demultiplexing(..., devices=[...]) on CPU: the batches are dealt over several classifier contexts (one thread
each in the native pipeline, batch k to context k % N in the Python path) and the results must be those of one context —
byte-identical files, equal counters, equal reports — whatever order the contexts finish in.  The contexts here are
doubles around the CPU oracle that sleep a batch-dependent time, so results come back out of order."""
import gzip
import os
import re
import threading
import time

import numpy as np
import pytest

import helpers as H
from biodemux_jl_amd import cli, nativeio, synth
from biodemux_jl_amd.classification import DemuxStats, merge_stats_tables


@pytest.fixture(scope="module", autouse=True)
def _built():
    nativeio.build()


class _Doubles:
    """A _classifier_factory whose n-th construction sleeps its own, batch-dependent time per batch and records what it did.
    ``fail_batch``: the (1-based) batch, counted over all doubles, that raises; ``fail_construction``: the (1-based)
    construction that raises."""

    def __init__(self, fail_batch=None, fail_construction=None, hook=None):
        self.made = []
        self.hook = hook
        self.calls = 0
        self.lock = threading.Lock()
        self.fail_batch = fail_batch
        self.fail_construction = fail_construction

    def __call__(self, cfg):
        if self.fail_construction is not None and len(self.made) + 1 == self.fail_construction:
            raise RuntimeError(f"construction {self.fail_construction} failed")
        d = _Double(self, cfg, len(self.made))
        self.made.append(d)
        return d


class _Double:
    def __init__(self, owner, cfg, k):
        self.owner = owner
        self.inner = H.oracle_factory(cfg)
        self.want_pass = self.inner.want_pass
        self.k = k
        self.batches = 0
        self.closed = False

    @property
    def counts(self):
        return self.inner.counts

    def classify(self, s, o):
        with self.owner.lock:
            self.owner.calls += 1
            call = self.owner.calls
        if self.owner.fail_batch is not None and call == self.owner.fail_batch:
            raise RuntimeError(f"classifier failed on batch {call}")
        if self.owner.hook is not None:
            self.owner.hook(call)
        time.sleep(0.001 * (1 + (call * (2 * self.k + 3)) % 7))  # batch-dependent, different for each double
        self.batches += 1
        return self.inner.classify(s, o)

    def close(self):
        self.closed = True


def _fastq(path, seqs, gz=False):
    blob = b"".join(b"@r%d some header\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n" for i, s in enumerate(seqs))
    (gzip.open if gz else open)(path, "wb").write(blob)


def _case(tmp_path, n=2500, seed=31, n_bc=8):
    bcs = synth.make_barcodes(n_bc, 12, seed=seed, min_hamming=4)
    seq, off, _ = synth.make_ragged_reads(bcs, n, 20, 90, seed=seed)
    seqs = [seq[off[i]:off[i + 1]].tobytes() for i in range(n)]
    bc = tmp_path / "bc.csv"
    bc.write_text("ID,Full_seq,Full_annotation\n" + "".join(f"b{i},{b},{'B' * len(b)}\n" for i, b in enumerate(bcs)))
    return seqs, str(bc)


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


def _run(args, out, io="native", factory=None, **kw):
    timings = {}
    stats = H.bdx.execute_demultiplexing(*args, out, _classifier_factory=factory or H.oracle_factory, _io=io,
                                         _timings=timings, **kw)
    return stats, timings


def test_dealt_batches_come_back_in_input_order(tmp_path):
    seqs, bc = _case(tmp_path)
    fq = str(tmp_path / "reads.fastq")
    _fastq(fq, seqs)
    kw = dict(max_error_rate=0.2, trim_side=5, _batch_reads=100)
    one, _ = _run((fq, bc), str(tmp_path / "one"), **kw)
    doubles = _Doubles()
    three, t = _run((fq, bc), str(tmp_path / "three"), factory=doubles, devices=[0, 0, 0], **kw)
    assert len(_same_tree(str(tmp_path / "one"), str(tmp_path / "three"))) > 3
    assert vars(one) == vars(three)
    assert len(doubles.made) == 3 and all(d.batches >= 1 for d in doubles.made), [d.batches for d in doubles.made]
    assert all(d.closed for d in doubles.made)
    assert t["devices"] == [0, 0, 0] and t["batches_per_device"] == [d.batches for d in doubles.made]
    assert t["batches"] == sum(t["batches_per_device"]) == 25
    assert len(t["classify_s_per_device"]) == 3 and t["classify_s"] == pytest.approx(sum(t["classify_s_per_device"]))


def test_single_device_keeps_its_timing_keys(tmp_path):
    seqs, bc = _case(tmp_path, n=600)
    fq = str(tmp_path / "reads.fastq")
    _fastq(fq, seqs)
    _, t0 = _run((fq, bc), str(tmp_path / "a"), _batch_reads=100)
    _, t1 = _run((fq, bc), str(tmp_path / "b"), _batch_reads=100, devices=[0])
    assert set(t0) == set(t1)
    assert not {"devices", "batches_per_device", "classify_s_per_device"} & set(t0)


def test_dealt_paired_classify_both_trim_gzip(tmp_path):
    seqs, bc = _case(tmp_path, seed=32)
    s2 = [s[::-1] for s in seqs]
    f1, f2 = str(tmp_path / "x_R1.fastq.gz"), str(tmp_path / "x_R2.fastq.gz")
    _fastq(f1, seqs, gz=True)
    _fastq(f2, s2, gz=True)
    kw = dict(classify_both=True, trim_side=3, gzip_output=True, _batch_reads=100)
    one, _ = _run((f1, f2, bc), str(tmp_path / "one"), **kw)
    doubles = _Doubles()
    three, _ = _run((f1, f2, bc), str(tmp_path / "three"), factory=doubles, devices=[0, 1, 2], **kw)
    names = _same_tree(str(tmp_path / "one"), str(tmp_path / "three"))
    assert any(n.startswith("x_R2.") for n in names) and all(n.endswith(".fastq.gz") for n in names)
    assert vars(one) == vars(three)
    assert all(d.batches >= 1 for d in doubles.made)


@pytest.mark.parametrize("fmt", ["txt", "json"])
def test_dealt_summary_reports_equal_single(tmp_path, fmt):
    seqs, bc = _case(tmp_path, seed=33)
    fq = str(tmp_path / "reads.fastq")
    _fastq(fq, seqs)
    kw = dict(max_error_rate=0.2, trim_side=5, summary=True, summary_format=fmt, _batch_reads=100)
    one, _ = _run((fq, bc), str(tmp_path / "one"), **kw)
    doubles = _Doubles()
    three, _ = _run((fq, bc), str(tmp_path / "three"), factory=doubles, devices=[0, 0, 0], **kw)
    assert f"summary.{fmt}" in _same_tree(str(tmp_path / "one"), str(tmp_path / "three"))
    assert vars(one) == vars(three) and one.bc1_pos_counts
    assert all(d.batches >= 1 for d in doubles.made)


def test_python_path_deals_like_native(tmp_path):
    seqs, bc = _case(tmp_path, n=2100, seed=34)
    fq = str(tmp_path / "reads.fastq")
    _fastq(fq, seqs)
    kw = dict(max_error_rate=0.2, trim_side=3, summary=True, summary_format="txt", _batch_reads=100, devices=[0, 0, 0])
    py_doubles = _Doubles()
    py, t = _run((fq, bc), str(tmp_path / "py"), io="python", factory=py_doubles, **kw)
    nat, _ = _run((fq, bc), str(tmp_path / "nat"), factory=_Doubles(), **kw)
    _same_tree(str(tmp_path / "py"), str(tmp_path / "nat"))
    assert vars(py) == vars(nat)
    assert t["batches_per_device"] == [7, 7, 7] == [d.batches for d in py_doubles.made]  # batch k -> context k % 3


def test_device_arguments():
    run = H.bdx.execute_demultiplexing
    with pytest.raises(ValueError, match="empty"):
        run("r.fastq", "bc.csv", "out", devices=[])
    with pytest.raises(ValueError, match="not both"):
        run("r.fastq", "bc.csv", "out", device=1, devices=[0, 1])
    with pytest.raises(ValueError, match="_io='device'"):
        run("r.fastq", "bc.csv", "out", devices=[0, 1], _io="device")
    with pytest.raises(TypeError):
        run("r.fastq", "bc.csv", "out", devices="0,1")
    with pytest.raises(ValueError, match=">= 0"):
        run("r.fastq", "bc.csv", "out", devices=[0, -1])


def test_cli_devices():
    calls = []

    def spy(*args, **kw):
        calls.append(kw)

    assert cli.build_parser().parse_args(["r", "bc", "out", "--devices", "0,1"]).devices == [0, 1]
    assert cli.main(["a.fastq", "bc.csv", "out", "--devices", "0,1,1"], _execute=spy) == 0
    assert calls[-1]["devices"] == [0, 1, 1]
    assert cli.main(["a.fastq", "bc.csv", "out", "--devices", "0,1", "--device", "1"], _execute=spy) == 2
    assert cli.main(["a.fastq", "bc.csv", "out", "--devices", "0,x"], _execute=spy) == 2
    assert len(calls) == 1
    calls.clear()
    assert cli.main(["a.fastq", "bc.csv", "out"], _execute=spy) == 0
    assert "devices" not in calls[-1]


def test_cli_directory_mode_passes_devices(tmp_path):
    d = tmp_path / "r1"
    d.mkdir()
    for n in ("a.fastq", "b.fastq"):
        (d / n).write_text("")
    calls = []
    assert cli.main([str(d), "bc.csv", "out", "--devices", "2,3"], _execute=lambda *a, **kw: calls.append(kw)) == 0
    assert [c["devices"] for c in calls] == [[2, 3], [2, 3]]


def _in_thread(fn, timeout=60):
    result = {}

    def go():
        try:
            fn()
            result["ok"] = True
        except BaseException as e:  # noqa: BLE001
            result["err"] = e

    t = threading.Thread(target=go, daemon=True)
    t.start()
    t.join(timeout)
    assert not t.is_alive(), "the dealer hangs on an error"
    return result


@pytest.mark.parametrize("io", ["native", "python"])
def test_errors_reach_the_caller_and_close_every_context(tmp_path, io):
    seqs, bc = _case(tmp_path, n=2000, seed=35)
    fq = str(tmp_path / "reads.fastq")
    _fastq(fq, seqs)
    nativeio.release_buffers()
    doubles = _Doubles(fail_batch=2)
    r = _in_thread(lambda: _run((fq, bc), str(tmp_path / "o1"), io=io, factory=doubles, devices=[0, 0, 0], _batch_reads=100))
    assert "batch 2" in str(r.get("err")), r
    assert len(doubles.made) == 3 and all(d.closed for d in doubles.made)
    if io == "native":  # the sets came back, and the pool keeps no more than a single-device run needs
        assert 1 <= len(nativeio._BUFFER_POOL) <= nativeio._BUFFER_POOL_MAX
    # a later context fails to open: the ones already open are closed before the error reaches the caller
    doubles = _Doubles(fail_construction=2)
    r = _in_thread(lambda: _run((fq, bc), str(tmp_path / "o2"), io=io, factory=doubles, devices=[0, 99], _batch_reads=100))
    assert "construction 2" in str(r.get("err")), r
    assert len(doubles.made) == 1 and doubles.made[0].closed
    # the process goes on working afterwards
    r = _in_thread(lambda: _run((fq, bc), str(tmp_path / "o3"), io=io, factory=_Doubles(), devices=[0, 0], _batch_reads=100))
    assert r.get("ok"), r


def test_writer_error_with_several_contexts(tmp_path):
    """The writer fails (a directory stands where an output file goes: open() gives EISDIR) while both contexts still
    have batches to classify: the error reaches the caller, nothing hangs, every context is closed."""
    seqs, bc = _case(tmp_path, n=2000, seed=36)
    fq = str(tmp_path / "reads.fastq")
    _fastq(fq, seqs)
    ref = tmp_path / "ref"
    _run((fq, bc), str(ref), _batch_reads=100)
    busiest = max(os.listdir(ref), key=lambda f: os.path.getsize(ref / f))  # (written by most of the 20 batches)
    out_dir = tmp_path / "out"
    (out_dir / busiest).mkdir(parents=True)
    doubles = _Doubles()
    r = _in_thread(lambda: _run((fq, bc), str(out_dir), factory=doubles, devices=[0, 0], _batch_reads=100))
    assert isinstance(r.get("err"), OSError), r
    assert len(doubles.made) == 2 and all(d.closed for d in doubles.made)


def test_merge_stats_tables_sums_over_the_union_of_key_ranges():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 5, size=(4, 3)).astype(np.int64)   # keys -2 .. 1
    b = rng.integers(0, 5, size=(7, 3)).astype(np.int64)   # keys -5 .. 1
    c = rng.integers(0, 5, size=(2, 3)).astype(np.int64)   # keys 0 .. 1
    raw_a = rng.integers(0, 5, size=(3, 3)).astype(np.int64)
    raw_b = rng.integers(0, 5, size=(6, 3)).astype(np.int64)
    empty = np.zeros((0, 3), dtype=np.int64)
    t = [{0: {"pos": (a, -2), "raw": (raw_a, 0), "len": (empty, 0)}},
         {0: {"pos": (b, -5), "raw": (raw_b, 0), "len": (c, 3)}},
         {0: {"pos": (c, 0), "raw": (empty, 0), "len": (empty, 0)}}]
    m = merge_stats_tables(t)
    tab, key0 = m[0]["pos"]
    assert key0 == -5 and tab.shape == (7, 3)
    exp = np.zeros((7, 3), dtype=np.int64)
    exp[3:7] += a
    exp += b
    exp[5:7] += c
    assert np.array_equal(tab, exp)
    tab, key0 = m[0]["raw"]
    assert key0 == 0 and tab.shape == (6, 3)
    exp = raw_b.copy()
    exp[:3] += raw_a
    assert np.array_equal(tab, exp)
    tab, key0 = m[0]["len"]
    assert key0 == 3 and np.array_equal(tab, c)
    # element by element: every key's count is the sum of that key's counts over the inputs
    for k in range(-5, 2):
        want = sum(int(x[k - k0, 1]) for x, k0 in ((a, -2), (b, -5), (c, 0)) if 0 <= k - k0 < len(x))
        assert int(m[0]["pos"][0][k + 5, 1]) == want
    # tables that disagree on the barcode count are an error, not a silent truncation
    with pytest.raises(ValueError):
        merge_stats_tables([{0: {"pos": (a, 0)}}, {0: {"pos": (np.zeros((2, 4), dtype=np.int64), 0)}}])


def test_merged_tables_decode_like_one_table():
    """add_device_tables over merged tables gives the statistics of one table holding the same counts."""
    cfg = H.bdx.DemuxConfig(bc_seqs=["ACGTAC", "CCCCCC"], bc_lengths_no_N=[6, 6], ids=["a", "b"], summary=True)
    whole = {0: {"pos": (np.array([[1, 0], [2, 3], [0, 1]], dtype=np.int64), -1),
                 "len": (np.array([[0, 2], [4, 0]], dtype=np.int64), 5),
                 "raw": (np.array([[3, 1], [1, 0]], dtype=np.int64), 0)}}
    part1 = {0: {"pos": (np.array([[2, 1]], dtype=np.int64), 0),
                 "len": (np.array([[0, 2]], dtype=np.int64), 5),
                 "raw": (np.array([[1, 1]], dtype=np.int64), 0)}}
    part2 = {0: {"pos": (np.array([[1, 0], [0, 2], [0, 1]], dtype=np.int64), -1),
                 "len": (np.array([[0, 0], [4, 0]], dtype=np.int64), 5),
                 "raw": (np.array([[2, 0], [1, 0]], dtype=np.int64), 0)}}
    s1, s2 = DemuxStats(), DemuxStats()
    s1.add_device_tables(whole, cfg)
    s2.add_device_tables(merge_stats_tables([part1, part2]), cfg)
    assert vars(s1) == vars(s2) and s1.bc1_pos_counts
    # one context: the merge of a single table is that table (execute_demultiplexing always merges)
    whole[0]["len"] = (np.zeros((0, 2), dtype=np.int64), 7)  # (a table without rows keeps its key0)
    m = merge_stats_tables([whole])
    for name, (tab, key0) in whole[0].items():
        assert m[0][name][1] == key0 and m[0][name][0].dtype == tab.dtype and np.array_equal(m[0][name][0], tab), name
