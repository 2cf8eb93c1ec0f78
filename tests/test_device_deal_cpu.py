"""_io="device-deal" without a GPU: the numpy restatement of the span index (tests/fastq_span_cases.py) against the host
library's index of the whole file, on every case text and span size; the cases' predicates; the span chain under seeded
random thread schedules; the new ValueErrors of execute_demultiplexing; the two new C-ABI symbols."""
import os
import queue
import threading
import time

import numpy as np
import pytest

import fastq_cases as FC
import fastq_span_cases as SP
import helpers as H
from biodemux_jl_amd import deviceio, hipabi, nativeio

JOIN_S = 30  # a join that takes this long is a hang


@pytest.fixture(scope="module", autouse=True)
def _host_library():
    nativeio.build()


# ---- the cases and the restatement ----
@pytest.mark.parametrize("c", SP.span_texts(), ids=lambda c: c.name)
def test_case_reaches_its_edge(c):
    assert c.ok, (c.name, c.edge)


def test_cases_cover_the_issue_list():
    names = {c.name for c in SP.span_texts()}
    assert names >= {"newline_on_last_byte", "newline_on_first_byte", "cr_lf_across_boundary", "line_longer_than_two_spans",
                     "line_starts_no_record_start", "all_phase_pairs", "header_on_last_byte", "unterminated_last_line",
                     "last_record_1_lines", "last_record_2_lines", "last_record_3_lines", "trailing_blank_lines", "empty_text",
                     "shorter_than_one_span"}


@pytest.mark.parametrize("S", SP.SPANS)
@pytest.mark.parametrize("c", SP.span_texts(), ids=lambda c: c.name)
def test_spans_concatenated_equal_the_host_index(tmp_path, c, S):
    """the partition property, with FastqFile.next_batch of the whole file as the other side"""
    off, ln, per_span = SP.walk_spans(c.text, S)
    hn, hcur, hoff, hln = FC.host_index(tmp_path / "t.fastq", c.text, len(c.text) + 8)
    assert hcur == len(c.text) and sum(per_span) == hn
    assert np.array_equal(off, hoff) and np.array_equal(ln, hln), (c.name, S)
    # ... and the device index's own restatement
    rn, _, roff, rln = FC.ref_index(c.text, 1, len(c.text) + 8)
    assert rn == hn and np.array_equal(off, roff) and np.array_equal(ln, rln)


def test_restatement_reports_a_short_tail_and_an_empty_span():
    c = next(c for c in SP.span_texts() if c.name == "line_longer_than_two_spans")
    first_tails = [SP.ref_span_index(c.text, 16, k, 0)[1] for k in range(SP.n_spans(c.text, 16))]
    assert 0 in first_tails and 1 in first_tails
    _, _, per_span = SP.walk_spans(c.text, 16)
    assert 0 in per_span and sum(per_span) == 6


def test_big_text_takes_more_than_1024_tiles():
    t, span = SP.big_text()
    assert span == 8 << 20 and (t[:span] == SP.NL).all() and FC.tiles(len(t)) > FC.FQ_SCAN_BLOCK >= 1024


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(FC.ROOT, "include", "biodemux_hip.h")).read()
    lib = hipabi.load_library()
    for name in ("bdx_fq_count_lines_device", "bdx_fq_index_span_device"):
        assert name in hipabi.ABI_SYMBOLS and hasattr(lib, name) and name + "(" in header


def test_default_span_never_depends_on_the_contexts():
    assert deviceio.default_span_bytes(1 << 19) == -(-((1 << 19) * 330) // 65536) * 65536
    assert deviceio.default_span_bytes(1) == 65536 and deviceio.default_span_bytes(199) == 131072


# ---- the span chain ----
N_SPANS, N_WORKERS = 40, 3


def _jitter(rng):
    for _ in range(int(rng.integers(0, 4))):
        time.sleep(0)  # (gives the processor away; waits for nothing)


def _run_chain(seed):
    """three workers with two slots each and a writer, as demux_device_dealt runs them -> what each thread saw"""
    counts = np.random.default_rng(1000 + seed).integers(0, 9, N_SPANS)
    empty = set(np.flatnonzero(np.random.default_rng(2000 + seed).integers(0, 3, N_SPANS) == 0).tolist())
    chain = deviceio._SpanChain()
    phases, written, taken = {}, [], [[] for _ in range(N_WORKERS)]

    def worker(w):
        rng = np.random.default_rng(seed * 10 + w)
        slots = queue.Queue()
        for s in range(2):
            slots.put(s)
        try:
            while True:
                _jitter(rng)
                k = chain.take()
                if k is None:
                    break
                if k >= N_SPANS:
                    chain.end_at(k)
                    break
                taken[w].append(k)
                _jitter(rng)
                chain.publish(k, int(counts[k]))
                _jitter(rng)
                phases[k] = chain.wait_phase(k)
                _jitter(rng)
                chain.hand_over(k, None if k in empty else (slots, slots.get(), k))
        except BaseException as e:  # noqa: BLE001
            chain.fail(e)

    def writer():
        rng = np.random.default_rng(seed * 10 + 9)
        for k, item in iter(chain.next_in_order, None):
            _jitter(rng)
            written.append((k, item is None))
            if item is not None:
                assert item[2] == k
                item[0].put(item[1])

    threads = [threading.Thread(target=worker, args=(w,), daemon=True) for w in range(N_WORKERS)]
    threads.append(threading.Thread(target=writer, daemon=True))
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_S)
    assert not any(t.is_alive() for t in threads), "the span chain hangs"
    assert not chain.errors, chain.errors
    return counts, empty, phases, written, taken


@pytest.mark.parametrize("seed", range(8))
def test_span_chain_under_random_schedules(seed):
    counts, empty, phases, written, taken = _run_chain(seed)
    want = np.concatenate([[0], np.cumsum(counts)[:-1]]) % 4
    assert [phases[k] for k in range(N_SPANS)] == want.tolist()
    assert [k for k, _ in written] == list(range(N_SPANS)), "the hand-over is in span order"
    assert {k for k, none in written if none} == empty and empty, "empty spans pass the writer"
    assert sorted(k for t in taken for k in t) == list(range(N_SPANS)) and all(t == sorted(t) for t in taken)


def test_span_chain_publish_out_of_order_and_end():
    chain = deviceio._SpanChain()
    assert [chain.take() for _ in range(3)] == [0, 1, 2]
    chain.publish(2, 5)
    chain.publish(1, 2)
    assert chain._phase == [0]
    chain.publish(0, 3)
    assert chain._phase == [0, 3, 1, 2] and chain.wait_phase(3) == 2 and not chain._counts
    chain.hand_over(1, "b")
    chain.hand_over(0, None)
    assert chain.next_in_order() == (0, None) and chain.next_in_order() == (1, "b")
    chain.end_at(4)
    chain.end_at(3)
    chain.end_at(5)
    assert chain.take() is None
    chain.hand_over(2, "c")
    assert chain.next_in_order() == (2, "c") and chain.next_in_order() is None


def test_span_chain_fail_wakes_every_waiter():
    chain = deviceio._SpanChain()
    assert chain.take() == 0  # span 0 never publishes: everybody behind it waits
    seen = {}

    def worker(w):
        k = chain.take()
        chain.publish(k, 1)
        try:
            chain.wait_phase(k)
            seen[w] = "phase"
        except deviceio._ChainFailed:
            seen[w] = "failed"

    def writer():
        seen["writer"] = chain.next_in_order()

    threads = [threading.Thread(target=worker, args=(w,), daemon=True) for w in range(N_WORKERS)]
    threads.append(threading.Thread(target=writer, daemon=True))
    for t in threads:
        t.start()
    while chain._next < 1 + N_WORKERS:  # every worker holds its span (they then wait, or are about to)
        time.sleep(0)
    boom = OSError("boom")
    chain.fail(boom)
    chain.fail(deviceio._ChainFailed())
    chain.fail(ValueError("later"))
    for t in threads:
        t.join(JOIN_S)
    assert not any(t.is_alive() for t in threads), "fail() left a waiter behind"
    assert seen == {0: "failed", 1: "failed", 2: "failed", "writer": None}
    assert chain.errors[0] is boom
    with pytest.raises(deviceio._ChainFailed):
        chain.take()


# ---- execute_demultiplexing: what the new mode refuses, before the output directory is made ----
def _refused(tmp_path, match, *fastqs, **kw):
    out = tmp_path / "out"
    with pytest.raises(ValueError, match=match):
        H.bdx.execute_demultiplexing(*fastqs, str(tmp_path / "bc.csv"), str(out), **kw)
    assert not out.exists()


def test_new_value_errors(tmp_path):
    fq = str(tmp_path / "r.fastq")
    deal = dict(_io="device-deal")
    _refused(tmp_path, "takes single-end input: a second FASTQ file", fq, fq, **deal)
    for mode in ("device", "device-stream", "device-window"):
        _refused(tmp_path, "_gunzip must be 'host', not '%s'" % mode, fq, _gunzip=mode, **deal)
    _refused(tmp_path, r"_io='device-deal': the device FASTQ pipeline needs the HIP classifier \(no _classifier_factory\)", fq,
             _classifier_factory=lambda cfg: None, **deal)
    for io in ("device", "native", "auto", "python"):
        _refused(tmp_path, "_span_bytes is the span of _io='device-deal'", fq, _io=io, _span_bytes=4096)
    for bad in (15, 0, -1, 4096.0, "4096", True):
        _refused(tmp_path, "_span_bytes must be an int of at least 16 bytes, got", fq, _span_bytes=bad, **deal)
    _refused(tmp_path, "_gzip_level selects a level of the device encoder", fq, _gzip_level=2, **deal)


def test_old_value_errors_stay(tmp_path):
    fq = str(tmp_path / "r.fastq")
    _refused(tmp_path, "_io='device' drives one device context", fq, _io="device", devices=[0, 1])
    _refused(tmp_path, "it needs _io='device'", fq, _io="native", _gzip="device")
    _refused(tmp_path, "it needs _io='device'", fq, _io="native", _gunzip="device-stream")
