"""The cases of tests/fastq_cases.py, without a GPU: every case reaches the edge it is named for (its predicate), and the
Python references the GPU tests hold the device to are themselves held to the host library here: ref_index to
FastqFile.next_batch, ref_pack to FastqFile.pack, ref_gather to the files bdx_fq_demux_write writes."""
import numpy as np
import pytest

import fastq_cases as FC
from biodemux_jl_amd import nativeio


@pytest.fixture(scope="module", autouse=True)
def _io_lib():
    nativeio.build()


# ---- the geometry and the predicates ----
def test_geometry_is_read_from_the_kernel_source():
    c = FC.parse_constants()
    for k in ("FQ_THREADS", "FQ_LANE_BYTES", "FQ_STEPS", "FQ_TILE", "FQ_SCAN_BLOCK"):
        assert c.get(k, 0) > 0, k
    assert FC.FQ_TILE == FC.FQ_THREADS * FC.FQ_LANE_BYTES * FC.FQ_STEPS
    assert FC.FQ_THREADS % 64 == 0 and FC.FQ_SCAN_BLOCK % FC.FQ_THREADS == 0
    assert FC.EDGES == tuple(sorted(set(FC.EDGES))), "lane < wave < step < tile"


@pytest.mark.parametrize("t", FC.index_texts(), ids=lambda t: t.name)
def test_index_text_reaches_its_edge(t):
    assert t.ok, t.edge


def test_index_texts_cover_what_they_must():
    names = {t.name for t in FC.index_texts()}
    for B in FC.EDGES:
        assert "newlines_around_%d" % B in names
        for n in (B - 1, B, B + 1):
            assert {"length_%d" % n, "length_%d_closed" % n} <= names
    for n in (1, 15, 16, 17, 2 * FC.FQ_TILE):
        assert "length_%d" % n in names
    for m in FC.NEAR_MISSES:
        assert "near_miss_%02x" % m in names
    assert set(FC.caps_for(next(t for t in FC.index_texts() if t.name == "cap_tiles").text)) == {
        "one", "inside_tile0", "tile_end", "inside_tile2", "beyond"}


@pytest.mark.parametrize("c", FC.gather_cases(), ids=lambda c: c.name)
def test_gather_case_reaches_its_edge(c):
    assert c.ok, c.edge
    assert c.n == len(c.bc1) == len(c.bc2) and len(c.off) == len(c.len) == 4 * c.n
    assert (c.keep_start is None) == (c.keep_end is None) and (c.keep_start is not None or not c.trim)


def test_gather_cases_cover_what_they_must():
    cases = {c.name: c for c in FC.gather_cases()}
    for n in FC.COUNTS:
        for p in FC.PATTERNS:
            assert cases["n%d_%s" % (n, p)].n == n
    assert [FC.radix_passes(n) for n in FC.CLASS_COUNTS] == [1, 1, 2, 2, 3, 3] == [v[1] for v in FC.CLASS_COUNTS.values()]
    assert list(FC.CLASS_COUNTS)[:5] == [2, 256, 257, 65536, 65537] and 89000 < list(FC.CLASS_COUNTS)[5] < 91000
    for n in FC.CLASS_COUNTS:
        assert "classes_%d" % n in cases
    for name in ("barcode_values", "line_lengths_trim1", "line_lengths_trim0", "trim_grid", "trim_grid_trim0",
                 "trim_grid_trim0_null_keeps", "crlf_table", "truncated_table"):
        assert name in cases
    assert cases["trim_grid_trim0_null_keeps"].keep_start is None


def test_out_of_range_classes_are_refused_by_the_reference_too():
    i32 = lambda *v: np.array(v, dtype=np.int32)  # noqa: E731
    for bc1, bc2, stride, ncl in ((i32(6), i32(1), 4, 22), (i32(5), i32(5), 4, 22), (i32(FC.INT32_MAX), i32(1), FC.INT32_MAX, 10)):
        with pytest.raises(ValueError):
            FC.ref_classes(bc1, bc2, stride, ncl)
    assert FC.ref_classes(i32(5), i32(4), 4, 22)[0] == 21


# ---- the references against the host library ----
def _same_index(got, exp):
    return got[0] == exp[0] and got[1] == exp[1] and np.array_equal(got[2], exp[2]) and np.array_equal(got[3], exp[3])


@pytest.mark.parametrize("t", FC.index_texts(), ids=lambda t: t.name)
def test_ref_index_equals_host_index(tmp_path, t):
    nls = t.text.count(b"\n")
    for label, cap in FC.caps_for(t.text).items():
        got = FC.ref_index(t.text, 1, cap)
        assert got[2].dtype == np.int64 and got[3].dtype == np.int32
        assert _same_index(got, FC.host_index(tmp_path / "t.fastq", t.text, cap)), (label, cap)
        # final == 0: whole records of terminated lines only — what the host index gives for the text cut at the cursor, and
        # the text behind the cursor holds no further record unless the cap is reached
        n0, nxt, off, ln = FC.ref_index(t.text, 0, cap)
        assert n0 == min(cap, nls // 4) and len(off) == 4 * n0 and t.text[:nxt].count(b"\n") == 4 * n0, (label, cap)
        assert nxt == 0 or t.text[nxt - 1] == 10
        if nxt:
            assert _same_index((n0, nxt, off, ln), FC.host_index(tmp_path / "t.fastq", t.text[:nxt], cap)), (label, cap, "final=0")


@pytest.mark.parametrize("c", FC.gather_cases(), ids=lambda c: c.name)
def test_ref_pack_and_ref_gather_equal_the_host_library(tmp_path, c):
    f = FC.host_open(tmp_path / "in.fastq", c.text)
    try:
        hseq, hso = f.pack(np.ascontiguousarray(c.off), np.ascontiguousarray(c.len), c.n, 4)
        seq, so = FC.ref_pack(c.text, c.off, c.len, c.n)
        assert so.dtype == np.int64 and np.array_equal(so, hso) and seq.tobytes() == hseq.tobytes()
        exp, exp_bytes = FC.host_gather(tmp_path / "out", f, c)
    finally:
        f.close()
    got, class_bytes = FC.ref_gather(c.text, c.off, c.len, c.bc1, c.bc2, c.stride, c.n_classes, c.keep_start, c.keep_end, c.trim)
    assert np.array_equal(class_bytes, exp_bytes) and int(class_bytes.sum()) == len(got)
    assert got.tobytes() == exp
    assert b"\r" not in exp
    # and record by record by plain slicing, in the order a stable sort by class gives
    cls = FC.ref_classes(c.bc1, c.bc2, c.stride, c.n_classes)
    order = sorted(range(c.n), key=lambda i: int(cls[i]))
    assert b"".join(FC.ref_record(c.text, c.off, c.len, i, c.keep_start, c.keep_end, c.trim) for i in order) == exp


def test_large_case_reaches_its_edges_and_the_references_hold_there(tmp_path):
    c = FC.large_case()
    assert c.ok, c.edge
    assert len(c.text) > 16 << 20 and FC.tiles(len(c.text)) > FC.FQ_SCAN_BLOCK
    assert FC.scan_partials(c.n) > FC.FQ_SCAN_BLOCK and FC.scan_partials(FC.hist_items(c.n)) > FC.FQ_SCAN_BLOCK
    f = FC.host_open(tmp_path / "in.fastq", c.text)
    try:
        n, off, ln = f.next_batch(c.n + 5, 4)
        assert n == c.n and f.cursor == len(c.text)
        assert np.array_equal(off[:4 * n], c.off) and np.array_equal(ln[:4 * n], c.len)
        hseq, hso = f.pack(c.off, c.len, c.n, 4)
        seq, so = FC.ref_pack(c.text, c.off, c.len, c.n)
        assert np.array_equal(so, hso) and np.array_equal(seq, hseq)
        exp, exp_bytes = FC.host_gather(tmp_path / "out", f, c)
    finally:
        f.close()
    got, class_bytes = FC.ref_gather(c.text, c.off, c.len, c.bc1, c.bc2, c.stride, c.n_classes, c.keep_start, c.keep_end, c.trim)
    assert np.array_equal(class_bytes, exp_bytes) and (class_bytes > 0).all()
    assert got.tobytes() == exp
    r = FC.ref_index(c.text, 1, c.n + 5)
    assert r[0] == c.n and r[1] == len(c.text) and np.array_equal(r[2], c.off) and np.array_equal(r[3], c.len)


# ---- the record of what the cases reach ----
def test_coverage_file_is_current():
    """profiles/fastq_case_coverage.txt is what the cases say of themselves now (python tests/fastq_cases.py rewrites it)"""
    assert open(FC.COVERAGE).read().splitlines() == FC.coverage_lines()
