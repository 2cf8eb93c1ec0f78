"""The opt-in FASTQ checks without a GPU: the cases' predicates; the numpy restatement (tests/fastq_check_cases.py) against
the host library's bdx_fq_check / bdx_fq_check_pair on every case; _check=True through _io="python" and _io="native" (the
oracle as classifier) — the goldens come out unchanged, every failure stops the run with its exact message after the
batches in front of it were written; the ValueError for a non-bool _check; the new command line options; the symbols."""
import functools
import gzip
import os

import numpy as np
import pytest

import fastq_cases as FC
import fastq_check_cases as CC
import helpers as H
from biodemux_jl_amd import checks, cli, hipabi, nativeio

run_py = functools.partial(H.bdx.execute_demultiplexing, _classifier_factory=H.oracle_factory, _io="python")
run_nat = functools.partial(H.bdx.execute_demultiplexing, _classifier_factory=H.oracle_factory, _io="native")
RUNS = {"python": run_py, "native": run_nat}


@pytest.fixture(scope="module", autouse=True)
def _host_library():
    nativeio.build()


# ---- the cases and the restatement ----
@pytest.mark.parametrize("c", CC.check_cases() + CC.name_cases(), ids=lambda c: c.name)
def test_case_reaches_its_edge(c):
    assert c.ok, (c.name, c.edge)


def test_big_cases_reach_their_edge():
    assert CC.BIG_N > CC.SWEEP and all(c.ok for c in CC.big_check_cases())


def test_restatement_of_the_name_rule():
    for header, name in ((b"@read1", b"read1"), (b"@r 1", b"r"), (b"@r\t1", b"r"), (b"@r/1", b"r"), (b"@r/2 x", b"r"), (b"@r/3", b"r/3"),
                         (b"@a/1b", b"a/1b"), (b"@/1", b""), (b"@", b""), (b"", b""), (b"xabc", b"abc"), (b"@r/1/2", b"r/1")):
        assert CC.ref_name(header) == name == checks.read_name(header), header


def _host_walks(f, c, rules):
    return CC.walk(lambda s, k: f.check(c.off[4 * s:], c.len[4 * s:], k, rules, 4), c.n)


@pytest.mark.parametrize("c", CC.check_cases(), ids=lambda c: c.name)
def test_host_check_equals_the_restatement(tmp_path, c):
    masks = CC.ref_masks(c.text, c.off, c.len, c.n)
    f = FC.host_open(tmp_path / "t.fastq", c.text)
    try:
        for rules in CC.MASKS:
            assert _host_walks(f, c, rules) == CC.expected_walk(masks, rules), rules
            assert f.check(c.off, c.len, c.n, rules, 4) == CC.ref_check(c.text, c.off, c.len, c.n, rules)
    finally:
        f.close()


def test_host_check_of_the_big_cases(tmp_path):
    for c in CC.big_check_cases():
        masks = CC.ref_masks(c.text, c.off, c.len, c.n)
        f = FC.host_open(tmp_path / "t.fastq", c.text)
        try:
            for rules in (7, 1, 6):
                assert _host_walks(f, c, rules) == CC.expected_walk(masks, rules), (c.name, rules)
        finally:
            f.close()


@pytest.mark.parametrize("c", CC.name_cases(), ids=lambda c: c.name)
def test_host_pair_check_equals_the_restatement(tmp_path, c):
    flags = CC.ref_pair_flags(c.text1, c.off1, c.len1, c.text2, c.off2, c.len2, c.n)
    f1, f2 = FC.host_open(tmp_path / "a.fastq", c.text1), FC.host_open(tmp_path / "b.fastq", c.text2)
    try:
        got = CC.walk(lambda s, k: (f1.check_pair(c.off1[4 * s:], c.len1[4 * s:], f2, c.off2[4 * s:], c.len2[4 * s:], k, 4), 0), c.n)
        assert [i for i, _ in got] == np.flatnonzero(flags).tolist()
        assert f1.check_pair(c.off1, c.len1, f2, c.off2, c.len2, c.n, 4) == CC.ref_check_pair(c.text1, c.off1, c.len1, c.text2, c.off2, c.len2, c.n)
    finally:
        f1.close()
        f2.close()


def test_host_refusals(tmp_path):
    c = CC.check_cases()[0]
    f = FC.host_open(tmp_path / "t.fastq", c.text)
    try:
        for rules in (0, 8, -1, 15):
            with pytest.raises(hipabi.BdxError, match="rules must be a mask of 1, 2 and 4"):
                f.check(c.off, c.len, c.n, rules, 1)
        with pytest.raises(hipabi.BdxError, match="n is negative"):
            f.check(c.off, c.len, -1, 7, 1)
        with pytest.raises(hipabi.BdxError, match="more than 2\\^32 - 1 records"):
            f.check(c.off, c.len, 1 << 32, 7, 1)
        off = c.off.copy()
        off[3] = len(c.text)  # its line of 4 bytes ends behind the text
        with pytest.raises(hipabi.BdxError, match="a line of the line table lies outside the text"):
            f.check(off, c.len, c.n, 7, 1)
        with pytest.raises(hipabi.BdxError, match="a line of the line table lies outside the text"):
            f.check_pair(np.array([len(c.text) - 1, 0, 0, 0]), c.len, f, c.off, c.len, c.n, 1)
        assert f.check(c.off, c.len, 0, 7, 1) == (-1, 0) and f.check_pair(c.off, c.len, f, c.off, c.len, 0, 1) == -1
        assert f.check(c.off, c.len, c.n, 7, 1) == (-1, 0)  # a correct call after the refusals
    finally:
        f.close()


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(FC.ROOT, "include", "biodemux_hip.h")).read()
    lib = hipabi.load_library()
    for name in ("bdx_fq_check_device", "bdx_fq_check_pair_device"):
        assert name in hipabi.ABI_SYMBOLS and hasattr(lib, name) and name + "(" in header
    io = nativeio._load()
    assert hasattr(io, "bdx_fq_check") and hasattr(io, "bdx_fq_check_pair")
    for name, value in (("BDX_FQ_CHECK_HEADER", 1), ("BDX_FQ_CHECK_PLUS", 2), ("BDX_FQ_CHECK_LENGTH", 4)):
        assert "#define %s %d" % (name, value) in header
    assert (checks.HEADER, checks.PLUS, checks.LENGTH, checks.ALL_RULES) == (1, 2, 4, 7)


# ---- the goldens pass the rules, and come out unchanged with the checks on ----
def _golden_text(path):
    with (gzip.open if path.endswith(".gz") else open)(path, "rb") as fh:
        return fh.read()


def test_every_golden_input_passes_the_rules():
    root = os.path.join(H.REF, "FASTQ_files")
    tables = {}
    for d in sorted(os.listdir(root)):
        for name in sorted(os.listdir(os.path.join(root, d))):
            text = _golden_text(os.path.join(root, d, name))
            n, _, off, ln = FC.ref_index(text, 1, text.count(b"\n") // 4 + 2)
            assert n > 0 and CC.ref_check(text, off, ln, n, 7) == (-1, 0), (d, name)
            tables.setdefault(d, []).append((text, off, ln, n))
    assert CC.ref_name(b"@read1") == b"read1" and tables["demo1_R1"][0][0].startswith(b"@read1\n") and tables["demo1_R2"][0][0].startswith(b"@read1\n")
    for a, b in (("demo1_R1", "demo1_R2"), ("demo2_R1", "demo2_R2")):
        assert len(tables[a]) == len(tables[b])
        for (t1, o1, l1, n1), (t2, o2, l2, n2) in zip(tables[a], tables[b]):
            assert n1 == n2 and CC.ref_check_pair(t1, o1, l1, t2, o2, l2, n1) == -1, (a, b)


@pytest.mark.parametrize("io", list(RUNS))
def test_goldens_with_the_checks_on(tmp_path, io):
    tm = {}
    run = functools.partial(RUNS[io], _check=True, _timings=tm)
    assert H.scenario_demo1_R1(run, str(tmp_path / "a")) == 24
    assert tm["checked_records"] > 0 and tm["check_s"] >= 0
    assert H.scenario_demo1_R2(run, str(tmp_path / "b")) == 24
    assert H.scenario_demo2(run, str(tmp_path / "c")) == 76  # gz in, classify_both
    for scenario in (H.scenario_dual_trim, H.scenario_n_and_ranges):
        os.mkdir(str(tmp_path / scenario.__name__))
        scenario(run, str(tmp_path / scenario.__name__))


def test_timings_without_the_check_have_no_check_keys(tmp_path):
    tm = {}
    H.scenario_n_and_ranges(functools.partial(run_nat, _timings=tm), str(tmp_path))
    assert "check_s" not in tm and "checked_records" not in tm


# ---- failures: the message, the record, the byte, and what was written before ----
BARCODES = "ID,Full_seq,Full_annotation\nb0,ACGTACGTAC,BBBBBBBBBB\nb1,TTGCATTGCA,BBBBBBBBBB\n"


def _records(n, name=lambda i: b"@r%d" % i):
    seqs = (b"ACGTACGTACGGA", b"TTGCATTGCATTT", b"GGGGGGGGGGGGG")
    return [(name(i), seqs[i % 3], b"+", b"I" * 13) for i in range(n)]


def _text(records):
    return b"".join(b"\n".join(r) + b"\n" for r in records)


def _offset(records, i):
    return len(_text(records[:i]))


def failing_inputs():
    """name -> (text 1, text 2 or None, the message behind the paths' part, records written before the failure);
    10 records, batches of 4: the failure lies in the third batch, at record 9 (1-based)"""
    good = _records(10)
    out = {}
    for name, change, why in (("header", lambda r: (b"r8", r[1], r[2], r[3]), "the header line does not begin with '@'"),
                              ("plus", lambda r: (r[0], r[1], b"-", r[3]), "the third line does not begin with '+'"),
                              ("length", lambda r: (r[0], r[1], r[2], r[3][:-2]), "sequence and quality differ in length (13 against 11)"),
                              ("header_and_length", lambda r: (b"", r[1], r[2], r[3] + b"I"), "the header line does not begin with '@'")):
        bad = list(good)
        bad[8] = change(bad[8])
        out[name] = (_text(bad), None, "{p1}: record 9 (at byte %d of the text): %s" % (_offset(bad, 8), why), 8)
        out[name + "_in_file_2"] = (_text(good), _text(bad), "{p2}: record 9 (at byte %d of the text): %s" % (_offset(bad, 8), why), 8)
    cut = _text(good)[:-6]  # (the quality line of the last record loses its newline and five bytes)
    out["cut"] = (cut, None, "{p1}: record 10 (at byte %d of the text): sequence and quality differ in length (13 against 8)" % _offset(good, 9), 8)
    mates = _records(10, lambda i: b"@r%d/2 mate" % (i + (i >= 8)))
    out["names"] = (_text(_records(10, lambda i: b"@r%d/1 first" % i)), _text(mates),
                    "{p1} and {p2}: record 9: the read names differ (b'r8' against b'r9')", 8)
    out["file_2_goes_on"] = (_text(good[:9]), _text(good), "{p1} and {p2}: {p2} goes on from record 10, {p1} ends after 9 records", 9)
    out["file_1_goes_on"] = (_text(good), _text(good[:8]), "{p1} and {p2}: {p1} goes on from record 9, {p2} ends after 8 records", 8)
    # both files fail: file 1's records are judged first, whatever the record
    bad1, bad2 = list(good), list(good)
    bad1[9] = (bad1[9][0], bad1[9][1], b"", bad1[9][3])
    bad2[8] = (b"x", bad2[8][1], bad2[8][2], bad2[8][3])
    out["file_1_first"] = (_text(bad1), _text(bad2), "{p1}: record 10 (at byte %d of the text): the third line does not begin with '+'" % _offset(bad1, 9), 8)
    return out


def write_inputs(tmp_path, name):
    t1, t2, msg, before = failing_inputs()[name]
    p1, p2 = str(tmp_path / "x_R1.fastq"), str(tmp_path / "x_R2.fastq")
    with open(p1, "wb") as fh:
        fh.write(t1)
    if t2 is not None:
        with open(p2, "wb") as fh:
            fh.write(t2)
    bc = str(tmp_path / "bc.csv")
    with open(bc, "w") as fh:
        fh.write(BARCODES)
    return ([p1] if t2 is None else [p1, p2]), bc, msg.format(p1=p1, p2=p2), before, t1, t2


def tree(out):
    return {f: H._read_maybe_gz(os.path.join(out, f)) for f in sorted(os.listdir(out))}


def expected_tree(run, tmp_path, fastqs, texts, before, bc, **kw):
    """what the batches in front of the failure write: the run, unchecked, over the first `before` records of each input"""
    d = tmp_path / "head"
    d.mkdir()
    heads = []
    for p, t in zip(fastqs, texts):
        h = str(d / os.path.basename(p))
        with open(h, "wb") as fh:
            fh.write(b"".join(t.split(b"\n")[k] + b"\n" for k in range(4 * before)))
        heads.append(h)
    run(*heads, bc, str(tmp_path / "want"), **kw)
    return tree(str(tmp_path / "want"))


@pytest.mark.parametrize("io", list(RUNS))
@pytest.mark.parametrize("name", list(failing_inputs()))
def test_failure_message_and_what_was_written(tmp_path, io, name):
    fastqs, bc, msg, before, t1, t2 = write_inputs(tmp_path, name)
    kw = dict(max_error_rate=0.2, _batch_reads=4, **(dict(classify_both=True) if t2 is not None else {}))
    out = str(tmp_path / "out")
    with pytest.raises(hipabi.BdxError) as e:
        RUNS[io](*fastqs, bc, out, _check=True, **kw)
    assert str(e.value) == msg
    assert tree(out) == expected_tree(RUNS[io], tmp_path, fastqs, [t for t in (t1, t2) if t is not None], before, bc, **kw)
    assert before >= 8 and sum(v.count(b"\n") for v in tree(out).values()) == 4 * before * len(fastqs)
    # the same inputs without the check: the reference's behaviour, no error
    RUNS[io](*fastqs, bc, str(tmp_path / "unchecked"), **kw)


def test_check_must_be_a_bool(tmp_path):
    out = tmp_path / "out"
    for bad in (1, 0, None, "yes", 7.0):
        with pytest.raises(ValueError, match="_check must be True or False"):
            H.bdx.execute_demultiplexing(str(tmp_path / "r.fastq"), str(tmp_path / "bc.csv"), str(out), _check=bad)
    assert not out.exists()


# ---- the command line ----
def _spy():
    calls = []
    return calls, lambda *a, **kw: calls.append((a, kw))


def test_cli_options_reach_execute_under_their_keywords():
    calls, spy = _spy()
    base = ["a.fastq", "bc.csv", "out"]
    assert cli.main(base, _execute=spy) == 0
    today = set(calls[0][1])
    assert today == {"barcode_file2", "gzip_output", "max_error_rate", "min_delta", "match", "mismatch", "indel", "nindel", "bc_complement",
                     "bc_rev", "ref_search_range", "barcode_start_range", "barcode_end_range", "ref_search_range2", "barcode_start_range2",
                     "barcode_end_range2", "chunk_size", "channel_capacity", "trim_side", "trim_side2", "summary", "summary_format",
                     "matching_algorithm", "log", "output_prefix"}
    for argv, key, value in ((["--check"], "_check", True), (["--io", "device"], "_io", "device"), (["--gzip", "device"], "_gzip", "device"),
                             (["--gzip-level", "2"], "_gzip_level", 2), (["--gunzip", "device-window"], "_gunzip", "device-window"),
                             (["--gunzip-window", "4096"], "_gunzip_window", 4096), (["--span-bytes", "65536"], "_span_bytes", 65536)):
        calls.clear()
        assert cli.main(base + argv, _execute=spy) == 0
        (_, kw), = calls
        assert set(kw) == today | {key} and kw[key] == value and type(kw[key]) is type(value), argv
    calls.clear()
    assert cli.main(base + ["--fastq2", "b.fastq", "--check", "--io", "device-deal", "--span-bytes", "32"], _execute=spy) == 0
    (args, kw), = calls
    assert args == ("a.fastq", "b.fastq", "bc.csv", "out") and (kw["_check"], kw["_io"], kw["_span_bytes"]) == (True, "device-deal", 32)


def test_cli_leaves_validation_to_execute(tmp_path, capsys):
    fq = tmp_path / "r.fastq"
    fq.write_bytes(_text(_records(2)))
    bc = tmp_path / "bc.csv"
    bc.write_text(BARCODES)
    rc = cli.main([str(fq), str(bc), str(tmp_path / "o"), "--io", "native", "--span-bytes", "64"], _execute=run_nat)
    assert rc == 1 and "_span_bytes is the span of _io='device-deal'" in capsys.readouterr().err


def test_cli_check_stops_a_bad_file(tmp_path, capsys):
    fastqs, bc, msg, _, _, _ = write_inputs(tmp_path, "plus")
    rc = cli.main([fastqs[0], bc, str(tmp_path / "o"), "--check", "--io", "python"], _execute=functools.partial(
        H.bdx.execute_demultiplexing, _classifier_factory=H.oracle_factory))
    assert rc == 1 and msg in capsys.readouterr().err
