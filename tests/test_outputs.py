"""outputs.OutputLayout, the one statement of the output layout: the class numbering against its scalar definition
(0 unknown, 1 ambiguous, 2 + (bc1 - 1) * stride + (bc2 - 1)), class -> verdict -> file path, and the streams of
core.jl:175-196."""
import itertools
import os

import numpy as np
import pytest

import helpers as H
from biodemux_jl_amd.classification import filename_for
from biodemux_jl_amd.outputs import OutputLayout


def _config(dual, **kw):
    extra = dict(is_dual=True, bc_seqs2=["AAAACC", "CCCCAA"], bc_lengths_no_N2=[6, 6], ids2=["x", "y"]) if dual else {}
    return H.bdx.DemuxConfig(bc_seqs=["ACGTAC", "CCCCCC", "GGGTTT"], bc_lengths_no_N=[6, 6, 6], ids=["a", "b", "c"],
                             **extra, **kw)


def _verdicts(cfg):
    """every verdict a classifier can give: unknown, ambiguous, each barcode (pair)"""
    matched = itertools.product(range(1, 4), range(1, 3)) if cfg.is_dual else ((b, 0) for b in range(1, 4))
    return [(0, 0), (-1, 0), *matched]


def _scalar_class(cfg, bc1, bc2):
    if bc1 == 0:
        return 0
    if bc1 < 0:
        return 1
    return 2 + (bc1 - 1) * (2 if cfg.is_dual else 1) + (bc2 - 1 if cfg.is_dual else 0)


@pytest.mark.parametrize("dual", [False, True])
def test_classes_verdicts_and_paths(tmp_path, dual):
    cfg = _config(dual, gzip_output=dual)
    lay = OutputLayout(cfg, str(tmp_path), "p1", "p2", False)
    assert (lay.stride, lay.n_classes, lay.gz) == ((2, 8, 1) if dual else (1, 5, 0))
    v = _verdicts(cfg)
    assert len(v) == lay.n_classes
    bc1 = np.array([a for a, _ in v] * 2, dtype=np.int32)
    bc2 = np.array([b for _, b in v] * 2, dtype=np.int32)
    out = np.full(len(bc1), -7, dtype=np.int32)
    cls = lay.classes(bc1, bc2, out)
    assert cls is out and cls.dtype == np.int32
    assert cls.tolist() == [_scalar_class(cfg, a, b) for a, b in v] * 2
    assert sorted(cls[:len(v)].tolist()) == list(range(lay.n_classes))  # a bijection onto the classes
    assert [lay.verdict(int(c)) for c in cls[:len(v)]] == v
    # an ambiguous first pass may carry any second verdict: still class 1
    assert lay.classes(np.array([-1, 0], dtype=np.int32), np.array([2, 1], dtype=np.int32),
                       np.empty(2, dtype=np.int32)).tolist() == [1, 0]
    for used in ([], [0], [1, lay.n_classes - 1], list(range(lay.n_classes))):
        arr = lay.c_paths("p1", np.array(used, dtype=np.int64))
        assert len(arr) == lay.n_classes
        for c in range(lay.n_classes):
            want = os.path.join(str(tmp_path), "p1." + filename_for(cfg, *v[cls[:len(v)].tolist().index(c)])).encode()
            assert arr[c] == (want if c in used else None), (used, c)


@pytest.mark.parametrize("trim", [{}, {"trim_side": 5}, {"trim_side2": 3}])
def test_streams(trim):
    t = bool(trim)
    lay = lambda paired, **kw: OutputLayout(_config("trim_side2" in trim, **trim, **kw), "o", "r1", "r2", paired)  # noqa: E731
    assert lay(False).streams == [(0, "r1", t)]  # core.jl:191-196
    assert lay(False, classify_both=True).streams == [(0, "r1", t)]  # (classify_both means nothing without R2)
    assert lay(True).streams == [(1, "r2", False)]  # core.jl:186-190
    assert lay(True, classify_both=True).streams == [(0, "r1", t), (1, "r2", False)]  # core.jl:175-185: only R1 is trimmed
