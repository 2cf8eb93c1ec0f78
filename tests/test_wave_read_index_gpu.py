"""GPU checks of the wave kernel's hit -> read mapping in its LEAN forms (csrc/bdx_read_index.h, the resolve of
csrc/bdx_wave_kernel.h): in a tile of equal-length reads the read of a seed hit is floor(x / len) by one multiply-high, with the
multiplier of the planned read length from the kernel's arguments and a tile of any other length working out its own.

The C2 barcode set (96 of 24 nt) at rate 0.1, 32-read tiles, one pretended compute unit (16 waves), 659 reads (21 tiles, the
last one of 19 reads) unless a case says otherwise.  Reads are random bases with a copy of a barcode (0 .. 3 substitutions; a
prefix of it where the read is shorter) in nine of ten.  Every case compares every output and the counter vector bit for bit
with the CPU oracle and with the general kernel alone (BDX_NO_WAVE), and asserts through the launch log that the wave kernel
took the whole batch in the headline's form (the 160-base case: its ten-vector sibling, which keeps the earlier mapping).
"""
from __future__ import annotations

import numpy as np
import pytest

from test_wave_tile_deal_gpu import HEADLINE, _need_gpu, c2_barcodes, c2_config, check_case  # noqa: F401  (_need_gpu: the module's GPU fixture)

pytestmark = pytest.mark.gpu

ENV = {"BDX_CU_COUNT": 1, "BDX_WAVE_RW": 32}
N = 32 * 20 + 19
LONGEST = 158  # 32 x 158 + 64 = 5 x 1024: the longest reads whose 32-read tile fits five vectors per lane
TEN_VECTORS = HEADLINE.replace("<32, 20, 5,", "<32, 20, 10,")


def _reads(lens, seed):
    """-> (seq, off, planted barcode or -1, substitutions) for reads of the given lengths."""
    bcs = [np.frombuffer(b.encode(), dtype=np.uint8) for b in c2_barcodes()]
    rng = np.random.Generator(np.random.PCG64(seed))
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    seq = acgt[rng.integers(0, 4, size=int(off[-1]))].copy()
    which = np.full(len(lens), -1, dtype=np.int64)
    subs = np.zeros(len(lens), dtype=np.int64)
    for i, n in enumerate(lens):
        if i % 10 == 9 or n == 0:
            continue
        b = bcs[i % 96].copy()
        subs[i] = i % 4
        for j in rng.choice(24, size=int(subs[i]), replace=False):
            b[j] = acgt[(int(np.flatnonzero(acgt == b[j])[0]) + 1 + int(rng.integers(0, 3))) % 4]
        m = min(24, int(n))
        c = int(rng.integers(0, n - m + 1))
        seq[off[i] + c:off[i] + c + m] = b[:m]
        which[i] = i % 96
    return seq, off, which, subs


def _expect_plants(exp, lens, which, subs):
    """Copies with at most two substitutions in reads that hold a whole barcode match it (budget floor(0.1 x 24) = 2); the test's
    own check that the batch exercises matches and misses."""
    whole = (which >= 0) & (np.asarray(lens) >= 24)
    hit = whole & (subs <= 2)
    assert (exp["bc1"][hit] == which[hit] + 1).all()
    assert (exp["bc1"][np.asarray(lens) < 22] == 0).all()  # (a read of fewer than m - kb bases holds no alignment within the budget)
    if whole.any():
        assert hit.sum() > 0 and (exp["bc1"][whole & (subs == 3)] > 0).mean() < 0.5


@pytest.mark.parametrize("length", [8, 9, 24, 149, 150, 151, LONGEST, 160])
def test_equal_length_batches(length, monkeypatch):
    lens = [length] * N
    seq, off, which, subs = _reads(lens, seed=1000 + length)
    exp = check_case(("len", length), c2_config(), seq, off, monkeypatch, ENV, kernel=HEADLINE if length <= LONGEST else TEN_VECTORS, units=16)
    _expect_plants(exp, lens, which, subs)


@pytest.mark.parametrize("shift", [1, 7, 15])
def test_first_read_off_a_vector_boundary(shift, monkeypatch):
    """The batch's first byte lies 1 .. 15 bytes past a 16-byte boundary: every tile's first base sits `head` positions into the
    flat image (149-base reads: the head changes from tile to tile), and the seeds of the padding in front map to no read."""
    lens = [149] * N
    seq, off, which, subs = _reads(lens, seed=2000 + shift)
    exp = check_case(("shift", shift), c2_config(), seq, off, monkeypatch, ENV, units=16, shift=shift)
    _expect_plants(exp, lens, which, subs)


@pytest.mark.parametrize("length", [150, 157])
def test_barcode_at_the_tiles_first_and_last_base(length, monkeypatch):
    """An exact copy at position 0 of every tile's first read and one that ends at the last base of every tile's last read (the
    ragged tile's too): x = 0 and x = nr x len - 1, the ends of the range the multiply-high maps into the tile."""
    lens = [length] * N
    seq, off, which, subs = _reads(lens, seed=3000 + length)
    bcs = [np.frombuffer(b.encode(), dtype=np.uint8) for b in c2_barcodes()]
    rng = np.random.Generator(np.random.PCG64(5))
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    want = {}
    for t0 in range(0, N, 32):
        first, last = t0, min(t0 + 32, N) - 1
        for r in (first, last):  # (the two reads start from random bases: no other copy in them)
            seq[off[r]:off[r + 1]] = acgt[rng.integers(0, 4, size=length)]
        seq[off[first]:off[first] + 24] = bcs[(3 * t0) % 96]
        seq[off[last + 1] - 24:off[last + 1]] = bcs[(3 * t0 + 1) % 96]
        want[first], want[last] = (3 * t0) % 96 + 1, (3 * t0 + 1) % 96 + 1
    exp = check_case(("ends", length), c2_config(), seq, off, monkeypatch, ENV, units=16)
    for r, b in want.items():
        assert exp["bc1"][r] == b, (r, b, int(exp["bc1"][r]))


def test_wrong_length_hint(monkeypatch):
    """The hint says 150, the reads have 149 bases: no tile has the planned length, each works out its own multiplier."""
    lens = [149] * N
    seq, off, which, subs = _reads(lens, seed=4000)
    exp = check_case("wrong-hint", c2_config(), seq, off, monkeypatch, ENV, units=16, hint=150)
    _expect_plants(exp, lens, which, subs)


def test_mixed_lengths(monkeypatch):
    """Tiles of 150-base reads (the planned length), of 140-base reads (their own multiplier), of one-base reads (no
    multiplier: the mixed-length path) and tiles of 100 .. 150 bases (the mixed-length path, untouched), in turn."""
    rng = np.random.Generator(np.random.PCG64(6))
    lens = []
    for t in range(21):
        nr = 32 if t < 20 else 19
        lens += {0: [150] * nr, 1: [140] * nr, 2: [int(x) for x in rng.integers(100, 151, size=nr)], 3: [1] * nr if t == 3 else [149] * (nr - 1) + [150]}[t % 4]
    assert len(lens) == N
    seq, off, which, subs = _reads(lens, seed=5000)
    exp = check_case("mixed", c2_config(), seq, off, monkeypatch, ENV, units=16)
    _expect_plants(exp, lens, which, subs)
