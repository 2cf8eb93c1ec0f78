"""The classify entries at read offsets that do not start at 0 and that cross 2^31 and 2^32, and batches in hostile
surroundings (offset_cases.py).

Device entry: one allocation of 2^31 + 2^32 + 16 MiB bytes; the byte pointer handed to bdx_classify_device is its start plus
2^31 (rounded up to 16, plus a phase of 0..15), the offsets are a lattice recipe's plus a base.  Before every call a decoy
batch (same offsets, other reads) is written wherever an offset cut to 32 bits, zero- or sign-extended, would point: all inside
the allocation, so a truncation shows as a wrong verdict, not as a fault.  One recipe per fetch site (offset_cases.SITES), six
bases each, both batches, two or three phases per base, all calls of a recipe on one context; the launch log must show the
site, and every output (doubles by bit pattern) and the counters must equal the oracle's on the plain batch.

Hostile surroundings: the first read begins and the last read ends with a barcode cut by 1 or 3 bases, the missing bases lie
just outside the batch among back-to-back copies of another barcode.  Expected: the oracle on the batch alone.

Host entry: the staged, plain, window-upload routes of bdx_classify_host through a sparse host array of the same size (the
pipelined route: test_pipelined_host_upload_equals_the_single_upload in test_gpu_parity.py), and a non-monotone offset vector
at a large base.  The device-entry cases come first: the host routes hand the same kernels a pointer outside its allocation.

BDX_OFFSET_COVERAGE=<file>: one line per case and batch is appended there: the recipe, the base, the phases, the launch-log
line that shows the site, the time of the calls (profiles/offset_base_coverage.txt is such a run)."""
import functools
import os
import time

import numpy as np
import pytest

import fuzz
import helpers as H
import kernel_lattice as KL
import offset_cases as OC
from test_kernel_lattice_gpu import KNOBS, check_cell_launches, check_launches, check_list_launch

pytestmark = pytest.mark.gpu

NTHREADS = min(16, os.cpu_count() or 1)
VERDICT = ("bc1", "bc2", "keep_start", "keep_end")
PASS_I32 = ("pass_start", "pass_end", "pass_raw", "pass_bc")
PASS_F64 = ("pass_score", "pass_delta")


def _cover(*fields):
    path = os.environ.get("BDX_OFFSET_COVERAGE")
    if path:
        with open(path, "a") as f:
            f.write("\t".join(str(x) for x in fields) + "\n")


class Arena:
    """The device allocation and the index of the origin O in it: O is 16-byte aligned, 2^31 bytes or a little more behind
    the allocation's start."""

    def __init__(self, buf):
        self.buf = buf
        self.origin = OC.P31 + (-(buf.data_ptr() + OC.P31)) % 16
        assert (buf.data_ptr() + self.origin) % 16 == 0 and OC.P31 <= self.origin and self.origin + 16 + OC.P32 + (8 << 20) <= buf.numel()

    def place(self, shift: int, rel: int, data):
        """data -> the bytes at offset `rel` from the byte pointer O + shift."""
        import torch

        at = self.origin + shift + rel
        assert 0 <= at and at + len(data) <= self.buf.numel(), (shift, rel, len(data))
        self.buf[at: at + len(data)] = torch.from_numpy(np.ascontiguousarray(data)).to(self.buf.device)

    def classify(self, hc, want_pass: bool, seq, off, base: int, shift: int, dec, before=None, after=None):
        """One bdx_classify_device call on the batch placed at `base` behind O + shift, decoys in every alias window first.
        -> outputs as numpy arrays."""
        import torch

        n, total = len(off) - 1, len(seq)
        for a, lo, hi in OC.alias_runs(base, total):
            self.place(shift, a, dec[lo:hi])
        if before is not None:
            self.place(shift, base - len(before), before)
            self.place(shift, base + total, after)
        self.place(shift, base, seq)
        dev = self.buf.device
        d_off = torch.from_numpy(np.ascontiguousarray(off + base, dtype=np.int64)).to(dev)
        # (outputs start as garbage: an element no kernel writes does not come back as the call before left it)
        d_out = {k: torch.full((n,), -77, dtype=torch.int32, device=dev) for k in VERDICT}
        if want_pass:
            d_out.update({k: torch.full((n, 2), -77, dtype=torch.int32, device=dev) for k in PASS_I32})
            d_out.update({k: torch.full((n, 2), -77.0, dtype=torch.float64, device=dev) for k in PASS_F64})
        hc.reset_counts()
        hc.classify_device(self.buf.data_ptr() + self.origin + shift, d_off.data_ptr(), n, **{k: v.data_ptr() for k, v in d_out.items()})
        hc.sync()
        return {k: v.cpu().numpy() for k, v in d_out.items()}


@pytest.fixture(scope="module")
def arena():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert os.path.exists(H.bdx.LIB_PATH), "HIP extension missing: run __graft_entry__.build()"
    free, _total = torch.cuda.mem_get_info()
    if free < OC.ARENA_MIN_FREE:
        pytest.skip(f"the offset arena needs {OC.ARENA_MIN_FREE >> 30} GiB of free device memory, {free >> 30} GiB are free")
    buf = torch.empty(OC.ARENA_BYTES, dtype=torch.uint8, device="cuda:0")  # (not initialised: only what a case writes is ever touched)
    yield Arena(buf)
    del buf
    torch.cuda.empty_cache()


class Contexts:
    """One live context: the calls of a recipe follow one another on it, whatever their base; the next recipe gets a new one
    (the developer switches are read when a context is created)."""

    def __init__(self):
        self.name, self.hc = None, None

    def close(self):
        if self.hc is not None:
            self.hc.close()
        self.name, self.hc = None, None

    def get(self, name):
        if self.name != name:
            self.close()
            obj = OC.get(name)
            saved = {k: os.environ.get(k) for k in KNOBS}
            try:
                for k in KNOBS:
                    os.environ.pop(k, None)
                os.environ.update(obj.env)
                self.hc = H.bdx.HipClassifier(obj.config(), **OC.hc_kwargs(name))
            finally:
                for k, v in saved.items():
                    os.environ.pop(k, None)
                    if v is not None:
                        os.environ[k] = v
            if OC.hint(name) is not None:
                self.hc.set_read_length_hint(OC.hint(name))
            self.name = name
        return self.hc


@pytest.fixture(scope="module")
def contexts():
    c = Contexts()
    yield c
    c.close()


def _oracle(name, seq, off):
    obj = OC.get(name)
    oc = H.orc.OracleClassifier(obj.config(), nthreads=NTHREADS, want_pass=obj.want_pass)
    exp = oc.classify(seq, off)
    return exp, oc.counts.copy()


@functools.lru_cache(maxsize=None)
def expected(name, which):
    """(batch, oracle outputs, oracle counters, decoy) of a recipe's batch: computed once, shared, never written to."""
    seq, off, _ = OC.get(name).batch(which)
    exp, counts = _oracle(name, seq, off)
    return seq, off, exp, counts, OC.decoy(name, off)


@functools.lru_cache(maxsize=None)
def expected_hostile(name, variant, c):
    seq, off, before, after, plants = OC.hostile(name, variant, c)
    exp, counts = _oracle(name, seq, off)
    return seq, off, before, after, exp, counts, OC.decoy(name, off)


def check_site(name, hc, launches, n, what, band_before):
    """The launch log shows the fetch site the recipe stands for; -> the line that proves it."""
    site, target = OC.SITE_OF[name], OC.target(name)
    line = lambda ln: " ".join(f"{k}={ln[k]}" for k in ("kernel", "blocks", "threads", "tile", "units", "reads", "list"))  # noqa: E731
    if site in ("wave_contiguous", "wave_split", "wave_scattered", "window"):
        check_launches(launches, target, n, what)
        if site == "wave_split":
            assert launches[-1]["family"] == "generic", what
        if site == "window":
            assert "wave(win)" in hc.kernel_path, what
        return line([ln for ln in launches if ln["kernel"] == target][0])
    if site == "wave_carry":
        ks = KL.code_object_kernels()
        assert all(ln["kernel"] in ks for ln in launches), what
        hits = [ln for ln in launches if ln["kernel"] == target and ln["list"]]
        listed = hc.last_list_reads
        assert len(hits) == 1 and listed >= 2 * 16 * hits[0]["units"] > 0, f"{what}: {listed} listed reads"
        return line(hits[0]) + f" listed={listed}"
    if site == "pairs_list":
        listed = hc.last_list_reads
        check_list_launch(launches, target, listed, n, what)
        return line([ln for ln in launches if ln["kernel"] == target][0]) + f" listed={listed}"
    check_cell_launches(launches, target, n, what)
    proof = [ln for ln in launches if ln["kernel"] == target and not ln["list"]][0]
    if site == "fused_list":
        fused = [ln for ln in launches if ln["family"] == "bitpar" and ln["list"]]
        listed = hc.last_list_reads
        assert fused and listed > 0, f"{what}: {listed} listed reads"
        return line(fused[0]) + f" listed={listed}"
    if site == "exact_band":
        assert hc.band_launches - band_before >= 1, what
        return line(proof) + f" band_launches=+{hc.band_launches - band_before}"
    if site in ("exact_alone", "exact_alone_m1"):
        assert [ln["family"] for ln in launches] == ["generic"], what
    return line(proof)


@pytest.mark.parametrize("label", OC.BASE_LABELS)
@pytest.mark.parametrize("name", OC.NAMES)
def test_device_entry_at_a_base(name, label, arena, contexts):
    obj = OC.get(name)
    hc = contexts.get(name)
    for which in ("main", "edge"):
        seq, off, exp, counts, dec = expected(name, which)
        n = len(off) - 1
        base = OC.bases(off)[label]
        t0 = time.perf_counter()
        for shift in OC.SHIFTS[label]:
            band_before = hc.band_launches
            got = arena.classify(hc, obj.want_pass, seq, off, base, shift, dec)
            launches = hc.last_launches
            what = f"{OC.SITE_OF[name]} {name} {which} batch ({n} reads) at base {base} ({label}), phase {shift} [{hc.kernel_path}] {launches}"
            fuzz.assert_same(got, exp, what)
            assert np.array_equal(hc.counts, counts), f"{what}: counters"
            assert hc.rejected_windows == 0, what
            proof = check_site(name, hc, launches, n, what, band_before)
        _cover("base", OC.SITE_OF[name], name, which, label, base, "phases " + ",".join(map(str, OC.SHIFTS[label])), proof,
               "%.2f ms" % (1e3 * (time.perf_counter() - t0)))


@pytest.mark.parametrize("label", ("small", "in_2p32"))
@pytest.mark.parametrize("name", OC.HOSTILE_NAMES)
def test_hostile_surroundings(name, label, arena, contexts):
    obj = OC.get(name)
    hc = contexts.get(name)
    target = OC.target(name)
    for j, variant in enumerate(OC.hostile_variants(name)):
        t0 = time.perf_counter()
        for c in OC.PLANT_CUTS:
            seq, off, before, after, exp, counts, dec = expected_hostile(name, variant, c)
            n = len(off) - 1
            base = OC.bases(off)[label]
            shift = (3 + 5 * j + c) % 16
            got = arena.classify(hc, obj.want_pass, seq, off, base, shift, dec, before, after)
            launches = hc.last_launches
            what = f"{OC.SITE_OF[name]} {name} hostile {variant} c={c} ({n} reads) at base {base} ({label}), phase {shift} [{hc.kernel_path}] {launches}"
            fuzz.assert_same(got, exp, what)
            assert np.array_equal(hc.counts, counts), f"{what}: counters"
            assert hc.rejected_windows == 0, what
            if variant == "full":  # (the main batch's size: the plan is the main batch's)
                assert any(ln["kernel"] == target for ln in launches), what
        _cover("hostile", OC.SITE_OF[name], name, f"{variant} ({n} reads), cut 1 and 3", label, base, "phases %d,%d" % ((4 + 5 * j) % 16, (6 + 5 * j) % 16),
               " | ".join(ln["kernel"] for ln in launches), "%.2f ms" % (1e3 * (time.perf_counter() - t0)))


# ---- the host entry ----
@pytest.fixture(scope="module")
def host_view(arena):
    """The host entry's seq_bytes: a view 2^31 bytes into a sparse array of the arena's size (pages no case writes are never
    committed).  Depends on the device arena so that the device-entry cases are what this module is skipped with."""
    big = np.empty(OC.ARENA_BYTES, dtype=np.uint8)
    yield big[OC.P31:]
    del big


def _host_call(hc, view, seq, off, base):
    view[base: base + len(seq)] = seq
    hc.reset_counts()
    return hc.classify(view, off + base)


def test_host_staged_route(host_view, contexts):
    """At most 2 MiB of bytes and offsets: one page-locked staging buffer, the kernels see d_seq - seq_off[0]."""
    name = OC.HEADLINE
    seq, off, exp, counts, _ = expected(name, "main")
    n = len(off) - 1
    assert len(seq) + 8 * (n + 1) <= (2 << 20)
    hc = contexts.get(name)
    for base in (1, 15, 4103, OC.bases(off)["in_2p32"]):
        got = _host_call(hc, host_view, seq, off, base)
        what = f"staged route at base {base} [{hc.kernel_path}] {hc.last_launches}"
        fuzz.assert_same(got, exp, what)
        assert np.array_equal(hc.counts, counts) and hc.rejected_windows == 0, what
        assert hc.pipelined_calls == 0 and hc.window_uploads == 0, what
        check_launches(hc.last_launches, name, n, what)


def test_host_plain_route(host_view):
    """Above 2 MiB, below the pipelined route's 96 MiB: bytes and offsets in one copy each, the offsets as given."""
    cfg = OC.c2_config()
    seq, off = OC.plain_route_batch()
    n = len(off) - 1
    assert len(seq) + 8 * (n + 1) > (2 << 20)
    oc = H.orc.OracleClassifier(cfg, nthreads=NTHREADS, want_pass=False)
    exp = oc.classify(seq, off)
    b = OC.bases(off)
    with H.bdx.HipClassifier(cfg, want_pass=False) as hc:
        for base in (1, b["in_2p31"], b["in_2p32"]):
            got = _host_call(hc, host_view, seq, off, base)
            what = f"plain route at base {base} [{hc.kernel_path}]"
            fuzz.assert_same(got, exp, what)
            assert np.array_equal(hc.counts, oc.counts) and hc.rejected_windows == 0, what
            assert hc.pipelined_calls == 0 and hc.window_uploads == 0, what


def test_host_window_upload_route(host_view):
    """Long reads with a short window: only each read's window goes up, gathered on the host from seq_bytes + seq_off[i]."""
    cfg, seq, off = OC.window_route_case()
    oc = H.orc.OracleClassifier(cfg, nthreads=NTHREADS)
    exp = oc.classify(seq, off)
    assert (exp["bc1"] > 0).mean() > 0.2
    with H.bdx.HipClassifier(cfg, want_pass=True) as hc:
        for k, base in enumerate((15, OC.bases(off)["in_2p32"])):
            got = _host_call(hc, host_view, seq, off, base)
            what = f"window upload at base {base} [{hc.kernel_path}]"
            assert hc.window_uploads == k + 1 and hc.pipelined_calls == 0, what
            fuzz.assert_same(got, exp, what)
            assert np.array_equal(hc.counts, oc.counts) and hc.rejected_windows == 0, what


def test_non_monotone_offsets_at_a_large_base_are_refused(host_view, contexts):
    name = OC.HEADLINE
    seq, off, exp, counts, _ = expected(name, "main")
    hc = contexts.get(name)
    base = OC.bases(off)["in_2p32"]
    host_view[base: base + len(seq)] = seq
    bad = off + base
    bad[10] = bad[12]  # (read 10 would have a negative length; the first and the last offset are as they were)
    with pytest.raises(H.bdx.BdxError, match="seq_off is not non-decreasing"):
        hc.classify(host_view, bad)
    hc.reset_counts()
    got = hc.classify(host_view, off + base)
    fuzz.assert_same(got, exp, f"after the refused call [{hc.kernel_path}]")
    assert np.array_equal(hc.counts, counts) and hc.rejected_windows == 0
