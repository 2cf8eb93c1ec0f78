"""Cases for the device entry point as hosts drive it: bdx_classify_device call after call on a
caller's stream with nothing in between.  A case is a config, the developer switches it runs under and six batches; a SCHEDULE
puts the batches into an order; every call of a schedule carries the outputs it asks for, the read-length hint in force and the
kernel_path the per-call planner (csrc/bdx_call.cpp) must report after it.  The expected paths are written down here;
test_device_async_cases_cpu.py holds them against tests/call_host.cpp (the planner alone, on the CPU) at 7 and at 256 compute
units, and checks with the oracle that every batch has matched, unknown and (min_delta > 0) ambiguous reads.

No GPU import here: the builders run on the CPU."""
from __future__ import annotations

import numpy as np

import call_cases as CC
import helpers as H
import plan_cases as PC
from biodemux_jl_amd import synth

# the smallest sizes that still go wrong: one read, a tile and a bit, several tiles, one beyond 4096, and with 7 compute units a
# walked tile queue and several tiles per wave
SIZES = (1, 33, 700, 4097, 9000, 20011)
SCHEDULES = {
    "growth": (1, 0, 3, 2, 5, 4),     # 33, 1, 4097, 700, 20011, 9000: every hand-over buffer grows twice after the first call
    "no_growth": (5, 0, 4, 1, 3, 2),  # 20011, 1, 9000, 33, 4097, 700: the first call sizes every buffer
}
VERDICTS = ("bc1", "bc2", "keep_start", "keep_end")
POSITIONS = VERDICTS + ("pass_start", "pass_end")
EVERYTHING = POSITIONS + ("pass_raw", "pass_bc", "pass_score", "pass_delta")
ABI_ORDER = ("bc1", "bc2", "keep_start", "keep_end", "pass_start", "pass_end", "pass_raw", "pass_bc", "pass_score", "pass_delta")
KNOBS = {"BDX_CU_COUNT": "n_cu", "BDX_NO_WAVE": "no_wave", "BDX_NO_KALN": "no_kaln"}
SWITCHES = tuple(KNOBS)  # what a test clears before it sets a case's own
I32_SENTINEL = -0x5A5A5A5B
F64_SENTINEL = -1.2345e300
ALG = {"semiglobal": PC.SEMIGLOBAL, "hamming": PC.HAMMING, "exact": PC.EXACT}


class Call:
    """One bdx_classify_device call: which batch, what it asks for, the hint in force (None: the schedule's longest read)."""
    def __init__(self, size, min_len, max_len, seed, wanted, hint, path):
        self.size, self.min_len, self.max_len, self.seed, self.wanted, self.hint, self.path = size, min_len, max_len, seed, tuple(wanted), hint, path

    @property
    def key(self):
        return (self.size, self.min_len, self.max_len, self.seed)

    @property
    def mask(self):
        return sum(1 << ABI_ORDER.index(k) for k in self.wanted)


class AsyncCase:
    """kw: DemuxConfig switches; lens / wanted / hints: per batch (index into SIZES) unless by_position (then per call of the
    schedule: read length rising over the schedule, whatever the order of the sizes); paths: one string (every call), a list
    (per batch, like the others) or, where a call's path depends on the calls before it, schedule -> path per call."""
    def __init__(self, name, family, kw, paths, bcs, bcs2=None, env=None, filter="auto", lens=(75, 150), wanted=VERDICTS, hints=None,
                 reads=None, by_position=False, seed=0, again=None):
        self.name, self.family, self.kw, self.paths, self.bcs, self.bcs2 = name, family, dict(kw), paths, list(bcs), list(bcs2 or [])
        self.env, self.filter, self.lens, self.wanted, self.hints = dict(env or {}), filter, lens, wanted, hints
        self.reads, self.by_position, self.seed = dict(reads or {}), by_position, seed
        self.again = again  # schedule -> path per call when the same schedule runs a second time on the context (None: as the first time)

    @property
    def summary(self):
        return bool(self.kw.get("summary"))

    @property
    def min_delta(self):
        return float(self.kw.get("min_delta", 0.0))

    def config(self):
        ids = dict(bc_seqs=self.bcs, bc_lengths_no_N=[len(b) for b in self.bcs], ids=["a%d" % i for i in range(len(self.bcs))])
        if self.bcs2:
            ids.update(is_dual=True, bc_seqs2=self.bcs2, bc_lengths_no_N2=[len(b) for b in self.bcs2], ids2=["b%d" % i for i in range(len(self.bcs2))])
        kw = dict(self.kw)
        if "ref_search_range" in kw:
            kw["ref_search_range"] = H.bdx.parse_dynamic_range(kw["ref_search_range"])
        return H.bdx.DemuxConfig(**ids, **kw)

    def _per(self, what, batch, pos):
        if isinstance(what, list):
            return what[(pos if self.by_position else batch) % len(what)]
        return what

    def calls(self, schedule, again=False):
        order = SCHEDULES[schedule]
        out = []
        for pos, batch in enumerate(order):
            lo, hi = self._per(self.lens, batch, pos)
            slot = pos if self.by_position else batch
            path = self.paths[schedule][pos] if isinstance(self.paths, dict) else self.paths if isinstance(self.paths, str) else self.paths[slot]
            if again and self.again is not None:
                path = self.again[schedule][pos]
            out.append(Call(SIZES[batch], lo, hi, 7000 + 100 * self.seed + slot + (50 if self.by_position and schedule != "growth" else 0),
                            self._per(self.wanted, batch, pos), self._per(self.hints, batch, pos), path))
        return out

    def hint_for(self, schedule, call):
        """The hint the host sets before the call (bdx_set_read_length_hint): the call's own, else the schedule's longest read."""
        return call.hint if call.hint is not None else max(c.max_len for c in self.calls(schedule))

    def length_rows(self, schedule):
        """Per call what bdx_batch_len (csrc/bdx_call.cpp) is asked as a host drives the device entry point: no window upload,
        nothing seen on the host, the hint in force, and the batch's true longest read were the device to measure it.
        (filter: as the config asks for one; a config outside every filter's domain runs the generic kernel at any length.)"""
        return [(0, 0, self.hint_for(schedule, c), int(self.summary), int(self.filter != "off"), int(np.diff(make_batch(self, c)[1]).max()))
                for c in self.calls(schedule)]

    def plan_case(self, schedule, n_cu, planned):
        """The case as tests/call_host.cpp reads it: the same barcodes, switches and calls, the schedule twice over.  planned: per
        call of the schedule the read length the library plans it for (the driver's answer to length_rows)."""
        def rng(key):
            r = self.kw.get(key)
            if r is None:
                return PC.WHOLE
            d = H.bdx.parse_dynamic_range(r)
            return (int(d.start_offset), int(d.end_offset), int(bool(d.start_from_end)), int(bool(d.end_from_end)))
        passes = [PC.one_pass(self.bcs, trim=self.kw.get("trim_side") or 0, ref=rng("ref_search_range"))]
        if self.bcs2:
            passes.append(PC.one_pass(self.bcs2, trim=self.kw.get("trim_side2") or 0))
        tune = {KNOBS[k]: int(v) for k, v in self.env.items()}
        tune["n_cu"] = n_cu
        calls = [CC.call(c.size, L, wanted=c.mask, stats=int(self.summary)) for c, L in list(zip(self.calls(schedule), planned)) * 2]
        return CC.CallCase(self.name + "." + schedule, None, calls, passes=passes, rate=self.kw["max_error_rate"], min_delta=self.min_delta,
                           costs=(self.kw.get("match", 0), self.kw.get("mismatch", 1), self.kw.get("indel", 1)),
                           algorithm=ALG[self.kw.get("matching_algorithm", "semiglobal")], summary=int(self.summary),
                           filter=PC.OFF if self.filter == "off" else PC.AUTO, tune=tune)


# ---- reads -----------------------------------------------------------------------------------------------------------------
_READS = {}


def _put(seq, off, i, at, text):
    n = int(off[i + 1] - off[i])
    b = np.frombuffer(text.encode(), dtype=np.uint8)[:max(0, n - at)]
    seq[off[i] + at: off[i] + at + len(b)] = b


def make_batch(case: AsyncCase, call: Call):
    """Ragged reads with planted barcodes, sequencing errors and concatemers (as tests/fuzz.py makes them), a few percent of
    low-complexity reads (many chance seeds: the hand-over lists are never empty), read 0 with an intact barcode (a batch of
    one read is a match) and, from 33 reads on, two reads with two different intact barcodes (ambiguous under min_delta > 0)."""
    key = (case.name,) + call.key
    if key in _READS:
        return _READS[key]
    n, lo, hi = call.size, call.min_len, call.max_len
    kw = dict(plant_frac=0.8, sub=0.03, ins=0.008, dele=0.008, n_rate=0.003)
    kw.update(case.reads)
    second_at = kw.pop("second_at", None)
    if case.bcs2:
        kw["second"] = (case.bcs2, second_at[0], second_at[1])
    if n >= 33:
        kw["repeat"] = dict(frac=0.15)
    seq, off, _ = synth.make_ragged_reads(case.bcs, n, lo, hi, seed=call.seed, **kw)
    seq = seq.copy()
    rng = np.random.Generator(np.random.PCG64(call.seed ^ 0xA51C))
    m = len(case.bcs[0])
    at = int(kw.get("plant_lo", 0))
    _put(seq, off, 0, at, case.bcs[call.seed % len(case.bcs)])
    if case.bcs2:
        _put(seq, off, 0, second_at[0], case.bcs2[call.seed % len(case.bcs2)])
    if n >= 33:
        for i in rng.choice(np.arange(1, n), size=max(2, n * 3 // 100), replace=False):
            period = int(rng.integers(1, 4))
            motif = "".join("ACGT"[int(c)] for c in rng.integers(0, 4, size=period))
            _put(seq, off, int(i), 0, motif * (hi // period + 1))
        room = np.flatnonzero(off[2:] - off[1:-1] >= at + 2 * m + 4) + 1  # (not read 0)
        for j, i in enumerate(room[:2]):
            a, b = (call.seed + j) % len(case.bcs), (call.seed + j + 1 + len(case.bcs) // 2) % len(case.bcs)
            _put(seq, off, int(i), at, case.bcs[a] + "TTGA" + case.bcs[b])
    _READS[key] = (seq, off)
    return seq, off


# ---- the oracle, once per batch ---------------------------------------------------------------------------------------------
_EXPECTED = {}


def expected(case: AsyncCase, call: Call, nthreads: int = 8):
    """(per-read outputs incl. the per-pass ones, counter vector) of the oracle for this batch alone."""
    key = (case.name,) + call.key
    if key not in _EXPECTED:
        seq, off = make_batch(case, call)
        oc = H.orc.OracleClassifier(case.config(), nthreads=nthreads, want_pass=True)
        out = oc.classify(seq, off)
        _EXPECTED[key] = (out, oc.counts.copy())
    return _EXPECTED[key]


# ---- the families -----------------------------------------------------------------------------------------------------------
B96 = synth.make_barcodes(96, 24, seed=20260515)
B24, B16 = synth.make_barcodes(24, 24, seed=1), synth.make_barcodes(16, 24, seed=2)
B130 = synth.make_barcodes(8, 130, seed=9, min_hamming=40)
B20S, B12S = synth.make_barcodes(20, 16, seed=83, min_hamming=5), synth.make_barcodes(12, 16, seed=84, min_hamming=5)
CASES = []


def case(*a, **kw):
    CASES.append(AsyncCase(*a, seed=len(CASES), **kw))


TIER = "tier1:wave > pairs > qgram2+bitpar+verify"
# 1. the headline: the wave kernel answers, the known-score exact list takes the rest
case("headline", 1, dict(max_error_rate=0.1), "wave > qgram+bitpar+verify", B96)
# 2. tiered budgets with the pairs mode between the tiers
case("rate02", 2, dict(max_error_rate=0.2), TIER, B96)
# 3. dual, trim 5 / 3: known-end forms of both kernels, carried passes (min_delta = 0, verdicts only)
case("dual_trim53", 3, dict(max_error_rate=0.2, trim_side=5, trim_side2=3), "tier1:wave(end) > pairs(end) > bitpar+verify", B24, bcs2=B16,
     lens=(140, 160), reads=dict(plant_lo=0, plant_hi=40, second_at=(90, 110)))
# 4. the wanted outputs alternate from one unsynchronised call to the next: (end) <-> (aln) forms
case("trim5_alternating", 4, dict(max_error_rate=0.2, min_delta=0.1, trim_side=5),
     ["tier1:wave(aln) > pairs(aln) > qgram2+bitpar+verify" if b % 2 else "tier1:wave(end) > pairs(end) > qgram2+bitpar+verify" for b in range(6)], B96,
     wanted=[VERDICTS, POSITIONS])
#    ... and the shape whose second call once inherited the first one's list mode (call_cases.seq_kend_then_pass_start)
case("kend_then_pass_start", 4, dict(max_error_rate=0.1, trim_side=5),
     ["wave+verify" if b % 2 else "wave(end) > qgram+bitpar+verify" for b in range(6)], B96, env={"BDX_NO_KALN": "1"}, wanted=[VERDICTS, POSITIONS])
# 5. :hamming: the wave kernel as the filter of a split launch, with windows
case("hamming", 5, dict(max_error_rate=0.1, matching_algorithm="hamming"), "wave+verify", B96, reads=dict(ins=0.002, dele=0.002))
# 6. a 60-column window; the hint changes between the calls: window mode for 120 and 300, not for 100
case("window60_hints", 6, dict(max_error_rate=0.1, ref_search_range="1:60"),
     [("wave(win)", "wave", "wave(win)")[b % 3] + " > qgram+bitpar+verify" for b in range(6)], B96,
     lens=[(60, 120), (50, 100), (150, 300)], hints=[120, 100, 300], reads=dict(plant_lo=0, plant_hi=30))
# 7. no wave kernel; both schedules start at 150 bases with the two-intact-pieces index, 313 bases demote it, and it stays demoted
T1 = "tier1:qgram+bitpar > "
case("no_wave_demotion", 7, dict(max_error_rate=0.2), {s: [T1 + "qgram2+bitpar+verify"] + [T1 + "bitpar+verify"] * 5 for s in SCHEDULES}, B96,
     again={s: [T1 + "bitpar+verify"] * 6 for s in SCHEDULES}, env={"BDX_NO_WAVE": "1"}, lens=[(157, 313), (75, 150)], hints=[313, 150])
# 8. weighted costs with trimming: the fused kernel as the filter of a split launch, band DP in the exact kernel (two operations)
case("weighted_trim3", 8, dict(max_error_rate=0.1, mismatch=1, indel=2, trim_side=3), "qgram+bitpar+verify", B96, env={"BDX_NO_WAVE": "1"})
#    ... and with the wave kernels: tiered, the pairs mode as tier 0's split filter
case("weighted_pairs_split", 8, dict(max_error_rate=0.15, mismatch=1, indel=2, trim_side=3), "tier1:wave > pairs+verify", B96)
# 9. the generic kernel alone: filter off; barcodes beyond 128 nt; and one context that does both (a hint no tile of the fused
#    kernel holds, 20 000 bases, for the batches of even index; the attempt leaves the plain sweep behind for the filtered calls)
case("filter_off", 9, dict(max_error_rate=0.1), "generic", B96, filter="off")
case("barcodes130", 9, dict(max_error_rate=0.1), "generic", B130, lens=(150, 300))
case("filtered_and_not", 9, dict(max_error_rate=0.1),
     {s: ["wave > qgram+bitpar+verify"] + ["wave > bitpar+verify" if b % 2 else "generic" for b in o[1:]] for s, o in SCHEDULES.items()}, B96,
     hints=[20000, 150], again={s: ["wave > bitpar+verify" if b % 2 else "generic" for b in o] for s, o in SCHEDULES.items()})
# 10. summary: the statistics tables grow with the read length, which rises over the schedule
RISING = [(30, 60), (40, 80), (50, 100), (75, 150), (110, 220), (150, 300)]
case("summary_single", 10, dict(max_error_rate=0.2, summary=True), "tier1:wave(aln) > pairs(aln) > qgram2+bitpar+verify", B96, lens=RISING, by_position=True,
     wanted=EVERYTHING)
case("summary_dual", 10, dict(max_error_rate=0.25, trim_side=5, trim_side2=3, summary=True), "tier1:wave > bitpar+verify", B20S, bcs2=B12S,
     lens=[(52, 60), (60, 80), (70, 100), (90, 150), (120, 220), (150, 300)], by_position=True, wanted=EVERYTHING,
     reads=dict(plant_lo=0, plant_hi=8, second_at=(28, 34)))

BY_NAME = {c.name: c for c in CASES}
NO_SUMMARY = [c.name for c in CASES if not c.summary]


def predicted_paths(directory, exe=None):
    """{(case, schedule, n_cu): [path per call of the schedule run twice on one context]} from the stand-alone planner driver."""
    exe = exe or CC.build_driver(directory)
    asked = [(c, s) for c in CASES for s in SCHEDULES]
    rows = [c.length_rows(s) for c, s in asked]
    answers = iter(CC.run_lengths(exe, directory, [r for per_case in rows for r in per_case]))
    planned = {(c.name, s): [next(answers)[2] for _ in per_case] for (c, s), per_case in zip(asked, rows)}
    cases, keys = [], []
    for c in CASES:
        for s in SCHEDULES:
            for n_cu in (7, 256):
                pc = c.plan_case(s, n_cu, planned[(c.name, s)])
                pc.name = "%s.%s.%d" % (c.name, s, n_cu)
                cases.append(pc)
                keys.append((c.name, s, n_cu))
    rep = CC.run_driver(exe, directory, cases=cases)
    out = {}
    for k, pc in zip(keys, cases):
        r = rep[pc.name]
        out[k] = [r.path(i) if r.i("c%d.filtered" % i) else "generic" for i in range(len(pc.calls))]
    return out
