"""Named call shapes for the per-call planner (csrc/bdx_call.cpp): each case is a config of tests/plan_cases.py (or one built
here the same way), the developer switches it runs under, one or more calls — several calls are a SEQUENCE on one context: the
seed choice is kept between them — and a predicate over the driver's report that proves the case sits on the intended side of
the threshold it is named for.  The stand-alone driver tests/call_host.cpp plans them on the CPU; test_call_plan_cpu.py asserts
the predicates, compares every reported value with tests/golden/call_plans.json and runs the same driver under ASan / UBSan.
No case needs read data."""
import os
import subprocess

import plan_cases as PC

HERE = PC.HERE
CSRC = PC.CSRC
GOLDEN = os.path.join(HERE, "golden", "call_plans.json")
BC1, BC2, KEEP_START, KEEP_END, PASS_START, PASS_END, PASS_RAW, PASS_BC, PASS_SCORE, PASS_DELTA = (1 << i for i in range(10))
FRONT = ["none", "bitpar", "wave", "wave_win", "wave_split", "wave_end", "pairs"]
MIDDLE = ["none", "end", "list", "split", "all"]
FULL = ["none", "wave_split", "bitpar"]
EXACT = ["known", "split", "split_list"]
PLAN_KEYS = "npass tier_len batch_len split windows dense_w short_lb0 short_lb1 front t1_exact middle full exact carry aln".split()
BAND_KEYS = "dense_w m kb0 kb1 lb0 lb1 launches".split()
FUSED_KEYS = "reads_per_block stage_bytes slot_bytes seed_span r_cap diag_nw diag_qcap lds".split()
TILE_KEYS = "rw waves blocks span_cap hq_cap sq_cap slot cpr scan_gpr winm read_len_hint".split()
BY_NAME = {c.name: c for c in PC.CASES}


def call(n_reads, read_len, wanted=0, stats=0, window_upload=0):
    return (n_reads, read_len, window_upload, wanted, stats)


class CallCase(PC.Case):
    """A config + its calls.  why: the threshold (parent's code) the predicate places the case against."""
    def __init__(self, name, pred, calls, base=None, tune=None, **kw):
        if base is not None:
            b = BY_NAME[base]
            a, dual, rate, delta, m, x, g, has_n, nindel, summary, filt = b.cfg
            kw = dict(dict(passes=b.passes, algorithm=a, rate=rate, min_delta=delta, costs=(m, x, g), nindel=nindel if has_n else None, summary=summary,
                           filter=filt), **kw)
            tune = dict(b.tune, **(tune or {}))
        super().__init__(name, pred, kw.pop("passes"), tune=tune, **kw)
        self.calls = [calls] if isinstance(calls, tuple) else list(calls)

    def text(self):
        lines = super().text().splitlines()
        assert lines[-1] == "end"
        return "\n".join(lines[:-1] + ["call %d %d %d %d %d" % c for c in self.calls] + ["end"]) + "\n"


class Report(dict):
    """One case of the driver's output: key -> list of tokens."""
    def i(self, key, at=0):
        return int(self[key][at])

    def plan(self, c=0):
        d = dict(zip(PLAN_KEYS, map(int, self["c%d.plan" % c])))
        d.update(front=FRONT[d["front"]], middle=MIDDLE[d["middle"]], full=FULL[d["full"]], exact=EXACT[d["exact"]])
        return d

    def fused(self, c=0, which="fused"):
        return dict(zip(FUSED_KEYS, map(int, self["c%d.%s" % (c, which)])))

    def tiles(self, which, c=0):
        return dict(zip(TILE_KEYS, map(int, self["c%d.%s" % (c, which)])))

    def band(self, which, c=0):
        """The band fields of tier 1's exact launch (band_t1) / the exact stage (band_exact); None: the call has no such launch."""
        t = self.get("c%d.%s" % (c, which))
        return None if t is None else dict(zip(BAND_KEYS, map(int, t)))

    def band_launches(self, c=0):
        """What the call adds to bdx_band_launches."""
        return sum((self.band(w, c) or {}).get("launches", 0) for w in ("band_t1", "band_exact"))

    def path(self, c=0):
        return " ".join(self["c%d.path" % c])

    def seed(self, c=0):
        return tuple(map(int, self["c%d.seed" % c]))

    def launches(self, c=0):
        """The launches the plan of call c leads to: family, blocks, threads, tile, list + the template arguments it decides."""
        out, j = [], 0
        while "c%d.launch%d" % (c, j) in self:
            t = self["c%d.launch%d" % (c, j)]
            out.append(dict(family=t[0], blocks=int(t[1]), threads=int(t[2]), tile=int(t[3]), list=int(t[4]), args=tuple(map(int, t[5:]))))
            j += 1
        return out

    def flat(self):
        return {k: " ".join(v) for k, v in sorted(self.items())}


def build_driver(directory, flags=("-O1",)):
    exe = os.path.join(str(directory), "call_host")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-o", exe,
                           os.path.join(HERE, "call_host.cpp"), os.path.join(CSRC, "bdx_plan.cpp"), os.path.join(CSRC, "bdx_call.cpp")])
    return exe


def run_driver(exe, directory, cases=None, env=None, launches=False):
    """Runs the cases through the driver; returns {name: Report}.  launches: with the predicted launch lines."""
    cases = CASES if cases is None else cases
    path = os.path.join(str(directory), "call_cases.txt")
    with open(path, "w") as f:
        f.write("".join(c.text() for c in cases))
    out = subprocess.run([exe, path] + (["launches"] if launches else []), env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "call driver ok: %d cases" % len(cases) in out.stdout
    return parse(out.stdout)


def _run_lines(exe, directory, mode, lines, env=None):
    path = os.path.join(str(directory), mode + ".txt")
    with open(path, "w") as f:
        f.write("".join(line + "\n" for line in lines))
    out = subprocess.run([exe, mode, path], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    got = out.stdout.splitlines()
    assert got[-1].endswith("driver ok: %d lines" % len(lines)) and len(got) == len(lines) + 1, got[-1]
    return got[:-1]


def run_lengths(exe, directory, rows, env=None):
    """bdx_batch_len (csrc/bdx_call.cpp) for rows of (window_len, host_len, hint, stats, filter, measured): per row
    (measure, longest, planned) — measure: the device is asked, and the other two are the answer once it said `measured`."""
    return [tuple(map(int, ln.split())) for ln in _run_lines(exe, directory, "lengths", ["%d %d %d %d %d %d" % tuple(map(int, r)) for r in rows], env)]


def run_scratch(exe, directory, sequences, env=None):
    """BdxScratchTurn over event sequences (call, copy, fail, plain, stream): per sequence, per event (memset, mine, other);
    memset None: the event begins no call."""
    return [[(None if a == "-" else int(a), int(b), int(c)) for a, b, c in (ev.split(":") for ev in ln.split())]
            for ln in _run_lines(exe, directory, "scratch", [" ".join(seq) for seq in sequences], env)]


def parse(stdout):
    reports, cur = {}, None
    for line in stdout.splitlines():
        key, _, rest = line.partition(" ")
        if key == "case":
            cur = reports[rest] = Report()
        elif key.endswith(".err") or key == "err":
            cur[key] = [rest]
        elif key != "call":  # ("call driver ok": the driver's last line)
            cur[key] = rest.split()
    return reports


# ---- the cases ----
CASES = []
SEQUENCES = []  # names of the cases with more than one call
# the one step where the parent's plan depended on the calls before it: (case, call) -> the single-call case on a
# fresh context whose golden value is asserted instead
FRESH_INSTEAD = {}


def case(name, pred, calls, base="headline", **kw):
    CASES.append(CallCase(name, pred, calls, base=base, **kw))
    if len(CASES[-1].calls) > 1:
        SEQUENCES.append(name)


N = 1 << 20  # a batch large enough for every tile to grow (n_cu = 256: r_cap 256 needs 2^18 reads, 32-read wave tiles 2^17)

# -- n_reads --
case("n1", lambda r: r.fused()["r_cap"] == 16 and r.tiles("wfront")["rw"] == 8 and r.plan()["front"] == "wave", call(1, 150))
for cu in (2, 7, 256):
    # fused kernel (size_bitpar): r_cap halves while n / r_cap < 4 n_cu, from 256 down to 16
    for cap in (256, 128, 64, 32):
        t = 4 * cu * cap
        case("rcap%d_cu%d_below" % (cap, cu), lambda r, cap=cap: r.fused()["r_cap"] == cap // 2, call(t - 1, 150), tune=dict(n_cu=cu))
        case("rcap%d_cu%d_at" % (cap, cu), lambda r, cap=cap: r.fused()["r_cap"] == cap, call(t, 150), tune=dict(n_cu=cu))
    # wave kernel (size_wave): a tile of rw > 8 reads only once n / rw >= 16 n_cu
    for rw in (32, 16):
        t = 16 * cu * rw
        case("rw%d_cu%d_below" % (rw, cu), lambda r, rw=rw: r.tiles("wfront")["rw"] == rw // 2, call(t - 1, 150), tune=dict(n_cu=cu))
        case("rw%d_cu%d_at" % (rw, cu), lambda r, rw=rw: r.tiles("wfront")["rw"] == rw, call(t, 150), tune=dict(n_cu=cu))
# carried passes: n_reads < 2^30
case("carry_below_2p30", lambda r: r.plan()["carry"] == 1 and r.plan()["front"] == "wave_end" and r.plan()["middle"] == "end", call((1 << 30) - 1, 150),
     base="smoke_dual_trim53")
case("carry_at_2p30", lambda r: r.plan()["carry"] == 0 and r.plan()["front"] == "wave_end" and r.plan()["middle"] == "end", call(1 << 30, 150),
     base="smoke_dual_trim53")
case("n_fffffff0", lambda r: r.i("c0.rc") == 0 and r.plan()["front"] == "wave", call(0xFFFFFFF0, 150))
case("n_fffffff1_refused", lambda r: r.i("c0.rc") == -1 and r["c0.err"] == ["more than 2^32 reads in one batch"], call(0xFFFFFFF1, 150))

# -- read length --
case("len0", lambda r: r.plan()["batch_len"] == 0 and r.fused()["seed_span"] >= 1 and r.tiles("wfront")["read_len_hint"] == 1, call(N, 0))
case("len_minus1", lambda r: r.plan()["batch_len"] == -1 and r.tiles("wfront")["read_len_hint"] == 1, call(N, -1))
case("len0_tiered_config", lambda r: r.plan()["tier_len"] == 0 and r.plan()["front"] == "none", call(N, 0), base="smoke_tiered_trim5")
D = "diag_with_alt"  # the two-intact-pieces index with weak single seeds kept beside it (untiered)
case("diag_nw_152", lambda r: r.fused()["diag_nw"] == 5 and r.fused()["seed_span"] == 152 and r.seed()[0] == 0, call(N, 152), base=D, tune=dict(no_wave=1))
case("diag_nw_153", lambda r: r.fused()["diag_nw"] == 10 and r.fused()["seed_span"] == 153 and r.seed()[0] == 0, call(N, 153), base=D, tune=dict(no_wave=1))
case("demote_312", lambda r: r.seed()[0] == 0 and r.path() == "qgram2+bitpar+verify", call(N, 312), base=D, tune=dict(no_wave=1))
case("demote_313", lambda r: r.seed()[0] == 1 and r.path() == "qgram+bitpar+verify" and r.fused()["diag_nw"] == 0, call(N, 313), base=D, tune=dict(no_wave=1))
# a contiguous wave tile's 10 KiB: rw x len + 64 <= 10240
# (at full residency the planner prefers 16-read tiles well before 318 bases: the 32-read tile is forced to show its own bound)
case("tile32_318", lambda r: r.tiles("wfront")["rw"] == 32 and r.tiles("wfront")["span_cap"] == 10240, call(N, 318), tune=dict(wave_rw=32))
case("tile32_319", lambda r: r.plan()["front"] == "none", call(N, 319), tune=dict(wave_rw=32))
case("tile8_1272", lambda r: r.tiles("wfront")["rw"] == 8 and r.tiles("wfront")["span_cap"] == 10240, call(N, 1272))
case("tile8_1273", lambda r: r.plan()["front"] == "none" and r.path() == "qgram+bitpar+verify", call(N, 1273))
# the pairs mode's span: 16 x slot + 16 <= 6 KiB + 16, slot = (len + 30) & ~15: 384 positions up to 369 bases
case("pairs_span_369", lambda r: r.plan()["middle"] == "list" and r.tiles("wmid")["slot"] == 384, call(N, 369), base="pairs_kb4")
case("pairs_span_370", lambda r: r.plan()["middle"] == "none", call(N, 370), base="pairs_kb4")
# (reads that long are staged as window slots or not at all: a 60-column window)
DW = dict(base="short10_rate02", passes=[PC.one_pass(PC.barcodes(96, 10, 12), ref=(1, 60, 0, 0))], tune=dict(no_known=1, no_seed=1))
case("dense_w_60000", lambda r: r.plan()["dense_w"] == 1 and r.plan()["split"] == 1 and r.fused()["slot_bytes"] > 0, call(N, 60000), **DW)
case("dense_w_60001", lambda r: r.plan()["dense_w"] == 0 and r.plan()["split"] == 1 and r.fused()["slot_bytes"] > 0, call(N, 60001), **DW)
case("below_pair_mmin", lambda r: r.tiles("wmid")["cpr"] == 1 and r.plan()["middle"] == "list", call(N, 20), base="pairs_kb4")
case("at_pair_mmin", lambda r: r.tiles("wmid")["cpr"] == 2 and r.plan()["middle"] == "list", call(N, 24), base="pairs_kb4")
# window mode: the ref_search_range window at most half the read
case("win_half", lambda r: r.plan()["front"] == "wave_win" and r.tiles("wfront")["slot"] == 80, call(N, 120), base="ranged")
case("win_half_plus1", lambda r: r.plan()["front"] == "wave" and r.tiles("wfront")["winm"] == 0, call(N, 120),
     passes=[PC.one_pass(PC.B96, ref=(1, 61, 0, 0))])
L28 = 1 << 28
case("win_start_minus_2p28", lambda r: r.plan()["front"] == "wave_win", call(N, 150), passes=[PC.one_pass(PC.B96, ref=(-L28, 60, 0, 0))])
case("win_start_beyond_minus_2p28", lambda r: r.plan()["front"] == "wave", call(N, 150), passes=[PC.one_pass(PC.B96, ref=(-L28 - 1, 60, 0, 0))])
case("win_end_plus_2p28", lambda r: r.plan()["front"] == "wave_win", call(N, 150), passes=[PC.one_pass(PC.B96, ref=(-59, L28, 1, 1))])
case("win_end_beyond_2p28", lambda r: r.plan()["front"] == "wave", call(N, 150), passes=[PC.one_pass(PC.B96, ref=(-59, L28 + 1, 1, 1))])
# slot staging of the fused kernel: 2 wmax + 96 <= len (wmax 60: the window of `ranged`)
case("slot_216", lambda r: r.fused()["slot_bytes"] > 0 and r.fused()["seed_span"] == 60 and r.plan()["front"] == "none", call(N, 216), base="ranged",
     tune=dict(no_wave=1))
case("slot_215", lambda r: r.fused()["slot_bytes"] == 0 and r.fused()["seed_span"] == 215, call(N, 215), base="ranged", tune=dict(no_wave=1))

# -- outputs wanted --
case("want_none", lambda r: r.plan()["front"] == "wave_end" and r.plan()["aln"] == 0 and r.plan()["short_lb0"] == 1, call(N, 150), base="smoke_tiered_trim5")
case("want_pass_start", lambda r: r.plan()["front"] == "wave_end" and r.plan()["aln"] == 1 and r.plan()["short_lb0"] == 0 and "wave(aln)" in r.path(),
     call(N, 150, wanted=PASS_START), base="smoke_tiered_trim5")
case("want_pass_end_trim3", lambda r: r.plan()["aln"] == 1 and "pairs(aln)" in r.path(), call(N, 150, wanted=PASS_END), base="smoke_trim3")
case("want_none_trim3", lambda r: r.plan()["aln"] == 0 and "wave(end)" in r.path(), call(N, 150), base="smoke_trim3")
case("want_stats", lambda r: r.plan()["aln"] == 1 and r.plan()["front"] == "wave_end", call(N, 150, stats=1), base="need_traceback")
case("want_pass_bc_dual", lambda r: r.plan()["carry"] == 0 and r.plan()["front"] == "wave_end", call(N, 150, wanted=PASS_BC), base="smoke_dual_trim53")
case("want_none_dual", lambda r: r.plan()["carry"] == 1, call(N, 150), base="smoke_dual_trim53")
case("exact_want_pass_end", lambda r: r.plan()["split"] == 1 and r.plan()["exact"] == "split", call(N, 150, wanted=PASS_END), base="exact")
case("exact_want_none", lambda r: r.plan()["split"] == 0 and r.plan()["front"] == "wave", call(N, 150), base="exact")

# -- switches --
case("sw_no_wave", lambda r: r.plan()["front"] == "none" and r.fused()["slot_bytes"] == 0, call(N, 150), tune=dict(no_wave=1))
case("sw_no_win", lambda r: r.plan()["front"] == "wave", call(N, 120), base="ranged", tune=dict(no_win=1))
case("sw_no_pairs", lambda r: r.plan()["middle"] == "none" and r.plan()["tier_len"] == 150, call(N, 150), base="pairs_kb4", tune=dict(no_pairs=1))
case("sw_pairs", lambda r: r.plan()["middle"] == "list" and r.plan()["tier_len"] == 150, call(N, 150), base="pairs_kb4")
case("sw_no_kend", lambda r: r.plan()["front"] != "wave_end" and r.plan()["split"] == 1, call(N, 150), base="no_kend")
case("sw_no_kaln", lambda r: r.plan()["aln"] == 0 and r.plan()["front"] != "wave_end", call(N, 150, wanted=PASS_START), base="no_kaln")
case("sw_no_carry", lambda r: r.plan()["carry"] == 0 and r.plan()["middle"] == "end", call(N, 150), base="smoke_dual_trim53", tune=dict(no_carry=1))
case("sw_no_dense", lambda r: r.plan()["dense_w"] == 0, call(N, 150), base="short10_rate02", tune=dict(no_known=1, no_seed=1, no_dense=1))
case("sw_dense", lambda r: r.plan()["dense_w"] == 1, call(N, 150), base="short10_rate02", tune=dict(no_known=1, no_seed=1))
case("sw_no_windows", lambda r: r.plan()["windows"] == 0 and r.plan()["front"] == "bitpar" and r.plan()["middle"] == "none", call(N, 150),
     base="smoke_tiered_trim5", tune=dict(no_windows=1))
case("sw_no_slot", lambda r: r.fused()["slot_bytes"] == 0 and r.fused()["seed_span"] == 216, call(N, 216), base="ranged", tune=dict(no_wave=1, no_slot=1))
case("sw_tier0_div1", lambda r: r.fused()["r_cap"] == 256, call(1 << 18, 150), base="pairs_kb4", tune=dict(tier0_div=1))
case("sw_tier0_div16", lambda r: r.fused()["r_cap"] == 16, call(1 << 18, 150), base="pairs_kb4")
case("sw_wave_rw16", lambda r: r.tiles("wfront")["rw"] == 16, call(N, 150), tune=dict(wave_rw=16))
case("sw_wave_waves4", lambda r: r.tiles("wfront")["waves"] == 4, call(N, 150), tune=dict(wave_waves=4))
case("sw_wave_maxres8", lambda r: r.tiles("wfront")["blocks"] * r.tiles("wfront")["waves"] == 8 * 256, call(N, 150), tune=dict(wave_maxres=8))
case("sw_wave_default", lambda r: r.tiles("wfront") == dict(r.tiles("wfront"), rw=32) and r.tiles("wfront")["blocks"] * r.tiles("wfront")["waves"] == 16 * 256,
     call(N, 150))
case("sw_bitpar_r32", lambda r: r.fused()["reads_per_block"] == 32, call(N, 150), tune=dict(no_wave=1, bitpar_r=32))
case("sw_bitpar_default", lambda r: r.fused()["reads_per_block"] > 32, call(N, 150), tune=dict(no_wave=1))
case("window_upload", lambda r: r.plan()["front"] == "none" and r.fused()["slot_bytes"] > 0 and r.fused()["seed_span"] == 150,
     call(N, 150, window_upload=1))
case("window_upload_tiered", lambda r: r.plan()["front"] == "bitpar" and r.plan()["middle"] == "none" and r.fused(0, "t1")["slot_bytes"] > 0,
     call(N, 150, window_upload=1), base="smoke_tiered_trim5")
# the other paths of the call, once each
case("c4_dual", lambda r: r.path() == "tier1:wave(end) > pairs(end) > qgram2+bitpar+verify" or r.plan()["middle"] == "end", call(N, 150), base="smoke_dual_trim53")
case("pairs_tier", lambda r: r.plan()["front"] == "pairs" and r.plan()["t1_exact"] == 1, call(N, 150), base="pairs_tier_demo2")
case("pairs_all", lambda r: r.plan()["middle"] == "all" and r.plan()["full"] == "none" and r.path() == "pairs(diag)+verify", call(N, 150),
     base="pairs_kb9_plain", tune=dict(no_tier=1))
case("wave_split_plain", lambda r: r.plan()["full"] == "wave_split" and r.path() == "wave+verify", call(N, 150), base="hamming")
case("generic_only", lambda r: r.i("c0.filtered") == 0, call(N, 150), base="filter_off")
case("words128", lambda r: r.fused()["reads_per_block"] <= 64, call(N, 150), base="words128")

# -- sequences on one context --
case("seq_long_then_short", lambda r: r.seed(0)[0] == 1 and r.seed(1)[0] == 1 and r.path(1) == "qgram+bitpar+verify", [call(N, 313), call(N, 150)], base=D,
     tune=dict(no_wave=1))
case("seq_short_then_long", lambda r: r.seed(0)[0] == 0 and r.path(0) == "qgram2+bitpar+verify" and r.seed(1)[0] == 1, [call(N, 150), call(N, 313)], base=D,
     tune=dict(no_wave=1))
case("seq_tiered_two_sizes", lambda r: r.fused(0)["r_cap"] == 256 and r.fused(1)["r_cap"] == 16 and r.plan(1)["tier_len"] == 150,
     [call(1 << 24, 150), call(2000, 150)], base="pairs_kb4")
# a split known-trim config without tiers: the known-end front stage puts the full-budget set into list mode (slot staging); the
# next call wants pass_start, has no front stage (no_kaln) and launches dense
KT = dict(passes=[PC.one_pass(PC.B96, trim=5)], tune=dict(no_kaln=1))
case("seq_kend_then_pass_start", lambda r: r.plan(0)["front"] == "wave_end" and r.fused(0)["slot_bytes"] > 0 and r.plan(1)["front"] == "none" and
     r.fused(1)["slot_bytes"] == 0, [call(N, 150), call(N, 150, wanted=PASS_START)], base=None, **KT)
case("kt_pass_start_fresh", lambda r: r.plan()["front"] == "none" and r.fused()["slot_bytes"] == 0, call(N, 150, wanted=PASS_START), base=None, **KT)
FRESH_INSTEAD[("seq_kend_then_pass_start", 1)] = "kt_pass_start_fresh"
