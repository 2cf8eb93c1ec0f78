"""Named configs for the create-time planner (csrc/bdx_plan.cpp): each case is a config, the developer switches it runs
under and a predicate over the planner's report that proves the case reaches the branch it is named for.  The stand-alone
driver tests/plan_host.cpp plans them on the CPU; test_plan_cpu.py asserts the predicates, compares every scalar, offset
and table digest with tests/golden/plan_tables.json, and runs the same driver under ASan / UBSan."""
import hashlib
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "biodemux.jl_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden", "plan_tables.json")
SEMIGLOBAL, HAMMING, EXACT = 0, 1, 2
AUTO, OFF, QGRAM, BITPAR = 0, 1, 2, 3
WHOLE = (1, 0, 0, 1)  # start_offset, end_offset, start_from_end, end_from_end: "1:end"


def barcodes(B, m, seed=1, letters="ACGT"):
    """B deterministic barcodes; m: one length or a list of lengths (cycled)."""
    rng = np.random.RandomState(seed)
    lens = [m] * B if isinstance(m, int) else [m[i % len(m)] for i in range(B)]
    return ["".join(letters[j] for j in rng.randint(0, len(letters), n)) for n in lens]


def one_pass(bcs, trim=0, window=0, win=(0, 0, 0, 0), ref=WHOLE, start=WHOLE, end=WHOLE):
    return dict(bcs=list(bcs), trim=trim, window=window, win=win, ranges=(ref, start, end))


class Case:
    def __init__(self, name, pred, passes, tune=None, golden=True, algorithm=SEMIGLOBAL, rate=0.1, min_delta=0.0, costs=(0, 1, 1), nindel=None,
                 summary=0, filter=AUTO):
        self.name, self.pred, self.passes, self.tune, self.golden = name, pred, passes, dict(tune or {}), golden
        self.cfg = (algorithm, int(len(passes) == 2), rate, min_delta, *costs, int(nindel is not None), nindel or 0, summary, filter)

    def text(self):
        a, dual, rate, delta, *rest = self.cfg
        out = ["case %s" % self.name, "cfg %d %d %s %s %s" % (a, dual, repr(float(rate)), repr(float(delta)), " ".join(map(str, rest)))]
        out += ["tune %s %s" % kv for kv in self.tune.items()]
        for p in self.passes:
            flat = [v for r in p["ranges"] for v in r]
            out.append("pass %d %d %s %s %d" % (p["trim"], p["window"], " ".join(map(str, p["win"])), " ".join(map(str, flat)), len(p["bcs"])))
            out += ["bc %s %d" % (b, len(b) - b.count("N")) for b in p["bcs"]]
        return "\n".join(out + ["end"]) + "\n"


class Report(dict):
    """One case of the driver's output: key -> list of tokens, plus .blobs: table -> (bytes, sha256)."""
    def i(self, key, at=0):
        return int(self[key][at])

    def f(self, key, at=0):
        return float.fromhex(self[key][at]) if self[key][at] not in ("inf", "-inf") else float(self[key][at])

    def s(self, key):
        return " ".join(self[key])

    def flat(self):  # what the golden file keeps: the driver prints a fixed set of keys, so all-zero values go without saying
        scalars = {k: " ".join(v) for k, v in sorted(self.items()) if any(t not in ("0", "0x0p+0") for t in v)}
        return dict(scalars=scalars, blobs={k: list(v) for k, v in sorted(self.blobs.items())})


def build_driver(directory, flags=("-O1",)):
    exe = os.path.join(str(directory), "plan_host")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-o", exe,
                           os.path.join(HERE, "plan_host.cpp"), os.path.join(CSRC, "bdx_plan.cpp")])
    return exe


def run_driver(exe, directory, cases=None, env=None):
    """Runs the cases through the driver; returns {name: Report}."""
    cases = CASES if cases is None else cases
    out_dir = os.path.join(str(directory), "blobs")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(str(directory), "cases.txt")
    with open(path, "w") as f:
        f.write("".join(c.text() for c in cases))
    out = subprocess.run([exe, path, out_dir], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "plan driver ok: %d cases" % len(cases) in out.stdout
    return parse(out.stdout, out_dir)


def parse(stdout, out_dir):
    reports, cur = {}, None
    for line in stdout.splitlines():
        key, _, rest = line.partition(" ")
        if key == "case":
            cur = reports[rest] = Report()
            cur.name, cur.blobs = rest, {}
        elif key == "blob":
            table, size = rest.split()
            with open(os.path.join(out_dir, "%s.%s.bin" % (cur.name, table)), "rb") as f:
                data = f.read()
            assert len(data) == int(size)
            cur.blobs[table] = (len(data), hashlib.sha256(data).hexdigest())
        elif key == "err":
            cur["err"] = [rest]
        elif key != "plan":  # ("plan driver ok": the driver's last line)
            cur[key] = rest.split()
    return reports


# ---- the cases ----
B96 = barcodes(96, 24, seed=20260515)
CASES = []


def case(name, pred, passes=None, **kw):
    CASES.append(Case(name, pred, passes if passes is not None else [one_pass(B96)], **kw))


def wave_known(r, s="fs0"):
    return r.i(s + ".wplan.enabled") == 1 and r.i(s + ".wplan.split") == 0


# headline and smoke shapes
case("headline", lambda r: wave_known(r) and r.i("fs0.wplan.q") == 8 and r.i("fs0.wplan.track_from") == 21 and r.i("top.tiered") == 0 and
     r.s("top.path") == "qgram+bitpar+verify")  # (track_from 21: the kernel ladder's TF = 20 instantiation)
case("smoke_tiered_trim5", lambda r: r.i("top.tiered") == 1 and r.i("top.pairs_tier") == 0 and r.i("fs0.pplan.enabled") == 1 and
     r.i("fs0.pplan_k.kend") == 1 and r.i("fs1.wplan_k.kend") == 1, rate=0.2, min_delta=0.1, passes=[one_pass(B96, trim=5)])
case("smoke_trim3", lambda r: r.i("fs1.wplan_k.kend") == 2 and r.i("fs0.pplan_k.kend") == 2, rate=0.2, passes=[one_pass(B96, trim=3)])
case("smoke_dual_trim53", lambda r: r.i("dev.is_dual") == 1 and r.i("fs1.wplan_k.kend") == 2 and r.i("fs1.wplan_k.cand_words") == 4 and
     r.i("dev.counts_stride2") == 16, rate=0.2, passes=[one_pass(barcodes(24, 24, 1), trim=5), one_pass(barcodes(16, 24, 2), trim=3)])
# pairs variants
case("pairs_tier_demo2", lambda r: r.i("top.pairs_tier") == 1 and r.i("top.tier_cap_fixed") in (3, 4) and r.i("fs1.pplan.pairs_kb") == 8 and
     r.i("fs0.pplan.pairs_kb") == 9, rate=0.25, min_delta=0.15, costs=(0, 1, 2))
case("pairs_kb9_plain", lambda r: r.i("fs0.pplan.pairs_kb") == 9 and r.i("fs0.pplan.pairs_spread") == 3 and r.i("top.pairs_tier") == 0,
     rate=0.25, costs=(0, 1, 2))  # (no min_delta: the full-budget set takes eight 3-base pieces, no pairs tier)
case("pairs_kb4", lambda r: r.i("fs0.pplan.pairs_kb") == 4 and r.i("fs0.pplan.split") == 0 and r.i("top.tiered") == 1, rate=0.2)
case("pairs_kb3", lambda r: r.i("fs0.pplan.pairs_kb") == 3 and r.i("fs0.pplan.enabled") == 1, rate=0.13)
case("pairs_nw4", lambda r: r.i("fs0.pplan.nw") == 4 and r.i("fs0.pplan.enabled") == 1, rate=0.2, tune=dict(pairs_nw=4))
# what a rejected tier attempt leaves behind in fs[1]
case("tier1_rejected_min_delta", lambda r: r.i("top.tiered") == 0 and r.i("fs1.bplan.enabled") == 1 and r.i("fs1.splan.enabled") == 1 and
     r.i("fs1.wplan.enabled") == 1 and "fs1.wave_tables" in r.blobs, rate=0.2, min_delta=0.3)
case("pairs_tier_rejected", lambda r: r.i("top.tiered") == 0 and r.i("top.tier_cap_fixed") == -1 and r.i("fs1.bplan.enabled") == 0 and
     r.i("fs1.bplan.tier_capped") == 1 and r.i("fs1.wplan.enabled") == 0, rate=0.25, min_delta=0.25, costs=(0, 1, 2))
# sweep word widths
case("words64", lambda r: r.i("fs0.bplan.word_bytes") == 8 and r.i("fs0.wplan.enabled") == 0 and r.i("plan.band_roll") == 1,
     passes=[one_pass(barcodes(48, 64, 7), trim=3)])
case("words128", lambda r: r.i("fs0.bplan.word_bytes") == 16 and r.i("fs0.bplan.enabled") == 1, passes=[one_pass(barcodes(24, 100, 8))])
case("long130_no_filter", lambda r: r.i("fs0.bplan.enabled") == 0 and r.s("top.path") == "generic", passes=[one_pass(barcodes(8, 130, 9))])
case("long160_band_roll_off", lambda r: r.i("top.band_roll_off") == 1 and r.i("plan.band_roll") == 0 and r.i("plan.dp_rows") == 161,
     passes=[one_pass(barcodes(8, 160, 9))])
case("long160_no_band_roll", lambda r: r.i("top.band_roll_off") == 0 and r.i("plan.band_roll") == 0, passes=[one_pass(barcodes(8, 160, 9))],
     tune=dict(no_band_roll=1))
case("too_long_700", lambda r: r.i("rc") == -1 and "barcodes too long for the on-chip DP columns: max length 700" in r.s("err"),
     passes=[one_pass(barcodes(2, 700, 9))])
# algorithms and scoring
case("hamming", lambda r: r.i("fs0.wplan.enabled") == 1 and r.i("fs0.wplan.split") == 1 and r.i("plan.reg_rows") == 0, algorithm=HAMMING)
case("exact", lambda r: r.i("fs0.bplan.known_ok", 0) == 1 and wave_known(r) and r.i("fs0.wplan_a.kend") == 3 and r.i("fs0.bplan.kb_uniform") == 0,
     algorithm=EXACT)
case("exact_no_known_exact", lambda r: r.i("fs0.bplan.known_ok", 0) == 0 and r.i("fs0.wplan.split") == 1 and r.i("fs0.wplan_a.enabled") == 0,
     algorithm=EXACT, tune=dict(no_known_exact=1))
B_N = [b[:5] + "N" + b[6:] if i % 8 == 0 else b for i, b in enumerate(B96)]
case("nscoring_with_N", lambda r: r.i("fs0.splan.n_always", 0) == 12 and r.i("fs0.bplan.ncode_N") != 255 and r.i("top.tiered") == 0 and
     r.i("fs0.wplan.enabled") == 0, passes=[one_pass(B_N)], rate=0.2, nindel=1)
case("nscoring_without_N", lambda r: r.i("fs0.bplan.ncode_N") == 255 and r.i("top.tiered") == 1 and r.i("fs0.wplan.enabled") == 0 and
     r.i("dev.has_nindel") == 1, rate=0.2, nindel=1)
# alphabet
case("non_acgt_letter", lambda r: r.i("fs0.bplan.ncodes") == 6 and r.i("fs0.bplan.enabled") == 1 and r.i("fs0.wplan.enabled") == 0 and
     r.i("fs0.pplan.enabled") == 0 and r.i("fs0.splan.enabled") == 1, passes=[one_pass(["R" + B96[0][1:]] + B96[1:])])
case("alphabet16", lambda r: r.i("fs0.bplan.enabled") == 0 and r.i("top.filter_used") == OFF,
     passes=[one_pass(barcodes(24, 24, 3, letters="ACGTRYSWKMBDHVNU"))])
# seeding
case("diag_with_alt", lambda r: r.i("fs0.splan.diag") == 1 and r.i("fs0.splan_alt.enabled") == 1 and r.i("top.tiered") == 0 and
     r.s("top.path") == "qgram2+bitpar+verify" and r.i("fs0.splan_alt.q") == 6, rate=0.13, tune=dict(no_tier=1))
case("diag_min_b_above", lambda r: r.i("fs0.splan.diag") == 0, rate=0.2, passes=[one_pass(barcodes(40, 24, 4))], tune=dict(no_tier=1))
case("diag_min_b_below", lambda r: r.i("fs0.splan.diag") == 1, rate=0.2, passes=[one_pass(barcodes(40, 24, 4))], tune=dict(no_tier=1, diag_min_b=40))
case("no_seed", lambda r: r.i("fs0.splan.enabled") == 0 and r.s("top.path") == "bitpar+verify" and r.i("top.filter_used") == BITPAR, tune=dict(no_seed=1))
case("no_diag", lambda r: r.i("fs0.splan.diag") == 0 and r.i("fs0.splan.enabled") == 1 and r.i("fs0.splan.q") == 6, rate=0.13, tune=dict(no_diag=1, no_tier=1))
case("no_wave", lambda r: r.i("fs0.wplan.enabled") == 0 and r.i("fs0.pplan.enabled") == 0 and r.i("fs0.splan.q") == 8, tune=dict(no_wave=1))
case("no_known", lambda r: r.i("fs0.bplan.known_ok", 0) == 0 and r.i("fs0.wplan.split") == 1 and r.i("fs0.wplan_k.enabled") == 0, tune=dict(no_known=1))
case("no_kend", lambda r: r.i("fs1.wplan.enabled") == 1 and r.i("fs1.wplan_k.enabled") == 0 and r.i("fs1.wplan_a.enabled") == 0, rate=0.2,
     passes=[one_pass(B96, trim=5)], tune=dict(no_kend=1))
case("no_kaln", lambda r: r.i("fs1.wplan_k.kend") == 1 and r.i("fs1.wplan_a.enabled") == 0 and r.i("fs0.pplan_a.enabled") == 0, rate=0.2,
     passes=[one_pass(B96, trim=5)], tune=dict(no_kaln=1))
case("no_pairs", lambda r: r.i("fs0.pplan.enabled") == 0 and r.i("top.tiered") == 1, rate=0.2, tune=dict(no_pairs=1))
case("tier_q7_m14", lambda r: r.i("top.tier_q") == 7 and r.i("top.tiered") == 1 and r.i("fs1.bplan.kb_uniform") == 1, rate=0.2,
     passes=[one_pass(barcodes(96, 14, 5))])
case("tier_q6_m12", lambda r: r.i("top.tier_q") == 6 and r.i("top.tiered") == 1 and r.i("fs1.bplan.kb_uniform") == 1, rate=0.2,
     passes=[one_pass(barcodes(96, 12, 5))])
case("tier_q_forced6", lambda r: r.i("top.tier_q") == 6 and r.i("fs1.bplan.kb_uniform") == 3, rate=0.2, tune=dict(tier_q=6))
case("seed_bm_log2_6", lambda r: r.i("fs0.splan.bm_log2") == 6 and r.i("fs0.splan.bm_words") == 2 and r.i("fs0.splan.off.single", 3) % 16 == 8,
     tune=dict(seed_bm_log2=6, no_wave=1))  # (an 8-byte bitmap: the `always` lists follow sizes rounded to 16, not offsets)
case("seed_hash_l2", lambda r: r.i("fs0.splan.hash_in_lds") == 0 and r.i("fs0.splan.enabled") == 1, tune=dict(seed_hash_l2=1))
# barcode counts
case("b129_pair_groups", lambda r: r.i("fs0.pplan.groups") == 2 and r.i("fs0.pplan.nw") == 4 and r.i("fs0.bplan.bpad", 0) == 256, rate=0.2,
     passes=[one_pass(barcodes(129, 24, 6))])
case("b129_split_no_pairs", lambda r: r.i("fs0.pplan.enabled") == 0 and r.i("fs0.bplan.known_ok", 0) == 0, rate=0.2,
     passes=[one_pass(barcodes(129, 24, 6), trim=5)])
case("b192", lambda r: wave_known(r) and r.i("fs0.wplan.n_barcodes") == 192 and r.i("dev.pass0.cand_words") == 6, passes=[one_pass(barcodes(192, 24, 6))])
case("b513_no_pairs", lambda r: r.i("fs0.pplan.enabled") == 0 and r.i("fs0.bplan.enabled") == 1 and r.i("top.tiered") == 1, rate=0.2,
     passes=[one_pass(barcodes(513, 24, 6))])
case("b513_split_no_wave", lambda r: r.i("fs0.wplan.enabled") == 0 and r.i("fs0.splan.enabled") == 1 and r.i("fs0.splan.q") == 8,
     passes=[one_pass(barcodes(513, 24, 6), trim=5)], tune=dict(wave_chance=100))  # (17 candidate words: beyond split mode's 16)
case("b1025_no_wave", lambda r: r.i("fs0.wplan.enabled") == 0 and r.i("fs0.splan.enabled") == 1 and r.i("fs0.bplan.bpad", 0) == 2048,
     passes=[one_pass(barcodes(1025, 24, 6))], tune=dict(wave_chance=100))
case("b1", lambda r: r.i("fs0.bplan.enabled") == 1 and r.i("fs0.splan.enabled") == 0 and r.i("dev.n_counts") == 5, passes=[one_pass(barcodes(1, 24, 6))])
# lengths
case("mixed_lengths", lambda r: r.i("fs0.bplan.kb_uniform", 0) == -1 and r.i("fs0.splan.q") < 8 and r.i("plan.uniform_len") == 0 and
     r.i("plan.reg_rows") == 32, passes=[one_pass(barcodes(96, [24, 21, 28, 14], 11))])
case("short10_rate02", lambda r: r.i("fs0.bplan.slot_cap") > 4 and r.i("fs0.bplan.dense_d") == 1 and r.i("plan.uniform_len") == 10, rate=0.2,
     passes=[one_pass(barcodes(96, 10, 12))])
case("short10_no_dense", lambda r: r.i("fs0.bplan.slot_cap") > 4 and r.i("fs0.bplan.dense_d") == 0, rate=0.2, passes=[one_pass(barcodes(96, 10, 12))],
     tune=dict(no_dense=1))
# rates
# (no barcode can be recorded: no pieces, so no wave table carries the budget field 255; the diagonal plan's meta words are all 0,
# and tier 1's sweep tables stay behind although nothing is tiered)
case("negative_rate", lambda r: r.i("fs0.bplan.enabled") == 1 and r.i("fs0.bplan.kb_uniform", 0) == -1 and r.i("fs0.splan.diag") == 1 and
     r.i("fs0.splan.diag_kmax") == 0 and r.i("fs0.wplan.enabled") == 0 and r.i("top.tiered") == 0 and r.i("fs1.bplan.enabled") == 1, rate=-0.1)
case("rate0", lambda r: r.i("fs0.bplan.kb_uniform", 0) == 0 and wave_known(r) and r.i("fs0.wplan.track_from") == 23, rate=0.0)
# ranges and windows
case("ranged", lambda r: r.i("fs0.wplan.ranged") == 1 and wave_known(r), passes=[one_pass(B96, ref=(1, 60, 0, 0))])
case("ranged_hamming_refused", lambda r: r.i("fs0.wplan.enabled") == 0 and r.i("fs0.splan.enabled") == 1, algorithm=HAMMING,
     passes=[one_pass(B96, ref=(1, 60, 0, 0))])
case("binding_start_range", lambda r: r.i("fs0.wplan.enabled") == 0 and r.i("plan.clean") == 0 and r.i("fs0.splan.enabled") == 1,
     passes=[one_pass(B96, start=(5, 0, 0, 1))])
case("explicit_window", lambda r: r.i("dev.pass0.explicit_window") == 1 and r.i("fs0.wplan.enabled") == 0 and r.i("top.tiered") == 0 and
     r.i("fs0.bplan.known_ok", 0) == 1, rate=0.2, passes=[one_pass(B96, window=1, win=(10, 80, 70, 20))])
case("window_align_one", lambda r: r.i("dev.pass0.explicit_window") == 2 and r.i("fs0.bplan.known_ok", 0) == 0,
     passes=[one_pass(B96, window=2, win=(10, 33, 10, 33))])
# other
case("need_traceback", lambda r: r.i("dev.any_traceback") == 1 and r.i("fs0.wplan.split") == 1 and r.i("fs0.wplan_k.enabled") == 0 and
     r.i("fs0.wplan_a.kend") == 3, summary=1)
case("lds_dp", lambda r: r.i("plan.reg_rows") == 0 and r.i("plan.dp_rows") == 25 and r.i("dev.force_lds_dp") == 1, tune=dict(lds_dp=1))
case("no_clean", lambda r: r.i("plan.reg_rows") == 24 and r.i("plan.clean") == 0, tune=dict(no_clean=1))
case("filter_off", lambda r: r.i("fs0.bplan.enabled") == 0 and r.s("top.path") == "generic", filter=OFF)
case("filter_bitpar", lambda r: r.i("fs0.bplan.enabled") == 1 and r.i("fs0.splan.enabled") == 0 and r.i("fs0.pplan.enabled") == 0 and
     r.i("top.tiered") == 0, rate=0.2, filter=BITPAR)
case("n_cu_64", lambda r: r.i("plan.n_cu") == 64, tune=dict(n_cu=64))
# the create-time refusals
case("counts_too_large", lambda r: r.i("rc") == -1 and r.s("err") == "sample_counts table too large (268960004 entries)",
     passes=[one_pass(barcodes(16400, 4, 13)), one_pass(barcodes(16400, 4, 14))])
# (bdx_create's validation bounds |rate| at 1e4 and lengths at 8192, so this refusal is the planner's own guard: no golden entry)
case("rate_times_length", lambda r: r.i("rc") == -1 and r.s("err") == "max_error_rate * barcode length exceeds the supported range", rate=1.0e7,
     golden=False)
