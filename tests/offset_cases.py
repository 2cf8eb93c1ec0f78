"""Builders for the read-offset tests (no GPU): batches whose offsets do not start at 0 and cross 2^31 and 2^32, and batches
whose first and last read lie in hostile surroundings.

Every classify kernel turns seq_off[i] into an address (include/biodemux_hip.h: "seq_off[0] may be non-zero").  The tests
place a lattice recipe's batch (kernel_lattice.py) at a base b inside one large allocation: the kernels get a byte pointer O
and the offsets off + b.  An offset whose low 32 bits were zero-extended would address O + ((off + b) mod 2^32), one that was
sign-extended O + sext32(off + b): alias_runs() names these ranges, which all lie inside the same allocation, and decoy()
builds the batch that is written there — the same offsets, other reads — so that a truncated offset yields a wrong verdict and
never a fault.  hostile() builds batches whose first read begins with a barcode cut at the front and whose last read ends
with one cut at the back, the missing bases lying just outside the batch among back-to-back copies of another barcode: a
16-byte granule mask that is off by one at either end of a batch then finds a match the oracle does not.

SITES names one recipe per place where a kernel fetches read bytes; test_offset_cases_cpu.py holds each against the planner
(tests/call_host.cpp), test_offset_base_gpu.py runs them.  Not a conftest."""
import copy
import functools

import numpy as np

import kernel_lattice as KL

P31, P32 = 1 << 31, 1 << 32
ARENA_BYTES = P31 + P32 + (16 << 20)  # [origin - 2^31, origin + 2^32 + 16 MiB): every alias of every base below lies inside
ARENA_MIN_FREE = 8 << 30  # device memory the arena's module asks for before it allocates
SURROUND = 4096  # bytes of back-to-back barcode copies on either side of a hostile batch
PLANT_CUTS = (1, 3)  # bases a planted end misses inside the batch (they lie just outside it)

HEADLINE = "bdx_wave_kernel<32, 20, 5, 8, false, 0, 0, false, 0, false, false>"
ALONE_M1 = "alone_match_minus1"
# fetch site -> the recipe that reaches it (a kernel_lattice.recipe name, a PAIRS_EXTRAS key, or ALONE_M1), and what reads the
# bytes there.  The wave kernel's tiles are scattered in the pairs mode and in window mode (SCAT, bdx_wave_kernel.h)
SITES = {
    "wave_contiguous": (HEADLINE, "geometry() / load_bytes of a contiguous tile, known-score (bdx_wave_kernel.h)"),
    "wave_split": ("bdx_wave_kernel<32, 20, 5, 8, true, 0, 0, false, 0, false, false>",
                   "the split form: contiguous tiles, candidate windows handed to the exact kernel"),
    "wave_scattered": ("kb8_all", "load_scat / scat_geo over the whole batch, no list in front (Middle::all)"),
    "wave_carry": ("dual_kend1_delta0.0", "load_scat with carried passes: the offset index is id & idmask"),
    "window": ("bdx_wave_kernel<32, 12, 3, 8, false, 0, 0, false, 0, true, true>", "window mode: scat_geo adds the window's first column (wlo)"),
    "pairs_list": ("bdx_wave_kernel<16, 12, 3, 4, false, 4, 2, false, 0, true, false>", "the pairs mode over tier 1's list (load_scat through idmap)"),
    "fused_dense": ("bdx_bitpar_kernel<256, 64, true, false, 5, 0>", "span0 / ro of the fused filter's dense form (bdx_bitpar.hip)"),
    "fused_list": ("bdx_generic_kernel<256, 24, true, false>", "ro / rb of the fused filter's list form: per-read slots behind tier 1"),
    "exact_staged": ("bdx_generic_kernel<256, 32, true, false>", "the exact kernel's staged span, CLEAN register DP (bdx_device.hip)"),
    "exact_band": ("bdx_generic_kernel<256, 24, true, true>", "the exact kernel with the diagonal band"),
    "exact_roll": ("bdx_generic_kernel<128, 0, true, false>", "the exact kernel's rolling band on 128 lanes"),
    "exact_unstaged": ("bdx_generic_kernel<256, 0, false, false>", "Bytes<false>{a.seq + ro}: workgroups whose reads do not fit the stage (LDS columns)"),
    "exact_alone": ("bdx_generic_kernel<64, 0, false, false>", "the exact kernel with no filter in front (154-nt barcodes)"),
    "exact_alone_m1": (ALONE_M1, "the exact kernel with no filter in front (match = -1: no filter takes the costs)"),
}
SITE_OF = {name: site for site, (name, _) in SITES.items()}
NAMES = [name for name, _ in SITES.values()]
# the recipes that also run in hostile surroundings
HOSTILE_SITES = ("wave_contiguous", "wave_scattered", "window", "pairs_list", "fused_dense", "exact_staged")
HOSTILE_NAMES = [SITES[s][0] for s in HOSTILE_SITES]
BASE_LABELS = ("at_2p31", "in_2p31", "at_2p32", "in_2p32", "beyond_2p32", "small")
# the sixteen 16-byte phases of the byte pointer, dealt over the six bases: two or three alignments each
SHIFTS = {label: [s for s in range(16) if s % len(BASE_LABELS) == j] for j, label in enumerate(BASE_LABELS)}


def _alone_m1():
    """The exact kernel alone by its costs: match = -1 lies outside every filter's and the clean class's domain
    (plan_generic, bdx_plan.cpp: clean_costs), so a 24-nt set runs the plain register DP with no launch in front."""
    return KL.CellRecipe("bdx_generic_kernel<256, 24, false, false>", "b24", dict(max_error_rate=0.2, match=-1, mismatch=2, indel=3), 3 * 256 + 1, 1,
                         KL.EXACT_EDGE_LEN, KL.TEN + KL.INDEL, want_pass=True, end_why=KL.EXACT_END)


@functools.lru_cache(maxsize=None)
def get(name: str):
    """The recipe behind a name of SITES: None when kernel_lattice.py no longer has it."""
    if name == ALONE_M1:
        return _alone_m1()
    extra = [x for x in KL.PAIRS_EXTRAS if x.key == name]
    return extra[0] if extra else KL.recipe(name)


def target(name: str) -> str:
    """The instantiation the recipe is about."""
    return get(name).target


def hc_kwargs(name: str) -> dict:
    obj = get(name)
    return dict(filter=getattr(obj, "filter", "auto"), want_pass=obj.want_pass)


def hint(name: str):
    """The read length a window recipe is planned at (set_read_length_hint); None: the device measures the batch."""
    return getattr(get(name), "hint", None)


def tile_reads(name: str) -> int:
    """Reads per tile of a wave recipe (0: not a wave kernel's recipe)."""
    obj = get(name)
    if isinstance(obj, (KL.PairsRecipe, KL.PairsExtra)):
        return 16
    return getattr(obj, "rw", 0)


def driver_case(name: str, key: str, shapes=None):
    """The planner-driver case (tests/call_cases.py) of the recipe's two calls, main then edge, on one context."""
    import call_cases as CC
    import plan_cases as PC

    obj = get(name)
    if isinstance(obj, KL.PairsExtra):
        return obj.case(key)
    shapes = shapes or [(obj.n_main, obj.main_len), (obj.n_edge, obj.edge_len)]
    if isinstance(obj, KL.Recipe):
        kw = obj.form["kw"]
        tune = dict(n_cu=1, **({"wave_rw": int(obj.env["BDX_WAVE_RW"])} if "BDX_WAVE_RW" in obj.env else {}))
        return CC.CallCase(key, None, [CC.call(n, L, wanted=KL.WANT_ALL if obj.want_pass else KL.WANT_VERDICT) for n, L in shapes],
                           passes=[PC.one_pass(obj.barcodes(), trim=kw.get("trim_side") or 0)], rate=KL.RATE,
                           costs=(kw.get("match", 0), kw.get("mismatch", 1), kw.get("indel", 1)), tune=tune)
    return obj.case(key, shapes)


def exact_stage_bytes(bcs, threads: int = 256, dp_rows: int = 1) -> int:
    """plan_generic (bdx_plan.cpp) restated for a single-pass config with trace-back outside the rolling band: the bytes of
    reads a workgroup of `threads` lanes stages.  dp_rows: 1 for the register DP, the longest barcode + 1 for the LDS columns."""
    lds_max = 160 * 1024
    b, total = len(bcs), sum(len(x) for x in bcs)
    assert total <= 32 * 1024
    fixed = (2 * b + 2) * 4 + 16 + ((total + 15) & ~15) + 16 + min(4 + b, 2048) * 4 + 16
    need = fixed + dp_rows * 8 * threads
    assert need + 4096 <= lds_max
    budget = max(80 * 1024 - need, 0)
    if budget < threads * 192:
        budget = lds_max - need
    stage = min(budget, 64 * 1024) & ~15
    return stage if stage >= 1024 else 0


def workgroup_spans(off, threads: int = 256):
    """Bytes of the reads of every dense workgroup of the exact kernel (reads [b x threads, (b + 1) x threads))."""
    n = len(off) - 1
    return [int(off[min(r0 + threads, n)] - off[r0]) for r0 in range(0, n, threads)]


# ---- bases ----
def crossing_read(off) -> int:
    """A read in the middle of the batch with sixteen bases or more: the 2^31 / 2^32 boundary is put at its first base or inside it."""
    lens = np.diff(off)
    n = len(lens)
    return next(i for i in list(range(n // 2, n)) + list(range(n // 2)) if lens[i] >= 16)


def bases(off) -> dict:
    """label -> base b for the batch with offsets `off` (off[0] == 0): off[k] + b is exactly 2^31 / 2^32 for the read k in the
    middle (at_*), the boundary lies behind the seventh base of that read (in_*), every offset lies beyond 32 bits
    (beyond_2p32), a small odd base."""
    h = int(off[crossing_read(off)])
    return {"at_2p31": P31 - h, "in_2p31": P31 - h - 7, "at_2p32": P32 - h, "in_2p32": P32 - h - 7, "beyond_2p32": P32 + 16 * 5 + 3, "small": 5}


def alias_runs(b: int, total: int):
    """Where the bytes [b, b + total) would be looked for by an address whose offset went through 32 bits: a list of
    (a, lo, hi): byte lo + j of the batch (lo + j < hi) has the alias offset a + j, relative to the byte pointer, zero-extended
    or sign-extended; only aliases that differ from the true offset are listed.  All of them lie in [-2^31, 2^32)."""
    runs = set()
    for signed in (False, True):
        lo = 0
        while lo < total:
            t = (b + lo) & (P32 - 1)
            hi = min(total, lo + P32 - t)
            if signed and t < P31:
                hi = min(hi, lo + P31 - t)
            a = t - P32 if (signed and t >= P31) else t
            if a != b + lo:
                runs.add((a, lo, hi))
            lo = hi
    return sorted(runs)


# ---- decoys ----
def _rotated(obj):
    """The recipe with its barcode lists rotated by one: its generators plant barcode j + 1 wherever the recipe plants j."""
    rot = copy.copy(obj)
    inner = obj.barcodes
    rot.barcodes = lambda *a: (lambda b: b[1:] + b[:1])(list(inner(*a)))
    if hasattr(obj, "planted"):
        planted = obj.planted
        rot.planted = lambda: (lambda b: b[1:] + b[:1])(list(planted()))
    if hasattr(obj, "base"):
        rot.base = _rotated(obj.base)
    return rot


def fit_reads(src_seq, src_off, off):
    """The reads of (src_seq, src_off) laid under the offsets `off`, in turn: slot i takes a source read of its own length where
    one is left, else the next source read cut or repeated to the slot's length."""
    lens = np.diff(off)
    slens = np.diff(src_off)
    pools = {}
    for j, ln in enumerate(slens.tolist()):
        pools.setdefault(ln, []).append(j)
    out = np.empty(int(off[-1] - off[0]), dtype=np.uint8)
    for i, ln in enumerate(lens.tolist()):
        if ln == 0:
            continue
        pool = pools.get(ln)
        j = pool.pop() if pool else i % len(slens)
        out[off[i] - off[0]: off[i + 1] - off[0]] = np.resize(src_seq[src_off[j]:src_off[j + 1]], ln)
    return out


@functools.lru_cache(maxsize=None)
def _decoy_source(name: str):
    import fuzz
    import helpers as H

    obj = get(name)
    rseq, roff, _ = _rotated(obj).batch("main")
    pseq, poff, _keep = fuzz.permuted_batch(rseq, roff, seed=len(roff))
    # (only reads the oracle assigns: an edge batch's unassigned reads then differ from their decoys as well)
    hit = np.flatnonzero(H.orc.OracleClassifier(obj.config(), nthreads=8, want_pass=False).classify(pseq, poff)["bc1"] > 0)
    assert len(hit) >= 64, (name, len(hit))
    lens = np.diff(poff)[hit]
    off = np.zeros(len(hit) + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    return np.concatenate([pseq[poff[j]:poff[j + 1]] for j in hit]), off


def decoy(name: str, off):
    """The decoy of a batch of the recipe with the offsets `off` (the main batch's, the edge batch's or a hostile variant's): the
    main batch made again with the barcodes rotated by one, its reads permuted (fuzz.permuted_batch), those of them the oracle
    assigns laid under the same offsets."""
    pseq, poff = _decoy_source(name)
    return fit_reads(pseq, poff, off)


def verdicts_differ(a: dict, b: dict):
    """Per read: any of the four verdict vectors differs."""
    return np.any([a[k] != b[k] for k in ("bc1", "bc2", "keep_start", "keep_end")], axis=0)


# ---- hostile surroundings ----
HOSTILE_VARIANTS = ("full", "first_empty", "last_empty", "both_empty", "one_read", "tile", "tile_plus1")


def hostile_variants(name: str):
    return [v for v in HOSTILE_VARIANTS if not v.startswith("tile") or tile_reads(name)]


def _plain_barcodes(obj):
    return [b for b in (obj.planted() if hasattr(obj, "planted") else obj.barcodes()) if set(b) <= set("ACGT")]


def _window_ends(obj, n: int):
    """(head, tail): the read's first / last base lies inside the column window the config looks at."""
    if not hasattr(obj, "window"):
        return True, True
    first, last = obj.window(n)
    return first <= 1 <= last, first <= n <= last


def hostile(name: str, variant: str, c: int):
    """A batch of the recipe's main reads in hostile surroundings.  Returns (seq, off, before, after, plants):
    read 0 (random bases otherwise, as the last read) begins with barcode 1 of the set minus its first c bases and `before` (SURROUND bytes, to be placed in front of
    off[0]) ends with exactly those c bases; the last read ends with barcode 2 minus its last c bases and `after` begins with
    them; the rest of `before` and `after` are back-to-back copies of barcode 0.  Variants: full (every main read), first_empty /
    last_empty / both_empty (an empty read in front of read 0 / behind the last), one_read (read 0 alone, planted at both
    ends), tile / tile_plus1 (the first RW / RW + 1 reads).  plants: [(read index, "head" | "tail")], the ends the config's
    column window reaches."""
    obj = get(name)
    seq, off, _ = obj.batch("main")
    bcs = _plain_barcodes(obj)
    fill, b_head, b_tail = (np.frombuffer(b.encode(), dtype=np.uint8) for b in bcs[:3])
    n_all = len(off) - 1
    take = {"one_read": 1, "tile": tile_reads(name), "tile_plus1": tile_reads(name) + 1}.get(variant, n_all)
    reads = [seq[off[i]:off[i + 1]].copy() for i in range(take)]
    keep_h, keep_t = len(b_head) - c, len(b_tail) - c
    rng = np.random.default_rng(9000 + take + c)
    for i in {0, take - 1}:  # (the planted reads carry nothing but their plants)
        reads[i] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=len(reads[i]))].copy()
    assert len(reads[0]) >= keep_h + keep_t and len(reads[-1]) >= keep_t, (name, len(reads[0]))
    reads[0][:keep_h] = b_head[c:]
    reads[-1][len(reads[-1]) - keep_t:] = b_tail[:keep_t]
    first, last = 0, len(reads) - 1
    empty = np.zeros(0, dtype=np.uint8)
    if variant in ("first_empty", "both_empty"):
        reads.insert(0, empty)
        first, last = 1, last + 1
    if variant in ("last_empty", "both_empty"):
        reads.append(empty)
    out_off = np.zeros(len(reads) + 1, dtype=np.int64)
    out_off[1:] = np.cumsum([len(r) for r in reads])
    before = np.resize(fill, SURROUND).copy()
    before[SURROUND - c:] = b_head[:c]
    after = np.roll(np.resize(fill, SURROUND), c).copy()
    after[:c] = b_tail[keep_t:]
    head_in, _ = _window_ends(obj, len(reads[first]))
    _, tail_in = _window_ends(obj, len(reads[last]))
    plants = ([(first, "head")] if head_in else []) + ([(last, "tail")] if tail_in else [])
    return np.concatenate(reads).astype(np.uint8), out_off, before, after, plants


def plant_pair(seq, off, before, after, plant, c: int):
    """(the planted read alone, the read extended by the c bytes outside the batch) of one plant of hostile()."""
    i, end = plant
    alone = seq[off[i]:off[i + 1]]
    return alone, (np.concatenate([before[len(before) - c:], alone]) if end == "head" else np.concatenate([alone, after[:c]]))


# ---- the host entry's routes ----
def c2_config(**kw):
    """The C2 shape: 96 barcodes of 24 nt (the synthetic generator's own seed)."""
    from biodemux_jl_amd import DemuxConfig, synth

    bcs = synth.make_barcodes(96, 24, seed=synth.SEED)
    base = dict(bc_seqs=bcs, bc_lengths_no_N=[24] * 96, ids=[f"bc{i + 1}" for i in range(96)], max_error_rate=0.1)
    base.update(kw)
    return DemuxConfig(**base)


@functools.lru_cache(maxsize=None)
def plain_route_batch():
    """20 001 reads of 150 bases: above the 2 MiB of the staged route, far below the pipelined one."""
    from biodemux_jl_amd import synth

    seq, off, _ = synth.make_reads(synth.make_barcodes(96, 24, seed=synth.SEED), 20001, 150, seed=synth.SEED + 31)
    return seq, off


@functools.lru_cache(maxsize=None)
def window_route_case():
    """(config, seq, off): the first shape of test_window_upload_of_the_host_entry_point (test_gpu_parity.py): 1200 ragged reads
    of 1500..5000 bases with barcodes near both ends, a window of 200 columns, short and empty reads in between."""
    from biodemux_jl_amd import DemuxConfig, pack_reads, parse_dynamic_range, synth

    bcs = synth.make_barcodes(24, 20, seed=131, min_hamming=6)
    seq0, off0, _ = synth.make_ragged_reads(bcs, 1200, 1500, 5000, seed=131, plant_lo=0, plant_hi=None)
    rng = np.random.Generator(np.random.PCG64(132))
    reads = []
    for i in range(1200):
        r = seq0[off0[i]:off0[i + 1]].copy()
        b = np.frombuffer(bcs[int(rng.integers(0, 24))].encode(), dtype=np.uint8)
        for pos in (int(rng.integers(0, 170)), len(r) - 200 + int(rng.integers(0, 175))):
            r[pos:pos + 20] = b
        reads.append(r.tobytes().decode())
    for i in range(0, 1200, 97):
        reads[i] = reads[i][:int(rng.integers(0, 260))]
    reads[5] = ""
    seq, off = pack_reads(reads)
    cfg = DemuxConfig(bc_seqs=bcs, bc_lengths_no_N=[20] * 24, ids=[f"bc{i + 1}" for i in range(24)], max_error_rate=0.15, summary=True,
                      ref_search_range=parse_dynamic_range("1:200"))
    return cfg, seq, off
