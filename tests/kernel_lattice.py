"""The classify kernels of the built library, one template instantiation at a time: the code-object reader (shared with
test_geometry_fuzz_gpu.py), a parser from a kernel name to its named template arguments, the planner's selection rules
restated in Python, and recipe(name): a deterministic case whose whole-batch launch runs exactly that instantiation.
The wave kernel's single-pass whole-range recipes (Recipe) follow the restated rules; the fused filter's and the exact
kernel's (CellRecipe), window mode's (WinRecipe), the general forms' (GenRecipe) and the pairs mode's (PairsRecipe, with
further argument states and entry routes in PAIRS_EXTRAS) state their cells as numbers, which the planner itself confirms
through tests/call_host.cpp: wave_name / pairs_name spell the instantiation from its launch lines.

Imported by test_kernel_lattice_cpu.py (bookkeeping: every instantiation is accounted for, every recipe's target follows
from the rules) and test_kernel_lattice_gpu.py (every recipe runs on the device against the oracle).  Not a conftest."""
import functools
import math
import re
import struct

from biodemux_jl_amd import hipabi


def _demangle(sym: str) -> str:
    """Itanium names of this library's kernels -> "name<a, b, ...>" (integer and bool template arguments, the spelling of
    bdx_last_launches); anything else comes back as it is."""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)|_Z(\d+)", sym)
    if not m:
        return sym
    n = int(m.group(1) or m.group(2))
    name = sym[m.end():m.end() + n]
    rest = sym[m.end() + n:]
    if not rest.startswith("I"):
        return name
    args = []
    for t, neg, v in re.findall(r"L([ibj])(n?)(\d+)E", rest[1:rest.index("EE") + 1] if "EE" in rest else rest[1:]):
        args.append(("true" if v == "1" else "false") if t == "b" else ("-" if neg else "") + v)
    return f"{name}<{', '.join(args)}>"


@functools.lru_cache(maxsize=1)
def code_object_kernels() -> frozenset:
    """Every kernel of the gfx950 code objects in the built library: its .hip_fatbin section holds one offload bundle per
    translation unit (what tools/kernel_regs.sh unbundles object by object); the kernels are the ELF symbols with a
    kernel descriptor (NAME.kd)."""
    data = open(hipabi.LIB_PATH, "rb").read()
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + k * shentsize) for k in range(shnum)]
    names_off = secs[shstrndx][4]

    def sec_name(s):
        return data[names_off + s[0]: data.index(b"\0", names_off + s[0])].decode()

    fat = [s for s in secs if sec_name(s) == ".hip_fatbin"]
    assert len(fat) == 1, "no .hip_fatbin section in the library"
    fat = data[fat[0][4]: fat[0][4] + fat[0][5]]
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    kernels = set()
    pos = fat.find(magic)
    n_objects = 0
    while pos >= 0:
        n_entries, = struct.unpack_from("<Q", fat, pos + 24)
        p = pos + 32
        for _ in range(n_entries):
            off, size, tlen = struct.unpack_from("<QQQ", fat, p)
            triple = fat[p + 24: p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" not in triple:
                continue
            co = fat[pos + off: pos + off + size]
            assert co[:4] == b"\x7fELF", f"code object for {triple} is not an ELF (compressed bundle?)"
            n_objects += 1
            c_shoff, = struct.unpack_from("<Q", co, 0x28)
            c_entsize, c_num = struct.unpack_from("<HH", co, 0x3A)
            csecs = [struct.unpack_from("<IIQQQQIIQQ", co, c_shoff + k * c_entsize) for k in range(c_num)]
            for s in csecs:
                if s[1] not in (2, 11):  # SHT_SYMTAB, SHT_DYNSYM
                    continue
                so = csecs[s[6]][4]
                for j in range(s[5] // 24):
                    st_name, = struct.unpack_from("<I", co, s[4] + j * 24)
                    nm = co[so + st_name: co.index(b"\0", so + st_name)].decode()
                    if nm.endswith(".kd"):
                        kernels.add(_demangle(nm[:-3]))
        pos = fat.find(magic, pos + len(magic))
    assert n_objects >= 6 and kernels, (n_objects, len(kernels))
    return frozenset(kernels)


# ---- instantiation names ----
# the template parameters of the three classify families, in order (bdx_wave_kernel.h, bdx_bitpar.hip, bdx_device.hip)
PARAMS = {
    "bdx_wave_kernel": ("RW", "TF", "NV", "Q", "SPLIT", "KB", "NW", "MG", "KEND", "GEN", "WINM"),
    "bdx_bitpar_kernel": ("BS", "R", "SEED", "DIAG", "NW", "WL"),
    "bdx_generic_kernel": ("BS", "REGM", "CLEAN", "UM"),
}


def parse(name: str):
    """"bdx_wave_kernel<32, 20, 5, 8, false, ...>" -> ("bdx_wave_kernel", {"RW": 32, "TF": 20, ..., "SPLIT": False, ...});
    None for a kernel outside the classify families."""
    m = re.fullmatch(r"(\w+)<(.*)>", name)
    if not m or m.group(1) not in PARAMS:
        return None
    vals = [v.strip() for v in m.group(2).split(",")]
    names = PARAMS[m.group(1)]
    assert len(vals) == len(names), f"{name}: {len(vals)} template arguments, expected {len(names)}"
    return m.group(1), {k: (v == "true") if v in ("true", "false") else int(v) for k, v in zip(names, vals)}


def spell(family: str, args: dict) -> str:
    """parse() undone: the name bdx_last_launches and the code object use."""
    return f"{family}<{', '.join(('true' if v else 'false') if isinstance(v, bool) else str(v) for v in (args[k] for k in PARAMS[family]))}>"


def classify_kernels() -> list:
    """Every instantiation of the three classify families in the built library's gfx950 code objects."""
    return sorted(k for k in code_object_kernels() if parse(k) is not None)


# ---- the wave planner, restated (bdx_plan.cpp: build_seed_tables, build_wave_tables; bdx_call.cpp: size_wave; bdx_wave_kernel.h: the
# dispatch ladder seeded_ladder; bdx_wave.hip: bdx_wave_table_bytes, bdx_wave_area_bytes) ----
LDS_MAX = 160 * 1024  # bdx_internal.h BDX_LDS_MAX


def wave_seed_plan(ms, rate: float) -> dict:
    """Seed and sweep parameters of a single-set, unit-cost or weighted (cost >= 1) config of barcodes `ms` (lengths) at
    `rate`, outside any tier: kb = floor(rate * m) (build_seed_tables / build_wave_tables, cmin = 1); Q = the shortest
    piece floor(m / (kb + 1)), capped at 8 (build_seed_tables); track = min (m - kb - 1), clamped to 0..28
    (build_wave_tables: wp.track_from); TF = 20 / 12 / 0 as the dispatch ladder (seeded_tfq) picks it from Q and track;
    chance = 150 x pieces / 4^Q (build_wave_tables: at most 6 outside a tier); expected = chance + 1 (build_seed_tables'
    selectivity, no barcode without seeds)."""
    kbs = [int(rate * m) for m in ms]
    q = min(8, min(m // (kb + 1) for m, kb in zip(ms, kbs)))
    pieces = sum(kb + 1 for kb in kbs)
    track = max(0, min(28, min(m - kb - 1 for m, kb in zip(ms, kbs))))
    if q == 8:
        tf = 20 if track >= 20 else 12 if track >= 12 else 0
    elif q == 7:
        tf = 12 if track >= 12 else 0
    else:
        tf = 0
    chance = 150.0 * pieces / 4.0 ** q
    return dict(kbs=kbs, q=q, tf=tf, track=track, pieces=pieces, chance=chance, expected=chance + 1.0, n_bc=len(ms))


def wave_table_bytes(sp: dict, kend: int) -> int:
    """bdx_wave_table_bytes of a non-pairs plan: seed bitmap, rank words, entries (one per piece), peq rows (stride 9), the
    reversed rows of a KEND >= 2 plan, meta + settle words, the LDS histogram (4 + B counters: bdx_plan.cpp n_counts)."""
    al = lambda x: (x + 31) & ~31  # noqa: E731
    bm = (1 << (2 * sp["q"])) // 8
    b = sp["n_bc"]
    return al(bm) + al(bm // 2) + al(sp["pieces"] * 4) + al(b * 36) + al(b * 36 if kend >= 2 else 0) + 2 * al(b * 4) + al((4 + b) * 4)


def wave_area_bytes(rw: int, span: int, hq: int, sq: int, cand_words: int) -> int:
    """bdx_wave_area_bytes of a contiguous-tile (not pairs, not window-mode) plan."""
    nvec = span >> 4
    fixed = ((rw + 1) * 4 + 15) // 16 * 16 + 2 * rw * 8 * 4 + rw * 16 + 3 * rw * 4 + 256
    o = fixed + ((nvec + 2 + 3) & ~3) * 4 + ((2 * nvec + 6 + 3) & ~3) * 4 + (hq + sq + rw * cand_words) * 4
    return (o + 31) & ~31


def wave_span(rw: int, read_len: int) -> int:
    """size_wave: a tile's bytes, (rw x longest read + 64) rounded up to 16; at most 10 KiB."""
    return (rw * read_len + 64 + 15) & ~15


def wave_nv(span: int) -> int:
    """The dispatch ladder (seeded_nv): span_cap <= 5 KiB -> 5 vectors per lane, else 10."""
    return 5 if span <= 5 * 1024 else 10


def size_wave(sp: dict, kend: int, cand_words: int, read_len: int, n_reads: int, n_cu: int, forced_rw: int = 0):
    """size_wave: tile size and workgroup shape (rw, waves, blocks, span) of a contiguous-tile plan, None when no shape keeps
    four waves resident (the batch then leaves the wave kernel)."""
    tables = wave_table_bytes(sp, kend)
    best = None
    best_waves = 0
    for rw in (32, 16, 8):
        if forced_rw and rw != forced_rw:
            continue
        if not forced_rw and rw > 8 and n_reads // rw < n_cu * 16:  # small batches: a tile per resident wave first
            continue
        span = wave_span(rw, max(read_len, 1))
        if span > 10 * 1024:
            continue
        hq = rw * math.ceil(max(6.0, 4.0 + 2.5 * sp["chance"]))
        sq = rw * math.ceil(max(3.0, 1.8 + 1.6 * sp["chance"]))
        area = wave_area_bytes(rw, span, hq, sq, cand_words)
        for w in (8, 16, 4):
            lds = tables + w * area
            if lds > LDS_MAX:
                continue
            per_cu = LDS_MAX // (((lds + 1279) // 1280) * 1280)
            if per_cu * w > 16:
                per_cu = 16 // w
            if per_cu < 1:
                continue
            if per_cu * w > best_waves:
                best_waves = per_cu * w
                best = dict(rw=rw, waves=w, blocks=per_cu * n_cu, span=span)
        if best_waves >= 12:
            break
    return best if best_waves >= 4 else None


def longest_in_cell(sp: dict, kend: int, cand_words: int, rw: int, nv: int) -> int:
    """The longest read at which a forced / planned `rw` still gives an NV = `nv` tile: the span bound ((5 or 10 KiB - 64)
    / rw), lowered while the LDS budget turns the shape away (size_wave)."""
    hi = (nv * 1024 - 64) // rw
    while hi > 0 and size_wave(sp, kend, cand_words, hi, 1 << 20, 1, forced_rw=rw) is None:
        hi -= 1
    return hi


# ---- recipes ----
# wave form (the template arguments after RW, TF, NV, Q) -> the config switches that select it, single pass, whole ranges
WAVE_FORMS = {
    # known-score class: unit costs, no trim side, no summary (bdx_plan.cpp known_ok) -> the non-split kernel (bdx_launch_wave)
    "false, 0, 0, false, 0, false, false": dict(kw={}, want_pass=False),
    # weighted costs: not the known class (known_ok false, kclass false: no KEND plan) -> split mode (build_wave_tables)
    "true, 0, 0, false, 0, false, false": dict(kw={"indel": 2}, want_pass=False),
    # known-trim class, trim_side 5 (build_wave_tables: F.wplan_k.kend = 1; bdx_wave_end.hip)
    "false, 0, 0, false, 1, true, false": dict(kw={"trim_side": 5}, want_pass=False),
    # known-trim class with a trim_side 3 pass: reversed sweeps (F.wplan_k.kend = 2; bdx_wave_rev.hip)
    "false, 0, 0, false, 2, true, false": dict(kw={"trim_side": 3}, want_pass=False),
    # known-alignment class: a known-trim config whose caller asks for per-pass start positions, which the known-trim class
    # does not know (build_wave_tables: F.wplan_a.kend = 3, taken per launch by bdx_classify_device; bdx_wave_aln.hip).  A
    # known-score config never builds that plan (it needs split mode or :exact)
    "false, 0, 0, false, 3, true, false": dict(kw={"trim_side": 5}, want_pass=True),
}
# (TF, Q) -> barcode length m at rate 0.1 (kb = floor(0.1 m)), the minimum Hamming distance of the synthetic set, the
# number of barcodes: Q = floor(m / (kb + 1)) capped at 8, track = m - kb - 1 (wave_seed_plan).  Q = 6 keeps 8 barcodes:
# its chance hits (2.3 per 150 bases at 32 barcodes) would overflow the hit queues of reads of 600+ bases, which size_wave
# sizes per 150 bases, and hand most reads on
WAVE_TFQ = {
    (20, 8): (24, 8, 32),  # kb 2, pieces of 8, track 21
    (12, 8): (16, 6, 32),  # kb 1, pieces of 8, track 14
    (0, 8): (8, 3, 32),  # kb 0, one piece of 8, track 7
    (12, 7): (14, 5, 32),  # kb 1, pieces of 7, track 12
    (0, 7): (7, 3, 32),  # kb 0, one piece of 7, track 6
    (0, 6): (12, 4, 8),  # kb 1, pieces of 6, track 10
}
RATE = 0.1
MAX_LEN = 1272  # the longest read any contiguous tile holds (size_wave: 8 reads x 1272 + 64 <= 10 KiB)
TILES = 40  # whole tiles of a batch (+ one ragged read): >= 2 x the 16 resident waves of one CU (size_wave caps them)


def wave_form_of(kw: dict, want_pass: bool) -> dict:
    """The wave form a single-pass config with whole ranges gets, from its switches `kw` (DemuxConfig fields) and whether
    the caller wants per-pass outputs: known_ok = unit costs, no trim side, no summary (bdx_plan.cpp, build_bitpar_tables);
    split = not known_ok (build_wave_tables); with unit costs a split config also gets the known-trim plan (no summary:
    KEND 1, or 2 with a trim_side 3 pass) and the known-alignment plan (KEND 3); bdx_classify_device takes the known-trim
    plan unless the caller wants per-pass start positions or statistics (kend_ok), else the known-alignment one (p.aln).
    Returns the form's spelling (the arguments after RW, TF, NV, Q), KEND and whether the launched kernel is split."""
    unit = kw.get("match", 0) == 0 and kw.get("mismatch", 1) == 1 and kw.get("indel", 1) == 1 and kw.get("nindel") is None
    trim = kw.get("trim_side")
    summary = bool(kw.get("summary", False))
    split = not (unit and trim is None and not summary)
    kend = 0
    if split and unit:
        kend_ok = not want_pass and not summary
        kend = (2 if trim == 3 else 1) if kend_ok else 3
    launched_split = split and kend == 0
    gen = kend > 0  # (the KEND instantiations keep the template's default GEN = true)
    form = f"{'true' if launched_split else 'false'}, 0, 0, false, {kend}, {'true' if gen else 'false'}, false"
    return dict(form=form, kend=kend, split=launched_split)


class Recipe:
    """One deterministic case for instantiation `target`: a DemuxConfig, two batches (main: the synthetic generator at the
    shortest read length of the cell that holds a barcode with flanks; edge: hand-planted reads up to the longest length
    that stays in the cell), want_pass and the developer switches (read once in bdx_create).  The lengths come from the
    planner's own choice on one CU (plain geometry) wherever some read length reaches the cell; only cells that no plain
    batch reaches force BDX_WAVE_RW, and `forced_why` says why."""

    def __init__(self, target, form, m, min_hamming, n_bc, rw, nv):
        self.target = target
        self.form = WAVE_FORMS[form]
        self.m = m
        self.n_bc = n_bc
        self.min_hamming = min_hamming
        self.rw = rw
        self.nv = nv
        self.want_pass = self.form["want_pass"]
        self.derived = wave_form_of(self.form["kw"], self.want_pass)
        sp = wave_seed_plan([m] * self.n_bc, RATE)
        self.cand_words = -(-self.n_bc // 32) if self.derived["split"] else 0
        # batches: n mod RW = 1 (a ragged last tile), >= 40 tiles (>= 2 per resident wave of the one CU), and >= 512 reads so
        # that the plain planner weighs every tile size (size_wave: RW 32 only once n / 32 >= 16 tiles per CU)
        self.n_main = max(TILES + 8, 512 // rw + 8) * rw + 1
        self.n_edge = max(TILES, 512 // rw) * rw + 1
        self.env = {"BDX_CU_COUNT": "1"}
        plain = [L for L in range(1, MAX_LEN + 1) if self.predict(self.n_edge, L) == target]
        self.forced_why = None
        if not plain:
            picks = sorted({(g["rw"], wave_nv(g["span"])) for L in range(1, MAX_LEN + 1)
                            for g in [size_wave(sp, self.derived["kend"], self.cand_words, L, self.n_edge, 1)] if g})
            self.forced_why = (f"no read length reaches RW {rw} / NV {nv} with plain geometry on one CU: size_wave picks "
                               f"(RW, NV) in {picks} over 1..{MAX_LEN} bases")
            self.env["BDX_WAVE_RW"] = str(rw)
            plain = [L for L in range(1, MAX_LEN + 1) if self.predict(self.n_edge, L) == target]
        self.low, self.edge_len = min(plain), max(plain)
        self.main_len = min(max(self.low, m + 40), self.edge_len)
        # reads the target may hand on (bdx_last_list_reads) per batch of n: a quarter, but Q = 6 reads beyond 600 bases
        # carry ~0.6 chance seed hits per 150 bases each (8 barcodes), against hit queues that size_wave sizes per 150
        # bases (hq_cap = rw x max(6, 4 + 2.5 chance)): at 1272 bases a tile overflows and hands on about a quarter of
        # its reads by design (measured: 87 of 321)
        self.list_div = 3 if (sp["q"] == 6 and self.edge_len > 600) else 4

    def barcodes(self):
        from biodemux_jl_amd import synth

        return synth.make_barcodes(self.n_bc, self.m, seed=1000 + self.m, min_hamming=self.min_hamming)

    def config(self):
        from biodemux_jl_amd import DemuxConfig

        bcs = self.barcodes()
        return DemuxConfig(bc_seqs=bcs, bc_lengths_no_N=[self.m] * self.n_bc, ids=[f"bc{i + 1}" for i in range(self.n_bc)],
                           max_error_rate=RATE, **self.form["kw"])

    def batch(self, which: str):
        """(seq bytes, offsets, longest read) of the main or the edge batch."""
        from biodemux_jl_amd import synth

        bcs = self.barcodes()
        if which == "main":
            seq, off, _ = synth.make_reads(bcs, self.n_main, read_len=self.main_len, seed=7000 + self.m * 31 + self.rw)
            return seq, off, self.main_len
        seq, off = edge_reads(bcs, int(RATE * self.m), self.edge_len, self.n_edge, seed=8000 + self.m * 31 + self.rw + self.nv)
        return seq, off, self.edge_len

    def predict(self, n_reads: int, longest: int) -> str:
        """The instantiation the rules give this recipe's config and switches for a batch of `n_reads` reads whose longest
        read is `longest` (None: not the wave kernel).  The form comes from the config (wave_form_of), not the target."""
        sp = wave_seed_plan([self.m] * self.n_bc, RATE)
        forced = int(self.env.get("BDX_WAVE_RW", 0))
        d = self.derived
        g = size_wave(sp, d["kend"], self.cand_words, longest, n_reads, int(self.env.get("BDX_CU_COUNT", 256)), forced)
        if g is None:
            return None
        args = dict(RW=g["rw"], TF=sp["tf"], NV=wave_nv(g["span"]), Q=sp["q"])
        return "bdx_wave_kernel<" + ", ".join(str(args[k]) for k in ("RW", "TF", "NV", "Q")) + ", " + d["form"] + ">"


def wave_form(name: str) -> str:
    """The form of a wave instantiation: its template arguments after RW, TF, NV, Q, as spelt in the name."""
    return ", ".join(name[:-1].split("<")[1].split(", ")[4:])


def edge_reads(bcs, kb: int, longest: int, n: int, seed: int):
    """Hand-planted reads at the edges of a cell, cycling through: a barcode at column 1; one ending at the read's last
    column; one straddling a 16-byte boundary of the batch's bytes (a tile holds
    them as they are: a vector boundary of the tile); a copy at distance kb (the budget) and one at kb + 1 (one
    beyond it), by substitutions; two different barcodes, exact (a tie: the ambiguity and min_delta rules decide); a read
    shorter than every barcode; an empty read; a planted read with N; a read without a barcode.  Read 0 has the longest
    length.  Returns (seq bytes, offsets)."""
    import numpy as np

    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    m = min(len(b) for b in bcs)

    def rand(k):
        return acgt[rng.integers(0, 4, size=k)].copy()

    def mutated(b, d):
        s = np.frombuffer(b.encode(), dtype=np.uint8).copy()
        for j in rng.choice(len(s), size=min(d, len(s)), replace=False):
            s[j] = acgt[(int(np.flatnonzero(acgt == s[j])[0]) + 1 + int(rng.integers(0, 3))) & 3]
        return s

    reads = []
    pos = 0  # the read's offset in the batch
    for i in range(n):
        kind = i % 10
        L = longest if (i == 0 or rng.random() < 0.7) else int(rng.integers(m, longest + 1))
        r = rand(L)
        b = bcs[int(rng.integers(0, len(bcs)))]
        bb = np.frombuffer(b.encode(), dtype=np.uint8)
        if kind == 0:
            r[: len(bb)] = bb
        elif kind == 1:
            r[L - len(bb):] = bb
        elif kind == 2:  # (a tile holds the batch's bytes as they are: the boundary is one of the batch, at pos + at)
            k = int(rng.integers(1, max(1, (L - len(bb) - 15) // 16) + 1))
            at = min(max(0, 16 * ((pos + 15) // 16 + k) - len(bb) // 2 - pos), L - len(bb))
            r[at: at + len(bb)] = bb
        elif kind in (3, 4):
            s = mutated(b, kb if kind == 3 else kb + 1)
            at = int(rng.integers(0, L - len(s) + 1))
            r[at: at + len(s)] = s
        elif kind == 5:
            b2 = np.frombuffer(bcs[(bcs.index(b) + 1) % len(bcs)].encode(), dtype=np.uint8)
            if L >= len(bb) + len(b2):
                at = int(rng.integers(0, L - len(bb) - len(b2) + 1))
                r[at: at + len(bb)] = bb
                at2 = int(rng.integers(at + len(bb), L - len(b2) + 1))
                r[at2: at2 + len(b2)] = b2
            else:
                r[: len(bb)] = bb
        elif kind == 6:
            r = rand(int(rng.integers(1, m)))
        elif kind == 7:
            r = r[:0]
        elif kind == 8:
            at = int(rng.integers(0, L - len(bb) + 1))
            r[at: at + len(bb)] = bb
            r[rng.choice(L, size=min(3, L), replace=False)] = ord("N")
        reads.append(r)
        pos += len(r)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate(reads).astype(np.uint8), off


def _wave_recipe(name: str):
    fam, a = parse(name)
    form = wave_form(name)
    if form not in WAVE_FORMS or (a["TF"], a["Q"]) not in WAVE_TFQ:
        return None
    m, hd, nb = WAVE_TFQ[(a["TF"], a["Q"])]
    return Recipe(name, form, m, hd, nb, a["RW"], a["NV"])


# ---- the fused filter (bdx_bitpar.hip) and the exact kernel (bdx_device.hip) ----
# Their geometry is not restated here: tests/call_host.cpp plans a recipe's calls with csrc/bdx_plan.cpp and
# csrc/bdx_call.cpp themselves, and the two ladders below spell the instantiation from the launch lines it reports.
def fused_name(args) -> str:
    """A `bitpar` launch line's arguments (R, SEED, DIAG, NW, WL: the ladder of bdx_launch_bitpar) -> the instantiation."""
    r, seed, diag, nw, wl = args
    return spell("bdx_bitpar_kernel", dict(BS=256, R=r, SEED=bool(seed), DIAG=bool(diag), NW=nw, WL=wl))


def generic_name(args) -> str:
    """A `generic` launch line's arguments (threads, reg_rows, clean, uniform_m, band_roll) -> the instantiation, by the
    ladder of bdx_launch_generic: the register DP only on 256 lanes, CLEAN / UM only there; REGM 0 with CLEAN is the
    rolling band."""
    bs, reg, clean, um, roll = args
    if reg in (24, 32) and bs == 256:
        return spell("bdx_generic_kernel", dict(BS=256, REGM=reg, CLEAN=bool(clean), UM=bool(clean and um)))
    return spell("bdx_generic_kernel", dict(BS=bs, REGM=0, CLEAN=bool(roll), UM=False))


def _tfq(q: int, track_from: int):
    """seeded_tfq (bdx_wave_kernel.h): seeds of 8 bases with every tracking start (20 / 12 / 0), 7 with 12 / 0, else 6 with 0."""
    if q == 8:
        return (20 if track_from >= 20 else 12 if track_from >= 12 else 0), 8
    if q == 7:
        return (12 if track_from >= 12 else 0), 7
    return 0, 6


def wave_name(args) -> str:
    """A `wave` launch line's arguments (rw, split, kend, winm, q, track_from, span_cap, slot, gen, pairs_kb, nw, groups) ->
    the instantiation, by seeded_ladder / seeded_tfq / seeded_nv (bdx_wave_kernel.h) and the leaves: window mode
    (bdx_wave_win.hip) has a tile and NV rule of its own over the tile's vectors and is <false, 0, GEN, WINM>; the known-end
    forms keep the template's GEN = true; the others (bdx_wave.hip) take GEN from gen.  None: the ladder refuses the plan."""
    rw, split, kend, winm, q, track_from, span_cap, slot, gen, pairs_kb, nw, groups = args
    tf, qq = _tfq(q, track_from)
    if winm:
        vecs = rw * (slot >> 4)
        nv = 3 if (rw == 32 and vecs <= 64 * 3) else 7 if (rw == 32 and vecs <= 64 * 7) else 4 if (rw == 16 and vecs <= 64 * 4) else None
        if nv is None or split or kend:
            return None
        return spell("bdx_wave_kernel", dict(RW=rw, TF=tf, NV=nv, Q=qq, SPLIT=False, KB=0, NW=0, MG=False, KEND=0, GEN=True, WINM=True))
    if rw not in (32, 16, 8) or pairs_kb > 0:
        return None
    nv = 5 if span_cap <= 5 * 1024 else 10
    return spell("bdx_wave_kernel", dict(RW=rw, TF=tf, NV=nv, Q=qq, SPLIT=bool(split), KB=0, NW=0, MG=False, KEND=kend, GEN=bool(kend > 0 or gen), WINM=False))


def pairs_name(args) -> str:
    """A `pairs` launch line's arguments (as wave_name's) -> the instantiation, by pairs_ladder / pairs_kb / pairs_nw
    (bdx_wave_kernel.h) and the leaf of bdx_launch_pairs (bdx_pairs.hip): tiles of 16 slots, TF 12, Q 4; NV 3 / 6 from the
    span; the same-diagonal variants (8 / 9) are split; more than one group of 128 barcodes is MG with four mask words."""
    rw, split, kend, winm, q, track_from, span_cap, slot, gen, pairs_kb, nw, groups = args
    if rw != 16 or span_cap > 6 * 1024 + 16 or pairs_kb <= 0:
        return None
    nv = 3 if span_cap <= 3 * 1024 + 16 else 6
    kb = pairs_kb if pairs_kb in (8, 9) else 3 if pairs_kb <= 3 else 4
    nww = 2 if nw <= 2 else 3 if nw == 3 else 4
    mg = kb < 8 and groups > 1 and kend < 2
    a = dict(RW=16, TF=12, NV=nv, Q=4, SPLIT=bool(split or kb >= 8) and not mg, KB=kb, NW=4 if mg else nww, MG=mg, KEND=0 if mg else kend, GEN=True, WINM=False)
    return spell("bdx_wave_kernel", a)


def planned_launches(report, c: int = 0) -> list:
    """The classify launches the driver plans for call c of a case: dicts of kernel (spelt by the ladders above), family,
    list, blocks, tile, threads."""
    ladder = dict(bitpar=fused_name, generic=generic_name, wave=wave_name, pairs=pairs_name)
    out = []
    for ln in report.launches(c):
        out.append(dict(kernel=ladder[ln["family"]](ln["args"]), family=ln["family"], list=ln["list"], blocks=ln["blocks"], tile=ln["tile"],
                        threads=ln["threads"]))
    return out


# developer switch (read once in bdx_create) -> the driver's tuning key
SWITCHES = {"BDX_CU_COUNT": "n_cu", "BDX_BITPAR_R": "bitpar_r", "BDX_NO_SEED": "no_seed", "BDX_NO_WAVE": "no_wave", "BDX_NO_TIER": "no_tier",
            "BDX_NO_PAIRS": "no_pairs", "BDX_DIAG_MIN_B": "diag_min_b", "BDX_NO_CLEAN": "no_clean", "BDX_LDS_DP": "lds_dp",
            "BDX_NO_BAND_ROLL": "no_band_roll"}
WANT_ALL, WANT_VERDICT = 0x3FF, 0xF  # the outputs a want_pass caller asks for / the verdict alone (biodemux_hip.h BDX_WANT_*)
FUSED_MAX_LEN = 12000  # the sweeps of read lengths end here: beyond ~10 000 bases not even 16 reads of a tile fit the LDS (fit_bitpar)
EXACT_EDGE_LEN = 300  # the longest read of an exact-kernel recipe: its instantiation does not depend on the batch


def mixed_barcodes(n: int, lo: int, hi: int, seed: int, min_hamming: int):
    """n barcodes, alternately `lo` and `hi` bases long."""
    from biodemux_jl_amd import synth

    return synth.make_barcodes(n, hi, seed=seed, min_hamming=min_hamming, lengths=[hi if i % 2 else lo for i in range(n)])


# barcode sets: name -> (count, shortest, longest, seed, min Hamming distance, letter put in place of barcode 0's last base)
SETS = {
    "b24": (32, 24, 24, 1024, 8, None),
    "b24R": (32, 24, 24, 1024, 8, "R"),  # one IUPAC letter: outside the wave kernel's alphabet (bdx_plan.cpp wave_domain), seeds stay
    "b2024R": (32, 20, 24, 1020, 8, "R"),
    "b32": (32, 32, 32, 1032, 10, None),
    "b32R": (32, 32, 32, 1032, 10, "R"),
    "b2832R": (32, 28, 32, 1028, 10, "R"),
    "b3364": (32, 33, 64, 1033, 12, None),  # the shortest and the longest barcode of a 64-bit sweep word
    "b65128": (16, 65, 128, 1065, 24, None),  # ... of a 128-bit sweep word
    "b128": (8, 128, 128, 1128, 40, None),
    "b128x250": (250, 128, 128, 1228, 40, None),
    "b80": (8, 80, 80, 1080, 26, None),
    "b154": (8, 154, 154, 1154, 50, None),
    "b24N96": (96, 24, 24, 1096, 8, "N"),  # >= 48 barcodes (diag_min_b), one with N: N-scoring keeps the config off the wave kernel and the tiers
}
END_BINDS = "1:end-1"  # a barcode_end_range that can bind: outside the clean class and the rolling band (plan_generic: free_ranges)
ROWS_WL1 = (31, 32, 33)  # barcode rows either side of the carry between the 32-bit halves of a 64-bit sweep word
ROWS_WL2 = (31, 32, 33, 63, 64, 65, 95, 96, 97)  # ... of a 128-bit one
TEN = ("col1", "last_col", "straddle16", "sub_kb", "sub_kb1", "two_exact", "short", "empty", "with_N", "none")
INDEL = ("indel_kb", "indel_kb1")
DIAG_KINDS = ("diag_adjacent", "diag_first_last", "diag_ins_between", "diag_del_between", "diag_one_piece")
BAND_KINDS = ("ins_kb", "del_kb", "read_m", "read_m_minus_kb", "read_m_plus_kb")
AT_KB1 = ("sub_kb1", "indel_kb1", "diag_one_piece")  # one operation beyond the budget: such reads come out unassigned


def row_kinds(rows):
    return tuple(f"row{r}_{t}" for r in rows for t in ("sub", "ins", "del"))


def at_kb(kind: str) -> bool:
    """Kinds planted at exactly the budget: they must be assigned."""
    return kind in ("sub_kb", "indel_kb", "ragged_last", "sd_gmax", "ins_kb", "del_kb", "read_m", "read_m_minus_kb", "read_m_plus_kb") or kind.startswith("row") or (
        kind in DIAG_KINDS and kind != "diag_one_piece")


class CellRecipe:
    """One deterministic case for a fused-filter or exact-kernel instantiation `target`: a DemuxConfig over barcode set
    `bset`, the `filter` argument of HipClassifier, want_pass, the developer switches, and two batches of `n` reads: main
    (the synthetic generator at the shortest read length of the cell that holds a barcode with flanks) and edge
    (cell_edge_reads up to `edge_len`, the longest read of the cell).  [low, edge_len] is the cell as the driver plans it
    (test_kernel_lattice_cpu.py holds the numbers against it); `end_why` says what ends the cell where the next length
    would still plan to the target.  A switch other than BDX_CU_COUNT is set only where `forced_why` says why."""

    def __init__(self, target, bset, kw, n, low, edge_len, kinds, filter="auto", want_pass=False, force=None, forced_why=None, end_why=None,
                 edge_seed=0, bare_kb1=False):
        self.bare_kb1 = bare_kb1
        self.target, self.bset, self.kw, self.n, self.low, self.edge_len = target, bset, dict(kw), n, low, edge_len
        self.kinds, self.filter, self.want_pass, self.forced_why, self.end_why, self.edge_seed = tuple(kinds), filter, want_pass, forced_why, end_why, edge_seed
        self.family = parse(target)[0]
        self.env = dict({"BDX_CU_COUNT": "1"}, **(force or {}))
        self.rate = self.kw["max_error_rate"]
        self.n_main = self.n_edge = n
        nb, lo, hi, seed, hd, letter = SETS[bset]
        self.max_m, self.min_m = hi, lo
        self.main_len = min(max(low, hi + 40), edge_len)

    def barcodes(self):
        nb, lo, hi, seed, hd, letter = SETS[self.bset]
        from biodemux_jl_amd import synth

        bcs = mixed_barcodes(nb, lo, hi, seed, hd) if lo != hi else synth.make_barcodes(nb, hi, seed=seed, min_hamming=hd)
        if letter:
            # the letter goes last: the planner numbers the alphabet by first appearance (code_alphabet, bdx_plan.cpp) and the seed keys
            # keep two bits of a code, so a letter that comes before all four bases have appeared would share its key bits with a base
            assert set(bcs[0][:-1]) == set("ACGT"), bcs[0]
            bcs[0] = bcs[0][:-1] + letter
        return bcs

    def planted(self):
        """What the batches carry: the barcodes, the one with a letter outside A C G T left out."""
        return [b for b in self.barcodes() if set(b) <= set("ACGT")]

    def config(self):
        from biodemux_jl_amd import DemuxConfig, parse_dynamic_range

        bcs = self.barcodes()
        kw = dict(self.kw)
        if "barcode_end_range" in kw:
            kw["barcode_end_range"] = parse_dynamic_range(kw["barcode_end_range"])
        return DemuxConfig(bc_seqs=bcs, bc_lengths_no_N=[len(b) - b.count("N") for b in bcs], ids=[f"bc{i + 1}" for i in range(len(bcs))], **kw)

    def batch(self, which: str):
        """(seq bytes, offsets, longest read) of the main or the edge batch."""
        if which == "main":
            from biodemux_jl_amd import synth

            seq, off, _ = synth.make_reads(self.planted(), self.n_main, read_len=self.main_len, seed=7100 + self.max_m * 31 + self.n)
            return seq, off, self.main_len
        seq, off, _ = self.edge_batch()
        return seq, off, self.edge_len

    def edge_batch(self):
        """(seq bytes, offsets, kind of every read) of the edge batch."""
        return cell_edge_reads(self.planted(), self.rate, self.edge_len, self.n_edge, 8100 + self.max_m * 31 + self.n + self.edge_seed, self.kinds,
                               bare_kb1=self.bare_kb1)

    def case(self, name: str, shapes, force=True):
        """The driver case (tests/call_cases.py) of this recipe's config for calls of (n_reads, longest read), in order on one
        context; force=False: without the switches other than BDX_CU_COUNT."""
        import call_cases as CC
        import plan_cases as PC

        kw = self.kw
        end = (1, -1, 0, 1) if kw.get("barcode_end_range") == END_BINDS else PC.WHOLE
        assert kw.get("barcode_end_range") in (None, END_BINDS)
        env = self.env if force else {"BDX_CU_COUNT": "1"}
        return CC.CallCase(name, None, [CC.call(n, L, wanted=WANT_ALL if self.want_pass else WANT_VERDICT) for n, L in shapes],
                           passes=[PC.one_pass(self.barcodes(), trim=kw.get("trim_side") or 0, end=end)], rate=self.rate,
                           costs=(kw.get("match", 0), kw.get("mismatch", 1), kw.get("indel", 1)), nindel=kw.get("nindel"),
                           filter={"auto": PC.AUTO, "off": PC.OFF, "bitpar": PC.BITPAR}[self.filter], tune={SWITCHES[k]: int(v) for k, v in env.items()})


def whole_batch_target(launches, target) -> bool:
    """The planned launches hold `target` over the whole batch (not in list mode); for the fused filter as the full-budget
    launch: the last fused launch of the call, which a tiered call makes in list mode."""
    fam = parse(target)[0]
    if fam == "bdx_bitpar_kernel":
        fused = [ln for ln in launches if ln["family"] == "bitpar"]
        return bool(fused) and fused[-1]["kernel"] == target and not fused[-1]["list"]
    return any(ln["kernel"] == target and not ln["list"] for ln in launches if ln["family"] == "generic")


def _edited(rng, b: str, ops):
    """Barcode `b` (bytes as a uint8 array) after `ops`, a list of (row, "sub" | "ins" | "del") on distinct rows of the
    barcode, applied from the last row to the first so that every row is the barcode's own."""
    import numpy as np

    acgt = b"ACGT"
    s = bytearray(b.encode())
    for row, op in sorted(ops, reverse=True):
        if op == "sub":
            s[row] = acgt[(acgt.find(bytes([s[row]])) + 1 + int(rng.integers(0, 3))) & 3]
        elif op == "del":
            del s[row]
        else:  # a base in front of `row` that repeats neither neighbour (the insertion cannot slide into a match)
            s.insert(row, next(c for c in acgt if c != s[row] and (row == 0 or c != s[row - 1])))
    return np.frombuffer(bytes(s), dtype=np.uint8).copy()


def _spread_rows(rng, m: int, k: int, avoid=()):
    """k distinct rows of an m-row barcode, three apart from one another and from `avoid` (edits that far apart do not
    combine into fewer operations), none of them the first or the last row."""
    grid = [r for r in range(1, m - 1, 3) if all(abs(r - a) >= 3 for a in avoid)]
    if len(grid) < k:  # (budgets beyond a third of the rows: every second row)
        grid = [r for r in range(1, m - 1, 2) if all(abs(r - a) >= 3 for a in avoid)]
    assert len(grid) >= k, (m, k, avoid)
    return [int(r) for r in rng.choice(grid, size=k, replace=False)]


def diag_pieces(m: int, kb: int):
    """build_diag_tables (bdx_plan.cpp): kb + 2 pieces of floor(m / (kb + 2)) bases; the index keys each by its first four."""
    p = kb + 2
    return [t * (m // p) for t in range(p)]


def unit_distance(b, s) -> int:
    """The smallest unit edit distance of barcode `b` (whole) to a stretch of `s` (uint8 arrays): the semiglobal DP, row by row."""
    import numpy as np

    cols = np.arange(len(s) + 1)
    row = np.zeros(len(s) + 1, dtype=np.int64)
    for i in range(len(b)):
        new = np.empty_like(row)
        new[0] = i + 1
        new[1:] = np.minimum(row[:-1] + (s != b[i]), row[1:] + 1)
        row = np.minimum.accumulate(new - cols) + cols  # (a run of insertions: + 1 per column)
    return int(row.min())


def cell_edge_reads(bcs, rate: float, longest: int, n: int, seed: int, kinds, bare_kb1=False):
    """Hand-planted reads at the edges of a fused-filter or exact-kernel cell, cycling through `kinds`: the ten kinds of
    edge_reads (TEN; barcodes of several lengths allowed) and
      indel_kb / indel_kb1: a copy at unit distance kb / kb + 1 made with one insertion, one deletion and substitutions;
      row<r>_sub / _ins / _del: a copy at distance kb with that edit at barcode row r (ROWS_WL1 / ROWS_WL2: either side of a
        carry between the 32-bit halves of a sweep word), the other kb - 1 edits substitutions elsewhere;
      diag_*: one edit in the indexed four bases of kb of the kb + 2 pieces of the two-intact-pieces index, the two intact ones
        adjacent / the first and the last / the first and the last with an insertion or a deletion in every piece between
        (diagonals kb apart, either direction); diag_one_piece: kb + 1 pieces edited;
      ins_kb / del_kb: kb insertions / deletions only (start and end column the whole budget apart, either side);
      read_m / read_m_minus_kb / read_m_plus_kb: the read IS the copy, from column 1 to its last column;
      cut_front: the read begins with a barcode's second base (the alignment's origin lies before the read: start <= 0 for a sweep
        from the other end);  sd_gmax (indels at cost 2, the pairs mode's same-diagonal variants): the first two pieces intact on
        one diagonal, then as many insertions as the budget pays for, one per piece, and a substitution for what is left of it;
    and the batch's last read, alone in its tile or workgroup, is a copy at distance kb (ragged_last).  kb = floor(rate x
    length) of the planted barcode.  bare_kb1 (budgets so large that a random flank lies within them of SOME barcode, and that
    kb + 1 scattered edits have a shorter alignment): the sub_kb1 / indel_kb1 copy gets further substitutions until
    unit_distance says kb + 1, and the read is the copy alone.  Read 0 has the longest length.  Returns (seq bytes, offsets, kind per read)."""
    import numpy as np

    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    m_min, m_max = min(len(b) for b in bcs), max(len(b) for b in bcs)
    kb_of = lambda b: int(rate * len(b))  # noqa: E731
    room = min(longest, m_max + kb_of(max(bcs, key=len)) + 2)  # a read that holds any copy (or the longest the cell takes)

    def rand(k):
        return acgt[rng.integers(0, 4, size=k)].copy()

    def arr(b):
        return np.frombuffer(b.encode(), dtype=np.uint8)

    def pick(min_len=0):
        ok = [b for b in bcs if len(b) >= min_len]
        return ok[int(rng.integers(0, len(ok)))]

    def copy_of(kind):
        """The planted bytes of a mutated-copy kind."""
        if kind.startswith("row"):
            row, op = int(kind[3:kind.index("_")]), kind[kind.index("_") + 1:]
            b = pick(row + 3)
            kb = kb_of(b)
            return _edited(rng, b, [(row, op)] + [(r, "sub") for r in _spread_rows(rng, len(b), max(kb - 1, 0), avoid=(row,))])
        b = pick()
        kb, m = kb_of(b), len(b)
        if kind in ("sub_kb", "sub_kb1", "ragged_last", "indel_kb", "indel_kb1"):
            rows = _spread_rows(rng, m, kb + kind.endswith("kb1"))
            ops = (["ins", "del"] if kind.startswith("indel") else []) + ["sub"] * len(rows)
            s = _edited(rng, b, list(zip(rows, ops)))
            if bare_kb1 and kind in AT_KB1:
                free = [int(r) for r in rng.permutation(m) if int(r) not in rows]
                while unit_distance(arr(b), s) <= kb:
                    rows.append(free.pop())
                    s = _edited(rng, b, list(zip(rows, ops + ["sub"] * m)))
            return s
        if kind == "sd_gmax":  # (budget 3: six 4-base pieces, budget 6: eight 3-base pieces; an indel costs 2)
            pl, g = m // (6 if kb < 6 else 8), kb // 2
            return _edited(rng, b, [((2 + t) * pl + 1, "ins") for t in range(g)] + [((2 + g) * pl + 1, "sub")] * (kb - 2 * g))
        if kind in ("ins_kb", "read_m_plus_kb"):
            return _edited(rng, b, [(r, "ins") for r in _spread_rows(rng, m, kb)])
        if kind in ("del_kb", "read_m_minus_kb"):
            return _edited(rng, b, [(r, "del") for r in _spread_rows(rng, m, kb)])
        if kind == "read_m":
            return arr(b).copy()
        at = diag_pieces(m, kb)
        p = len(at)
        if kind == "diag_adjacent":
            s = int(rng.integers(0, p - 1))
            return _edited(rng, b, [(at[t] + int(rng.integers(0, 4)), "sub") for t in range(p) if t not in (s, s + 1)])
        if kind == "diag_first_last":
            return _edited(rng, b, [(at[t] + int(rng.integers(0, 4)), "sub") for t in range(1, p - 1)])
        if kind == "diag_ins_between":
            return _edited(rng, b, [(at[t] + 2, "ins") for t in range(1, p - 1)])
        if kind == "diag_del_between":
            return _edited(rng, b, [(at[t] + 1, "del") for t in range(1, p - 1)])
        assert kind == "diag_one_piece", kind
        s = int(rng.integers(0, p))
        return _edited(rng, b, [(at[t] + int(rng.integers(0, 4)), "sub") for t in range(p) if t != s])

    reads, names = [], []
    pos = 0  # the read's offset in the batch
    for i in range(n):
        kind = "ragged_last" if i == n - 1 else kinds[i % len(kinds)]
        L = longest if (i == 0 or rng.random() < 0.7 or room >= longest) else int(rng.integers(room, longest + 1))
        r = rand(L)
        if kind == "cut_front":
            bb = arr(pick())
            r[: len(bb) - 1] = bb[1:]
        elif kind in ("col1", "last_col", "straddle16", "two_exact", "with_N"):
            bb = arr(pick())
            if len(bb) > L:
                bb = arr(min(bcs, key=len))
            if kind == "col1":
                r[: len(bb)] = bb
            elif kind == "last_col":
                r[L - len(bb):] = bb
            elif kind == "straddle16":  # (a tile holds the batch's bytes as they are: the boundary is one of the batch, at pos + at)
                k = int(rng.integers(1, max(1, (L - len(bb) - 15) // 16) + 1))
                at = min(max(0, 16 * ((pos + 15) // 16 + k) - len(bb) // 2 - pos), L - len(bb))
                r[at: at + len(bb)] = bb
            elif kind == "two_exact":
                i1 = int(rng.integers(0, len(bcs)))
                bb, b2 = arr(bcs[i1]), arr(bcs[(i1 + 1) % len(bcs)])
                if len(bb) > L:
                    bb = arr(min(bcs, key=len))
                if L >= len(bb) + len(b2):
                    at = int(rng.integers(0, L - len(bb) - len(b2) + 1))
                    r[at: at + len(bb)] = bb
                    at2 = int(rng.integers(at + len(bb), L - len(b2) + 1))
                    r[at2: at2 + len(b2)] = b2
                else:
                    r[: len(bb)] = bb
            else:
                at = int(rng.integers(0, L - len(bb) + 1))
                r[at: at + len(bb)] = bb
                r[rng.choice(L, size=min(3, L), replace=False)] = ord("N")
        elif kind == "short":
            r = rand(int(rng.integers(1, m_min)))
        elif kind == "empty":
            r = r[:0]
        elif kind in ("read_m", "read_m_minus_kb", "read_m_plus_kb") or (bare_kb1 and kind in AT_KB1):
            r = copy_of(kind)
        elif kind != "none":
            s = copy_of(kind)
            if len(s) > L:
                r = rand(len(s))
                L = len(s)
            at = int(rng.integers(0, L - len(s) + 1))
            r[at: at + len(s)] = s
        reads.append(r)
        names.append(kind)
        pos += len(r)
    assert max(len(r) for r in reads) == longest == len(reads[0]), (longest, max(len(r) for r in reads))
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate(reads).astype(np.uint8), off, names


CELL_RECIPES = {}


def _cell(target, *a, **kw):
    assert target not in CELL_RECIPES, target
    CELL_RECIPES[target] = (a, kw)


# -- the fused filter: known-score configs (the filter settles the verdicts itself, what it cannot goes to the exact kernel as
# a list), so the full-budget launch runs over the whole batch.  Product configs throughout: barcodes of 33..64 / 65..128 nt
# choose the sweep word (WL 1 / 2) and lie outside the wave kernel; 24-nt sets stay off it through one IUPAC letter; SEED
# false is HipClassifier(filter="bitpar"); the two-intact-pieces index (DIAG) gets 96 barcodes of 24 nt at rate 0.2 under
# N-scoring (no tiers, no wave or pairs tables: bdx_plan.cpp wave_domain).  Batches of 16 R + 1 reads on one CU: at most 8
# workgroups (grid_bitpar), two tiles each and a ragged one; the DIAG cells take 513 reads (r_cap 128: size_bitpar).
# (WL, SEED) -> barcode set, filter
FUSED_SETS = {(0, True): ("b24R", "auto"), (0, False): ("b24", "bitpar"), (1, True): ("b3364", "auto"), (1, False): ("b3364", "bitpar"),
              (2, True): ("b65128", "auto"), (2, False): ("b65128", "bitpar")}
FUSED_KINDS = {0: TEN + INDEL, 1: TEN + INDEL + row_kinds(ROWS_WL1), 2: TEN + INDEL + row_kinds(ROWS_WL2)}
# (R, SEED, WL) -> the cell [low, edge_len] in bases as the planner gives it for 16 R + 1 reads on one CU; forced: no read length
# of 1..FUSED_MAX_LEN reaches the tile size by the planner's own choice (fit_bitpar's ranking by LDS residency; without
# seeds tiles above 64 reads are skipped for reads <= 1024 bases), BDX_BITPAR_R sets it
FUSED_CELLS = {
    (16, False, 0): (4994, 10069), (16, False, 1): (4970, 10021), (16, False, 2): (4934, 9949),
    (16, True, 0): (3792, 7764), (16, True, 1): (3693, 7565), (16, True, 2): (3715, 7610),
    (32, False, 0): (736, 2433), (32, False, 1): (724, 2409), (32, False, 2): (706, 2373),
    (32, True, 0): (429, 1743), (32, True, 1): (380, 1644), (32, True, 2): (391, 1666),
    (64, False, 0): (1, 735), (64, False, 1): (1, 723), (64, False, 2): (1, 705),
    (64, True, 0): (124, 428), (64, True, 1): (99, 379), (64, True, 2): (1, 390),
    (128, True, 0): (1, 123), (128, True, 1): (1, 98),
    (128, False, 0): (1, 1186, "forced"), (128, False, 1): (1, 1180, "forced"),
    (256, False, 0): (1, 552, "forced"), (256, False, 1): (1, 549, "forced"), (256, True, 0): (1, 315, "forced"), (256, True, 1): (1, 302, "forced"),
}
# (R, NW) -> the cell of the DIAG instantiations at 513 reads: NW 5 up to 152 bases, 10 up to the index's 312 (fit_bitpar)
DIAG_CELLS = {(32, 5): (1, 59), (16, 5): (60, 138), (8, 5): (139, 152), (16, 10): (153, 184), (8, 10): (185, 312),
              (32, 10): (153, 312, "forced"), (4, 5): (1, 152, "forced"), (4, 10): (153, 312, "forced")}


def _fused_recipes():
    for (r, seed, wl), cell in FUSED_CELLS.items():
        bset, filt = FUSED_SETS[(wl, seed)]
        forced = len(cell) == 3
        why = (f"no read length of 1..{FUSED_MAX_LEN} bases reaches a {r}-read tile with the planner's own choice at {16 * r + 1} reads on one "
               f"CU (fit_bitpar, bdx_call.cpp): BDX_BITPAR_R sets the tile.  The sweep varies the read length only, at this batch size and "
               f"barcode set: a stated limit of the recipe, not a proof that no product config reaches the cell") if forced else None
        _cell(fused_name((r, seed, False, 5, wl)), bset, dict(max_error_rate=0.1), 16 * r + 1, cell[0], cell[1], FUSED_KINDS[wl], filter=filt,
              force={"BDX_BITPAR_R": str(r)} if forced else None, forced_why=why)
    for (r, nw), cell in DIAG_CELLS.items():
        forced = len(cell) == 3
        why = (f"no read length of 1..312 bases reaches a {r}-read tile with the {nw * 32}-position index by the planner's own choice at 513 reads "
               f"on one CU (fit_bitpar, bdx_call.cpp): BDX_BITPAR_R sets the tile.  The sweep varies the read length only, at this batch size "
               f"and barcode set: a stated limit of the recipe, not a proof that no product config reaches the cell") if forced else None
        _cell(fused_name((r, True, True, nw, 0)), "b24N96", dict(max_error_rate=0.2, nindel=1), 513, cell[0], cell[1], TEN + INDEL + DIAG_KINDS,
              force={"BDX_BITPAR_R": str(r)} if forced else None, forced_why=why)


# -- the exact kernel: split configs without a front stage (trim_side 5 with want_pass: start and end columns are compared),
# so the exact kernel runs over the whole batch behind the fused filter, or alone where no filter stands.  Its instantiation
# is decided at create time (plan_generic, bdx_plan.cpp): every read length plans to it, the recipes state EXACT_EDGE_LEN as
# their end.  3 BS + 1 reads: three whole workgroups and a ragged one.
EXACT_END = "the instantiation is chosen when the context is created (plan_generic, bdx_plan.cpp): no read length leaves the cell"
TRIM5 = dict(max_error_rate=0.1, trim_side=5)
EXACT_KINDS = TEN + INDEL + BAND_KINDS


def _exact_recipes():
    def ex(args, bset, kw, kinds=EXACT_KINDS, **more):
        name = generic_name(args)
        if "barcode_end_range" in kw:  # (no occurrence may end in the read's last column: the reads that ARE a copy stay out)
            kinds = tuple(k for k in kinds if not k.startswith("read_m"))
        _cell(name, bset, kw, 3 * args[0] + 1, 1, EXACT_EDGE_LEN, kinds, want_pass=True, end_why=EXACT_END, **more)

    # the register DP: every barcode REGM rows (UM) / some shorter / a barcode_end_range that can bind (outside the clean class)
    ex((256, 24, 1, 1, 0), "b24R", TRIM5)
    ex((256, 24, 1, 0, 0), "b2024R", TRIM5)
    ex((256, 24, 0, 0, 0), "b24", dict(TRIM5, barcode_end_range=END_BINDS))
    ex((256, 32, 1, 1, 0), "b32R", TRIM5)
    ex((256, 32, 1, 0, 0), "b2832R", TRIM5)
    ex((256, 32, 0, 0, 0), "b32", dict(TRIM5, barcode_end_range=END_BINDS))
    # beyond 32 rows: the rolling band behind the 64-bit filter (256 lanes); at rate 0.27 the 128-nt band's H = 2 x 34 + 9 cells
    # with trace-back no longer fit 256 lanes (128); the LDS columns of 33..64 nt (256 lanes), 80 nt (128) and 154 nt (64)
    ex((256, 0, 0, 0, 1), "b3364", TRIM5, kinds=EXACT_KINDS + row_kinds(ROWS_WL1))
    ex((128, 0, 0, 0, 1), "b128", dict(TRIM5, max_error_rate=0.27))
    # the band on 64 lanes: plan_generic's `fixed` term decides it (the staged barcode bytes, up to 32 KiB, 12 B per barcode and the
    # histogram): with 250 barcodes of 128 nt, 128 lanes x (2 x 56 + 9 + 1) cells x 8 B + fixed + 4 KiB pass the 160 KiB at rate
    # 0.44; 240 barcodes need rate 0.45, 220 need 0.46, and at 0.5 the band no longer stands (hcap + 1 >= max_m + 1)
    # (at that budget every 300-base random read lies within it of one of the 250 barcodes: bare_kb1)
    ex((64, 0, 0, 0, 1), "b128x250", dict(TRIM5, max_error_rate=0.44), bare_kb1=True)
    ex((256, 0, 0, 0, 0), "b3364", dict(TRIM5, barcode_end_range=END_BINDS), kinds=EXACT_KINDS + row_kinds(ROWS_WL1))
    ex((128, 0, 0, 0, 0), "b80", dict(TRIM5, barcode_end_range=END_BINDS))
    ex((64, 0, 0, 0, 0), "b154", TRIM5)


_fused_recipes()
_exact_recipes()


# -- window mode (bdx_wave_win.hip): single-pass known-score configs whose ref_search_range window is at most half the planned
# read.  The cell follows the slot, (window + 30) & ~15 positions per read (size_wave_win, bdx_call.cpp), which the dispatch
# ladder turns into (RW, NV), and the residency of either tile size, which depends on the seed tables: with seeds of 8 bases
# (a bitmap of 8 KiB) 16-read tiles keep more waves resident from 114 columns on.  The numbers below are the window columns
# of each cell as the planner gives them on one CU (test_kernel_lattice_cpu.py holds them against the driver, one column
# beyond either end).  32-read tiles are not instantiated beyond 7 vectors per lane, so the widest slots take 16-read tiles
# without a forced switch.  (RW, NV) -> (narrowest, widest window) for Q = 8 / for Q = 7 and 6
WIN_CELLS = {(32, 3): ((1, 81), (1, 81)), (32, 7): ((82, 113), (82, 209)), (16, 4): ((114, 241), (210, 241))}
WIN_STYLES = ("start", "end", "mix")  # the window counted from the read's start / from its end / its start from the end and its end from the start
WIN_K = 8  # columns in front of a window counted from the start: reads of up to 8 bases have an empty window
WIN_KINDS = ("win_first", "win_last", "win_before1", "win_after1", "win_outside", "straddle16", "sub_kb", "sub_kb1", "two_exact", "short", "empty",
             "with_N", "N_out", "none", "clipped", "before_start", "long2x", "long_ends")


class WinRecipe:
    """One deterministic case for a window-mode instantiation `target`: the barcode set of its (TF, Q) (WAVE_TFQ) at RATE,
    known-score, with a ref_search_range of `w` columns at the planned read length — the widest window of the cell — in one of
    three styles, spread over the six (TF, Q) of every (RW, NV).  Both batches are planned at 2 w + 1 bases
    (set_read_length_hint, as a pipeline that knows its reads does): the main batch from the synthetic generator with the
    barcodes planted inside the window, the edge batch hand-planted (win_edge_reads) with reads of many lengths, some longer
    than twice the planned one.  [low, high] are the planned read lengths of the cell; high None: `end_why` says why no
    longer read leaves it."""

    def __init__(self, target):
        fam, a = parse(target)
        self.target, self.rw, self.nv = target, a["RW"], a["NV"]
        self.m, self.min_hamming, self.n_bc = WAVE_TFQ[(a["TF"], a["Q"])]
        self.style = WIN_STYLES[list(WAVE_TFQ).index((a["TF"], a["Q"])) % 3]
        self.w_lo, self.w = WIN_CELLS[(self.rw, self.nv)][0 if a["Q"] == 8 else 1]
        self.main_len = self.edge_len = self.hint = 2 * self.w + 1
        # a window counted from both ends shrinks as the planned read grows and grows as it shrinks: its cell has two ends
        self.low = self.main_len if self.style == "mix" else 2 * self.w
        self.high = self.main_len + self.w - self.w_lo if self.style == "mix" else None
        self.end_why = None if self.style == "mix" else ("size_wave_win (bdx_call.cpp) sizes the slot by the window, which a range counted from one end "
                                                         "keeps at every longer planned read")
        # two tiles per resident wave of the one CU (at most 16) and more, a ragged last tile; RW 32 needs n / 32 >= 16 (size_wave_win)
        self.n_main = self.n_edge = (40 if self.rw == 32 else 33) * self.rw + 1
        self.env = {"BDX_CU_COUNT": "1"}
        self.forced_why = None
        self.want_pass = False
        self.list_div = 4
        self.kinds = WIN_KINDS

    def range_str(self) -> str:
        w, L = self.w, self.main_len
        return {"start": f"{WIN_K + 1}:{WIN_K + w}", "end": f"end-{w - 1}:end", "mix": f"end-{L - WIN_K - 1}:{WIN_K + w}"}[self.style]

    def range(self):
        """The range as its four integers (what range_str parses to: test_kernel_lattice_cpu.py)."""
        from biodemux_jl_amd.ranges import DynamicRange

        w, L = self.w, self.main_len
        return {"start": DynamicRange(WIN_K + 1, False, WIN_K + w, False), "end": DynamicRange(-(w - 1), True, 0, True),
                "mix": DynamicRange(-(L - WIN_K - 1), True, WIN_K + w, False)}[self.style]

    def barcodes(self):
        from biodemux_jl_amd import synth

        return synth.make_barcodes(self.n_bc, self.m, seed=1000 + self.m, min_hamming=self.min_hamming)

    def config(self):
        from biodemux_jl_amd import DemuxConfig

        bcs = self.barcodes()
        return DemuxConfig(bc_seqs=bcs, bc_lengths_no_N=[self.m] * self.n_bc, ids=[f"bc{i + 1}" for i in range(self.n_bc)], max_error_rate=RATE,
                           ref_search_range=self.range())

    def window(self, n: int):
        """(first, last), 1-based, of a read of n bases; empty: last < first."""
        from biodemux_jl_amd import resolve

        return resolve(self.range(), n)

    def batch(self, which: str):
        """(seq bytes, offsets, planned read length) of the main or the edge batch."""
        if which == "main":
            from biodemux_jl_amd import synth

            first, last = self.window(self.main_len)
            seq, off, _ = synth.make_reads(self.barcodes(), self.n_main, read_len=self.main_len, seed=7200 + self.m * 31 + self.rw + self.nv,
                                           plant_lo=first - 1, plant_hi=last - self.m - 2)
            return seq, off, self.main_len
        seq, off, _ = self.edge_batch()
        return seq, off, self.edge_len

    def edge_batch(self):
        """(seq bytes, offsets, kind of every read) of the edge batch."""
        return win_edge_reads(self.barcodes(), int(RATE * self.m), self.window, self.edge_len, self.n_edge, 8200 + self.m * 31 + self.rw + self.nv, self.kinds)

    def case(self, name: str, shapes, w=None):
        """The driver case (tests/call_cases.py) of this recipe's config — or of the same config with a window of `w`
        columns — for calls of (n_reads, planned read length), in order on one context."""
        import call_cases as CC
        import plan_cases as PC

        r = self.range() if w is None else WinRecipe._with_w(self, w).range()
        return CC.CallCase(name, None, [CC.call(n, L, wanted=WANT_VERDICT) for n, L in shapes],
                           passes=[PC.one_pass(self.barcodes(), ref=(r.start_offset, r.end_offset, int(r.start_from_end), int(r.end_from_end)))],
                           rate=RATE, tune={SWITCHES[k]: int(v) for k, v in self.env.items()})

    @staticmethod
    def _with_w(rc, w):
        other = WinRecipe(rc.target)
        other.w = w
        other.main_len = other.edge_len = 2 * w + 1
        return other


def win_edge_reads(bcs, kb: int, window, planned: int, n: int, seed: int, kinds, k_front: int = WIN_K, spread: int = 40, second=None):
    """Hand-planted reads at the edges of a window-mode cell, cycling through `kinds`.  window(n) is the 1-based column window
    (first, last) of a read of n bases.  Most reads have the planned length, the others a random shorter one, so that the
    window's first byte takes every 16-byte phase within the batch.  The kinds, all relative to the read's own window:
      win_first / win_last: a barcode from the window's first column / to its last;  win_before1 / win_after1: the same, one
      column outside;  win_outside: a barcode wholly outside the window (the oracle leaves the read unassigned unless chance
      has it);  straddle16: a barcode across a 16-byte boundary of the batch's bytes inside the window;  sub_kb / sub_kb1: a copy
      at the budget / one beyond it;  two_exact: two different barcodes;  short: a read shorter than every barcode;  empty: no
      bases;  with_N: N inside the window;  N_out: N outside it only;  none: no barcode;  clipped: a read shorter than the window
      (which ends with the read);  before_start: a read of at most WIN_K bases (shorter than the start of a window counted from
      the start: an empty window);  long2x: a read longer than twice the planned length;  long_ends: a read a barcode and up to 8
      bases longer than planned, with one barcode behind its first k_front columns and another in its last columns: a window
      counted from the end holds the second only where it is counted from the read's own end, and a window whose start is
      counted from the end leaves the first out only there (at the planned length it would hold it).
    The general forms' recipes use it too (k_front: the columns in front of their window; spread: how far below `planned`, there
    the longest read, the other lengths go).  second = (barcodes of pass 2, its window function) for dual configs:
      p2_only: a barcode of pass 2 inside its window and none of pass 1;  both: one of each pass, inside their windows, pass 1
      in the read's first half and pass 2 in its second;
    and every other kind gets a barcode of pass 2 half of the time, where it does not overlap what the kind planted.
    Read 0 has the planned length.  Returns (seq bytes, offsets, kind per read)."""
    import numpy as np

    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    m = min(len(b) for b in bcs)
    w_planned = window(planned)[1] - window(planned)[0] + 1

    def rand(k):
        return acgt[rng.integers(0, 4, size=k)].copy()

    def arr(b):
        return np.frombuffer(b.encode(), dtype=np.uint8)

    def mutated(b, d):
        s = arr(b).copy()
        for j in rng.choice(len(s), size=min(d, len(s)), replace=False):
            s[j] = acgt[(int(np.flatnonzero(acgt == s[j])[0]) + 1 + int(rng.integers(0, 3))) & 3]
        return s

    reads, names = [], []
    pos = 0  # the read's offset in the batch
    for i in range(n):
        kind = kinds[i % len(kinds)]
        if kind == "long2x":
            L = int(rng.integers(2 * planned + 1, 3 * planned + 1))
        elif kind == "long_ends":
            L = planned + m + int(rng.integers(0, 9))
        elif kind == "clipped":
            L = int(rng.integers(m + k_front, max(w_planned, m + k_front + 1)))
        elif kind == "before_start":
            L = int(rng.integers(1, k_front + 1))
        elif kind == "short":
            L = int(rng.integers(1, m))
        elif kind == "empty":
            L = 0
        else:
            L = planned if (i == 0 or rng.random() < 0.8) else int(rng.integers(max(planned - spread, m), planned))
        r = rand(L)
        first, last = window(L) if L > 0 else (1, 0)
        lo, wl = first - 1, last - first + 1  # the window, 0-based: [lo, lo + wl)
        bi = int(rng.integers(0, len(bcs)))
        bb = arr(bcs[bi])
        fits = wl >= len(bb)
        inside = lo + int(rng.integers(0, wl - len(bb) + 1)) if fits else 0
        before = r.copy()
        if kind == "long_ends":
            r[k_front: k_front + len(bb)] = bb
            b2 = arr(bcs[(bi + 1) % len(bcs)])
            r[L - len(b2):] = b2
        elif kind in ("short", "empty", "before_start", "none", "p2_only") or not fits:
            pass
        elif kind == "both":  # (pass 1 in the first half of the read where its window reaches that far)
            hi = min(lo + wl, max(L // 2, lo + len(bb))) - len(bb)
            at = lo + int(rng.integers(0, hi - lo + 1))
            r[at: at + len(bb)] = bb
        elif kind == "win_first":
            r[lo: lo + len(bb)] = bb
        elif kind == "win_last":
            r[lo + wl - len(bb): lo + wl] = bb
        elif kind == "win_before1":
            at = max(lo - 1, 0)
            r[at: at + len(bb)] = bb
        elif kind == "win_after1":
            at = min(lo + wl - len(bb) + 1, L - len(bb))
            r[at: at + len(bb)] = bb
        elif kind == "win_outside":
            if lo >= len(bb):
                at = int(rng.integers(0, lo - len(bb) + 1))
                r[at: at + len(bb)] = bb
            elif L - (lo + wl) >= len(bb):
                at = int(rng.integers(lo + wl, L - len(bb) + 1))
                r[at: at + len(bb)] = bb
        elif kind == "straddle16":  # (a slot holds the batch's bytes as they are, aligned: the boundary is one of the batch, at pos + at)
            k = int(rng.integers(0, max(1, (wl - len(bb)) // 16)))
            at = 16 * ((pos + lo + len(bb) // 2 + 15) // 16 + k) - len(bb) // 2 - pos
            at = min(max(lo, at), lo + wl - len(bb))
            r[at: at + len(bb)] = bb
        elif kind in ("sub_kb", "sub_kb1"):
            r[inside: inside + len(bb)] = mutated(bcs[bi], kb if kind == "sub_kb" else kb + 1)
        elif kind == "two_exact":
            b2 = arr(bcs[(bi + 1) % len(bcs)])
            if wl >= len(bb) + len(b2):
                at = lo + int(rng.integers(0, wl - len(bb) - len(b2) + 1))
                r[at: at + len(bb)] = bb
                at2 = int(rng.integers(at + len(bb), lo + wl - len(b2) + 1))
                r[at2: at2 + len(b2)] = b2
            else:
                r[inside: inside + len(bb)] = bb
        elif kind == "with_N":
            r[inside: inside + len(bb)] = bb
            r[lo + rng.choice(wl, size=min(3, wl), replace=False)] = ord("N")
        elif kind == "N_out":
            r[inside: inside + len(bb)] = bb
            out = np.r_[0:lo, lo + wl:L]
            if len(out):
                r[rng.choice(out, size=min(3, len(out)), replace=False)] = ord("N")
        else:
            assert kind in ("clipped", "long2x"), kind
            r[inside: inside + len(bb)] = bb
        if second is not None and L > 0 and (kind in ("p2_only", "both") or rng.random() < 0.5):
            f2, l2 = second[1](L)
            b2 = arr(second[0][int(rng.integers(0, len(second[0])))])
            lo2 = max(f2 - 1, L // 2) if l2 - max(f2 - 1, L // 2) >= len(b2) else f2 - 1  # (in the second half where the window reaches it)
            if l2 - lo2 >= len(b2):
                at = lo2 + int(rng.integers(0, l2 - lo2 - len(b2) + 1))
                if kind in ("p2_only", "both") or (r[at: at + len(b2)] == before[at: at + len(b2)]).all():
                    r[at: at + len(b2)] = b2
        reads.append(r)
        names.append(kind)
        pos += len(r)
    assert len(reads[0]) == planned
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate(reads).astype(np.uint8), off, names


# -- the general forms (GEN = true, KEND = 0): dual configs and configs with a ref_search_range that window mode turns down;
# non-split: known-score (bdx_launch_wave_gen in bdx_wave_end.hip), split: weighted costs (indel = 2), ranged only
# (bdx_launch_wave_split_gen in bdx_pairs.hip).  One instantiation serves several argument states; the six (TF, Q) of every
# (RW, NV) take them in turn, so that every state runs at every RW and both NV.
GEN_STATES = {False: ("dual_whole", "ranged_flat", "ranged_scan", "dual_ranged"), True: ("ranged_flat", "ranged_scan", "dual_ranged")}
GEN_K = 10  # columns in front of a ranged_flat window ("11:end-10")
GEN_KINDS = ("win_first", "win_last", "win_before1", "win_after1", "win_outside", "straddle16", "sub_kb", "sub_kb1", "two_exact", "short", "empty",
             "with_N", "N_out", "none", "clipped", "before_start")
GEN_DUAL_KINDS = GEN_KINDS + ("p2_only", "both")
# (SPLIT, RW, NV, TF, Q) -> the cell [low, high] in bases of the longest read as the planner gives it for the recipe's config at
# its batch size on one CU, and the shortest read of the cell with scan_gpr > 0 (0: none); "forced": no read length of
# 1..MAX_LEN reaches the tile size by the planner's own choice, BDX_WAVE_RW sets it (test_kernel_lattice_cpu.py holds every
# number against the driver).  To re-derive the table after a planner retune: plan GenRecipe(target, cell=(1, top, 0)).case over
# every read length of 1..MAX_LEN at n_edge reads, without and then with force_rw; a cell is the last unbroken run of lengths whose
# whole-batch wave launch wave_name spells as the target (forced where the plain sweep finds none); repeat once with the cell's own
# top, from which ranged_scan takes its window; scan_low is the first length of the run whose wfront / wfull line has scan_gpr > 0.
# WIN_CELLS likewise: a window of w columns behind 8, planned at 2 w + 1 bases, w = 1..300
_GEN_CELLS = {
    (0, 8, 5, 0, 6): (1, 632, 0, "forced"), (0, 8, 5, 0, 7): (1, 632, 0, "forced"), (0, 8, 5, 0, 8): (600, 632, 600), (0, 8, 5, 12, 7): (1, 632, 0, "forced"),
    (0, 8, 5, 12, 8): (598, 632, 0), (0, 8, 5, 20, 8): (576, 632, 0), (0, 8, 10, 0, 6): (637, 1272, 0), (0, 8, 10, 0, 7): (637, 1272, 0),
    (0, 8, 10, 0, 8): (633, 1272, 938), (0, 8, 10, 12, 7): (637, 1272, 0), (0, 8, 10, 12, 8): (633, 1272, 0), (0, 8, 10, 20, 8): (633, 1272, 0),
    (0, 16, 5, 0, 6): (41, 316, 0, "forced"), (0, 16, 5, 0, 7): (288, 316, 0), (0, 16, 5, 0, 8): (202, 316, 252), (0, 16, 5, 12, 7): (266, 316, 0),
    (0, 16, 5, 12, 8): (200, 316, 0), (0, 16, 5, 20, 8): (190, 316, 0), (0, 16, 10, 0, 6): (319, 636, 0), (0, 16, 10, 0, 7): (317, 636, 0),
    (0, 16, 10, 0, 8): (317, 599, 458), (0, 16, 10, 12, 7): (317, 636, 0), (0, 16, 10, 12, 8): (317, 597, 0), (0, 16, 10, 20, 8): (317, 575, 0),
    (0, 32, 5, 0, 6): (41, 158, 0), (0, 32, 5, 0, 7): (1, 158, 0), (0, 32, 5, 0, 8): (1, 158, 138), (0, 32, 5, 12, 7): (1, 158, 0),
    (0, 32, 5, 12, 8): (41, 158, 0), (0, 32, 5, 20, 8): (1, 158, 0), (0, 32, 10, 0, 6): (159, 318, 0), (0, 32, 10, 0, 7): (159, 287, 0),
    (0, 32, 10, 0, 8): (159, 201, 183), (0, 32, 10, 12, 7): (159, 265, 0), (0, 32, 10, 12, 8): (159, 199, 0), (0, 32, 10, 20, 8): (159, 189, 0),
    (1, 8, 5, 0, 6): (1, 632, 0, "forced"), (1, 8, 5, 0, 7): (1, 632, 480, "forced"), (1, 8, 5, 0, 8): (571, 632, 0), (1, 8, 5, 12, 7): (1, 632, 0, "forced"),
    (1, 8, 5, 12, 8): (592, 632, 592), (1, 8, 5, 20, 8): (590, 632, 0), (1, 8, 10, 0, 6): (637, 1272, 0), (1, 8, 10, 0, 7): (637, 1272, 938),
    (1, 8, 10, 0, 8): (633, 1272, 0), (1, 8, 10, 12, 7): (637, 1272, 0), (1, 8, 10, 12, 8): (633, 1272, 938), (1, 8, 10, 20, 8): (633, 1272, 0),
    (1, 16, 5, 0, 6): (1, 316, 0, "forced"), (1, 16, 5, 0, 7): (292, 316, 292), (1, 16, 5, 0, 8): (182, 316, 0), (1, 16, 5, 12, 7): (291, 316, 0),
    (1, 16, 5, 12, 8): (195, 316, 252), (1, 16, 5, 20, 8): (194, 316, 0), (1, 16, 10, 0, 6): (319, 636, 0), (1, 16, 10, 0, 7): (317, 636, 480),
    (1, 16, 10, 0, 8): (317, 570, 0), (1, 16, 10, 12, 7): (317, 636, 0), (1, 16, 10, 12, 8): (317, 591, 458), (1, 16, 10, 20, 8): (317, 589, 0),
    (1, 32, 5, 0, 6): (1, 158, 0), (1, 32, 5, 0, 7): (1, 158, 138), (1, 32, 5, 0, 8): (1, 158, 0), (1, 32, 5, 12, 7): (1, 158, 0),
    (1, 32, 5, 12, 8): (1, 158, 138), (1, 32, 5, 20, 8): (1, 158, 0), (1, 32, 10, 0, 6): (159, 318, 0), (1, 32, 10, 0, 7): (159, 291, 252),
    (1, 32, 10, 0, 8): (159, 181, 0), (1, 32, 10, 12, 7): (159, 290, 0), (1, 32, 10, 12, 8): (159, 194, 183), (1, 32, 10, 20, 8): (159, 193, 0),
}
GEN_CELLS = {spell("bdx_wave_kernel", dict(RW=k[1], TF=k[3], NV=k[2], Q=k[4], SPLIT=bool(k[0]), KB=0, NW=0, MG=False, KEND=0, GEN=True, WINM=False)): v
             for k, v in _GEN_CELLS.items()}


class GenRecipe:
    """One deterministic case for a general-form instantiation `target`: the barcode set of its (TF, Q) (WAVE_TFQ; dual: a
    second set of the same shape, half of the barcodes in either) at RATE, in the argument state `state`:
      dual_whole   two passes, whole ranges;
      ranged_flat  one pass, "11:end-10": a window window mode turns down (longer than half the read), the whole flat image scanned;
      ranged_scan  one pass, "1:W" with W just above half the longest read of the cell: the seed scan walks only the
                   groups of sixteen positions over the window (scan_gpr > 0 in the planner's wfront / wfull line);
      dual_ranged  two passes, "1:W" and "end-(W-1):end" with W a third of that length.
    Two batches of TILES x RW + 1 reads and more, as Recipe's: main at the shortest read length of the cell that holds the
    barcodes with flanks (ranged_scan: and has scan_gpr > 0), edge (win_edge_reads) up to the longest."""

    def __init__(self, target, cell=None, force_rw=False):
        fam, a = parse(target)
        self.target, self.rw, self.nv, self.split = target, a["RW"], a["NV"], a["SPLIT"]
        self.m, self.min_hamming, self.n_bc = WAVE_TFQ[(a["TF"], a["Q"])]
        states = GEN_STATES[self.split]
        self.state = states[list(WAVE_TFQ).index((a["TF"], a["Q"])) % len(states)]
        self.dual = self.state.startswith("dual")
        if self.dual:  # half the set per pass: as many barcodes in all, and as many chance seed hits per read, as a single pass has
            self.n_bc //= 2
        self.kw = {"indel": 2} if self.split else {}
        self.want_pass = False
        top = (self.nv * 1024 - 64) // self.rw  # the span bound of the (RW, NV) cell (size_wave: rw x len + 64 <= NV KiB)
        self.n_main = max(TILES + 8, 512 // self.rw + 8) * self.rw + 1
        self.n_edge = max(TILES, 512 // self.rw) * self.rw + 1
        cell = cell or GEN_CELLS.get(target)
        self.low, self.high, self.scan_low = cell[:3] if cell else (None, top, None)
        # (ranged_scan: just above half the cell's longest read, which the LDS budget may hold below the span bound)
        self.w = self.high // 2 + 1 if self.state == "ranged_scan" else max(self.m + 8, top // 3)
        forced = force_rw or (cell is not None and len(cell) == 4)
        self.env = dict({"BDX_CU_COUNT": "1"}, **({"BDX_WAVE_RW": str(self.rw)} if forced else {}))
        self.forced_why = (f"no read length of 1..{MAX_LEN} bases reaches RW {self.rw} / NV {self.nv} with the planner's own choice at {self.n_edge} reads on "
                           f"one CU (size_wave, bdx_call.cpp): BDX_WAVE_RW sets the tile.  The sweep varies the read length only, at this batch size: a stated "
                           f"limit of the recipe, not a proof that no batch reaches the cell") if forced else None
        if cell:
            self.edge_len = self.high
            flanks = (2 * self.m + 24) if self.dual else (self.m + 40)
            self.main_len = min(max(self.low, flanks, self.scan_low if self.state == "ranged_scan" else 0), self.high)
        # reads the target may hand on per batch of n: a quarter (measured: at most 251 of 1281, the reads of the edge kinds that no
        # wave kernel answers).  Where a read of the cell's longest length expects more than 4 chance seed hits (pieces x
        # positions / 4^Q) the hit queue, which size_wave sizes per 150 bases at 6 entries per read, overflows and the tile hands
        # its reads on by design (Recipe.list_div's reason): the 1272-base cells of Q = 6 (4.97 hits; measured 176 of 513: half)
        # and of the 14-nt set in two ranged passes (4.94 hits and the survivors of pass 1; measured 288 of 513: two thirds)
        kb = int(RATE * self.m)
        hits = (self.n_bc * (2 if self.dual else 1) * (kb + 1)) * (self.high - a["Q"] + 1) / 4.0 ** a["Q"] if cell else 0.0
        self.list_div = (1.5 if self.dual else 2) if hits > 4 else 4
        self.kinds = GEN_DUAL_KINDS if self.dual else GEN_KINDS
        self.k_front = GEN_K if self.state == "ranged_flat" else 0

    def range_strs(self):
        """The ref_search_range of pass 1 and of pass 2 (None: the whole read)."""
        w = self.w
        return {"dual_whole": (None, None), "ranged_flat": (f"{GEN_K + 1}:end-{GEN_K}", None), "ranged_scan": (f"1:{w}", None),
                "dual_ranged": (f"1:{w}", f"end-{w - 1}:end")}[self.state]

    def ranges(self):
        from biodemux_jl_amd import parse_dynamic_range

        return tuple(parse_dynamic_range(s or "1:end") for s in self.range_strs())

    def window(self, n: int, p: int = 0):
        from biodemux_jl_amd import resolve

        return resolve(self.ranges()[p], n)

    def barcodes(self, p: int = 0):
        from biodemux_jl_amd import synth

        return synth.make_barcodes(self.n_bc, self.m, seed=1000 * (p + 1) + self.m, min_hamming=self.min_hamming)

    def config(self):
        from biodemux_jl_amd import DemuxConfig

        r1, r2 = self.ranges()
        more = {}
        if self.dual:
            more = dict(is_dual=True, bc_seqs2=self.barcodes(1), bc_lengths_no_N2=[self.m] * self.n_bc, ids2=[f"y{i + 1}" for i in range(self.n_bc)],
                        ref_search_range2=r2)
        return DemuxConfig(bc_seqs=self.barcodes(), bc_lengths_no_N=[self.m] * self.n_bc, ids=[f"bc{i + 1}" for i in range(self.n_bc)],
                           max_error_rate=RATE, ref_search_range=r1, **self.kw, **more)

    def batch(self, which: str):
        """(seq bytes, offsets, longest read) of the main or the edge batch."""
        if which == "main":
            from biodemux_jl_amd import synth

            L = self.main_len
            f1, l1 = self.window(L)
            second = None
            if self.dual:  # pass 1 in the first half of the read, pass 2 in the second
                l1 = min(l1, L // 2)
                f2, l2 = self.window(L, 1)
                second = (self.barcodes(1), max(f2 - 1, L // 2), max(l2 - self.m - 2, max(f2 - 1, L // 2)))
            seq, off, _ = synth.make_reads(self.barcodes(), self.n_main, read_len=L, seed=7300 + self.m * 31 + self.rw + self.nv + 7 * self.split,
                                           plant_lo=f1 - 1, plant_hi=max(l1 - self.m - 2, f1 - 1), second=second)
            return seq, off, L
        seq, off, _ = self.edge_batch()
        return seq, off, self.edge_len

    def edge_batch(self):
        """(seq bytes, offsets, kind of every read) of the edge batch."""
        second = (self.barcodes(1), lambda n: self.window(n, 1)) if self.dual else None
        return win_edge_reads(self.barcodes(), int(RATE * self.m), self.window, self.edge_len, self.n_edge,
                              8300 + self.m * 31 + self.rw + self.nv + 7 * self.split, self.kinds, k_front=max(self.k_front, 1),
                              spread=self.edge_len - self.m, second=second)

    def case(self, name: str, shapes, force=True):
        """The driver case (tests/call_cases.py) of this recipe's config for calls of (n_reads, longest read), in order on one
        context; force=False: without BDX_WAVE_RW."""
        import call_cases as CC
        import plan_cases as PC

        env = self.env if force else {"BDX_CU_COUNT": "1"}
        tup = lambda r: (r.start_offset, r.end_offset, int(r.start_from_end), int(r.end_from_end))  # noqa: E731
        r1, r2 = self.ranges()
        passes = [PC.one_pass(self.barcodes(), ref=tup(r1))] + ([PC.one_pass(self.barcodes(1), ref=tup(r2))] if self.dual else [])
        return CC.CallCase(name, None, [CC.call(n, L, wanted=WANT_VERDICT) for n, L in shapes], passes=passes, rate=RATE,
                           costs=(self.kw.get("match", 0), self.kw.get("mismatch", 1), self.kw.get("indel", 1)),
                           tune={dict(SWITCHES, BDX_WAVE_RW="wave_rw")[k]: int(v) for k, v in env.items()})


def _gen_recipe(name: str):
    fam, a = parse(name)
    if name not in GEN_CELLS or wave_form(name) not in ("false, 0, 0, false, 0, true, false", "true, 0, 0, false, 0, true, false"):
        return None
    return GenRecipe(name)


# -- the pairs mode (KB > 0; bdx_pairs.hip, bdx_wave_rev.hip, bdx_wave_aln.hip): tiered configs of 24-nt barcodes whose budget is
# too large for selective single seeds.  Tier 1 (a wave launch over the whole batch) lists the reads it cannot settle; the
# target walks that list, so its launch is a list launch.  Barcode counts give NW (64 / 96 / 128; 160: many groups, MG), the
# rate KB (0.15: 3, 0.2: 4; with indel = 2 the same-diagonal variants, 0.15: 8, 0.25: 9), the read length NV (slot bytes).
PAIRS_M = 24
PAIRS_N = 2001  # reads per batch: tier 1's list then holds two 16-read tiles per resident wave and more
PAIRS_CELLS = {3: (1, 177), 6: (178, 369)}  # NV -> the longest reads of the cell (size_pairs, bdx_call.cpp: 16 x slot + 16 <= 3 / 6 KiB + 16)
PAIRS_KINDS = TEN + INDEL + DIAG_KINDS + ("cut_front",)
PAIRS_SD_KINDS = TEN + INDEL + ("cut_front", "sd_gmax")  # the same-diagonal variants (sub_kb1 is their budget + 1)
# (NV, SPLIT, KB, NW, MG, KEND) of the cells whose edge batch takes a few reads more, and how many: at PAIRS_N reads tier 1's list
# came to a whole number of 16-read tiles (measured: 1408 or 1328 listed reads; 1168 for the same-diagonal cells, 1170 with three
# reads more), and the list-launch check asks for a ragged last tile.  Which reads tier 1 lists is the kernel's settle rule, which
# this module does not restate: the numbers are measured, and a change of tier 1 may ask for another entry
PAIRS_MORE = {(6, False, 3, 4, False, 1): 2, (3, False, 3, 2, False, 3): 1, (3, False, 3, 4, True, 0): 1, (6, False, 3, 3, False, 1): 1, (6, False, 3, 4, False, 3): 1,
              (6, True, 8, 3, False, 0): 3, (6, True, 9, 2, False, 0): 3, (6, True, 9, 3, False, 0): 3, (6, True, 9, 4, False, 0): 3}


class PairsRecipe:
    """One deterministic case for a pairs-mode instantiation `target`, its config read off the template arguments:
      KEND 0 known-score tiered; KEND 1 / 2 trim_side 5 / 3; KEND 3 trim_side 5 with summary = True (NW 2: the statistics
      tables are compared) or per-pass outputs (NW 3 / 4); SPLIT with KB 3 / 4 :hamming; KB 8 / 9 indel = 2 at rate 0.15 /
      0.25; MG 160 barcodes.
    Two batches of PAIRS_N reads: main with copies planted at stated distances (four reads in ten beyond tier 1's cap, three in
    ten without a barcode), edge from cell_edge_reads with the two-intact-pieces kinds on the mode's 4-base pieces."""

    def __init__(self, target):
        fam, a = parse(target)
        self.target, self.a = target, a
        self.nv, self.kb, self.nw, self.kend, self.split, self.mg = a["NV"], a["KB"], a["NW"], a["KEND"], a["SPLIT"], a["MG"]
        self.m = PAIRS_M
        self.n_bc = 160 if self.mg else {2: 64, 3: 96, 4: 128}[self.nw]
        self.rate = {3: 0.15, 4: 0.2, 8: 0.15, 9: 0.25}[self.kb]
        self.kw = {}
        if self.kb >= 8:
            self.kw["indel"] = 2
        elif self.split:
            self.kw["matching_algorithm"] = "hamming"
        if self.kend:
            self.kw["trim_side"] = 3 if self.kend == 2 else 5
        self.summary = self.kend == 3 and self.nw == 2
        if self.summary:
            self.kw["summary"] = True
        self.want_pass = self.kend == 3 and not self.summary
        self.low, self.high = PAIRS_CELLS[self.nv]
        self.edge_len = self.high
        self.edge_why = None
        if self.kb == 4 and self.nv == 6 and self.nw >= 3 and not self.split and not self.mg:
            # At kb 4 the mode flags ~31 chance pairs per 150 bases at 96 barcodes against a queue of 56 flags per read (size_pairs,
            # bdx_call.cpp): at the cell's longest reads (369 bases: ~76 flags with 96 barcodes, ~100 with 128) every tile runs its
            # queue over and is handed on whole (measured: 602..734 of 1412 listed reads at NW 3, 1352..1408 at NW 4), and the edge
            # kinds would be decided behind the target.  The edge batch stops where the queue still holds
            self.edge_len = 240 if self.nw == 3 else 195  # (195: one slot step, at 194 bases, still lies inside)
            self.edge_why = "the flag queue (56 per read, size_pairs in bdx_call.cpp) runs over beyond this length: longer reads are handed on whole"
        # (NV 6: just inside the cell.  The mode's flag queue holds 56 flags per read (size_pairs, bdx_call.cpp) against ~31 chance
        # flags per 150 bases at 96 barcodes and kb 4: a main batch of 300 bases runs every tile over and is handed on whole)
        self.main_len = 150 if self.nv == 3 else 180
        self.n_main = PAIRS_N
        self.n_edge = PAIRS_N + PAIRS_MORE.get((self.nv, self.split, self.kb, self.nw, self.mg, self.kend), 0)
        self.env = {"BDX_CU_COUNT": "1"}
        self.forced_why = None
        # the known forms answer the reads of their list themselves, all but a quarter (MG may run over its queue by design; split
        # forms hand every read with a candidate on)
        self.mid_div = None if (self.split or self.mg) else 4
        self.edge_mid_div = self.mid_div
        # (the two-intact-pieces kinds are built on kb + 2 pieces of 4 bases; the same-diagonal variants have six and eight pieces)
        self.kinds = PAIRS_KINDS if self.kb <= 4 else PAIRS_SD_KINDS

    def barcodes(self):
        from biodemux_jl_amd import synth

        return synth.make_barcodes(self.n_bc, self.m, seed=1024, min_hamming=8)

    def config(self):
        from biodemux_jl_amd import DemuxConfig

        bcs = self.barcodes()
        return DemuxConfig(bc_seqs=bcs, bc_lengths_no_N=[self.m] * self.n_bc, ids=[f"bc{i + 1}" for i in range(self.n_bc)], max_error_rate=self.rate,
                           **self.kw)

    def batch(self, which: str):
        """(seq bytes, offsets, longest read) of the main or the edge batch."""
        if which == "main":
            # three reads in ten without a barcode, four with a copy at a distance above tier 1's cap (3 .. budget, in turn), three
            # with one within it (0 .. 2); unit-cost semiglobal configs: every second copy trades a substitution for an indel
            import numpy as np

            rng = np.random.default_rng(7400 + self.kb * 31 + self.nw + self.kend + self.nv)
            acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
            bcs = self.barcodes()
            budget = int(self.rate * self.m)
            unit = not self.kw.get("indel") and "matching_algorithm" not in self.kw
            seq = acgt[rng.integers(0, 4, size=self.n_main * self.main_len)].copy()
            for i in range(self.n_main):
                if i % 10 < 3:
                    continue
                d = 3 + (i // 10) % (budget - 2) if i % 10 < 7 else (i // 10) % 3
                rows = _spread_rows(rng, self.m, d)
                ops = ["sub"] * d
                if unit and d and i % 2:
                    ops[0] = "ins" if i % 4 == 1 else "del"
                s = _edited(rng, bcs[int(rng.integers(0, len(bcs)))], list(zip(rows, ops)))
                at = i * self.main_len + int(rng.integers(0, self.main_len - len(s) + 1))
                seq[at: at + len(s)] = s
            return seq, np.arange(self.n_main + 1, dtype=np.int64) * self.main_len, self.main_len
        seq, off, _ = self.edge_batch()
        return seq, off, self.edge_len

    def edge_batch(self):
        """(seq bytes, offsets, kind of every read) of the edge batch."""
        return cell_edge_reads(self.barcodes(), self.rate, self.edge_len, self.n_edge, 8400 + self.kb * 31 + self.nw + self.kend + self.nv, self.kinds)

    def case(self, name: str, shapes):
        """The driver case (tests/call_cases.py) of this recipe's config for calls of (n_reads, longest read) on one context."""
        import call_cases as CC
        import plan_cases as PC

        return CC.CallCase(name, None, [CC.call(n, L, wanted=WANT_ALL if self.want_pass else WANT_VERDICT, stats=int(self.summary)) for n, L in shapes],
                           passes=[PC.one_pass(self.barcodes(), trim=self.kw.get("trim_side") or 0)], rate=self.rate,
                           costs=(0, 1, self.kw.get("indel", 1)), algorithm=PC.HAMMING if "matching_algorithm" in self.kw else PC.SEMIGLOBAL,
                           summary=int(self.summary), tune=dict(n_cu=1))


class PairsExtra:
    """A further case on a pairs instantiation that already has its recipe: another argument state or entry route of the same
    form.  `dual`: C4's shape, 32 + 32 barcodes at rate 0.2 with the trim sides KEND asks for; `delta` = 0 plans carried passes
    (carry = 1) for a caller that wants the verdict alone, > 0 does not.  `route`: "split" = over tier 1's list (Middle::split,
    what the recipe itself runs), "all" = over the whole batch with no tier in front (Middle::all), "front" = as or behind a
    pairs tier 1 (Front::pairs: the KB 8 form runs over the whole batch in front, the KB 9 form over its list)."""

    def __init__(self, key, target, dual=False, trims=(0, 0), delta=0.0, want_pass=False, rate=0.2, indel=1, route="split", carry=0, force=None,
                 forced_why=None, whole=False):
        self.key, self.target, self.dual, self.trims, self.delta, self.want_pass = key, target, dual, trims, delta, want_pass
        self.rate, self.indel, self.route, self.carry, self.whole, self.forced_why = rate, indel, route, carry, whole, forced_why
        self.env = dict({"BDX_CU_COUNT": "1"}, **(force or {}))
        self.base = PairsRecipe(target)
        self.m, self.n, self.len = PAIRS_M, PAIRS_N, 150

    def barcodes(self, p: int = 0):
        from biodemux_jl_amd import synth

        return synth.make_barcodes(32, self.m, seed=1024 * (p + 1), min_hamming=8) if self.dual else self.base.barcodes()

    def config(self):
        from biodemux_jl_amd import DemuxConfig

        b1 = self.barcodes()
        kw = dict(max_error_rate=self.rate, min_delta=self.delta, indel=self.indel)
        if self.trims[0]:
            kw["trim_side"] = self.trims[0]
        if self.dual:
            b2 = self.barcodes(1)
            kw.update(is_dual=True, bc_seqs2=b2, bc_lengths_no_N2=[self.m] * len(b2), ids2=[f"y{i + 1}" for i in range(len(b2))])
            if self.trims[1]:
                kw["trim_side2"] = self.trims[1]
        return DemuxConfig(bc_seqs=b1, bc_lengths_no_N=[self.m] * len(b1), ids=[f"bc{i + 1}" for i in range(len(b1))], **kw)

    def batch(self, which: str):
        """(seq bytes, offsets, longest read): main from the synthetic generator with many edits (dual: pass 1 in the first 40
        columns, pass 2 from column 100), edge hand-planted (dual: win_edge_reads over the whole read with both passes)."""
        from biodemux_jl_amd import synth

        if which == "main":
            second = (self.barcodes(1), 100, 124) if self.dual else None
            seq, off, _ = synth.make_reads(self.barcodes(), self.n, read_len=self.len, seed=7500 + len(self.key), plant_frac=0.8, sub=0.07, ins=0.015,
                                           dele=0.015, plant_lo=0, plant_hi=40 if self.dual else None, second=second)
            return seq, off, self.len
        if self.dual:
            whole = lambda n: (1, n)  # noqa: E731
            seq, off, _ = win_edge_reads(self.barcodes(), int(self.rate * self.m), whole, self.len, self.n, 8500 + len(self.key), GEN_DUAL_KINDS, k_front=1,
                                         spread=self.len - self.m, second=(self.barcodes(1), whole))
        else:
            seq, off, _ = cell_edge_reads(self.barcodes(), self.rate, self.len, self.n, 8500 + len(self.key), self.base.kinds)
        return seq, off, self.len

    def case(self, name: str):
        import call_cases as CC
        import plan_cases as PC

        passes = [PC.one_pass(self.barcodes(), trim=self.trims[0])] + ([PC.one_pass(self.barcodes(1), trim=self.trims[1])] if self.dual else [])
        return CC.CallCase(name, None, [CC.call(self.n, self.len, wanted=WANT_ALL if self.want_pass else WANT_VERDICT)] * 2, passes=passes, rate=self.rate,
                           min_delta=self.delta, costs=(0, 1, self.indel), tune={SWITCHES[k]: int(v) for k, v in self.env.items()})


def _pairs_extras():
    t = "bdx_wave_kernel<16, 12, 3, 4, %s, %d, %d, false, %d, true, false>"
    out = []
    # the dual argument state of every KEND at NV 3 / KB 4 / NW 2; a caller that wants per-pass outputs (KEND 3) gets no carry
    for kend, trims, want in ((0, (0, 0), False), (1, (5, 5), False), (2, (5, 3), False), (3, (5, 3), True)):
        for delta in (0.0, 0.1):
            out.append(PairsExtra("dual_kend%d_delta%s" % (kend, delta), t % ("false", 4, 2, kend), dual=True, trims=trims, delta=delta, want_pass=want,
                                  carry=int(delta == 0.0 and not want)))
    # the entry routes of a KB 8 and a KB 9 cell (96 barcodes, indel = 2)
    kb8, kb9 = t % ("true", 8, 3, 0), t % ("true", 9, 3, 0)
    out.append(PairsExtra("kb8_split", kb8, rate=0.15, indel=2, route="split"))
    out.append(PairsExtra("kb8_all", kb8, rate=0.15, indel=2, delta=0.15, route="all", whole=True))
    out.append(PairsExtra("kb8_front", kb8, rate=0.25, indel=2, delta=0.15, route="front", whole=True))
    out.append(PairsExtra("kb9_split", kb9, rate=0.25, indel=2, route="split"))
    out.append(PairsExtra("kb9_all", kb9, rate=0.25, indel=2, route="all", whole=True, force={"BDX_NO_TIER": "1"},
                          forced_why="at rate 0.25 every plan of this config has a tier in front of the KB 9 set (bdx_plan.cpp / bdx_call.cpp: a wave tier without "
                                     "min_delta, a pairs tier with it): BDX_NO_TIER gives Middle::all"))
    out.append(PairsExtra("kb9_front", kb9, rate=0.25, indel=2, delta=0.15, route="front"))
    return out


PAIRS_EXTRAS = _pairs_extras()


def _pairs_recipe(name: str):
    fam, a = parse(name)
    if a["NV"] not in PAIRS_CELLS or a["KB"] not in (3, 4, 8, 9) or (a["RW"], a["TF"], a["Q"]) != (16, 12, 4):
        return None
    return PairsRecipe(name)


def _win_recipe(name: str):
    fam, a = parse(name)
    if (a["RW"], a["NV"]) not in WIN_CELLS or (a["TF"], a["Q"]) not in WAVE_TFQ:
        return None
    if wave_form(name) != "false, 0, 0, false, 0, true, true":
        return None
    return WinRecipe(name)


@functools.lru_cache(maxsize=None)
def recipe(name: str):
    """The deterministic case of instantiation `name` (a Recipe, WinRecipe, GenRecipe, PairsRecipe or CellRecipe), or None when it has none yet
    (PENDING) or none can exist (UNREACHABLE)."""
    p = parse(name)
    if p is None or name in UNREACHABLE:
        return None
    if p[0] == "bdx_wave_kernel" and p[1]["WINM"]:
        return _win_recipe(name)
    if p[0] == "bdx_wave_kernel" and p[1]["KB"] > 0:
        return _pairs_recipe(name)
    if name in GEN_CELLS:
        return _gen_recipe(name)
    if p[0] == "bdx_wave_kernel":
        return _wave_recipe(name)
    if name in CELL_RECIPES:
        a, kw = CELL_RECIPES[name]
        return CellRecipe(name, *a, **kw)
    return None


# instantiations no config and batch can reach: name -> the planner condition that excludes it
UNREACHABLE = {}

# instantiations without a recipe yet, by exact name: reason -> names (frozen: an instantiation the code object gains later has
# neither a recipe nor an entry here and fails test_kernel_lattice_cpu.py).  Empty: every instantiation has a recipe.
PENDING = {}


def pending_reason(name: str):
    hits = [why for why, names in PENDING.items() if name in names]
    assert len(hits) <= 1, f"{name} is listed under {len(hits)} PENDING reasons"
    return hits[0] if hits else None
