"""The classify kernels of the built library, one template instantiation at a time: the code-object reader (shared with
test_geometry_fuzz_gpu.py), a parser from a kernel name to its named template arguments, the planner's selection rules
restated in Python, and recipe(name): a deterministic case whose whole-batch launch runs exactly that instantiation.
The wave kernel's recipes (Recipe) follow the restated rules; the fused filter's and the exact kernel's (CellRecipe) state
their cells as numbers, which the planner itself confirms through tests/call_host.cpp.

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


def planned_launches(report, c: int = 0) -> list:
    """The classify launches the driver plans for call c of a case: dicts of kernel (spelt by the ladders above; the wave
    family: None), family, list, blocks, tile."""
    out = []
    for ln in report.launches(c):
        k = fused_name(ln["args"]) if ln["family"] == "bitpar" else generic_name(ln["args"]) if ln["family"] == "generic" else None
        out.append(dict(kernel=k, family=ln["family"], list=ln["list"], blocks=ln["blocks"], tile=ln["tile"]))
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
    return kind in ("sub_kb", "indel_kb", "ragged_last", "ins_kb", "del_kb", "read_m", "read_m_minus_kb", "read_m_plus_kb") or kind.startswith("row") or (
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
        if kind in ("col1", "last_col", "straddle16", "two_exact", "with_N"):
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


@functools.lru_cache(maxsize=None)
def recipe(name: str):
    """The deterministic case of instantiation `name` (a Recipe or a CellRecipe), or None when it has none yet (PENDING) or
    none can exist (UNREACHABLE)."""
    p = parse(name)
    if p is None or name in UNREACHABLE:
        return None
    if p[0] == "bdx_wave_kernel":
        return _wave_recipe(name)
    if name in CELL_RECIPES:
        a, kw = CELL_RECIPES[name]
        return CellRecipe(name, *a, **kw)
    return None


# instantiations no config and batch can reach: name -> the planner condition that excludes it
UNREACHABLE = {}

# instantiations without a recipe yet, by exact name (frozen: an instantiation the code object gains later has neither a
# recipe nor an entry here and fails test_kernel_lattice_cpu.py).  Their configs (dual and ranged configs, the pairs tier,
# window mode) are not built by this module yet; the randomised families of
# test_gpu_parity.py / test_geometry_fuzz_gpu.py still check them where they draw them.
PENDING = {
    "general (dual / ranged) form: no recipe yet": (
        "bdx_wave_kernel<16, 0, 10, 6, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 0, 10, 6, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 0, 10, 7, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 0, 10, 7, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 0, 10, 8, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 0, 10, 8, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 0, 5, 6, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 0, 5, 6, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 0, 5, 7, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 0, 5, 7, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 0, 5, 8, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 0, 5, 8, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 10, 7, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 10, 7, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 10, 8, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 10, 8, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 5, 7, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 5, 7, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 5, 8, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 5, 8, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 20, 10, 8, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 20, 10, 8, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 20, 5, 8, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<16, 20, 5, 8, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 0, 10, 6, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 0, 10, 6, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 0, 10, 7, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 0, 10, 7, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 0, 10, 8, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 0, 10, 8, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 0, 5, 6, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 0, 5, 6, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 0, 5, 7, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 0, 5, 7, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 0, 5, 8, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 0, 5, 8, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 12, 10, 7, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 12, 10, 7, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 12, 10, 8, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 12, 10, 8, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 12, 5, 7, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 12, 5, 7, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 12, 5, 8, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 12, 5, 8, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 20, 10, 8, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 20, 10, 8, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 20, 5, 8, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<32, 20, 5, 8, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 0, 10, 6, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 0, 10, 6, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 0, 10, 7, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 0, 10, 7, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 0, 10, 8, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 0, 10, 8, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 0, 5, 6, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 0, 5, 6, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 0, 5, 7, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 0, 5, 7, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 0, 5, 8, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 0, 5, 8, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 12, 10, 7, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 12, 10, 7, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 12, 10, 8, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 12, 10, 8, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 12, 5, 7, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 12, 5, 7, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 12, 5, 8, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 12, 5, 8, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 20, 10, 8, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 20, 10, 8, true, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 20, 5, 8, false, 0, 0, false, 0, true, false>",
        "bdx_wave_kernel<8, 20, 5, 8, true, 0, 0, false, 0, true, false>",
    ),
    "window mode: no recipe yet": (
        "bdx_wave_kernel<16, 0, 4, 6, false, 0, 0, false, 0, true, true>",
        "bdx_wave_kernel<16, 0, 4, 7, false, 0, 0, false, 0, true, true>",
        "bdx_wave_kernel<16, 0, 4, 8, false, 0, 0, false, 0, true, true>",
        "bdx_wave_kernel<16, 12, 4, 7, false, 0, 0, false, 0, true, true>",
        "bdx_wave_kernel<16, 12, 4, 8, false, 0, 0, false, 0, true, true>",
        "bdx_wave_kernel<16, 20, 4, 8, false, 0, 0, false, 0, true, true>",
        "bdx_wave_kernel<32, 0, 3, 6, false, 0, 0, false, 0, true, true>",
        "bdx_wave_kernel<32, 0, 3, 7, false, 0, 0, false, 0, true, true>",
        "bdx_wave_kernel<32, 0, 3, 8, false, 0, 0, false, 0, true, true>",
        "bdx_wave_kernel<32, 0, 7, 6, false, 0, 0, false, 0, true, true>",
        "bdx_wave_kernel<32, 0, 7, 7, false, 0, 0, false, 0, true, true>",
        "bdx_wave_kernel<32, 0, 7, 8, false, 0, 0, false, 0, true, true>",
        "bdx_wave_kernel<32, 12, 3, 7, false, 0, 0, false, 0, true, true>",
        "bdx_wave_kernel<32, 12, 3, 8, false, 0, 0, false, 0, true, true>",
        "bdx_wave_kernel<32, 12, 7, 7, false, 0, 0, false, 0, true, true>",
        "bdx_wave_kernel<32, 12, 7, 8, false, 0, 0, false, 0, true, true>",
        "bdx_wave_kernel<32, 20, 3, 8, false, 0, 0, false, 0, true, true>",
        "bdx_wave_kernel<32, 20, 7, 8, false, 0, 0, false, 0, true, true>",
    ),
    "pairs tier: no recipe yet": (
        "bdx_wave_kernel<16, 12, 3, 4, false, 3, 2, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 3, 2, false, 1, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 3, 2, false, 2, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 3, 2, false, 3, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 3, 3, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 3, 3, false, 1, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 3, 3, false, 2, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 3, 3, false, 3, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 3, 4, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 3, 4, false, 1, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 3, 4, false, 2, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 3, 4, false, 3, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 3, 4, true, 0, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 4, 2, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 4, 2, false, 1, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 4, 2, false, 2, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 4, 2, false, 3, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 4, 3, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 4, 3, false, 1, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 4, 3, false, 2, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 4, 3, false, 3, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 4, 4, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 4, 4, false, 1, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 4, 4, false, 2, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 4, 4, false, 3, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, false, 4, 4, true, 0, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, true, 3, 2, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, true, 3, 3, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, true, 3, 4, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, true, 4, 2, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, true, 4, 3, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, true, 4, 4, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, true, 8, 2, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, true, 8, 3, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, true, 8, 4, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, true, 9, 2, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, true, 9, 3, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 3, 4, true, 9, 4, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 3, 2, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 3, 2, false, 1, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 3, 2, false, 2, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 3, 2, false, 3, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 3, 3, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 3, 3, false, 1, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 3, 3, false, 2, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 3, 3, false, 3, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 3, 4, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 3, 4, false, 1, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 3, 4, false, 2, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 3, 4, false, 3, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 3, 4, true, 0, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 4, 2, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 4, 2, false, 1, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 4, 2, false, 2, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 4, 2, false, 3, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 4, 3, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 4, 3, false, 1, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 4, 3, false, 2, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 4, 3, false, 3, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 4, 4, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 4, 4, false, 1, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 4, 4, false, 2, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 4, 4, false, 3, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, false, 4, 4, true, 0, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, true, 3, 2, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, true, 3, 3, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, true, 3, 4, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, true, 4, 2, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, true, 4, 3, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, true, 4, 4, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, true, 8, 2, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, true, 8, 3, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, true, 8, 4, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, true, 9, 2, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, true, 9, 3, false, 0, true, false>",
        "bdx_wave_kernel<16, 12, 6, 4, true, 9, 4, false, 0, true, false>",
    ),
}


def pending_reason(name: str):
    hits = [why for why, names in PENDING.items() if name in names]
    assert len(hits) <= 1, f"{name} is listed under {len(hits)} PENDING reasons"
    return hits[0] if hits else None
