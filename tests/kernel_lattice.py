"""The classify kernels of the built library, one template instantiation at a time: the code-object reader (shared with
test_geometry_fuzz_gpu.py), a parser from a kernel name to its named template arguments, the planner's selection rules
restated in Python, and recipe(name): a deterministic case whose whole-batch launch runs exactly that instantiation.

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


@functools.lru_cache(maxsize=None)
def recipe(name: str):
    """The deterministic case of instantiation `name` (a Recipe), or None when it has none yet (PENDING) or none can exist
    (UNREACHABLE)."""
    p = parse(name)
    if p is None or name in UNREACHABLE:
        return None
    if p[0] == "bdx_wave_kernel":
        return _wave_recipe(name)
    return None


# instantiations no config and batch can reach: name -> the planner condition that excludes it
UNREACHABLE = {}

# instantiations without a recipe yet, by exact name (frozen: an instantiation the code object gains later has neither a
# recipe nor an entry here and fails test_kernel_lattice_cpu.py).  Their configs (dual and ranged configs, the pairs tier,
# window mode, the fused filter, the general kernel) are not built by this module yet; the randomised families of
# test_gpu_parity.py / test_geometry_fuzz_gpu.py still check them where they draw them.
PENDING = {
    "fused filter: no recipe yet": (
        "bdx_bitpar_kernel<256, 128, false, false, 5, 0>",
        "bdx_bitpar_kernel<256, 128, false, false, 5, 1>",
        "bdx_bitpar_kernel<256, 128, true, false, 5, 0>",
        "bdx_bitpar_kernel<256, 128, true, false, 5, 1>",
        "bdx_bitpar_kernel<256, 16, false, false, 5, 0>",
        "bdx_bitpar_kernel<256, 16, false, false, 5, 1>",
        "bdx_bitpar_kernel<256, 16, false, false, 5, 2>",
        "bdx_bitpar_kernel<256, 16, true, false, 5, 0>",
        "bdx_bitpar_kernel<256, 16, true, false, 5, 1>",
        "bdx_bitpar_kernel<256, 16, true, false, 5, 2>",
        "bdx_bitpar_kernel<256, 16, true, true, 10, 0>",
        "bdx_bitpar_kernel<256, 16, true, true, 5, 0>",
        "bdx_bitpar_kernel<256, 256, false, false, 5, 0>",
        "bdx_bitpar_kernel<256, 256, false, false, 5, 1>",
        "bdx_bitpar_kernel<256, 256, true, false, 5, 0>",
        "bdx_bitpar_kernel<256, 256, true, false, 5, 1>",
        "bdx_bitpar_kernel<256, 32, false, false, 5, 0>",
        "bdx_bitpar_kernel<256, 32, false, false, 5, 1>",
        "bdx_bitpar_kernel<256, 32, false, false, 5, 2>",
        "bdx_bitpar_kernel<256, 32, true, false, 5, 0>",
        "bdx_bitpar_kernel<256, 32, true, false, 5, 1>",
        "bdx_bitpar_kernel<256, 32, true, false, 5, 2>",
        "bdx_bitpar_kernel<256, 32, true, true, 10, 0>",
        "bdx_bitpar_kernel<256, 32, true, true, 5, 0>",
        "bdx_bitpar_kernel<256, 4, true, true, 10, 0>",
        "bdx_bitpar_kernel<256, 4, true, true, 5, 0>",
        "bdx_bitpar_kernel<256, 64, false, false, 5, 0>",
        "bdx_bitpar_kernel<256, 64, false, false, 5, 1>",
        "bdx_bitpar_kernel<256, 64, false, false, 5, 2>",
        "bdx_bitpar_kernel<256, 64, true, false, 5, 0>",
        "bdx_bitpar_kernel<256, 64, true, false, 5, 1>",
        "bdx_bitpar_kernel<256, 64, true, false, 5, 2>",
        "bdx_bitpar_kernel<256, 8, true, true, 10, 0>",
        "bdx_bitpar_kernel<256, 8, true, true, 5, 0>",
    ),
    "general kernel: no recipe yet": (
        "bdx_generic_kernel<128, 0, false, false>",
        "bdx_generic_kernel<128, 0, true, false>",
        "bdx_generic_kernel<256, 0, false, false>",
        "bdx_generic_kernel<256, 0, true, false>",
        "bdx_generic_kernel<256, 24, false, false>",
        "bdx_generic_kernel<256, 24, true, false>",
        "bdx_generic_kernel<256, 24, true, true>",
        "bdx_generic_kernel<256, 32, false, false>",
        "bdx_generic_kernel<256, 32, true, false>",
        "bdx_generic_kernel<256, 32, true, true>",
        "bdx_generic_kernel<64, 0, false, false>",
        "bdx_generic_kernel<64, 0, true, false>",
    ),
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
