"""Gzip members for the device inflate that zlib's encoder never writes: a DEFLATE writer that takes the code lengths,
the code-length sequence and the tokens as they are to be written (wrong ones included), a small multi-block reader
(`anatomy`) that says what a member's bytes hold, a model of the decoder's token groups and bit-window refills, and the
lists built from them: EDGE_GOOD (name -> predicate over the member's anatomy: the case reaches the edge it is named
for, read from its bytes and not from the writer's arguments), bad members with the status csrc/bdx_inflate_core.h gives
them, libdeflate members kept as data under tests/golden/inflate/ and a seeded generator of random dynamic blocks.
zlib is the arbiter when the lists are built: every good member gunzips to its text, every bad one is refused.

`python tests/inflate_edge_cases.py` prints one line per case (profiles/inflate_case_coverage.txt)."""
import functools
import glob
import gzip
import os
from collections import namedtuple

import numpy as np

import inflate_cases as IC
from inflate_cases import MEMBER_MAX, Bits, Member, trailer, wrap

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = os.path.join(HERE, "golden", "inflate")
GROUP = 128  # INF_GROUP
LROOT, DROOT, LTAB, DTAB = 9, 6, 852, 592
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
         16385, 24577]
DEXT = [0, 0, 0, 0] + [(s - 2) >> 1 for s in range(4, 30)]
ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


# ---- the writer ----
class W(Bits):
    """Bits that remembers where every field it wrote begins and ends: marks = [(kind, first bit, end bit)]"""

    def __init__(self):
        super().__init__()
        self.marks = []

    def pos(self):
        return len(self.out) * 8 + self.n

    def mark(self, kind, start):
        self.marks.append((kind, start, self.pos()))

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)


def canon(lengths):
    """canonical codes of a list of code lengths (None where the length is 0)"""
    cnt = [0] * 16
    for l in lengths:
        cnt[l] += 1
    cnt[0] = 0
    code, nxt = 0, [0] * 16
    for l in range(1, 16):
        code = (code + cnt[l - 1]) << 1
        nxt[l] = code
    codes = [None] * len(lengths)
    for s, l in enumerate(lengths):
        if l:
            codes[s] = nxt[l] & ((1 << l) - 1)
            nxt[l] += 1
    return codes


def len_sym(length):
    ls = 28 if length == 258 else max(i for i in range(28) if LBASE[i] <= length)
    return 257 + ls, length - LBASE[ls], LEXT[ls]


def dist_sym(dist):
    ds = max(i for i in range(30) if DBASE[i] <= dist)
    return ds, dist - DBASE[ds], DEXT[ds]


def put_tokens(b, tokens, ll, dd, eob=True):
    """tokens: a literal (int), a match (length, distance), or a field as it is: ("sym", s) the code of literal/length
    symbol s alone, ("dsym", s) of distance symbol s, ("bits", value, n) n bits LSB first"""
    lc, dc = canon(ll), canon(dd)

    def code(kind, codes, lens, s):
        p = b.pos()
        b.code(codes[s], lens[s])
        b.mark(kind, p)

    def bits(kind, v, n):
        p = b.pos()
        b.put(v, n)
        if n:
            b.mark(kind, p)

    for t in tokens:
        if isinstance(t, int):
            code("lit", lc, ll, t)
        elif t[0] == "sym":
            code("sym", lc, ll, t[1])
        elif t[0] == "dsym":
            code("dsym", dc, dd, t[1])
        elif t[0] == "bits":
            bits("bits", t[1], t[2])
        else:
            s, x, n = len_sym(t[0])
            code("lcode", lc, ll, s)
            bits("lextra", x, n)
            s, x, n = dist_sym(t[1])
            code("dcode", dc, dd, s)
            bits("dextra", x, n)
    if eob:
        code("eob", lc, ll, 256)


def stored_block(b, data=b"", final=False, length=None):
    b.put(int(final), 3)
    b.align()
    n = len(data) if length is None else length
    b.out += n.to_bytes(2, "little") + (n ^ 0xFFFF).to_bytes(2, "little") + data


def fixed_block(b, tokens, final=True, eob=True):
    b.put(int(final) | 1 << 1, 3)
    put_tokens(b, tokens, FIXED_LL, FIXED_D, eob)


def complete_cl(used):
    """19 code-length code lengths: a complete code over the symbols `used` (a second one joins a lone symbol)"""
    used = sorted(set(used))
    if len(used) == 1:
        used = sorted(used + [1 if used[0] == 0 else 0])
    k = len(used)
    p = (k - 1).bit_length()
    lens = [0] * 19
    for i, s in enumerate(used):
        lens[s] = p - 1 if i < 2 ** p - k else p
    return lens


def dynamic_block(b, ll_lengths, d_lengths, tokens, final, cl_sequence=None, cl_lengths=None, hclen=None, eob=True, hlit=None,
                  hdist=None):
    """a dynamic block as told: cl_sequence is the list of code-length symbols (sym, extra) — default one symbol per
    length, no repeats; whatever it expands to is what is written, right or wrong"""
    if cl_sequence is None:
        cl_sequence = [(l, 0) for l in list(ll_lengths) + list(d_lengths)]
    if cl_lengths is None:
        cl_lengths = complete_cl(s for s, _ in cl_sequence)
    if hclen is None:
        hclen = max([4] + [i + 1 for i in range(19) if cl_lengths[ORDER[i]]])
    b.put(int(final) | 2 << 1, 3)
    b.put(len(ll_lengths) - 257 if hlit is None else hlit, 5)
    b.put(len(d_lengths) - 1 if hdist is None else hdist, 5)
    b.put(hclen - 4, 4)
    for i in range(hclen):
        p = b.pos()
        b.put(cl_lengths[ORDER[i]], 3)
        b.mark("cl_len", p)
    cc = canon(cl_lengths)
    for s, x in cl_sequence:
        p = b.pos()
        b.code(cc[s], cl_lengths[s])
        b.mark("cl_sym", p)
        if s >= 16:
            p = b.pos()
            b.put(x, {16: 2, 17: 3, 18: 7}[s])
            b.mark("cl_extra%d" % s, p)
    put_tokens(b, tokens, list(ll_lengths), list(d_lengths), eob)


def expand(cl_sequence):
    out = []
    for s, x in cl_sequence:
        out += [s] if s < 16 else [out[-1]] * (3 + x) if s == 16 else [0] * ((3 if s == 17 else 11) + x)
    return out


def apply(tokens, prefix=b""):
    out = bytearray(prefix)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out)


def member(name, body, plain, plen=None):
    body = body.bytes() if isinstance(body, Bits) else body
    return Member(name, wrap(body, trailer(plain)), plain, len(plain) if plen is None else plen)


# ---- the reader ----
class Refused(Exception):
    pass


Block = namedtuple("Block", "bit btype final nl nd hclen cl_lens cl_syms ll_lens d_lens ll_max d_max tokens tok_bits eob_bit end_bit "
                            "stored pad used_ll used_d")


class _Reader:
    def __init__(self, body):
        self.b, self.pos, self.end = body, 0, len(body) * 8

    def peek(self, n, at=None):
        at = self.pos if at is None else at
        return (int.from_bytes(self.b[at >> 3:(at >> 3) + 4], "little") >> (at & 7)) & ((1 << n) - 1)

    def get(self, n):
        if self.pos + n > self.end:
            raise Refused("input")
        v = self.peek(n)
        self.pos += n
        return v

    def sym(self, h):
        cnt, syms = h
        v = self.peek(15)
        code = first = index = 0
        for l in range(1, 16):
            code |= v & 1
            v >>= 1
            c = cnt[l]
            if code - c < first:
                if self.pos + l > self.end:
                    raise Refused("input")
                self.pos += l
                return syms[index + code - first]
            index += c
            first = (first + c) << 1
            code <<= 1
        raise Refused("symbol")


def _huff(lengths, codes_type=False):
    """zlib's inflate_table rule: over-subscribed refused; incomplete refused but for a single one-bit code (never for
    the code-length code)"""
    cnt = [0] * 16
    for l in lengths:
        cnt[l] += 1
    cnt[0] = 0
    left = 1
    for l in range(1, 16):
        left = 2 * left - cnt[l]
        if left < 0:
            raise Refused("codes")
    mx = max(lengths) if len(lengths) else 0
    if left > 0 and mx > 0 and (codes_type or mx != 1):
        raise Refused("codes")
    return cnt, [s for l, s in sorted((l, s) for s, l in enumerate(lengths) if l)]


def anatomy(comp, strict=True):
    """the blocks of a member, read from its bytes -> (blocks, plain, why it was refused or None)"""
    r = _Reader(comp[IC.member_body(comp):len(comp) - 8])
    blocks, out = [], bytearray()
    try:
        while True:
            bit = r.pos
            final, bt = r.get(1), r.get(2)
            if bt == 3:
                raise Refused("btype")
            if bt == 0:
                pad = -r.pos % 8
                r.get(pad)
                n, nn = r.get(16), r.get(16)
                if n ^ 0xFFFF != nn:
                    raise Refused("stored")
                if r.pos + 8 * n > r.end:
                    raise Refused("input")
                out += r.b[r.pos >> 3:(r.pos >> 3) + n]
                r.pos += 8 * n
                blocks.append(Block(bit, 0, final, 0, 0, 0, (), (), (), (), 0, 0, (), (), r.pos, r.pos, n, pad, frozenset(), frozenset()))
            else:
                if bt == 1:
                    nl, nd, hclen, cl, cl_syms, ll, dd = 288, 32, 0, (), (), FIXED_LL, FIXED_D
                else:
                    nl, nd, hclen = r.get(5) + 257, r.get(5) + 1, r.get(4) + 4
                    if nl > 286 or nd > 30:
                        raise Refused("codes")
                    cl = [0] * 19
                    for i in range(hclen):
                        cl[ORDER[i]] = r.get(3)
                    h = _huff(cl, True)
                    lens, cl_syms = [], []
                    while len(lens) < nl + nd:
                        at, s, x = len(lens), r.sym(h), 0
                        if s < 16:
                            lens.append(s)
                        elif s == 16:
                            if not lens:
                                raise Refused("codes")
                            x = r.get(2)
                            lens += [lens[-1]] * (3 + x)
                        else:
                            x = r.get(3 if s == 17 else 7)
                            lens += [0] * ((3 if s == 17 else 11) + x)
                        cl_syms.append((s, x, at))
                    if len(lens) > nl + nd or lens[256] == 0:
                        raise Refused("codes")
                    ll, dd = lens[:nl], lens[nl:]
                hl, hd = _huff(ll), _huff(dd)
                tokens, tok_bits, used_ll, used_d = [], [], set(), set()
                while True:
                    p = r.pos
                    s = r.sym(hl)
                    used_ll.add(s)
                    if s == 256:
                        break
                    if s < 256:
                        out.append(s)
                        tokens.append(s)
                    else:
                        if s > 285:
                            raise Refused("symbol")
                        length = LBASE[s - 257] + r.get(LEXT[s - 257])
                        ds = r.sym(hd)
                        if ds > 29:
                            raise Refused("symbol")
                        dist = DBASE[ds] + r.get(DEXT[ds])
                        if dist > len(out):
                            raise Refused("distance")
                        used_d.add(ds)
                        for _ in range(length):
                            out.append(out[-dist])
                        tokens.append((length, dist))
                    tok_bits.append(p)
                blocks.append(Block(bit, bt, final, nl, nd, hclen, tuple(cl), tuple(cl_syms), tuple(ll), tuple(dd), max(ll), max(dd),
                                    tuple(tokens), tuple(tok_bits), p, r.pos, 0, 0, frozenset(used_ll), frozenset(used_d)))
            if final:
                break
        if (r.pos + 7) >> 3 != len(r.b):
            raise Refused("stray")
    except Refused as e:
        if strict:
            raise
        return blocks, bytes(out), str(e)
    return blocks, bytes(out), None


def _rev(v, n):
    return int(format(v, "0%db" % n)[::-1], 2) if n else 0


def subtables(lengths, root):
    """the second-level tables of a code set as the decoder lays them out: {root index: sub bits}, entries in all"""
    sub = {}
    for l, c in zip(lengths, canon(lengths)):
        if l > root:
            i = _rev(c, l) & ((1 << root) - 1)
            sub[i] = max(sub.get(i, 0), l - root)
    return sub, (1 << root) + sum(1 << sb for sb in sub.values())


# ---- a model of what lane 0 does with the tokens: its groups and the refills of its bit window ----
Group = namedtuple("Group", "block base n nbytes first")  # first: index of its first token in the block


def groups(blocks):
    """token groups by the rule of inf_ph_tokens: INF_GROUP tokens at most, and a match whose source reaches into its own
    group opens the next one"""
    out, res = 0, []
    for k, B in enumerate(blocks):
        if B.btype == 0:
            out += B.stored
            continue
        i, toks = 0, B.tokens
        while True:
            base, n, first = out, 0, i
            while n < GROUP and i < len(toks):
                t = toks[i]
                if isinstance(t, int):
                    out += 1
                else:
                    if n > 0 and out - t[1] + min(t) > base:
                        break
                    out += t[0]
                n += 1
                i += 1
            res.append(Group(k, base, n, out - base, first))
            if i == len(toks) and n < GROUP:
                break
    return res


def refill_model(blocks, lim):
    """The bit window of the token phases (inf_open / inf_refill, in body offsets) -> (switch, opens).  switch: where the
    window goes from 8-byte loads to single bytes, as (valid bits in the window at the first refill that loads single
    bytes, body bytes not loaded yet); None when the token phases never load 8 bytes at once.  opens: for every group,
    how many body bytes lie at and behind the byte its first token begins in."""
    state = {"fast": False, "switch": None}

    def refill(ip, cnt):
        if ip + 8 <= lim:
            state["fast"] = True
            return ip + ((63 - cnt) >> 3), cnt | 56
        if state["switch"] is None and state["fast"] and ip < lim and cnt <= 56:
            state["switch"] = (cnt, lim - ip)
        while cnt <= 56 and ip < lim:
            ip, cnt = ip + 1, cnt + 8
        return ip, cnt

    opens = []
    for g in groups(blocks):
        B = blocks[g.block]
        bits = list(B.tok_bits) + [B.eob_bit, B.end_bit]
        start = bits[g.first]
        opens.append(lim - (start >> 3))
        ip, cnt = refill(start >> 3, 0)
        cnt -= start & 7
        for j in range(g.first, min(g.first + g.n + 1, len(bits) - 1)):
            ip, cnt = refill(ip, cnt)
            assert ip * 8 - cnt == bits[j], "the model lost the bit position"
            cnt -= bits[j + 1] - bits[j]
    return state["switch"], opens


# ---- code sets ----
def kraft_fill(ls, maxl=15):
    """the lengths `ls` and what makes them a complete code, none longer than maxl"""
    rem = (1 << maxl) - sum(1 << (maxl - l) for l in ls)
    assert rem >= 0
    return sorted(list(ls) + [l for l in range(1, maxl + 1) if rem >> (maxl - l) & 1])


def ll_set(ls, nl=286, deepest=285):
    """code lengths `ls` (a complete multiset) dealt to literals, the end of block, length symbols; the longest to `deepest`"""
    ls = sorted(ls)
    pool = [65, 67, 71, 84, 10, 256, 78, 64] + list(range(97, 123)) + list(range(257, 285)) + list(range(128, 256)) \
        + list(range(11, 64)) + list(range(0, 10))
    pool += [s for s in range(286) if s not in pool]
    pool = [s for s in pool if s != deepest and s < nl]
    assert len(ls) - 1 <= len(pool) == len(set(pool))
    out = [0] * nl
    for s, l in zip(pool, ls[:-1]):
        out[s] = l
    out[deepest] = ls[-1]
    return out


def d_set(ls, nd=30, deepest=29):
    ls = sorted(ls)
    pool = [s for s in range(nd) if s != deepest]
    out = [0] * nd
    for s, l in zip(pool, ls[:-1]):
        out[s] = l
    out[deepest] = ls[-1]
    return out


def use_all(ll, dd, out_len, rng=None):
    """tokens that use every coded symbol of both sets once or more (distances as far as `out_len` bytes in front allow)"""
    lits = [s for s in range(min(256, len(ll))) if ll[s]]
    lens = [s for s in range(257, min(286, len(ll))) if ll[s]]
    dsts = [s for s in range(min(30, len(dd))) if dd[s]]
    toks = list(lits)
    if rng is not None:
        rng.shuffle(toks)
    toks = [int(t) for t in toks]
    out = out_len + len(toks)
    dsts = [s for s in dsts if DBASE[s] <= out]
    if lens and dsts:
        for k in range(max(len(lens), len(dsts))):
            ls, ds = lens[k % len(lens)], dsts[k % len(dsts)]
            length = 258 if ls == 285 else min(257, LBASE[ls - 257] + ((1 << LEXT[ls - 257]) - 1 if k & 1 else 0))
            dist = min(DBASE[ds] + ((1 << DEXT[ds]) - 1 if k & 2 else 0), out)
            toks.append((length, dist))
            out += length
            if rng is not None and lits:
                toks.append(int(lits[int(rng.integers(len(lits)))]))
                out += 1
    return toks


def rle(lengths, rng=None):
    """the code-length sequence of `lengths` with repeat symbols: the longest runs (rng None) or random ones"""
    seq, n, N = [], 0, len(lengths)
    while n < N:
        v, r = lengths[n], 1
        while n + r < N and lengths[n + r] == v:
            r += 1
        pick = (lambda lo, hi: hi) if rng is None else (lambda lo, hi: int(rng.integers(lo, hi + 1)))
        lazy = rng is not None and rng.random() < 0.3
        if v == 0 and r >= 11 and not lazy:
            k = pick(11, min(r, 138))
            seq.append((18, k - 11))
        elif v == 0 and r >= 3 and not lazy:
            k = pick(3, min(r, 10))
            seq.append((17, k - 3))
        elif n > 0 and lengths[n - 1] == v and r >= 3 and not lazy:
            k = pick(3, min(r, 6))
            seq.append((16, k - 3))
        else:
            k = 1
            seq.append((v, 0))
        n += k
    return seq


# ---- predicates ----
def _dyn(blocks):
    return [B for B in blocks if B.btype == 2]


def _lens_present(lengths):
    return {l for l in lengths if l}


def uses_every_length(B):
    return {B.ll_lens[s] for s in B.used_ll} == _lens_present(B.ll_lens) \
        and (not B.used_d or {B.d_lens[s] for s in B.used_d} == _lens_present(B.d_lens))


def crossing(B, sym):
    """the code-length symbols `sym` of B whose run begins in the literal/length alphabet and ends in the distance one"""
    return [(s, x, at) for s, x, at in B.cl_syms if s == sym and at < B.nl < at + (3 if s < 18 else 11) + x]


def header_phases(blocks, kinds=(1, 2)):
    return {B.bit % 8 for B in blocks if B.btype in kinds}


# ---- good members ----
def _head(n, seed):
    return IC.random_bytes(n, seed)


def _depth_member(name, ll_ls, d_ls, head=24577):
    ll, dd = ll_set(ll_ls), d_set(d_ls)
    w = W()
    pre = _head(head, 7)
    stored_block(w, pre)
    toks = use_all(ll, dd, head)
    dynamic_block(w, ll, dd, toks, True, cl_sequence=rle(ll + dd))
    return member(name, w, apply(toks, pre))


def chain(depth):
    return kraft_fill([depth, depth], depth)


def _cases():
    """[(Member, predicate(blocks, groups) -> bool)]"""
    C = []

    def add(m, pred):
        C.append((m, pred))

    # -- code depth --
    for L in (9, 10, 12, 15):
        add(_depth_member("ll_depth_%d" % L, chain(L), chain(6)),
            lambda bl, gs, L=L: (lambda B: B.ll_max == L and B.d_max == 6 and B.ll_lens[285] == L and 285 in B.used_ll
                                 and max(subtables(B.ll_lens, LROOT)[0].values(), default=0) == max(L - 9, 0) and uses_every_length(B))(bl[1]))
    for D in (6, 7, 15):
        add(_depth_member("d_depth_%d" % D, chain(9), chain(D)),
            lambda bl, gs, D=D: (lambda B: B.d_max == D and B.ll_max == 9 and B.d_lens[29] == D and 29 in B.used_d
                                 and max(subtables(B.d_lens, DROOT)[0].values(), default=0) == max(D - 6, 0) and uses_every_length(B))(bl[1]))
    mixed = kraft_fill([10] * 2 + [11] * 4 + [12] * 8 + [15, 15])
    add(_depth_member("ll_subtables_of_four_sizes", mixed, kraft_fill([7] * 2 + [8] * 4 + [15, 15])),
        lambda bl, gs: (lambda B: sorted(set(subtables(B.ll_lens, LROOT)[0].values())) == [1, 2, 3, 6] and len(subtables(B.ll_lens, LROOT)[0]) >= 4
                        and sorted(set(subtables(B.d_lens, DROOT)[0].values())) == [1, 2, 9] and uses_every_length(B)
                        and B.ll_lens[285] == 15 and B.d_lens[29] == 15 and 285 in B.used_ll and 29 in B.used_d)(bl[1]))
    deep_ll = kraft_fill([15] * 256)  # four full 64-entry sub-tables behind the root table: 768 of ltab's 852 entries
    add(_depth_member("deep_tables", deep_ll, chain(15)),
        lambda bl, gs: (lambda B: subtables(B.ll_lens, LROOT)[1] >= 768 and subtables(B.d_lens, DROOT)[1] == 576 and uses_every_length(B))(bl[1]))

    def shallow_probe():
        """root-only codes right after a deep set: its last code is all ones, the root index where the deep set had a link"""
        ll, dd = ll_set(chain(9), nl=257, deepest=66), d_set(chain(6), nd=8, deepest=7)
        toks = use_all(ll, dd, 0) * 3
        w = W()
        dynamic_block(w, ll, dd, toks, True)
        return member("shallow_probe", w, apply(toks))

    def probes_stale(deep, shallow, body):
        """tokens of `shallow` whose root index was a link of `deep`, in either table"""
        r = _Reader(body)
        links = set(subtables(deep.ll_lens, LROOT)[0])
        return sum(r.peek(LROOT, at) in links for at in list(shallow.tok_bits) + [shallow.eob_bit]) \
            and not subtables(shallow.ll_lens, LROOT)[0] and not subtables(shallow.d_lens, DROOT)[0]

    deep_member = C[-1][0]
    sp = shallow_probe()
    add(sp, lambda bl, gs: probes_stale(anatomy(deep_member.comp)[0][1], bl[0], sp.comp[IC.member_body(sp.comp):-8]))

    # -- alphabet sizes --
    def sizes(name, nl, nd, ll_ls, d_ls, pred, cl_lengths=None, seq=None, head=0, ll=None):
        ll = ll or ll_set(ll_ls, nl=nl, deepest=nl - 1 if nl > 257 else 256)
        dd = d_set(d_ls, nd=nd, deepest=nd - 1) if d_ls else [0] * nd
        w = W()
        pre = _head(head, 9)
        if head:
            stored_block(w, pre)
        toks = use_all(ll, dd, head)
        dynamic_block(w, ll, dd, toks, True, cl_sequence=seq(ll + dd) if seq else None, cl_lengths=cl_lengths)
        add(member(name, w, apply(toks, pre)), lambda bl, gs: pred(bl[-1]))

    sizes("nl_257_nd_1_hclen_5", 257, 1, [8] * 256, [], lambda B: (B.nl, B.nd, B.hclen) == (257, 1, 5) and not B.used_d and max(B.d_lens) == 0,
          seq=rle)  # (hclen 4 codes no length but 0: it cannot be a good member, see bad_edge_members)
    sizes("nl_286_nd_30_hclen_19", 286, 30, chain(15), chain(15),
          lambda B: (B.nl, B.nd, B.hclen) == (286, 30, 19) and B.ll_lens[285] == 15 and B.d_lens[29] == 15 and B.cl_lens[15] > 0
          and 285 in B.used_ll and 29 in B.used_d, seq=rle, head=24577)
    every_cl = [0] * 19
    for s, l in zip([0, 18, 17] + [s for s in range(1, 17)], [1, 2, 3] + [7] * 16):
        every_cl[s] = l

    ll_every = [0] * 286  # every length 2 .. 15, five 6s in a row, zero runs of 4, 15, 24, 65 and 130; the distance set has the 1
    for s, l in [(65, 2), (70, 2), (84, 3), (85, 3), (90, 4), (91, 4), (120, 5), (122, 7), (123, 8), (124, 9), (125, 10), (256, 11), (257, 12),
                 (258, 13), (259, 14), (284, 15), (285, 15)] + [(s, 6) for s in range(100, 105)]:
        ll_every[s] = l
    sizes("every_cl_symbol_cl_lengths_to_7", 286, 30, None, chain(15),
          lambda B: {s for s, _, _ in B.cl_syms} == set(range(19)) and max(B.cl_lens) == 7 and min(B.cl_lens) == 1 and B.hclen == 19,
          cl_lengths=every_cl, seq=rle, head=24577, ll=ll_every)

    # -- the code-length sequence --
    def clseq(name, ll, dd, seq, pred, toks=None):
        assert seq is None or expand(seq) == ll + dd, name
        toks = use_all(ll, dd, 0) if toks is None else toks
        w = W()
        dynamic_block(w, ll, dd, toks, True, cl_sequence=seq)
        add(member(name, w, apply(toks)), lambda bl, gs: pred(bl[0]))

    ll3 = [0] * 260
    for s in (65, 67, 71, 84, 256, 257, 258, 259):
        ll3[s] = 3
    d3 = [3] * 8
    seq16 = [(18, 65 - 11), (3, 0), (0, 0), (3, 0), (17, 0), (3, 0), (17, 10 - 3), (0, 0), (0, 0), (3, 0), (18, 138 - 11), (18, 33 - 11),
             (3, 0), (16, 3), (16, 2)]
    assert expand(seq16) == ll3 + d3

    def last_run_ends_at_the_end(B):
        s, x, at = B.cl_syms[-1]
        return s >= 16 and at + (3 if s < 18 else 11) + x == B.nl + B.nd

    clseq("cl16_crosses_and_ends_the_sequence", ll3, d3, seq16,
          lambda B: crossing(B, 16) == [(16, 3, 257)] and last_run_ends_at_the_end(B) and B.cl_syms[-1][:2] == (16, 2)
          and {(s, x) for s, x, _ in B.cl_syms} >= {(17, 0), (17, 7), (18, 127), (16, 3)})
    clseq("cl_same_lengths_no_repeats", ll3, d3, None, lambda B: all(s < 16 for s, _, _ in B.cl_syms) and len(B.cl_syms) == 268)
    ll17 = ll3[:260] + [0] * 10
    d17 = [0, 0, 0, 0, 1, 1]
    seq17 = seq16[:12] + [(3, 0), (3, 0), (3, 0), (3, 0), (17, 0), (17, 7), (0, 0), (1, 0), (1, 0)]
    clseq("cl17_crosses", ll17, d17, seq17, lambda B: crossing(B, 17) == [(17, 7, 263)] and (17, 0, 260) in B.cl_syms,
          toks=[65, 67, 71, 84, 65, 67, 71, 84, (3, 5), (4, 8), (5, 6), (3, 7)])
    ll18 = ll3[:260] + [0] * 26
    seq18 = seq16[:12] + [(3, 0), (3, 0), (3, 0), (3, 0), (18, 0), (18, 19 - 11), (1, 0), (1, 0)]
    clseq("cl18_crosses", ll18, d17, seq18, lambda B: crossing(B, 18) == [(18, 8, 271)] and (18, 0, 260) in B.cl_syms and B.nl == 286,
          toks=[65, 67, 71, 84, 65, 67, 71, 84, (3, 5), (4, 8), (5, 6), (3, 7)])
    clseq("cl16_repeats_3_and_6", ll3, d3, seq16[:13] + [(16, 0), (3, 0), (16, 3), (3, 0)],
          lambda B: [(s, x, at) for s, x, at in B.cl_syms if s == 16] == [(16, 0, 257), (16, 3, 261)] and not crossing(B, 16))

    # -- distance code forms --
    ll_lit = [0] * 257
    for s, l in ((65, 2), (67, 2), (84, 2), (71, 3), (256, 3)):
        ll_lit[s] = l
    clseq("no_distance_code", ll_lit, [0], rle(ll_lit + [0]), lambda B: B.nd == 1 and B.d_max == 0 and not B.used_d and len(B.tokens) == 40,
          toks=[65, 67, 71, 84] * 10)
    ll_m = [0] * 258
    for s, l in ((65, 2), (67, 2), (84, 2), (256, 3), (257, 3)):
        ll_m[s] = l
    clseq("one_distance_code_of_one_bit", ll_m, [1], rle(ll_m + [1]),
          lambda B: B.nd == 1 and B.d_lens == (1,) and B.used_d == {0} and (3, 1) in B.tokens, toks=[65, 67, (3, 1), 84, (3, 1)])
    eob_only = [0] * 256 + [1]

    def one_bit_eob(w, final):
        dynamic_block(w, eob_only, [0], [], final, cl_sequence=rle(eob_only + [0]))

    w = W()
    one_bit_eob(w, True)
    add(member("only_eob_one_bit_code_final", w, b""),
        lambda bl, gs: len(bl) == 1 and bl[0].tokens == () and bl[0].ll_lens[256] == 1 and bl[0].ll_max == 1 and sum(bl[0].ll_lens) == 1)
    w = W()
    one_bit_eob(w, False)
    one_bit_eob(w, False)
    fixed_block(w, list(b"ACGT"), False)
    one_bit_eob(w, False)
    stored_block(w, b"TGCA", True)
    add(member("only_eob_one_bit_code_in_front", w, b"ACGTTGCA"),
        lambda bl, gs: [B.btype for B in bl] == [2, 2, 1, 2, 0] and all(B.tokens == () and sum(B.ll_lens) == 1 for B in _dyn(bl))
        and len(header_phases(bl)) >= 3)

    # -- the overlap lattice --
    DIST = list(range(1, 41)) + [63, 64, 65, 127, 128, 129, 255, 256, 257]
    LENS = [3, 4, 5, 7, 8, 9, 63, 64, 65, 66, 127, 128, 129, 257, 258]
    rng = np.random.default_rng(77)
    lattice = [int(x) for x in rng.integers(0, 256, 257)]
    for d in DIST:
        for l in LENS:
            lattice += [(l, d), int(rng.integers(0, 256))]

    def is_lattice(B):
        pairs = {t for t in B.tokens if not isinstance(t, int)}
        return pairs == {(l, d) for l in LENS for d in DIST} \
            and all(isinstance(B.tokens[i + 1], int) for i, t in enumerate(B.tokens[:-1]) if not isinstance(t, int))

    w = W()
    fixed_block(w, lattice)
    add(member("overlap_lattice_fixed", w, apply(lattice)), lambda bl, gs: bl[0].btype == 1 and is_lattice(bl[0]))
    w = W()
    flat_ll, flat_d = [8] * 226 + [9] * 60, [4] * 2 + [5] * 28
    dynamic_block(w, flat_ll, flat_d, lattice, True, cl_sequence=rle(flat_ll + flat_d))
    add(member("overlap_lattice_dynamic", w, apply(lattice)), lambda bl, gs: bl[0].btype == 2 and is_lattice(bl[0]))

    # (a length of 258 written as symbol 284 with all five extra bits set, which no encoder does and zlib accepts)
    w = W()
    fixed_block(w, [65, ("sym", 284), ("bits", 31, 5), ("dsym", 0), 67])
    add(member("length_258_as_symbol_284", w, b"A" * 259 + b"C"),
        lambda bl, gs: bl[0].tokens == (65, (258, 1), 67) and 284 in bl[0].used_ll and 285 not in bl[0].used_ll)

    # -- group boundaries --
    for n in (127, 128, 129):
        lits = [int(x) for x in rng.integers(0, 256, n)]
        w = W()
        fixed_block(w, lits)
        add(member("literals_%d_then_eob" % n, w, bytes(lits)),
            lambda bl, gs, n=n: [g.n for g in gs] == ([n] if n < GROUP else [GROUP, n - GROUP]))
        w = W()
        toks = lits + [(4, 4), 65]
        fixed_block(w, toks)
        # (at 128 the match is the first token of its group and copies the last bytes of the group before)
        add(member("literals_%d_then_match" % n, w, apply(toks)),
            lambda bl, gs, n=n: [g.n for g in gs] == ([n, 2] if n <= GROUP else [GROUP, n - GROUP, 2])
            and not isinstance(bl[0].tokens[gs[-1].first], int) and gs[-1].base == n)
    for name, tok, stays in (("match_source_ends_at_group_base", (3, 4), True), ("match_source_one_past_group_base", (3, 3), False),
                             ("match_overlapping_itself_past_group_base", (5, 2), False)):
        w = W()
        stored_block(w, b"0123456789")
        toks = [120, tok, 121]
        fixed_block(w, toks)

        def pred(bl, gs, tok=tok, stays=stays):
            base, out = gs[0].base, gs[0].base + 1
            edge = out - tok[1] + min(tok)
            return base == 10 and edge == (base if stays else base + 1) and [g.n for g in gs] == ([3] if stays else [1, 2])

        add(member(name, w, apply(toks, b"0123456789")), pred)
    # the largest group there is: 127 matches of 258 bytes at distance 32768 behind a stored head of 32768 bytes read bytes
    # [0, 32766) — the 128th would read past the group's base only by ending beyond byte 65536, the largest member — and a
    # literal makes it 128 tokens, 32767 bytes; the next literal opens a group of its own
    head = _head(32768, 5)
    toks = [(258, 32768)] * 127 + [33, 34]
    w = W()
    stored_block(w, head)
    fixed_block(w, toks)
    add(member("largest_group_32767_bytes", w, apply(toks, head)),
        lambda bl, gs: [(g.n, g.nbytes) for g in gs] == [(128, 32767), (1, 1)] and gs[0].base == 32768)
    # the rule breaks a run of far matches: at distance 32510 behind 32510 bytes the 127th match reads 4 bytes of its group
    head = _head(32510, 6)
    toks = [(258, 32510)] * 128
    w = W()
    stored_block(w, head)
    fixed_block(w, toks)
    add(member("far_matches_until_the_rule_breaks", w, apply(toks, head)),
        lambda bl, gs: [(g.n, g.nbytes) for g in gs] == [(126, 126 * 258), (2, 516)])

    # -- bit phase --
    w = W()
    plain = b""
    for j in range(9):
        for k in range(j):  # 3 + 9 + 7 bits each: the next header is 3 bits further on, mod 8
            fixed_block(w, [200 + k], False)
            plain += bytes([200 + k])
        stored_block(w, b"<%d>" % j)
        plain += b"<%d>" % j
    stored_block(w, b"")  # LEN 0, not final
    fixed_block(w, [], False)
    one_bit_eob(w, False)
    stored_block(w, b"", True)  # LEN 0, final
    add(member("headers_at_every_bit_offset", w, plain),
        lambda bl, gs: header_phases(bl) == set(range(8)) and {B.pad for B in bl if B.btype == 0} == set(range(8))
        and {B.bit % 8 for B in bl if B.btype == 0} == set(range(8)) and header_phases(bl, (2,))
        and [(B.stored, B.final) for B in bl if B.btype == 0][-2:] == [(0, 0), (0, 1)])
    big = IC.fastq_text(65535, 14)
    w = W()
    stored_block(w, big, True)
    add(member("stored_len_65535", w, big), lambda bl, gs: [B.stored for B in bl] == [65535])

    # -- the end of the body: 16 bodies that differ by one trailing literal each (set_predicates says what they reach together;
    # the seed is one of those for which they reach it) --
    r479 = np.random.default_rng(479)
    pre = [int(x) for x in r479.integers(60, 230, int(r479.integers(117, 123)))]
    tail = [int(x) for x in r479.integers(100, 200, 16)]
    for k in range(16):
        toks = pre + tail[:k]
        w = W()
        fixed_block(w, toks)
        add(member("body_end_%02d" % k, w, bytes(toks)),
            lambda bl, gs, k=k: len(bl[0].tokens) == len(pre) + k and [g.n for g in gs][1:] == ([len(pre) + k - GROUP] if len(pre) + k >= GROUP else []))

    # -- many blocks in one member --
    text = IC.fastq_text(700, 15)
    w = W()
    for _ in range(3000):
        stored_block(w, b"")
    fixed_block(w, list(text))
    add(member("stored_3000_empty_then_text", w, text), lambda bl, gs: len(bl) == 3001 and all(B.stored == 0 and B.btype == 0 for B in bl[:3000]))
    m200 = many_code_sets()
    add(m200, lambda bl, gs: many_code_sets_pred(bl, m200.comp[IC.member_body(m200.comp):-8]))
    return C


def many_code_sets(n_blocks=200, seed=2024):
    """dynamic blocks with a different code set each, deep and shallow sets in turn; every block uses every code it has"""
    rng = np.random.default_rng(seed)
    w = W()
    plain = bytearray()
    for k in range(n_blocks):
        deep = k % 2 == 0
        ll, dd = random_code_sets(rng, ll_depth=15 if deep else 9, d_depth=15 if deep else 6, force_depth=True)
        toks = use_all(ll, dd, len(plain), rng)
        dynamic_block(w, ll, dd, toks, k == n_blocks - 1, cl_sequence=rle(ll + dd, rng))
        plain = bytearray(apply(toks, bytes(plain)))
    return member("dynamic_200_code_sets", w, bytes(plain))


def many_code_sets_pred(bl, body):
    """200 different code sets; every deep block (15-bit codes in both sets) is followed by a root-only one, and tokens of
    that one begin with 9 bits that were the index of a sub-table link in the deep block's table"""
    if len(bl) != 200 or len({(B.ll_lens, B.d_lens) for B in bl}) != 200:
        return False
    r = _Reader(body)
    for A, B in zip(bl[0::2], bl[1::2]):
        links = set(subtables(A.ll_lens, LROOT)[0])
        if A.ll_max != 15 or A.d_max != 15 or subtables(B.ll_lens, LROOT)[0] or subtables(B.d_lens, DROOT)[0]:
            return False
        if not any(r.peek(LROOT, at) in links for at in list(B.tok_bits) + [B.eob_bit]):
            return False
    return True


def split_lengths(rng, k, maxl, force_depth=False):
    """k code lengths of a random complete code, none longer than maxl (the longest is maxl when forced)"""
    if k == 1:
        return [1]
    ls = [1, 1]
    if force_depth:
        ls = list(range(1, maxl)) + [maxl, maxl]
    while len(ls) < k:
        cand = [i for i, l in enumerate(ls) if l < maxl]
        if not cand:
            break
        i = cand[int(rng.integers(len(cand)))]
        ls[i] += 1
        ls.append(ls[i])
    return ls


def random_code_sets(rng, ll_depth=15, d_depth=15, force_depth=False):
    nl = int(rng.integers(257, 287))
    nd = int(rng.integers(1, 31))
    if force_depth:
        nl, nd = max(nl, 257 + ll_depth), max(nd, d_depth + 1)
    k = int(rng.integers(2, min(nl, 60) + 1))
    ls = split_lengths(rng, max(k, ll_depth + 1) if force_depth else k, ll_depth, force_depth)
    syms = [256] + [int(s) for s in rng.permutation([s for s in range(nl) if s != 256])[:len(ls) - 1]]
    ll = [0] * nl
    for s, l in zip(syms, rng.permutation(ls)):
        ll[s] = int(l)
    dd = [0] * nd
    kd = int(rng.integers(0, nd + 1))
    if force_depth:
        kd = max(kd, d_depth + 1)
    if kd:
        ds = split_lengths(rng, kd, d_depth, force_depth)
        for s, l in zip(rng.permutation(nd)[:len(ds)], rng.permutation(ds)):
            dd[int(s)] = int(l)
    return ll, dd


def random_member(seed):
    """one seeded case: 0-7 empty fixed blocks, then a dynamic block with random complete code sets to depth 15, random
    HLIT / HDIST and a random run-length coding of its code lengths (runs cross the alphabets' boundary); None never:
    whatever it writes must be a stream zlib takes"""
    rng = np.random.default_rng([seed, 0xDEF1A7E])
    w = W()
    for _ in range(int(rng.integers(0, 8))):
        fixed_block(w, [], False)
    head = b""
    if rng.random() < 0.25:
        head = IC.random_bytes(int(rng.integers(1, 3000)), seed)
        stored_block(w, head)
    if rng.random() < 0.35:  # (splitting random leaves seldom goes deep: a third of the cases start from a chain to 10 .. 15 bits)
        ll, dd = random_code_sets(rng, int(rng.integers(10, 16)), int(rng.integers(7, 16)), force_depth=True)
    else:
        ll, dd = random_code_sets(rng)
    toks = use_all(ll, dd, len(head), rng)
    dynamic_block(w, ll, dd, toks, True, cl_sequence=rle(ll + dd, rng))
    return member("random_%04d" % seed, w, apply(toks, head))


@functools.lru_cache(maxsize=4)
def random_members(n=1500):
    """the members and how many the writer had to throw away (zlib refused them, or inflated them to other bytes)"""
    out, discarded = [], []
    for seed in range(n):
        m = random_member(seed)
        try:
            ok = gzip.decompress(m.comp) == m.plain and m.plen <= MEMBER_MAX
        except Exception:  # noqa: BLE001
            ok = False
        (out if ok else discarded).append(m)
    return tuple(out), tuple(m.name for m in discarded)


# ---- libdeflate members, as data ----
@functools.lru_cache(maxsize=1)
def libdeflate_members():
    out = []
    for path in sorted(glob.glob(os.path.join(FIXTURES, "*.gz"))):
        comp = open(path, "rb").read()
        plain = gzip.decompress(comp)
        out.append(Member("libdeflate_" + os.path.basename(path)[:-3], comp, plain, len(plain)))
    assert len(out) >= 14, "tests/golden/inflate/*.gz are missing (tests/golden/make_inflate_fixtures.py writes them)"
    return tuple(out)


@functools.lru_cache(maxsize=1)
def _good():
    cases = _cases()
    for m in libdeflate_members():
        cases.append((m, lambda bl, gs: True))
    for m, _ in cases:
        assert gzip.decompress(m.comp) == m.plain and m.plen == len(m.plain) <= MEMBER_MAX, m.name
    assert len({m.name for m, _ in cases}) == len(cases)
    return tuple(cases)


def good_edge_members():
    return tuple(m for m, _ in _good())


def predicate(m):
    """does the member reach the edge it is named for?  Read from its bytes."""
    blocks, plain, why = anatomy(m.comp)
    pred = dict((c.name, p) for c, p in _good())[m.name]
    return why is None and plain == m.plain and bool(pred(blocks, groups(blocks)))


def set_predicates():
    """what a group of members reaches together -> {what: bool}"""
    good = {m.name: m for m in good_edge_members()}
    an = {n: anatomy(m.comp)[0] for n, m in good.items() if n.startswith(("libdeflate_", "body_end_"))}
    ld = [B for n, bl in an.items() if n.startswith("libdeflate_") for B in bl if B.btype == 2]
    ends = [refill_model(an[n], len(good[n].comp) - 8 - IC.member_body(good[n].comp)) for n in sorted(an) if n.startswith("body_end_")]
    return {
        "a libdeflate member has a code-length run that crosses the alphabets' boundary": any(crossing(B, s) for B in ld for s in (16, 17, 18)),
        # lane 0's window goes from 8-byte loads to single bytes (some 7 bytes before the body's end: it runs that far ahead
        # of the codes) holding every count of pending bits mod 8 ...
        "body_end_*: the refill switch comes with every phase of pending bits": {sw[0] % 8 for sw, _ in ends if sw} == set(range(8)),
        # ... and the last group of tokens — the last codes of the body — is opened, with an empty window, in each of the last 9
        # bytes before the trailer: 1 .. 7 bytes are then loaded one by one, 8 at once, 9 as 8 and 1
        "body_end_*: the last group opens in each of the last 9 bytes": {op[-1] for _, op in ends if len(op) > 1} == set(range(1, 10)),
    }


# ---- bad members ----
def _cut_inside(w, kind, pick=None):
    """the body cut at a byte boundary strictly inside a field of `kind`"""
    for k, s, e in w.marks:
        if k == kind and (pick is None or pick(s, e)) and (s // 8 + 1) * 8 < e:
            return w.bytes()[:s // 8 + 1]
    raise AssertionError("no %s field straddles a byte boundary" % kind)


@functools.lru_cache(maxsize=1)
def bad_edge_members():
    """[(Member, expected status)]: each refused by zlib, each with the status of csrc/bdx_inflate_core.h's table"""
    out = []

    def add(name, body, status, plain=b"", plen=None):
        body = body.bytes() if isinstance(body, Bits) else body
        out.append((Member(name, wrap(body, trailer(plain)), None, len(plain) if plen is None else plen), status))

    ll3 = [0] * 260
    for s in (65, 67, 71, 84, 256, 257, 258, 259):
        ll3[s] = 3
    d3 = [3] * 8
    head = [(18, 54), (3, 0), (0, 0), (3, 0), (17, 0), (3, 0), (17, 7), (0, 0), (0, 0), (3, 0), (18, 127), (18, 22), (3, 0)]  # 0 .. 256
    toks = [65, 67, 71, 84]

    def dyn(name, status, ll=ll3, dd=d3, tokens=toks, plain=b"ACGT", **kw):
        w = W()
        dynamic_block(w, ll, dd, tokens, True, **kw)
        add(name, w, status, plain)

    # code-set faults
    dyn("cl16_first", 4, cl_sequence=[(16, 0)] + [(0, 0)] * 62 + head[1:] + [(16, 3), (16, 2)], cl_lengths=complete_cl([0, 3, 16, 17, 18]))
    dyn("cl16_overflows_by_one", 4, cl_sequence=head + [(16, 3), (16, 3)])
    dyn("cl17_overflows_by_one", 4, ll=ll3 + [0] * 4, dd=[1, 1, 0, 0, 0],
        cl_sequence=head + [(3, 0)] * 3 + [(17, 1), (1, 0), (1, 0), (17, 1)], tokens=[], plain=b"")
    dyn("cl18_overflows_by_one", 4, ll=ll3 + [0] * 4, dd=[1, 1] + [0] * 11,
        cl_sequence=head + [(3, 0)] * 3 + [(17, 1), (1, 0), (1, 0), (18, 1)], tokens=[], plain=b"")
    for hlit in (30, 31):
        dyn("hlit_%d" % hlit, 4, hlit=hlit, cl_sequence=head + [(16, 3), (16, 2)])
    for hdist in (30, 31):
        dyn("hdist_%d" % hdist, 4, hdist=hdist, cl_sequence=head + [(16, 3), (16, 2)])
    cl = complete_cl([0, 3, 16, 17, 18])
    cl[16] += 1
    dyn("incomplete_code_length_code", 4, cl_sequence=head + [(16, 3), (16, 2)], cl_lengths=cl)
    dyn("hclen_4_codes_no_length", 4, ll=[0] * 257, dd=[0], cl_sequence=[(18, 127), (18, 109)], cl_lengths=complete_cl([0, 18]), hclen=4,
        tokens=[], plain=b"", eob=False)
    over = list(ll3)
    over[66] = 3
    dyn("oversubscribed_literal_set", 4, ll=over, tokens=[], plain=b"", eob=False)
    three = [0] * 257
    three[65] = three[67] = three[256] = 2
    dyn("incomplete_literal_set_three_2_bit_codes", 4, ll=three, dd=[1, 1], tokens=[65, 67], plain=b"AC")
    dyn("incomplete_distance_set_longest_2", 4, dd=[2, 2, 2])
    noeob = list(ll3)
    noeob[256], noeob[66] = 0, 3
    dyn("no_end_of_block_code", 4, ll=noeob, eob=False)

    # symbol faults
    ll_m = [0] * 258
    for s, l in ((65, 2), (67, 2), (84, 2), (256, 3), (257, 3)):
        ll_m[s] = l
    dyn("one_bit_distance_code_unused_pattern", 5, ll=ll_m, dd=[1], tokens=[65, 67, 84, ("sym", 257), ("bits", 1, 1)], plain=b"ACT")
    dyn("length_symbol_without_distance_code", 5, ll=ll_m, dd=[0], tokens=[65, 67, 84, ("sym", 257), ("bits", 0, 1)], plain=b"ACT")
    for s in (286, 287):
        w = W()
        fixed_block(w, [65, ("sym", s), ("bits", 0, 5)])
        add("fixed_symbol_%d" % s, w, 5, b"A")
    for s in (30, 31):
        w = W()
        fixed_block(w, [65, 66, 67, ("sym", 257), ("dsym", s), ("bits", 0, 13)])
        add("fixed_distance_symbol_%d" % s, w, 5, b"ABC")

    # a distance fault behind the member's start
    w = W()
    fixed_block(w, list(b"ACGT"), False)
    fixed_block(w, [65, (3, 6)])
    add("distance_out_plus_1_in_second_block", w, 6, b"ACGTA" + b"xxx")

    # one byte past the slot
    text = b"ACGTACGTTT"
    w = W()
    fixed_block(w, list(text))
    add("literal_one_past_the_slot", w, 7, text[:-1])
    w = W()
    fixed_block(w, list(text[:4]) + [(6, 4)])
    add("match_one_past_the_slot", w, 7, text[:9])
    w = W()
    fixed_block(w, list(text[:4]), False)
    stored_block(w, text[4:], True)
    add("stored_one_past_the_slot", w, 7, text[:-1])

    # the body ends too early
    w = W()
    stored_block(w, b"ACGTACGTAC", True, length=100)
    add("stored_len_beyond_the_body", w, 9, b"", plen=100)
    text = IC.fastq_text(400, 19)
    ztoks = list(text[:60])
    for i in range(20):
        ztoks += [(67 + 7 * i, 33 + 3 * i), text[60 + i]]
    text = apply(ztoks)
    ll_all, d_all = [8] * 226 + [9] * 60, [4] * 2 + [5] * 28
    for kind, name in (("cl_len", "code_length_code_lengths"), ("cl_sym", "code_length_sequence"), ("cl_extra18", "extra_bits_of_an_18"),
                       ("lextra", "length_extra_bits"), ("dcode", "distance_code"), ("dextra", "distance_extra_bits")):
        w = W()
        if kind.startswith("cl"):
            dynamic_block(w, ll3 + [0] * 26, [0] * 20 + [1, 1], [65, 67], True,
                          cl_sequence=head + [(3, 0)] * 3 + [(18, 0), (18, 4), (18, 9), (1, 0), (1, 0)], cl_lengths=complete_cl([0, 1, 3, 16, 17, 18]))
            plain = b"AC"
        else:
            dynamic_block(w, ll_all, d_all, list(ztoks), True, cl_sequence=rle(ll_all + d_all))
            plain = text
        assert gzip.decompress(wrap(w.bytes(), trailer(plain))) == plain, kind
        add("truncated_in_" + name, _cut_inside(w, kind), 9, plain)
    w = W()
    fixed_block(w, list(b"ACGTA"), eob=False)
    assert 0 < 8 - w.n < 7  # (fewer zero bits of padding than the end-of-block code has)
    add("no_end_of_block_after_the_last_literal", w, 9, b"ACGTA")

    # a spare byte in front of the trailer
    w = W()
    fixed_block(w, list(b"ACGT"))
    add("spare_byte_before_the_trailer", w.bytes() + b"\0", 1, b"ACGT")

    for m, st in out:
        try:
            gzip.decompress(m.comp)
        except Exception as e:  # noqa: BLE001 - refused, which is the point; for a fault of the code sets, symbols or distance: for that fault
            want = [w for k, w in ZLIB_SAYS.items() if m.name.startswith(k)]
            assert (len(want) == 1 and want[0] in str(e)) if st in (4, 5, 6) else not want, (m.name, str(e))
            continue
        raise AssertionError("gzip.decompress accepts " + m.name)
    assert len({m.name for m, _ in out}) == len(out)
    return tuple(out)


ZLIB_SAYS = {"cl1": "invalid bit length repeat", "hlit": "too many length or distance symbols", "hdist": "too many length or distance symbols",
             "incomplete_code_length": "invalid code lengths set", "hclen_4": "missing end-of-block", "oversubscribed": "invalid literal/lengths set",
             "incomplete_literal": "invalid literal/lengths set", "incomplete_distance": "invalid distances set",
             "no_end_of_block_code": "missing end-of-block", "one_bit_distance": "invalid distance code",
             "length_symbol_without": "invalid distance code", "fixed_symbol": "invalid literal/length code",
             "fixed_distance": "invalid distance code", "distance_out": "invalid distance too far back"}


# ---- the coverage listing ----
def _ranges(xs):
    xs = sorted(set(xs))
    return ",".join(str(x) for x in xs) if len(xs) <= 8 else "%d..%d (%d values)" % (xs[0], xs[-1], len(xs))


def describe(m, status):
    blocks, plain, why = anatomy(m.comp, strict=False)
    gs = groups(blocks)
    hb = [B for B in blocks if B.btype]
    dyn = _dyn(blocks)
    parts = ["%d blocks (stored %d, fixed %d, dynamic %d)" % (len(blocks), sum(B.btype == 0 for B in blocks), sum(B.btype == 1 for B in blocks),
                                                             len(dyn)),
             "header bit offsets mod 8: Huffman {%s} stored {%s}" % (_ranges(B.bit % 8 for B in hb), _ranges(B.bit % 8 for B in blocks if not B.btype))]
    if dyn:
        parts.append("nl %s nd %s hclen %s" % (_ranges(B.nl for B in dyn), _ranges(B.nd for B in dyn), _ranges(B.hclen for B in dyn)))
        parts.append("longest code ll %d d %d cl %d" % (max(B.ll_max for B in dyn), max(B.d_max for B in dyn), max(max(B.cl_lens) for B in dyn)))
        parts.append("sub bits ll {%s} d {%s}" % (_ranges(v for B in dyn for v in subtables(B.ll_lens, LROOT)[0].values()),
                                                  _ranges(v for B in dyn for v in subtables(B.d_lens, DROOT)[0].values())))
        parts.append("cl symbols {%s}" % _ranges(s for B in dyn for s, _, _ in B.cl_syms))
        cross = ["%d(+%d)" % (s, x) for B in dyn for sym in (16, 17, 18) for s, x, _ in crossing(B, sym)]
        if cross:
            parts.append("runs across nl: " + " ".join(cross[:6]))
    toks = [t for B in hb for t in B.tokens]
    parts.append("tokens %d (%d matches)" % (len(toks), sum(not isinstance(t, int) for t in toks)))
    if gs:
        g = max(gs, key=lambda g: (g.n, g.nbytes))
        parts.append("groups %d, largest %d tokens / %d bytes, sizes {%s}" % (len(gs), g.n, max(x.nbytes for x in gs), _ranges(x.n for x in gs)))
    if why:
        parts.append("reader: " + why)
    return "%-44s %6d -> %6d bytes  host status %d  | %s" % (m.name, len(m.comp), m.plen, status, "; ".join(parts))


def listing(dec):
    out = ["# python tests/inflate_edge_cases.py: what every edge member of the device inflate's suite holds, read from its bytes",
           "# good members (%d): host status 0 and zlib's bytes" % len(good_edge_members())]
    for m in good_edge_members():
        st, got = dec(m.comp, m.plen, fresh=True)
        out.append(describe(m, st) + ("" if st == 0 and got == m.plain and predicate(m) else "  WRONG"))
    for what, ok in set_predicates().items():
        out.append("# %s: %s" % (what, ok))
    out.append("# bad members (%d): refused by zlib; the host status is the expected one" % len(bad_edge_members()))
    for m, want in bad_edge_members():
        st, _ = dec(m.comp, m.plen, fresh=True)
        out.append(describe(m, st) + " | expected %d (%s)%s" % (want, IC.STATUS[want], "" if st == want else "  WRONG"))
    members, discarded = random_members()
    out.append("# random dynamic blocks: %d written, %d discarded" % (len(members) + len(discarded), len(discarded)))
    return out


if __name__ == "__main__":
    print("\n".join(listing(IC.host_decoder())))
