// bdx_inflate_core.h — one gzip member -> its plain bytes, written as barrier-separated phases of a 64-thread
// workgroup (one wavefront; private; included by bdx_inflate.hip).  The idiom of bdx_deflate_core.h: every phase is a
// function of (shared state, thread index), INF_PHASE runs it for the workgroup's threads and ends with a barrier, no
// phase keeps a value in a register across a barrier, none uses a cross-lane operation and none depends on the order
// in which its lanes run.  The same text compiles as plain C++, where INF_PHASE is a loop over the thread index: the
// decoder is tested and run under sanitizers on a CPU.  Between two phases the control flow reads words of the shared
// state that only a later phase writes again; the workgroup is ONE wavefront, whose LDS operations execute in order.
//
// A complete RFC 1951 decoder (stored, fixed and dynamic blocks, any number of them) behind an RFC 1952 header
// (FEXTRA, FNAME, FCOMMENT, FHCRC).  zlib is the arbiter of what is accepted: code sets as inflate_table takes them
// (over-subscribed refused; incomplete refused except a single one-bit code; symbols 286, 287 and distance symbols
// 30, 31 refused when they are used), the trailer's CRC-32 and ISIZE.
//
// Stages:
//   begin    lane 0 parses the gzip header
//   block    lane 0 reads a block header; a stored block is then copied by all lanes; a dynamic header's code lengths
//            are decoded by lane 0 through a 7-bit table
//   codes    lane 0: counts, the zlib acceptance rule, canonical codes, second-level tables laid out behind the root
//            table (root 9 bits + sub-tables <= 852 entries for 286 symbols, root 6 bits <= 592 for 30: zlib's
//            ENOUGH_LENS / ENOUGH_DISTS, the same construction); all lanes then fill the entries of their symbols
//   tokens   lane 0 walks the bit stream (64-bit window, refilled with one 8-byte load while 8 bytes of the body are
//            left, byte by byte after that) and writes up to INF_GROUP tokens.  A match whose source overlaps bytes of
//            its own group ends the group before it: every source byte of a group was stored by an EARLIER group
//   place    all lanes: byte j of the group's output finds its token by binary search; a literal is stored, a match
//            byte i comes from start - dist + (i mod dist), which lies before the token.  Output goes straight to the
//            member's slot in global memory; the barrier that ends the phase is the workgroup-scope fence between one
//            group's stores and the next group's loads
//   crc      64 slices over the slot, combined as in bdx_deflate_core.h, against the trailer
//
// Bounds: no byte outside comp[0, clen) is read (the bit reader stops at the trailer, clen - 8), none outside
// out[0, plen) is written; plen comes from an untrusted ISIZE, so every token is checked against it before it is listed.
#pragma once
#include <stdint.h>

#include "bdx_crc32_core.h"

#define INF_THREADS 64
#define INF_MEMBER_MAX 65536  // the largest plain size of a member (BGZF's; group offsets and positions fit 17 bits)
#define INF_GROUP 128         // tokens handed to the lanes at a time (at most 128 * 258 bytes: offsets fit 16 bits)
#define INF_LROOT 9
#define INF_DROOT 6
#define INF_LTAB 852          // zlib ENOUGH_LENS: enough 286 9 15
#define INF_DTAB 592          // zlib ENOUGH_DISTS: enough 30 6 15
#define INF_NL 288            // literal/length symbols of the fixed code (286 and 287 are never valid in a stream)
#define INF_ND 32             // distance symbols of the fixed code (30 and 31 are never valid)
#define INF_LINK 0x8000u      // table entry: a leaf is sym << 4 | code length (0: no code), a link is INF_LINK | offset << 4 | sub bits

// per-member status codes (bdx_fq_inflate_device's `status`)
#define INF_OK 0
#define INF_E_HEADER 1     // not a gzip/deflate header, a reserved flag, a header CRC mismatch, or bytes between the stream's end and the trailer
#define INF_E_BTYPE 2      // block type 3
#define INF_E_STORED 3     // LEN != ~NLEN
#define INF_E_CODES 4      // a code set zlib refuses (counts, over-subscribed, incomplete, bad repeat, no end-of-block code)
#define INF_E_SYMBOL 5     // bits that are no code, or a symbol that may not be used
#define INF_E_DISTANCE 6   // a distance that reaches before the member's first byte
#define INF_E_OVERRUN 7    // the stream holds more bytes than the slot
#define INF_E_SHORT 8      // the stream ends before the slot is full
#define INF_E_INPUT 9      // the body ends inside a block
#define INF_E_CRC 10
#define INF_E_ISIZE 11

#define INF_RUN 0   // InfShared::state: reading blocks
#define INF_END 1   // the final block is done
#define INF_BAD 2   // refused: `status` says why

#if defined(__HIPCC__)
#define INF_FN __device__ inline
#define INF_PHASE(call)                 \
    {                                   \
        const int t = (int)threadIdx.x; \
        call;                           \
    }                                   \
    __syncthreads();
#define INF_ATOMIC_XOR(p, v) atomicXor((p), (v))
#else
#define INF_FN inline
#define INF_PHASE(call) \
    for (int t = 0; t < INF_THREADS; ++t) { call; }
#define INF_ATOMIC_XOR(p, v) (*(p) ^= (v))
#endif

struct InfShared {
    uint32_t crc_tab[256];
    uint32_t x2n[32];
    uint16_t ltab[INF_LTAB];
    uint16_t dtab[INF_DTAB];
    uint16_t code[INF_NL + INF_ND];   // bit-reversed canonical codes
    uint8_t lens[INF_NL + INF_ND];    // code lengths: literal/length, then distance (at nl)
    uint8_t cltab[128];               // the code-length code: sym << 3 | length, by 7 reversed bits
    uint8_t cl[19];                   // its lengths
    uint32_t cnt[16], next[16];       // lane 0's work while it lays a code out: codes per length, next code per length
    uint16_t tk_start[INF_GROUP];     // first byte of the token, relative to g_base
    uint16_t tk_val[INF_GROUP];       // a literal, or 0x8000 | distance - 1
    uint64_t bitpos;                  // bits of comp consumed
    uint32_t lim;                     // the body ends here (clen - 8)
    uint32_t out;                     // plain bytes listed so far
    uint32_t state, status, final, kind;  // kind: 0 stored, 1 Huffman
    uint32_t nl, nd;                  // symbols of the block's two codes
    uint32_t cp_src, cp_dst, cp_n;    // stored block: comp[cp_src, +cp_n) -> out[cp_dst, +cp_n)
    uint32_t g_base, g_n, g_bytes, eob;
    uint32_t crc;
};

INF_FN uint64_t inf_load64(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// the bit reader of lane 0: a window of `cnt` valid bits over comp[.., lim)
struct InfBits {
    uint64_t buf;
    uint32_t cnt, ip;
};
INF_FN void inf_refill(InfBits &b, const uint8_t *comp, uint32_t lim) {
    if (b.ip + 8 <= lim) {
        b.buf |= inf_load64(comp + b.ip) << b.cnt;
        b.ip += (63 - b.cnt) >> 3;
        b.cnt |= 56;
    } else {
        while (b.cnt <= 56 && b.ip < lim) {
            b.buf |= (uint64_t)comp[b.ip++] << b.cnt;
            b.cnt += 8;
        }
    }
}
INF_FN InfBits inf_open(const InfShared &S, const uint8_t *comp) {
    InfBits b;
    b.buf = 0;
    b.cnt = 0;
    b.ip = (uint32_t)(S.bitpos >> 3);
    inf_refill(b, comp, S.lim);
    const uint32_t skip = (uint32_t)(S.bitpos & 7);
    if (b.cnt >= skip) {  // (cnt == 0 only at the body's end, where skip is 0 too or the bits are missing anyway)
        b.buf >>= skip;
        b.cnt -= skip;
    } else {
        b.buf = 0;
        b.cnt = 0;
    }
    return b;
}
INF_FN uint64_t inf_consumed(const InfBits &b) { return (uint64_t)b.ip * 8 - b.cnt; }
INF_FN void inf_drop(InfBits &b, uint32_t n) {
    b.buf >>= n;
    b.cnt -= n;
}
INF_FN void inf_refuse(InfShared &S, uint32_t why) {
    S.status = why;
    S.state = INF_BAD;
}

INF_FN uint32_t inf_rev(uint32_t v, int bits) {
    uint32_t r = 0;
    for (int i = 0; i < bits; ++i) r |= ((v >> i) & 1u) << (bits - 1 - i);
    return r;
}

// once per workgroup
INF_FN void inf_ph_tables(InfShared &S, int t) {
    for (int i = t; i < 256; i += INF_THREADS) S.crc_tab[i] = bdx_crc_table_entry(i);
    if (t == 0) bdx_crc_x2n_init(S.x2n);
}

// ---- begin: the gzip header (RFC 1952) ----
INF_FN void inf_ph_begin(InfShared &S, const uint8_t *comp, int clen, int plen, int t) {
    if (t != 0) return;
    S.state = INF_RUN;
    S.status = INF_OK;
    S.out = 0;
    S.final = 0;
    S.crc = 0;
    S.eob = 0;
    S.g_n = S.g_bytes = S.g_base = 0;
    S.cp_n = 0;
    S.bitpos = 0;
    S.lim = 0;
    if (clen < 18 || plen < 0 || plen > INF_MEMBER_MAX) return inf_refuse(S, INF_E_HEADER);
    const uint32_t lim = (uint32_t)clen - 8;
    S.lim = lim;
    if (comp[0] != 0x1f || comp[1] != 0x8b || comp[2] != 8 || (comp[3] & 0xE0)) return inf_refuse(S, INF_E_HEADER);
    const uint32_t flg = comp[3];
    uint32_t p = 10;
    if (flg & 4) {  // FEXTRA
        if (p + 2 > lim) return inf_refuse(S, INF_E_HEADER);
        const uint32_t xlen = (uint32_t)comp[p] | ((uint32_t)comp[p + 1] << 8);
        p += 2;
        if (xlen > lim - p) return inf_refuse(S, INF_E_HEADER);
        p += xlen;
    }
    for (uint32_t bit = 8; bit <= 16; bit <<= 1) {  // FNAME, FCOMMENT: zero-terminated
        if (!(flg & bit)) continue;
        while (p < lim && comp[p]) ++p;
        if (p >= lim) return inf_refuse(S, INF_E_HEADER);
        ++p;
    }
    if (flg & 2) {  // FHCRC: the low 16 bits of the CRC-32 of the header so far
        if (p + 2 > lim) return inf_refuse(S, INF_E_HEADER);
        uint32_t c = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < p; ++i) c = S.crc_tab[(c ^ comp[i]) & 0xFF] ^ (c >> 8);
        c ^= 0xFFFFFFFFu;
        if ((c & 0xFFFFu) != ((uint32_t)comp[p] | ((uint32_t)comp[p + 1] << 8))) return inf_refuse(S, INF_E_HEADER);
        p += 2;
    }
    S.bitpos = (uint64_t)p * 8;
}

// ---- block: a block header; for a dynamic block also its code lengths ----
INF_FN void inf_ph_block(InfShared &S, const uint8_t *comp, int plen, int t) {
    if (t != 0) return;
    InfBits b = inf_open(S, comp);
    if (b.cnt < 3) return inf_refuse(S, INF_E_INPUT);
    S.final = (uint32_t)b.buf & 1;
    const uint32_t btype = ((uint32_t)b.buf >> 1) & 3;
    inf_drop(b, 3);
    if (btype == 3) return inf_refuse(S, INF_E_BTYPE);
    if (btype == 0) {
        uint32_t p = (uint32_t)((inf_consumed(b) + 7) >> 3);
        if (p + 4 > S.lim) return inf_refuse(S, INF_E_INPUT);
        const uint32_t len = (uint32_t)comp[p] | ((uint32_t)comp[p + 1] << 8);
        const uint32_t nlen = (uint32_t)comp[p + 2] | ((uint32_t)comp[p + 3] << 8);
        if ((len ^ 0xFFFFu) != nlen) return inf_refuse(S, INF_E_STORED);
        p += 4;
        if (len > S.lim - p) return inf_refuse(S, INF_E_INPUT);
        if (len > (uint32_t)plen - S.out) return inf_refuse(S, INF_E_OVERRUN);
        S.kind = 0;
        S.cp_src = p;
        S.cp_dst = S.out;
        S.cp_n = len;
        S.out += len;
        S.bitpos = (uint64_t)(p + len) * 8;
        return;
    }
    S.kind = 1;
    if (btype == 1) {
        for (int s = 0; s < INF_NL; ++s) S.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
        for (int s = 0; s < INF_ND; ++s) S.lens[INF_NL + s] = 5;
        S.nl = INF_NL;
        S.nd = INF_ND;
        S.bitpos = inf_consumed(b);
        return;
    }
    if (b.cnt < 14) return inf_refuse(S, INF_E_INPUT);
    const uint32_t nl = ((uint32_t)b.buf & 31) + 257, nd = (((uint32_t)b.buf >> 5) & 31) + 1, ncl = (((uint32_t)b.buf >> 10) & 15) + 4;
    inf_drop(b, 14);
    if (nl > 286 || nd > 30) return inf_refuse(S, INF_E_CODES);
    // the code-length code: 19 lengths of 3 bits in the order of RFC 1951 §3.2.7
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t *cl = S.cl;
    uint32_t *cnt = S.cnt, *next = S.next;
    for (int i = 0; i < 19; ++i) cl[i] = 0;
    inf_refill(b, comp, S.lim);  // (at least 56 bits, or all that is left; 19 * 3 = 57: once more on the way)
    for (uint32_t i = 0; i < ncl; ++i) {
        if (b.cnt < 3) inf_refill(b, comp, S.lim);
        if (b.cnt < 3) return inf_refuse(S, INF_E_INPUT);
        cl[order[i]] = (uint8_t)(b.buf & 7);
        inf_drop(b, 3);
    }
    for (int i = 0; i < 8; ++i) cnt[i] = 0;
    for (int i = 0; i < 19; ++i) cnt[cl[i]]++;
    int left = 1;
    for (int l = 1; l <= 7; ++l) {
        left = 2 * left - (int)cnt[l];
        if (left < 0) return inf_refuse(S, INF_E_CODES);
    }
    if (left > 0) return inf_refuse(S, INF_E_CODES);  // (zlib: an incomplete code-length code is never accepted)
    for (int i = 0; i < 128; ++i) S.cltab[i] = 0;
    uint32_t c = 0;
    cnt[0] = 0;
    for (int l = 1; l <= 7; ++l) {
        c = (c + cnt[l - 1]) << 1;
        next[l] = c;
    }
    for (int s = 0; s < 19; ++s) {
        const int l = cl[s];
        if (!l) continue;
        for (uint32_t i = inf_rev(next[l]++, l); i < 128; i += 1u << l) S.cltab[i] = (uint8_t)(s << 3 | l);
    }
    // nl + nd code lengths, the repeat codes running across the boundary of the two alphabets
    uint32_t n = 0, prev = 0;
    while (n < nl + nd) {
        inf_refill(b, comp, S.lim);
        const uint32_t e = S.cltab[b.buf & 127];
        const uint32_t l = e & 7, sym = e >> 3;
        if (l > b.cnt) return inf_refuse(S, INF_E_INPUT);  // (the code is complete: every 7 bits are a code)
        inf_drop(b, l);
        uint32_t rep, val;
        if (sym < 16) {
            rep = 1;
            val = prev = sym;
        } else {
            const uint32_t eb = sym == 16 ? 2 : sym == 17 ? 3 : 7;
            if (eb > b.cnt) return inf_refuse(S, INF_E_INPUT);
            const uint32_t x = (uint32_t)b.buf & ((1u << eb) - 1);
            inf_drop(b, eb);
            if (sym == 16) {
                if (n == 0) return inf_refuse(S, INF_E_CODES);
                rep = 3 + x;
                val = prev;
            } else {
                rep = (sym == 17 ? 3 : 11) + x;
                val = prev = 0;
            }
        }
        if (n + rep > nl + nd) return inf_refuse(S, INF_E_CODES);
        for (uint32_t i = 0; i < rep; ++i, ++n) S.lens[n < nl ? n : INF_NL + (n - nl)] = (uint8_t)val;
    }
    if (S.lens[256] == 0) return inf_refuse(S, INF_E_CODES);  // no end-of-block code
    S.nl = nl;
    S.nd = nd;
    S.bitpos = inf_consumed(b);
}

INF_FN void inf_ph_stored(InfShared &S, const uint8_t *comp, uint8_t *out, int t) {
    for (uint32_t i = (uint32_t)t; i < S.cp_n; i += INF_THREADS) out[S.cp_dst + i] = comp[S.cp_src + i];
    if (t == 0 && S.final) S.state = INF_END;
}

// ---- codes ----
// One alphabet: lens[first, first + n) -> bit-reversed canonical codes, the cleared root table with a link at every
// prefix of a longer code and the cleared sub-tables behind it.  Lane 0 only; false: zlib refuses the set.
INF_FN bool inf_layout(InfShared &S, int first, int n, uint16_t *tab, int root, int cap) {
    uint32_t *cnt = S.cnt, *next = S.next;
    for (int i = 0; i < 16; ++i) cnt[i] = 0;
    for (int s = 0; s < n; ++s) cnt[S.lens[first + s]]++;
    int left = 1, maxl = 0;
    for (int l = 1; l <= 15; ++l) {
        left = 2 * left - (int)cnt[l];
        if (left < 0) return false;  // over-subscribed
        if (cnt[l]) maxl = l;
    }
    if (left > 0 && maxl > 1) return false;  // incomplete, and not the single one-bit code (no code at all: every use is refused)
    uint32_t c = 0;
    cnt[0] = 0;
    for (int l = 1; l <= 15; ++l) {
        c = (c + cnt[l - 1]) << 1;
        next[l] = c;
    }
    for (int i = 0; i < (1 << root); ++i) tab[i] = 0;
    for (int s = 0; s < n; ++s) {
        const int l = S.lens[first + s];
        if (!l) continue;
        const uint32_t r = inf_rev(next[l]++, l);
        S.code[first + s] = (uint16_t)r;
        if (l > root) {  // (for now: the most sub bits any code with this prefix needs)
            uint16_t &e = tab[r & ((1u << root) - 1)];
            if (e < l - root) e = (uint16_t)(l - root);
        }
    }
    int off = 1 << root;
    for (int i = 0; i < (1 << root); ++i) {
        const int sb = tab[i];
        if (!sb) continue;
        if (off + (1 << sb) > cap) return false;  // (cannot happen for a set that passed the rule above: zlib's ENOUGH)
        tab[i] = (uint16_t)(INF_LINK | (uint32_t)off << 4 | (uint32_t)sb);
        for (int j = 0; j < (1 << sb); ++j) tab[off + j] = 0;
        off += 1 << sb;
    }
    return true;
}

INF_FN void inf_ph_codes(InfShared &S, int t) {
    if (t != 0) return;
    if (!inf_layout(S, 0, (int)S.nl, S.ltab, INF_LROOT, INF_LTAB) || !inf_layout(S, INF_NL, (int)S.nd, S.dtab, INF_DROOT, INF_DTAB))
        inf_refuse(S, INF_E_CODES);
}

// the entries of symbol s (s < nl: literal/length, else distance symbol s - nl): disjoint from every other symbol's
INF_FN void inf_fill_symbol(InfShared &S, uint32_t s) {
    const bool lit = s < S.nl;
    const uint32_t at = lit ? s : INF_NL + (s - S.nl), sym = lit ? s : s - S.nl;
    uint16_t *tab = lit ? S.ltab : S.dtab;
    const uint32_t root = lit ? INF_LROOT : INF_DROOT;
    const uint32_t l = S.lens[at];
    if (!l) return;
    const uint32_t r = S.code[at];
    const uint16_t leaf = (uint16_t)(sym << 4 | l);
    if (l <= root) {
        for (uint32_t i = r; i < (1u << root); i += 1u << l) tab[i] = leaf;
    } else {
        const uint32_t e = tab[r & ((1u << root) - 1)];
        const uint32_t off = (e & 0x7FFFu) >> 4, sb = e & 15;
        for (uint32_t i = r >> root; i < (1u << sb); i += 1u << (l - root)) tab[off + i] = leaf;
    }
}
INF_FN void inf_ph_fill(InfShared &S, int t) {
    for (uint32_t s = (uint32_t)t; s < S.nl + S.nd; s += INF_THREADS) inf_fill_symbol(S, s);
}

// a code of `tab` at the window's low bits -> its leaf (0 in the low 4 bits: the bits are no code)
INF_FN uint32_t inf_lookup(const uint16_t *tab, uint32_t root, uint64_t buf) {
    uint32_t e = tab[(uint32_t)buf & ((1u << root) - 1)];
    if (e & INF_LINK) e = tab[((e & 0x7FFFu) >> 4) + (((uint32_t)(buf >> root)) & ((1u << (e & 15)) - 1))];
    return e;
}

// ---- tokens ----
INF_FN void inf_ph_tokens(InfShared &S, const uint8_t *comp, int plen, int t) {
    if (t != 0) return;
    InfBits b = inf_open(S, comp);
    const uint32_t base = S.out;
    uint32_t out = base, n = 0;
    S.g_base = base;
    S.eob = 0;
    while (n < INF_GROUP) {
        inf_refill(b, comp, S.lim);
        const uint64_t before = inf_consumed(b);
        uint32_t e = inf_lookup(S.ltab, INF_LROOT, b.buf);
        uint32_t l = e & 15;
        if (!l) {
            inf_refuse(S, INF_E_SYMBOL);
            break;
        }
        if (l > b.cnt) {
            inf_refuse(S, INF_E_INPUT);
            break;
        }
        inf_drop(b, l);
        const uint32_t sym = e >> 4;
        if (sym < 256) {
            if (out >= (uint32_t)plen) {
                inf_refuse(S, INF_E_OVERRUN);
                break;
            }
            S.tk_start[n] = (uint16_t)(out - base);
            S.tk_val[n] = (uint16_t)sym;
            ++n;
            ++out;
            continue;
        }
        if (sym == 256) {
            S.eob = 1;
            break;
        }
        if (sym > 285) {
            inf_refuse(S, INF_E_SYMBOL);
            break;
        }
        const uint32_t ls = sym - 257;
        uint32_t len, eb = 0;
        if (ls < 8) {
            len = 3 + ls;
        } else if (ls == 28) {
            len = 258;
        } else {
            eb = (ls - 4) >> 2;
            len = 3 + ((4 + (ls & 3)) << eb);
        }
        if (eb > b.cnt) {
            inf_refuse(S, INF_E_INPUT);
            break;
        }
        len += (uint32_t)b.buf & ((1u << eb) - 1);
        inf_drop(b, eb);
        e = inf_lookup(S.dtab, INF_DROOT, b.buf);
        l = e & 15;
        if (!l) {
            inf_refuse(S, INF_E_SYMBOL);
            break;
        }
        if (l > b.cnt) {
            inf_refuse(S, INF_E_INPUT);
            break;
        }
        inf_drop(b, l);
        const uint32_t ds = e >> 4;
        if (ds > 29) {
            inf_refuse(S, INF_E_SYMBOL);
            break;
        }
        uint32_t dist;
        eb = 0;
        if (ds < 4) {
            dist = 1 + ds;
        } else {
            eb = (ds - 2) >> 1;
            dist = 1 + ((2 + (ds & 1)) << eb);
        }
        if (eb > b.cnt) {
            inf_refuse(S, INF_E_INPUT);
            break;
        }
        dist += (uint32_t)b.buf & ((1u << eb) - 1);
        inf_drop(b, eb);
        if (dist > out) {
            inf_refuse(S, INF_E_DISTANCE);
            break;
        }
        if (len > (uint32_t)plen - out) {
            inf_refuse(S, INF_E_OVERRUN);
            break;
        }
        if (n > 0 && out - dist + (len < dist ? len : dist) > base) {  // its source is in this group: it opens the next one
            b.ip = (uint32_t)((before + 7) >> 3);
            b.cnt = (uint32_t)((uint64_t)b.ip * 8 - before);
            break;
        }
        S.tk_start[n] = (uint16_t)(out - base);
        S.tk_val[n] = (uint16_t)(0x8000u | (dist - 1));
        ++n;
        out += len;
    }
    S.g_n = n;
    S.g_bytes = out - base;
    S.out = out;
    S.bitpos = inf_consumed(b);
    if (S.state == INF_RUN && S.eob && S.final) S.state = INF_END;
}

// ---- place ----
INF_FN void inf_ph_place(const InfShared &S, uint8_t *out, int t) {
    const uint32_t n = S.g_n;
    for (uint32_t j = (uint32_t)t; j < S.g_bytes; j += INF_THREADS) {
        uint32_t lo = 0, hi = n;  // the last token that starts at or before j
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (S.tk_start[mid] <= j)
                lo = mid;
            else
                hi = mid;
        }
        const uint32_t v = S.tk_val[lo];
        uint8_t byte;
        if (!(v & 0x8000u)) {
            byte = (uint8_t)v;
        } else {
            const uint32_t d = (v & 0x7FFFu) + 1, start = S.g_base + S.tk_start[lo], i = j - S.tk_start[lo];
            byte = out[start - d + (i < d ? i : i % d)];
        }
        out[S.g_base + j] = byte;
    }
}

// ---- the trailer ----
INF_FN void inf_ph_end(InfShared &S, int plen, int t) {
    if (t != 0 || S.state != INF_END) return;
    if (S.out != (uint32_t)plen) return inf_refuse(S, INF_E_SHORT);  // (more than plen was refused when it was listed)
    if (((S.bitpos + 7) >> 3) != (uint64_t)S.lim) return inf_refuse(S, INF_E_HEADER);  // bytes between the stream and the trailer
}

INF_FN void inf_ph_crc(InfShared &S, const uint8_t *out, int n, int t) {
    if (S.state != INF_END) return;
    const int per = (n + INF_THREADS - 1) / INF_THREADS;
    const int a = t * per < n ? t * per : n;
    const int b = a + per < n ? a + per : n;
    if (a >= b) return;
    uint32_t c = 0xFFFFFFFFu;
    for (int i = a; i < b; ++i) c = S.crc_tab[(c ^ out[i]) & 0xFF] ^ (c >> 8);
    c ^= 0xFFFFFFFFu;
    INF_ATOMIC_XOR(&S.crc, bdx_crc_multmodp(bdx_crc_x8n(S.x2n, (uint32_t)(n - b)), c));
}

INF_FN void inf_ph_verdict(InfShared &S, const uint8_t *comp, int plen, int32_t *status, int t) {
    if (t != 0) return;
    if (S.state == INF_END) {
        const uint8_t *tr = comp + S.lim;
        const uint32_t crc = (uint32_t)tr[0] | ((uint32_t)tr[1] << 8) | ((uint32_t)tr[2] << 16) | ((uint32_t)tr[3] << 24);
        const uint32_t isize = (uint32_t)tr[4] | ((uint32_t)tr[5] << 8) | ((uint32_t)tr[6] << 16) | ((uint32_t)tr[7] << 24);
        if (crc != S.crc)
            S.status = INF_E_CRC;
        else if (isize != (uint32_t)plen)
            S.status = INF_E_ISIZE;
    }
    *status = (int32_t)S.status;
}

// One member comp[0, clen) -> out[0, plen); *status: INF_OK or why it was refused (the slot's content is then
// unspecified, but nothing outside it was touched).  Called by all threads of the workgroup, after inf_ph_tables.
INF_FN void inf_decode_member(InfShared &S, const uint8_t *comp, int clen, uint8_t *out, int plen, int32_t *status) {
    INF_PHASE(inf_ph_begin(S, comp, clen, plen, t))
    while (S.state == INF_RUN) {
        INF_PHASE(inf_ph_block(S, comp, plen, t))
        if (S.state != INF_RUN) break;
        if (S.kind == 0) {
            INF_PHASE(inf_ph_stored(S, comp, out, t))
            continue;
        }
        INF_PHASE(inf_ph_codes(S, t))
        if (S.state != INF_RUN) break;
        INF_PHASE(inf_ph_fill(S, t))
        bool more = true;
        while (more) {
            INF_PHASE(inf_ph_tokens(S, comp, plen, t))
            INF_PHASE(inf_ph_place(S, out, t))
            more = S.state == INF_RUN && !S.eob;
        }
    }
    INF_PHASE(inf_ph_end(S, plen, t))
    INF_PHASE(inf_ph_crc(S, out, plen, t))
    INF_PHASE(inf_ph_verdict(S, comp, plen, status, t))
}
