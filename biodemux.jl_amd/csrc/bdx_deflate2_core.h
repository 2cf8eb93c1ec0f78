// bdx_deflate2_core.h — level 2 of the chunk encoder of bdx_deflate_core.h: the same member, the same phase idiom (every
// phase a function of (shared state, thread index), nothing in a register across a barrier, no cross-lane operation: the
// text compiles as plain C++, and that build is the specification of the bytes), with the four remedies of DESIGN §6:
//
//   in-block   a position's candidates are the DFL2_K most recent EARLIER positions of its hash, wherever they lie: first
//              those of its own sub-block (the sub-block's 256 hashes lie in LDS; a thread compares them with its own 32
//              at a time, nearest group first; distance 1 and sources that overlap the match included), then the bucket
//   buckets    the table (the memory of DflShared::tab, 16-bit entries: position + 1, 0 empty) holds per hash the DFL2_K
//              most recent positions of the earlier sub-blocks, most recent first.  A bucket has ONE writer a sub-block:
//              the thread of the hash's last position there, which puts itself and the sub-block's earlier positions of
//              that hash in front and shifts the old entries back.  No atomics: the content is a function of the text.
//   lazy       thread 0's walk drops a match at p for a literal when the match at p + 1 is longer.  At a sub-block's
//              last position the next record does not exist yet: the match waits in `pend` and the next sub-block's
//              walk decides it first and appends its token itself (the chunk's last positions have no match to wait).
//   header     the code lengths go out run-length coded (symbols 16 / 17 / 18, runs across the literal/length-distance
//              border) under a code-length code of their own: Huffman lengths limited to 7 bits, complete, HCLEN
//              trimmed.  Its exact size feeds the stored rule.
//
// Everything else — histograms, the two codes, the bit packing, CRC, the member, the stored rule — is the level-1 text,
// called on the DflShared inside Dfl2Shared.  The DFL2_* switches exist for the ablation of
// profiles/r07_deflate_level2_ratio_host_build.txt; the library is built with their defaults.
#pragma once
#include "bdx_deflate_core.h"

#ifndef DFL2_K
#define DFL2_K 8  // candidates per hash (profiles/r07_deflate_level2_ratio_host_build.txt: 1, 2, 4 and 8 compared)
#endif
#ifndef DFL2_INBLOCK
#define DFL2_INBLOCK 1
#endif
#ifndef DFL2_LAZY
#define DFL2_LAZY 1
#endif
#ifndef DFL2_RLE
#define DFL2_RLE 1
#endif
#define DFL2_HASH_BITS (DFL2_K == 1 ? 14 : DFL2_K == 2 ? 13 : DFL2_K == 4 ? 12 : 11)  // 16 384 entries of 16 bits
#define DFL2_NCL 19
#define DFL2_CL_MAX_BITS 7
#define DFL2_NO_HASH 0xFFFFu

static_assert(DFL2_K == 1 || DFL2_K == 2 || DFL2_K == 4 || DFL2_K == 8, "the buckets fill DflShared::tab");
static_assert((DFL2_K << DFL2_HASH_BITS) * 2 == DFL_TAB * 4, "the buckets fill DflShared::tab");
static_assert(DFL_CHUNK < 65535, "position + 1 fits 16 bits");

struct Dfl2Shared {
    DflShared B;                       // level 1's state; B.tab: the buckets, then the bit buffer
    alignas(16) uint32_t hw[DFL_THREADS / 2];  // the sub-block's hashes, 16 bits each (DFL2_NO_HASH: none)
    uint16_t hsym[DFL_NSYM];           // header: code-length symbol | extra value << 5
    uint16_t hoff[DFL_NSYM];           //         the bit it starts at
    uint32_t cl_hist[DFL2_NCL], cl_key[DFL2_NCL];
    uint8_t cl_ord[DFL2_NCL], cl_len[DFL2_NCL], cl_code[DFL2_NCL];
    uint32_t nhs, hclen, hdr_bits;     // header symbols, code-length code lengths sent, bits of the whole header
    uint32_t pend, pend_len, pend_dist;  // a match at the previous sub-block's last position waits for the lazy decision
};

DFL_FN void dfl2_ph_init(Dfl2Shared &S, int t) {
    dfl_ph_init(S.B, t);
    if (t == 0) S.pend = 0;
}

// ---- tokens ----
DFL_FN void dfl2_ph_hash(Dfl2Shared &S, const uint8_t *in, int n, int base, int t) {
    const int p = base + t;
    if ((t & 3) == 0) S.B.flagw[t >> 2] = 0;
    ((uint16_t *)S.hw)[t] = p + DFL_MIN_MATCH <= n ? (uint16_t)((dfl_load32(in + p) * 2654435761u) >> (32 - DFL2_HASH_BITS)) : (uint16_t)DFL2_NO_HASH;
}

// bit j: position 32 g + j of the sub-block has the hash h
DFL_FN uint32_t dfl2_eq32(const Dfl2Shared &S, int g, uint32_t h) {
    uint32_t m = 0;
    for (int i = 0; i < 16; ++i) {
        const uint32_t w = S.hw[16 * g + i];
        m |= (((w & 0xFFFFu) == h ? 1u : 0u) | ((w >> 16) == h ? 2u : 0u)) << (2 * i);
    }
    return m;
}
DFL_FN uint32_t dfl2_hash_of(const Dfl2Shared &S, int t) { return ((const uint16_t *)S.hw)[t]; }

// length of the match of p against the earlier position c (0: their first four bytes differ)
DFL_FN int dfl2_match(const uint8_t *in, int c, int p, int maxl) {
    if (dfl_load32(in + c) != dfl_load32(in + p)) return 0;
    int l = 4;
    bool open = true;
    while (open && l + 8 <= maxl) {
        const uint64_t x = dfl_load64(in + c + l) ^ dfl_load64(in + p + l);
        if (x) {
            l += (int)(__builtin_ctzll(x) >> 3);
            open = false;
        } else {
            l += 8;
        }
    }
    while (open && l < maxl && in[c + l] == in[p + l]) ++l;
    return l;
}

// the longest match among the DFL2_K most recent earlier positions of p's hash; of equal lengths the nearest
DFL_FN void dfl2_ph_find(Dfl2Shared &S, const uint8_t *in, int n, int base, int t) {
    const int p = base + t;
    const uint32_t h = dfl2_hash_of(S, t);
    int len = 0, dist = 0;
    if (h != DFL2_NO_HASH) {
        const int maxl = n - p < DFL_MAX_MATCH ? n - p : DFL_MAX_MATCH;
        int seen = 0;
#if DFL2_INBLOCK
        for (int g = t >> 5; g >= 0 && seen < DFL2_K && len < maxl; --g) {
            uint32_t m = dfl2_eq32(S, g, h);
            if (g == (t >> 5)) m &= (1u << (t & 31)) - 1;  // earlier positions only
            while (m && seen < DFL2_K && len < maxl) {     // the nearest first
                const int b = 31 - __builtin_clz(m), j = 32 * g + b;
                m &= ~(1u << b);
                ++seen;
                const int l = dfl2_match(in, base + j, p, maxl);
                if (l > len) len = l, dist = t - j;
            }
        }
#endif
        const uint16_t *b = (const uint16_t *)S.B.tab + h * DFL2_K;
        for (int k = 0; k < DFL2_K - seen && len < maxl; ++k) {
            const int e = b[k];
            if (!e) break;
            const int l = dfl2_match(in, e - 1, p, maxl);
            if (l > len) len = l, dist = p - (e - 1);
        }
    }
    S.B.mlen[t] = (uint16_t)len;
    S.B.mdist[t] = (uint16_t)dist;
}

DFL_FN uint32_t dfl2_token(uint32_t len, uint32_t dist) { return 0x80000000u | ((dist - 1) << 8) | (len - 3); }

// thread 0 alone appends one token (the emit phases are not running)
DFL_FN void dfl2_append(DflShared &S, uint32_t *tok, const uint8_t *in, int p, uint32_t len, uint32_t dist) {
    uint32_t word = in[p];
    if (len) {
        uint32_t eb, ev;
        word = dfl2_token(len, dist);
        S.hist[dfl_len_sym(len - 3, &eb, &ev)]++;
        S.hist[DFL_NLL + dfl_dist_sym(dist - 1, &eb, &ev)]++;
    } else {
        S.hist[word]++;
    }
    tok[S.ntok++] = word;
}

DFL_FN void dfl2_ph_insert_walk(Dfl2Shared &S, const uint8_t *in, int n, int base, uint32_t *tok, int t) {
    const uint32_t h = dfl2_hash_of(S, t);
    if (h != DFL2_NO_HASH) {
        bool last = true;  // of its hash in this sub-block: the bucket's one writer
        for (int g = t >> 5; g < DFL_THREADS / 32 && last; ++g) {
            uint32_t m = dfl2_eq32(S, g, h);
            if (g == (t >> 5)) m &= ~((2u << (t & 31)) - 1);  // later positions only
            last = m == 0;
        }
        if (last) {
            // the bucket as 8 lanes of 16 bits in two words: this position and the sub-block's earlier ones of the hash
            // in front, nearest first, the old entries moved back behind them
            uint64_t flo = (uint64_t)(base + t + 1), fhi = 0;
            int cnt = 1;
            for (int g = t >> 5; g >= 0 && cnt < DFL2_K; --g) {
                uint32_t m = dfl2_eq32(S, g, h);
                if (g == (t >> 5)) m &= (1u << (t & 31)) - 1;
                while (m && cnt < DFL2_K) {
                    const int b = 31 - __builtin_clz(m);
                    m &= ~(1u << b);
                    const uint64_t e = (uint64_t)(base + 32 * g + b + 1);
                    if (cnt < 4) flo |= e << (16 * cnt);
                    else fhi |= e << (16 * (cnt - 4));
                    ++cnt;
                }
            }
            uint16_t *b = (uint16_t *)S.B.tab + h * DFL2_K;
            uint64_t lo = 0, hi = 0;
            for (int k = 0; k < DFL2_K; ++k) {
                if (k < 4) lo |= (uint64_t)b[k] << (16 * k);
                else hi |= (uint64_t)b[k] << (16 * (k - 4));
            }
            const int sh = 16 * cnt;
            if (sh >= 128) {
                lo = hi = 0;
            } else if (sh >= 64) {
                hi = lo << (sh - 64);
                lo = 0;
            } else {
                hi = (hi << sh) | (lo >> (64 - sh));
                lo <<= sh;
            }
            lo |= flo;
            hi |= fhi;
            for (int k = 0; k < DFL2_K; ++k) b[k] = (uint16_t)(k < 4 ? lo >> (16 * k) : hi >> (16 * (k - 4)));
        }
    }
    if (t == 0) {
        uint8_t *flag = (uint8_t *)S.B.flagw;
        const int end = base + DFL_THREADS < n ? base + DFL_THREADS : n;
        int cur = (int)S.B.cur;
        if (S.pend) {  // cur == base - 1
            const bool lit = S.B.mlen[0] > S.pend_len;
            dfl2_append(S.B, tok, in, cur, lit ? 0u : S.pend_len, S.pend_dist);
            cur += lit ? 1 : (int)S.pend_len;
            S.pend = 0;
        }
        uint32_t cnt = 0;
        while (cur < end) {
            const int i = cur - base;
            int l = S.B.mlen[i];
#if DFL2_LAZY
            if (l && i + 1 < DFL_THREADS) {
                if (S.B.mlen[i + 1] > l) S.B.mlen[i] = 0, l = 0;  // (the emit phase reads the literal from mlen)
            } else if (l) {  // the sub-block's last position has a match: there is a next sub-block (l >= 4)
                S.pend = 1;
                S.pend_len = (uint32_t)l;
                S.pend_dist = S.B.mdist[i];
                break;
            }
#endif
            flag[i] = 1;
            cur += l ? l : 1;
            ++cnt;
        }
        S.B.cur = (uint32_t)cur;
        S.B.tokbase = S.B.ntok;
        S.B.ntok += cnt;
    }
}

// ---- codes ----
// code lengths (at most DFL2_CL_MAX_BITS) and codes of the code-length alphabet from cl_hist; thread 0 only.  The
// method is dfl_build_code's.  At least two symbols are in use: a literal/length code has two lengths or more of 257
// to 286 symbols, or unused symbols besides.
DFL_FN void dfl2_build_cl(Dfl2Shared &S) {
    int n = 0;
    for (int s = 0; s < DFL2_NCL; ++s) {
        S.cl_len[s] = 0;
        S.cl_code[s] = 0;
        const uint32_t f = S.cl_hist[s];
        if (!f) continue;
        int i = n++;  // insertion into rising (count, symbol)
        while (i > 0 && S.cl_hist[S.cl_ord[i - 1]] > f) {
            S.cl_ord[i] = S.cl_ord[i - 1];
            --i;
        }
        S.cl_ord[i] = (uint8_t)s;
    }
    uint32_t *A = S.cl_key;
    for (int i = 0; i < n; ++i) A[i] = S.cl_hist[S.cl_ord[i]];
    if (n == 1) {
        A[0] = 1;
    } else {
        A[0] += A[1];
        int root = 0, leaf = 2;
        for (int next = 1; next < n - 1; ++next) {
            if (leaf >= n || A[root] < A[leaf]) {
                A[next] = A[root];
                A[root++] = (uint32_t)next;
            } else {
                A[next] = A[leaf++];
            }
            if (leaf >= n || (root < next && A[root] < A[leaf])) {
                A[next] += A[root];
                A[root++] = (uint32_t)next;
            } else {
                A[next] += A[leaf++];
            }
        }
        A[n - 2] = 0;
        for (int next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
        int avbl = 1, used = 0, dpth = 0;
        root = n - 2;
        int next = n - 1;
        while (avbl > 0) {
            while (root >= 0 && (int)A[root] == dpth) {
                ++used;
                --root;
            }
            while (avbl > used) {
                A[next--] = (uint32_t)dpth;
                --avbl;
            }
            avbl = 2 * used;
            ++dpth;
            used = 0;
        }
    }
    uint32_t num[DFL2_CL_MAX_BITS + 1];
    for (int i = 0; i <= DFL2_CL_MAX_BITS; ++i) num[i] = 0;
    for (int i = 0; i < n; ++i) num[A[i] > DFL2_CL_MAX_BITS ? DFL2_CL_MAX_BITS : A[i]]++;
    if (n > 1) {
        uint32_t total = 0;
        for (int i = DFL2_CL_MAX_BITS; i > 0; --i) total += num[i] << (DFL2_CL_MAX_BITS - i);
        while (total != (1u << DFL2_CL_MAX_BITS)) {
            num[DFL2_CL_MAX_BITS]--;
            for (int i = DFL2_CL_MAX_BITS - 1; i > 0; --i)
                if (num[i]) {
                    num[i]--;
                    num[i + 1] += 2;
                    break;
                }
            --total;
        }
    }
    int j = n;
    for (int i = 1; i <= DFL2_CL_MAX_BITS; ++i)
        for (uint32_t l = num[i]; l > 0; --l) S.cl_len[S.cl_ord[--j]] = (uint8_t)i;
    uint32_t next_code[DFL2_CL_MAX_BITS + 2];
    uint32_t c = 0;
    num[0] = 0;
    for (int b = 1; b <= DFL2_CL_MAX_BITS; ++b) {
        c = (c + num[b - 1]) << 1;
        next_code[b] = c;
    }
    for (int s = 0; s < DFL2_NCL; ++s) {
        const int b = S.cl_len[s];
        if (b) S.cl_code[s] = (uint8_t)dfl_rev(next_code[b]++, b);
    }
}

DFL_FN void dfl2_hsym(Dfl2Shared &S, uint32_t sym, uint32_t extra) {
    S.hsym[S.nhs++] = (uint16_t)(sym | (extra << 5));
    S.cl_hist[sym]++;
}
DFL_FN uint32_t dfl2_cl_extra(uint32_t sym) { return sym < 16 ? 0u : sym == 16 ? 2u : sym == 17 ? 3u : 7u; }
DFL_FN uint32_t dfl2_cl_order(int i) {  // RFC 1951 §3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    return i < 3 ? 16u + (uint32_t)i : i == 3 ? 0u : (i & 1) ? 8u - (uint32_t)(i - 3) / 2 : 8u + (uint32_t)(i - 4) / 2;
}

// the HLIT + HDIST code lengths as one sequence of code-length symbols, their code, where each starts; thread 0 only
DFL_FN void dfl2_header_plan(Dfl2Shared &S) {
    const int hlit = (int)S.B.hlit, total = hlit + (int)S.B.hdist;
    for (int s = 0; s < DFL2_NCL; ++s) S.cl_hist[s] = 0;
    S.nhs = 0;
    int i = 0;
    while (i < total) {
        const uint32_t v = S.B.clen[i < hlit ? i : DFL_NLL + i - hlit];
        int run = 1;
        while (i + run < total && S.B.clen[i + run < hlit ? i + run : DFL_NLL + i + run - hlit] == v) ++run;
        i += run;
        if (v == 0) {
            while (run >= 11) {
                const int c = run < 138 ? run : 138;
                dfl2_hsym(S, 18, (uint32_t)c - 11);
                run -= c;
            }
            if (run >= 3) {
                dfl2_hsym(S, 17, (uint32_t)run - 3);
                run = 0;
            }
        } else {
            dfl2_hsym(S, v, 0);
            --run;
            while (run >= 3) {
                const int c = run < 6 ? run : 6;
                dfl2_hsym(S, 16, (uint32_t)c - 3);
                run -= c;
            }
        }
        for (; run > 0; --run) dfl2_hsym(S, v, 0);
    }
    dfl2_build_cl(S);
    int hclen = DFL2_NCL;
    while (hclen > 4 && !S.cl_len[dfl2_cl_order(hclen - 1)]) --hclen;
    S.hclen = (uint32_t)hclen;
    uint32_t pos = 17 + 3 * (uint32_t)hclen;  // BFINAL + BTYPE, HLIT, HDIST, HCLEN; the code-length code's lengths
    for (uint32_t k = 0; k < S.nhs; ++k) {
        const uint32_t sym = S.hsym[k] & 31;
        S.hoff[k] = (uint16_t)pos;
        pos += S.cl_len[sym] + dfl2_cl_extra(sym);
    }
    S.hdr_bits = pos;
}

DFL_FN void dfl2_ph_codes(Dfl2Shared &S2, int n, int t) {
    if (t != 0) return;
    DflShared &S = S2.B;
    dfl_build_code(S, 0, DFL_NLL);
    dfl_build_code(S, DFL_NLL, DFL_ND);
    int hlit = DFL_NLL, hdist = DFL_ND;
    while (hlit > 257 && !S.clen[hlit - 1]) --hlit;
    while (hdist > 1 && !S.clen[DFL_NLL + hdist - 1]) --hdist;
    S.hlit = (uint32_t)hlit;
    S.hdist = (uint32_t)hdist;
#if DFL2_RLE
    dfl2_header_plan(S2);
#else
    S2.hdr_bits = DFL_HDR_FIXED_BITS + 4u * (uint32_t)(hlit + hdist);
#endif
    uint64_t bits = S2.hdr_bits;
    for (int s = 0; s < DFL_NLL; ++s) bits += (uint64_t)S.hist[s] * (S.clen[s] + (s > 256 ? dfl_len_extra(s) : 0u));
    for (int s = 0; s < DFL_ND; ++s) bits += (uint64_t)S.hist[DFL_NLL + s] * (S.clen[DFL_NLL + s] + dfl_dist_extra(s));
    const uint64_t bytes = (bits + 7) >> 3;
    S.stored = (bytes >= (uint64_t)n + DFL_STORED_OVERHEAD || bytes > (uint64_t)(DFL_TAB - 1) * 4) ? 1u : 0u;
    S.dfl_bytes = S.stored ? (uint32_t)n + DFL_STORED_OVERHEAD : (uint32_t)bytes;
}

// ---- bits ----
DFL_FN void dfl2_ph_header(Dfl2Shared &S, int t) {
#if DFL2_RLE
    if (t == 0) {
        dfl_put(S.B, 0, 1u | (2u << 1), 3);  // BFINAL, BTYPE = 10
        dfl_put(S.B, 3, S.B.hlit - 257, 5);
        dfl_put(S.B, 8, S.B.hdist - 1, 5);
        dfl_put(S.B, 13, S.hclen - 4, 4);
        S.B.bitpos = S.hdr_bits;
    }
    if (t < (int)S.hclen) dfl_put(S.B, 17 + 3 * (uint32_t)t, S.cl_len[dfl2_cl_order(t)], 3);
    for (uint32_t k = (uint32_t)t; k < S.nhs; k += DFL_THREADS) {
        const uint32_t sym = S.hsym[k] & 31, len = S.cl_len[sym];
        dfl_put(S.B, S.hoff[k], S.cl_code[sym] | ((uint32_t)(S.hsym[k] >> 5) << len), len + dfl2_cl_extra(sym));
    }
#else
    dfl_ph_header(S.B, t);
#endif
}

// One chunk in[0, n), 1 <= n <= DFL_CHUNK, -> the member at slot: dfl_encode_chunk's contract, level 2's bytes.
DFL_FN void dfl2_encode_chunk(Dfl2Shared &S, const uint8_t *in, int n, uint32_t *tok, uint8_t *slot, uint32_t *msize) {
    DFL_PHASE(dfl2_ph_init(S, t))
    for (int base = 0; base < n; base += DFL_THREADS) {
        DFL_PHASE(dfl2_ph_hash(S, in, n, base, t))
        DFL_PHASE(dfl2_ph_find(S, in, n, base, t))
        DFL_PHASE(dfl2_ph_insert_walk(S, in, n, base, tok, t))
        DFL_PHASE(dfl_ph_emit(S.B, in, base, tok, t))
    }
    DFL_PHASE(dfl_ph_crc(S.B, in, n, t); dfl_ph_rank(S.B, t))
    DFL_PHASE(dfl2_ph_codes(S, n, t))
    if (!S.B.stored) {
        DFL_PHASE(dfl2_ph_header(S, t))
        const uint32_t ntok = S.B.ntok;
        for (uint32_t r0 = 0; r0 <= ntok; r0 += DFL_THREADS) {
            DFL_PHASE(dfl_ph_sizes(S.B, tok, r0, t))
            DFL_PHASE(dfl_ph_pack(S.B, tok, r0, t))
        }
    }
    DFL_PHASE(dfl_ph_member(S.B, in, n, slot, msize, t))
}
