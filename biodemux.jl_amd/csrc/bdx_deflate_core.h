// bdx_deflate_core.h — one chunk of text -> one complete gzip member, written as barrier-separated phases of a
// 256-thread workgroup (private; included by bdx_deflate.hip).  Every phase is a function of (shared state, thread
// index); DFL_PHASE runs it for the workgroup's threads and ends with a barrier.  No phase keeps a value in a
// register across a barrier and no phase uses a cross-lane operation, so the same text also compiles as plain C++,
// where DFL_PHASE is a loop over the thread index: the encoder can be stepped through on a CPU.
//
// Member (RFC 1952, the layout of deflate_gz_members in bdx_io.cpp): 10-byte header with FEXTRA and OS = 255,
// XLEN = 8, subfield 'D','X' (4 bytes LE: the member's total size), one deflate block, CRC-32, ISIZE.
//
// Stages:
//   tokens   sub-blocks of 256 positions: every thread looks its position's 4-byte hash up in an LDS table that holds
//            the positions of EARLIER sub-blocks only and extends the candidate by comparing bytes; then all threads
//            insert with an atomic max on the position (the table's content never depends on thread order) and thread 0
//            walks the greedy parse through the sub-block; flagged positions append their tokens in position order.
//   codes    rank sort of the histograms by all threads, then thread 0: Moffat-Katajainen code lengths, limited to 15
//            bits by moving Kraft weight (complete by construction), canonical codes.
//   bits     256 tokens a round: bit lengths, prefix sum, atomic OR into an LDS bit buffer (the hash table's memory)
//            — OR commutes, the bytes do not depend on the order.  A chunk that would not shrink is one stored block.
//   crc      256 slices, table in LDS, combined as XOR of crc_t * x^(8 * bytes after slice t) mod P.
#pragma once
#include <stdint.h>

#include "bdx_crc32_core.h"

#define DFL_CHUNK 32768      // uncompressed bytes of a member at most (distances and positions fit 15 bits)
#define DFL_THREADS 256
#define DFL_HASH_BITS 13
#define DFL_TAB (1 << DFL_HASH_BITS)
#define DFL_NLL 286
#define DFL_ND 30
#define DFL_NSYM (DFL_NLL + DFL_ND)
#define DFL_MIN_MATCH 4
#define DFL_MAX_MATCH 258
#define DFL_MAX_BITS 15
#define DFL_HDR_FIXED_BITS 74  // BFINAL + BTYPE (3), HLIT (5), HDIST (5), HCLEN (4), 19 code-length code lengths (57)
#define DFL_MEMBER_OVERHEAD 28 // gzip header with the 'D','X' subfield (20) + CRC-32 + ISIZE (8)
#define DFL_STORED_OVERHEAD 5  // stored block: header byte, LEN, NLEN
#define DFL_CRC_POLY BDX_CRC_POLY

#if defined(__HIPCC__)
#define DFL_FN __device__ inline
#define DFL_PHASE(call)                \
    {                                  \
        const int t = (int)threadIdx.x; \
        call;                          \
    }                                  \
    __syncthreads();
#define DFL_ATOMIC_MAX(p, v) atomicMax((p), (v))
#define DFL_ATOMIC_ADD(p, v) atomicAdd((p), (v))
#define DFL_ATOMIC_OR(p, v) atomicOr((p), (v))
#define DFL_ATOMIC_XOR(p, v) atomicXor((p), (v))
#else
#define DFL_FN inline
#define DFL_PHASE(call) \
    for (int t = 0; t < DFL_THREADS; ++t) { call; }
#define DFL_ATOMIC_MAX(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#define DFL_ATOMIC_ADD(p, v) (*(p) += (v))
#define DFL_ATOMIC_OR(p, v) (*(p) |= (v))
#define DFL_ATOMIC_XOR(p, v) (*(p) ^= (v))
#endif

struct DflShared {
    uint32_t tab[DFL_TAB];        // tokens: hash -> position + 1 (0: empty); bits: the bit buffer
    uint32_t hist[DFL_NSYM];      // literal/length counts, then distance counts
    uint32_t key[DFL_NSYM];       // counts in rising order; then depths
    uint16_t order[DFL_NSYM];     // symbols in rising order of (count, symbol)
    uint16_t code[DFL_NSYM];      // bit-reversed canonical codes
    uint8_t clen[DFL_NSYM];
    uint32_t scan[DFL_THREADS];
    uint16_t mlen[DFL_THREADS], mdist[DFL_THREADS], hsh[DFL_THREADS];
    uint32_t flagw[DFL_THREADS / 4];  // one byte per position of the sub-block: a token starts here
    uint32_t crc_tab[256];
    uint32_t x2n[32];             // x^(2^k) mod P
    uint32_t cur, ntok, tokbase, crc, hlit, hdist, stored, dfl_bytes, bitpos, round_bits;
};

DFL_FN uint32_t dfl_load32(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
DFL_FN uint64_t dfl_load64(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// ---- CRC-32 arithmetic: bdx_crc32_core.h (shared with the device inflate) ----
DFL_FN uint32_t dfl_multmodp(uint32_t a, uint32_t b) { return bdx_crc_multmodp(a, b); }
// x^(8 n) mod P
DFL_FN uint32_t dfl_x8n(const DflShared &S, uint32_t n) { return bdx_crc_x8n(S.x2n, n); }

// once per workgroup
DFL_FN void dfl_ph_tables(DflShared &S, int t) {
    S.crc_tab[t] = bdx_crc_table_entry(t);
    if (t == 0) bdx_crc_x2n_init(S.x2n);
}

DFL_FN void dfl_ph_init(DflShared &S, int t) {
    for (int i = t; i < DFL_TAB; i += DFL_THREADS) S.tab[i] = 0;
    for (int i = t; i < DFL_NSYM; i += DFL_THREADS) S.hist[i] = 0;
    if (t == 0) {
        S.hist[256] = 1;  // end of block (thread 0 also cleared it)
        S.cur = S.ntok = S.tokbase = S.crc = 0;
        S.bitpos = S.round_bits = 0;
    }
}

// ---- tokens ----
// token word: literal = the byte; match = bit 31 | (distance - 1) << 8 | (length - 3)
DFL_FN void dfl_ph_find(DflShared &S, const uint8_t *in, int n, int base, int t) {
    const int p = base + t;
    if ((t & 3) == 0) S.flagw[t >> 2] = 0;
    uint32_t len = 0, dist = 0, h = 0xFFFFu;
    if (p + DFL_MIN_MATCH <= n) {
        const uint32_t w = dfl_load32(in + p);
        h = (w * 2654435761u) >> (32 - DFL_HASH_BITS);
        const uint32_t e = S.tab[h];
        if (e && dfl_load32(in + e - 1) == w) {
            const int c = (int)e - 1;
            const int maxl = n - p < DFL_MAX_MATCH ? n - p : DFL_MAX_MATCH;
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
            len = (uint32_t)l;
            dist = (uint32_t)(p - c);
        }
    }
    S.mlen[t] = (uint16_t)len;
    S.mdist[t] = (uint16_t)dist;
    S.hsh[t] = (uint16_t)h;
}

DFL_FN void dfl_ph_insert_walk(DflShared &S, int n, int base, int t) {
    const uint32_t h = S.hsh[t];
    if (h != 0xFFFFu) DFL_ATOMIC_MAX(&S.tab[h], (uint32_t)(base + t + 1));
    if (t == 0) {
        uint8_t *flag = (uint8_t *)S.flagw;
        const int end = base + DFL_THREADS < n ? base + DFL_THREADS : n;
        int cur = (int)S.cur;
        uint32_t cnt = 0;
        while (cur < end) {
            const int i = cur - base;
            flag[i] = 1;
            const int l = S.mlen[i];
            cur += l ? l : 1;
            ++cnt;
        }
        S.cur = (uint32_t)cur;
        S.tokbase = S.ntok;
        S.ntok += cnt;
    }
}

DFL_FN uint32_t dfl_popc(uint32_t v) { return (uint32_t)__builtin_popcount(v); }

DFL_FN uint32_t dfl_len_sym(uint32_t l, uint32_t *ebits, uint32_t *eval) {  // l = length - 3
    if (l < 8) {
        *ebits = 0, *eval = 0;
        return 257 + l;
    }
    if (l == 255) {
        *ebits = 0, *eval = 0;
        return 285;
    }
    const uint32_t e = (31 - (uint32_t)__builtin_clz(l)) - 2;
    *ebits = e;
    *eval = l & ((1u << e) - 1);
    return 257 + 4 * (e + 1) + ((l >> e) & 3);
}
DFL_FN uint32_t dfl_dist_sym(uint32_t d, uint32_t *ebits, uint32_t *eval) {  // d = distance - 1
    if (d < 4) {
        *ebits = 0, *eval = 0;
        return d;
    }
    const uint32_t hb = 31 - (uint32_t)__builtin_clz(d);
    const uint32_t e = hb - 1;
    *ebits = e;
    *eval = d & ((1u << e) - 1);
    return 2 * hb + ((d >> e) & 1);
}

DFL_FN void dfl_ph_emit(DflShared &S, const uint8_t *in, int base, uint32_t *tok, int t) {
    const uint8_t *flag = (const uint8_t *)S.flagw;
    if (!flag[t]) return;
    uint32_t idx = 0;
    for (int j = 0; j < (t >> 2); ++j) idx += dfl_popc(S.flagw[j]);
    idx += dfl_popc(S.flagw[t >> 2] & ((1u << (8 * (t & 3))) - 1));
    const uint32_t l = S.mlen[t];
    uint32_t word;
    if (l) {
        const uint32_t d = (uint32_t)S.mdist[t] - 1;
        word = 0x80000000u | (d << 8) | (l - 3);
        uint32_t eb, ev;
        DFL_ATOMIC_ADD(&S.hist[dfl_len_sym(l - 3, &eb, &ev)], 1u);
        DFL_ATOMIC_ADD(&S.hist[DFL_NLL + dfl_dist_sym(d, &eb, &ev)], 1u);
    } else {
        word = in[base + t];
        DFL_ATOMIC_ADD(&S.hist[word], 1u);
    }
    tok[S.tokbase + idx] = word;
}

// ---- codes ----
DFL_FN void dfl_ph_rank(DflShared &S, int t) {
    for (int i = t; i < DFL_TAB; i += DFL_THREADS) S.tab[i] = 0;  // the hash table becomes the bit buffer
    for (int s = t; s < DFL_NSYM; s += DFL_THREADS) {
        S.clen[s] = 0;
        S.code[s] = 0;
        const uint32_t f = S.hist[s];
        if (!f) continue;
        const int lo = s < DFL_NLL ? 0 : DFL_NLL, hi = s < DFL_NLL ? DFL_NLL : DFL_NSYM;
        int rank = 0;
        for (int j = lo; j < hi; ++j) {
            const uint32_t g = S.hist[j];
            rank += (g && (g < f || (g == f && j < s))) ? 1 : 0;
        }
        S.order[lo + rank] = (uint16_t)(s - lo);
    }
}

DFL_FN uint32_t dfl_rev(uint32_t v, int bits) {
    uint32_t r = 0;
    for (int i = 0; i < bits; ++i) r |= ((v >> i) & 1u) << (bits - 1 - i);
    return r;
}

// code lengths and codes of one alphabet (symbols first .. first + nsym) from its sorted counts; thread 0 only
DFL_FN void dfl_build_code(DflShared &S, int first, int nsym) {
    int n = 0;
    for (int s = 0; s < nsym; ++s) n += S.hist[first + s] ? 1 : 0;
    if (n == 0) return;
    uint32_t *A = S.key + first;
    const uint16_t *ord = S.order + first;
    for (int i = 0; i < n; ++i) A[i] = S.hist[first + ord[i]];
    // Moffat & Katajainen, in-place minimum-redundancy code lengths over rising counts
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
    // A[i]: depth of the i-th rarest symbol.  Limit to 15 bits on the counts per length: fold the deeper codes into
    // length 15, then give Kraft weight back until the code is complete again.
    uint32_t num[DFL_MAX_BITS + 1];
    for (int i = 0; i <= DFL_MAX_BITS; ++i) num[i] = 0;
    for (int i = 0; i < n; ++i) num[A[i] > DFL_MAX_BITS ? DFL_MAX_BITS : A[i]]++;
    if (n > 1) {
        uint32_t total = 0;
        for (int i = DFL_MAX_BITS; i > 0; --i) total += num[i] << (DFL_MAX_BITS - i);
        while (total != (1u << DFL_MAX_BITS)) {
            num[DFL_MAX_BITS]--;
            for (int i = DFL_MAX_BITS - 1; i > 0; --i)
                if (num[i]) {
                    num[i]--;
                    num[i + 1] += 2;
                    break;
                }
            --total;
        }
    }
    int j = n;
    for (int i = 1; i <= DFL_MAX_BITS; ++i)
        for (uint32_t l = num[i]; l > 0; --l) S.clen[first + ord[--j]] = (uint8_t)i;
    // canonical codes (RFC 1951 §3.2.2), stored bit-reversed: the stream takes Huffman codes most significant bit first
    uint32_t next_code[DFL_MAX_BITS + 2];
    uint32_t c = 0;
    num[0] = 0;
    for (int b = 1; b <= DFL_MAX_BITS; ++b) {
        c = (c + num[b - 1]) << 1;
        next_code[b] = c;
    }
    for (int s = 0; s < nsym; ++s) {
        const int b = S.clen[first + s];
        if (b) S.code[first + s] = (uint16_t)dfl_rev(next_code[b]++, b);
    }
}

DFL_FN uint32_t dfl_len_extra(int sym) {  // extra bits of length symbol 257..285
    return (sym < 265 || sym == 285) ? 0u : (uint32_t)(sym - 261) >> 2;
}
DFL_FN uint32_t dfl_dist_extra(int sym) { return sym < 4 ? 0u : (uint32_t)(sym - 2) >> 1; }

DFL_FN void dfl_ph_codes(DflShared &S, int n, int t) {
    if (t != 0) return;
    dfl_build_code(S, 0, DFL_NLL);
    dfl_build_code(S, DFL_NLL, DFL_ND);
    int hlit = DFL_NLL, hdist = DFL_ND;
    while (hlit > 257 && !S.clen[hlit - 1]) --hlit;
    while (hdist > 1 && !S.clen[DFL_NLL + hdist - 1]) --hdist;
    uint64_t bits = DFL_HDR_FIXED_BITS + 4u * (uint32_t)(hlit + hdist);
    for (int s = 0; s < DFL_NLL; ++s) bits += (uint64_t)S.hist[s] * (S.clen[s] + (s > 256 ? dfl_len_extra(s) : 0u));
    for (int s = 0; s < DFL_ND; ++s) bits += (uint64_t)S.hist[DFL_NLL + s] * (S.clen[DFL_NLL + s] + dfl_dist_extra(s));
    const uint64_t bytes = (bits + 7) >> 3;
    S.hlit = (uint32_t)hlit;
    S.hdist = (uint32_t)hdist;
    // (the bit buffer takes DFL_TAB words; the last one stays free for the second word of the last code)
    S.stored = (bytes >= (uint64_t)n + DFL_STORED_OVERHEAD || bytes > (uint64_t)(DFL_TAB - 1) * 4) ? 1u : 0u;
    S.dfl_bytes = S.stored ? (uint32_t)n + DFL_STORED_OVERHEAD : (uint32_t)bytes;
}

// ---- bits ----
DFL_FN void dfl_put(DflShared &S, uint32_t bitpos, uint32_t val, uint32_t nbits) {  // nbits <= 28
    if (!nbits) return;
    const uint64_t v = (uint64_t)val << (bitpos & 31);
    const uint32_t w = bitpos >> 5;
    if ((uint32_t)v) DFL_ATOMIC_OR(&S.tab[w], (uint32_t)v);
    if ((uint32_t)(v >> 32)) DFL_ATOMIC_OR(&S.tab[w + 1], (uint32_t)(v >> 32));
}

DFL_FN void dfl_ph_header(DflShared &S, int t) {
    if (t == 0) {
        dfl_put(S, 0, 1u | (2u << 1), 3);  // BFINAL, BTYPE = 10
        dfl_put(S, 3, S.hlit - 257, 5);
        dfl_put(S, 8, S.hdist - 1, 5);
        dfl_put(S, 13, 15, 4);  // all 19 code-length code lengths follow
        // order 16 17 18 0 8 7 ...: the three run-length symbols are unused, the 16 plain lengths take 4 bits each
        for (uint32_t i = 3; i < 19; ++i) dfl_put(S, 17 + 3 * i, 4, 3);
        S.bitpos = DFL_HDR_FIXED_BITS + 4 * (S.hlit + S.hdist);
    }
    for (uint32_t i = (uint32_t)t; i < S.hlit + S.hdist; i += DFL_THREADS) {
        const uint32_t l = i < S.hlit ? S.clen[i] : S.clen[DFL_NLL + i - S.hlit];
        dfl_put(S, DFL_HDR_FIXED_BITS + 4 * i, dfl_rev(l, 4), 4);
    }
}

// the two pieces of token r (r == ntok: end of block): literal/length code + extra, distance code + extra
DFL_FN void dfl_token_bits(const DflShared &S, const uint32_t *tok, uint32_t r, uint32_t *v1, uint32_t *n1, uint32_t *v2,
                           uint32_t *n2) {
    *v1 = *n1 = *v2 = *n2 = 0;
    if (r > S.ntok) return;
    if (r == S.ntok) {
        *v1 = S.code[256];
        *n1 = S.clen[256];
        return;
    }
    const uint32_t w = tok[r];
    if (!(w & 0x80000000u)) {
        *v1 = S.code[w];
        *n1 = S.clen[w];
        return;
    }
    uint32_t eb, ev;
    const uint32_t ls = dfl_len_sym(w & 0xFF, &eb, &ev);
    *v1 = S.code[ls] | (ev << S.clen[ls]);
    *n1 = S.clen[ls] + eb;
    const uint32_t ds = DFL_NLL + dfl_dist_sym((w >> 8) & 0x7FFF, &eb, &ev);
    *v2 = S.code[ds] | (ev << S.clen[ds]);
    *n2 = S.clen[ds] + eb;
}

DFL_FN void dfl_ph_sizes(DflShared &S, const uint32_t *tok, uint32_t r0, int t) {
    if (t == 0) S.bitpos += S.round_bits;  // (the previous round's)
    uint32_t v1, n1, v2, n2;
    dfl_token_bits(S, tok, r0 + (uint32_t)t, &v1, &n1, &v2, &n2);
    S.scan[t] = n1 + n2;
}

DFL_FN void dfl_ph_pack(DflShared &S, const uint32_t *tok, uint32_t r0, int t) {
    uint32_t before = 0, all = 0;
    for (int j = 0; j < DFL_THREADS; ++j) {
        const uint32_t b = S.scan[j];
        before += j < t ? b : 0u;
        all += b;
    }
    uint32_t v1, n1, v2, n2;
    dfl_token_bits(S, tok, r0 + (uint32_t)t, &v1, &n1, &v2, &n2);
    const uint32_t at = S.bitpos + before;
    dfl_put(S, at, v1, n1);
    dfl_put(S, at + n1, v2, n2);
    if (t == 0) S.round_bits = all;
}

// ---- crc ----
DFL_FN void dfl_ph_crc(DflShared &S, const uint8_t *in, int n, int t) {
    const int per = (n + DFL_THREADS - 1) / DFL_THREADS;
    const int a = t * per < n ? t * per : n;
    const int b = a + per < n ? a + per : n;
    if (a >= b) return;
    uint32_t c = 0xFFFFFFFFu;
    for (int i = a; i < b; ++i) c = S.crc_tab[(c ^ in[i]) & 0xFF] ^ (c >> 8);
    c ^= 0xFFFFFFFFu;
    DFL_ATOMIC_XOR(&S.crc, dfl_multmodp(dfl_x8n(S, (uint32_t)(n - b)), c));
}

// ---- member ----
DFL_FN void dfl_ph_member(DflShared &S, const uint8_t *in, int n, uint8_t *slot, uint32_t *msize, int t) {
    const uint32_t nb = S.dfl_bytes;
    uint8_t *body = slot + 20;  // (slots are 64-byte aligned: body is word aligned)
    if (S.stored) {
        for (int i = t; i < n; i += DFL_THREADS) body[DFL_STORED_OVERHEAD + i] = in[i];
    } else {
        uint32_t *bw = (uint32_t *)body;
        for (uint32_t i = (uint32_t)t; i < (nb >> 2); i += DFL_THREADS) bw[i] = S.tab[i];
    }
    if (t != 0) return;
    const uint32_t total = nb + DFL_MEMBER_OVERHEAD;
    const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 255, 8, 0, 'D', 'X', 4, 0};
    for (int i = 0; i < 16; ++i) slot[i] = head[i];
    for (int i = 0; i < 4; ++i) slot[16 + i] = (uint8_t)(total >> (8 * i));
    if (S.stored) {
        body[0] = 1;  // BFINAL, BTYPE = 00
        body[1] = (uint8_t)n;
        body[2] = (uint8_t)(n >> 8);
        body[3] = (uint8_t)~n;
        body[4] = (uint8_t)(~n >> 8);
    } else {
        for (uint32_t i = nb & ~3u; i < nb; ++i) body[i] = (uint8_t)(S.tab[i >> 2] >> (8 * (i & 3)));
    }
    uint8_t *tail = body + nb;
    for (int i = 0; i < 4; ++i) tail[i] = (uint8_t)(S.crc >> (8 * i));
    for (int i = 0; i < 4; ++i) tail[4 + i] = (uint8_t)((uint32_t)n >> (8 * i));
    *msize = total;
}

// One chunk in[0, n), 1 <= n <= DFL_CHUNK, -> the member at slot (n + 33 bytes at most, 64-byte aligned); tok: DFL_CHUNK
// words of this workgroup's own.  Called by all threads of the workgroup, after dfl_ph_tables.
DFL_FN void dfl_encode_chunk(DflShared &S, const uint8_t *in, int n, uint32_t *tok, uint8_t *slot, uint32_t *msize) {
    DFL_PHASE(dfl_ph_init(S, t))
    for (int base = 0; base < n; base += DFL_THREADS) {
        DFL_PHASE(dfl_ph_find(S, in, n, base, t))
        DFL_PHASE(dfl_ph_insert_walk(S, n, base, t))
        DFL_PHASE(dfl_ph_emit(S, in, base, tok, t))
    }
    DFL_PHASE(dfl_ph_crc(S, in, n, t); dfl_ph_rank(S, t))
    DFL_PHASE(dfl_ph_codes(S, n, t))
    if (!S.stored) {
        DFL_PHASE(dfl_ph_header(S, t))
        const uint32_t ntok = S.ntok;
        for (uint32_t r0 = 0; r0 <= ntok; r0 += DFL_THREADS) {
            DFL_PHASE(dfl_ph_sizes(S, tok, r0, t))
            DFL_PHASE(dfl_ph_pack(S, tok, r0, t))
        }
    }
    DFL_PHASE(dfl_ph_member(S, in, n, slot, msize, t))
}
