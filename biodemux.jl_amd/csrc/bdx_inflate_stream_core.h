// bdx_inflate_stream_core.h — a whole .gz file (ordinary gzip members of any size, tagged or not) -> its plain bytes,
// inflated from SPECULATIVE block starts (pugz, Kerbiriou & Chikhi 2019).  Private; included by bdx_inflate_stream.hip.
// Written in the phase idiom of bdx_inflate_core.h, whose header parser, block reader, table layout, lookup and token
// walk it calls as they are: one wavefront per workgroup (the tails step alone takes a larger workgroup), every phase a
// function of (shared state, thread index), no cross-lane operation; the same text compiles as plain C++.
//
// The file is cut at multiples of chunk_bytes.  Six steps, each a kernel (ordering comes from kernel boundaries only,
// no workgroup ever waits for another one's flag):
//   scan     (steps 1 + 2) one wave per chunk k.  Chunk 0 parses the first gzip header: its first block start is exact.
//            Chunk k >= 1 SEARCHES: its lanes try consecutive bit offsets, the first one that passes the candidate rule
//            (BTYPE 2, HLIT <= 29, HDIST <= 29, a complete code-length code, exactly nl + nd lengths, both code sets
//            taken by inf_layout, a code for symbol 256) is s_k.  Stored and fixed blocks are not searched for.  The
//            wave then COUNTS: it decodes from s_k block by block, lengths only (no window is needed to count), up to
//            the first block end at or beyond the next chunk's first bit or a final block's end: InfsRecord
//   chain    (step 3) one wave.  It starts at the first header and hops: when the confirmed position equals the start
//            of the record of the chunk it lies in, the record's work is accepted; otherwise the wave walks on itself,
//            counting, until it lands on a later chunk's candidate or the member ends.  At a member's end it wants the
//            trailer, then parses the next header exactly as inf_ph_begin does.  -> InfsSegment list with exact start
//            bit, end bit, plain offset (prefix sum) and member; the plain size of the file is known here
//   decode   (step 4) one wave per segment into a 16-bit staging image: a literal is its value, a source byte that lies
//            in front of the segment's own start at relative position q in [-32768, 0) is the marker 0x8000 + q + 32768;
//            copies of markers copy the marker
//   tails    (step 5) ONE workgroup walks the segments in order and resolves each one's last 32 KiB (all of it when it
//            is shorter) against the final bytes in front of it: the union of the earlier tails covers them
//   rest     (step 6) one wave per segment resolves what is left of it against the tails in front of it, then takes
//            the segment's CRC-32 in 64 slices
//   verdict  one wave combines the segment CRCs per member and holds them and the sizes to the trailers
//
// Exactness never rests on a guess: a record is used only when a decoder that started from a confirmed position
// arrived exactly at its start bit (a block then really starts there, and the record is what a decode from there
// gives).  A wrong or missing guess costs speed only.
// No hang: every loop consumes bits of comp (at least 3 per block, 1 per token) or bytes of the output.
// Bounds: no byte outside comp[0, comp_len) is read; the staging image and the output are written inside
// [0, total) only, a segment inside [off, off + n).
//
// 64-bit positions on a 32-bit decoder: before every phase of bdx_inflate_core.h the view is REBASED — comp is handed
// over from the byte the bit position lies in, the limit is what is left of the file (clipped to 2^30), the output
// counter restarts at 32768 (every distance is then legal: what lies in front of the segment is a marker).
#pragma once
#include "bdx_inflate_core.h"

#define INFS_CHUNK_DEFAULT 131072  // the best of 16, 32, 64 and 128 KiB on the 10 M read file (profiles/r08_e2e_gunzip_stream.json)
#define INFS_CHUNK_MIN 64
#define INFS_CHUNK_MAX (1 << 24)
#define INFS_WINDOW 32768u
#ifndef INFS_REBASE  // (a test build sets a small one: the rebasing is then reached by files of a few hundred KB)
#define INFS_REBASE (1u << 30)
#endif
// one phase consumes at most a stored block of 65 535 bytes and its header, and lists at most 65 535 bytes
static_assert(INFS_REBASE >= (1u << 17) && INFS_REBASE <= (1u << 30), "INFS_REBASE: a phase's bytes fit the view, the view fits 31 bits");
#define INFS_TAIL_THREADS 1024
#define INFS_NONE (~(uint64_t)0)
#define INFS_E_INTERNAL 12  // a segment decoded to something else than it counted to (cannot happen)

#define INFS_F_FINAL 1u   // the segment ends with its member's final block: crc_want and isize_want are the trailer's
#define INFS_F_START 2u   // the segment begins its member ("member start")
#define INFS_F_GUESS 4u   // the segment is the accepted work of a chunk's guessed block start

#if defined(__HIPCC__)
#define INFS_PHASE_WG(call)             \
    {                                   \
        const int t = (int)threadIdx.x; \
        const int nt = (int)blockDim.x; \
        call;                           \
    }                                   \
    __syncthreads();
#else
#define INFS_PHASE_WG(call) \
    for (int t = 0, nt = INFS_TAIL_THREADS; t < nt; ++t) { call; }
#endif

struct InfsRecord {   // what chunk k's wave found
    uint64_t s, e, n;  // first candidate (INFS_NONE: none), where the count stopped, plain bytes between them
    uint32_t status, final;
};
struct InfsSegment {
    uint64_t s, e, off, n;  // bits of comp, place in the plain text
    uint64_t member_first;  // plain offset of its member's first byte
    uint64_t member_comp;   // byte of comp its member begins at
    uint32_t member, flags, crc_want, isize_want, crc, status;
};
struct InfsResult {
    uint64_t total, n_seg, at;  // plain bytes, segments (more than the list holds: call again with that room), byte of comp the refusal is at
    int64_t info[8];
    uint32_t status, member;
};

struct InfsShared {
    InfShared S;
    uint64_t bit, n, base, g_at, cp_at;  // absolute bit position; plain bytes of this run; the view's byte; where the group / the stored block goes
    uint64_t pos, found;                 // search
    uint8_t cand[INF_THREADS];
    uint64_t c_off, c_total, c_nseg, c_seg_s, c_first, c_member_comp, c_longest;  // chain
    uint32_t c_member, c_landed, c_hit, c_more, c_start, c_guess, c_confirmed;
    uint32_t crc, v_bad;
};

// ---- the rebased view ----
INF_FN void infs_enter(InfsShared &X, int64_t comp_len) {
    X.base = X.bit >> 3;
    const uint64_t left = (uint64_t)comp_len - X.base;  // (bit <= 8 * comp_len always)
    X.S.bitpos = X.bit & 7;
    X.S.lim = (uint32_t)(left < INFS_REBASE ? left : INFS_REBASE);
    X.S.out = INFS_WINDOW;
}
INF_FN void infs_leave(InfsShared &X) {
    X.bit = X.base * 8 + X.S.bitpos;
    X.n += X.S.out - INFS_WINDOW;
}
INF_FN int infs_plen(const InfsShared &X, uint64_t cap) {
    const uint64_t room = cap - X.n;
    return (int)(INFS_WINDOW + (room < INFS_REBASE ? room : INFS_REBASE));
}
INF_FN void infs_ph_start(InfsShared &X, uint64_t bit, int t) {
    if (t != 0) return;
    X.bit = bit;
    X.n = 0;
    X.S.state = INF_RUN;
    X.S.status = INF_OK;
    X.S.final = 0;
    X.S.eob = 0;
}
// a block header at X.bit; a stored block is then comp[base + cp_src, +cp_n) -> plain byte cp_at of the run
INF_FN void infs_ph_block(InfsShared &X, const uint8_t *comp, int64_t comp_len, uint64_t cap, int t) {
    if (t != 0) return;
    infs_enter(X, comp_len);
    X.cp_at = X.n;
    X.S.cp_n = 0;
    inf_ph_block(X.S, comp + X.base, infs_plen(X, cap), 0);
    if (X.S.state != INF_RUN) return;
    infs_leave(X);
    if (X.S.kind == 0 && X.S.final) X.S.state = INF_END;
}
INF_FN void infs_ph_tokens(InfsShared &X, const uint8_t *comp, int64_t comp_len, uint64_t cap, int t) {
    if (t != 0) return;
    infs_enter(X, comp_len);
    X.g_at = X.n;
    inf_ph_tokens(X.S, comp + X.base, infs_plen(X, cap), 0);
    infs_leave(X);
}
// a gzip header at byte X.c_off -> X.bit, its first block
INF_FN void infs_ph_member(InfsShared &X, const uint8_t *comp, int64_t comp_len, int t) {
    if (t != 0) return;
    const uint64_t left = (uint64_t)comp_len - X.c_off;
    inf_ph_begin(X.S, comp + X.c_off, (int)(left < INFS_REBASE ? left : INFS_REBASE), 0, 0);
    X.bit = X.c_off * 8 + X.S.bitpos;
    X.n = 0;
}

// one block from X.bit, lengths only; then X.bit is its end, X.n has its bytes, state says RUN / END (it was final) / BAD
INF_FN void infs_count_block(InfsShared &X, const uint8_t *comp, int64_t comp_len) {
    INF_PHASE(infs_ph_block(X, comp, comp_len, INFS_NONE, t))
    if (X.S.state != INF_RUN || X.S.kind == 0) return;
    INF_PHASE(inf_ph_codes(X.S, t))
    if (X.S.state != INF_RUN) return;
    INF_PHASE(inf_ph_fill(X.S, t))
    bool more = true;
    while (more) {
        INF_PHASE(infs_ph_tokens(X, comp, comp_len, INFS_NONE, t))
        more = X.S.state == INF_RUN && !X.S.eob;
    }
}

// ---- scan: search ----
// n <= 25 bits at `bit`, LSB first; false when they are not all inside the file
INF_FN bool infs_peek(const uint8_t *comp, int64_t comp_len, uint64_t bit, int n, uint32_t &v) {
    if (bit + (uint64_t)n > (uint64_t)comp_len * 8) return false;
    const uint64_t p = bit >> 3;
    uint32_t w = 0;
    for (int i = 0; i < 4; ++i)
        if (p + (uint64_t)i < (uint64_t)comp_len) w |= (uint32_t)comp[p + i] << (8 * i);
    v = (w >> (bit & 7)) & ((1u << n) - 1);
    return true;
}
// the cheap part of the candidate rule, in registers: BTYPE 2, HLIT <= 29, HDIST <= 29, a complete code-length code
INF_FN bool infs_prefilter(const uint8_t *comp, int64_t comp_len, uint64_t bit) {
    uint32_t h;
    if (!infs_peek(comp, comp_len, bit, 17, h)) return false;
    if (((h >> 1) & 3) != 2 || ((h >> 3) & 31) > 29 || ((h >> 8) & 31) > 29) return false;
    const int ncl = (int)((h >> 13) & 15) + 4;
    uint32_t kraft = 0;  // in 128ths
    for (int i = 0; i < ncl; i += 7) {
        const int k = ncl - i < 7 ? ncl - i : 7;
        uint32_t w;
        if (!infs_peek(comp, comp_len, bit + 17 + 3 * (uint64_t)i, 3 * k, w)) return false;
        for (int j = 0; j < k; ++j, w >>= 3)
            if (w & 7) kraft += 128u >> (w & 7);
    }
    return kraft == 128;
}
INF_FN void infs_ph_probe(InfsShared &X, const uint8_t *comp, int64_t comp_len, uint64_t end, int t) {
    const uint64_t bit = X.pos + (uint64_t)t;
    X.cand[t] = (uint8_t)(bit < end && infs_prefilter(comp, comp_len, bit));
}
// lane 0 holds the probes that passed to the whole rule, in order: the block reader and the table layout themselves
INF_FN void infs_ph_confirm(InfsShared &X, const uint8_t *comp, int64_t comp_len, int t) {
    if (t != 0) return;
    for (int i = 0; i < INF_THREADS; ++i) {
        if (!X.cand[i]) continue;
        infs_ph_start(X, X.pos + (uint64_t)i, 0);
        infs_ph_block(X, comp, comp_len, INFS_NONE, 0);
        if (X.S.state == INF_RUN) inf_ph_codes(X.S, 0);
        if (X.S.state == INF_RUN) {
            X.found = X.pos + (uint64_t)i;
            return;
        }
    }
    X.pos += INF_THREADS;
}
INF_FN void infs_ph_search_init(InfsShared &X, uint64_t from, int t) {
    if (t != 0) return;
    X.pos = from;
    X.found = INFS_NONE;
}
INF_FN void infs_ph_first_header(InfsShared &X, const uint8_t *comp, int64_t comp_len, int t) {
    if (t != 0) return;
    X.c_off = 0;
    infs_ph_member(X, comp, comp_len, 0);
    X.found = X.S.state == INF_RUN ? X.bit : INFS_NONE;
}
INF_FN void infs_ph_record(InfsShared &X, InfsRecord *rec, int t) {
    if (t != 0) return;
    rec->s = X.found;
    rec->e = X.bit;
    rec->n = X.n;
    rec->status = X.S.state == INF_BAD ? X.S.status : INF_OK;
    rec->final = X.S.state == INF_END;
}
// the two halves of a chunk's work: the first candidate at or behind bit `from` (X.found), and the count from X.found
INF_FN void infs_scan_search(InfsShared &X, const uint8_t *comp, int64_t comp_len, uint64_t from, uint64_t end) {
    INF_PHASE(infs_ph_search_init(X, from, t))
    while (X.found == INFS_NONE && X.pos < end) {
        INF_PHASE(infs_ph_probe(X, comp, comp_len, end, t))
        INF_PHASE(infs_ph_confirm(X, comp, comp_len, t))
    }
}
INF_FN void infs_scan_count(InfsShared &X, const uint8_t *comp, int64_t comp_len, uint64_t next, InfsRecord *rec) {
    if (X.found != INFS_NONE) {
        INF_PHASE(infs_ph_start(X, X.found, t))
        for (;;) {
            infs_count_block(X, comp, comp_len);
            if (X.S.state != INF_RUN || X.bit >= next) break;
        }
    }
    INF_PHASE(infs_ph_record(X, rec, t))
}
// chunk k of the file -> its record.  Called by all threads of the workgroup, after inf_ph_tables.
INF_FN void infs_scan_chunk(InfsShared &X, const uint8_t *comp, int64_t comp_len, int64_t chunk_bytes, int64_t k, InfsRecord *rec) {
    const uint64_t from = (uint64_t)k * (uint64_t)chunk_bytes * 8, next = from + (uint64_t)chunk_bytes * 8;
    const uint64_t end = next < (uint64_t)comp_len * 8 ? next : (uint64_t)comp_len * 8;
    if (k == 0) {
        INF_PHASE(infs_ph_first_header(X, comp, comp_len, t))
    } else {
        infs_scan_search(X, comp, comp_len, from, end);
    }
    infs_scan_count(X, comp, comp_len, next, rec);
}

// ---- chain ----
INF_FN void infs_ph_chain_init(InfsShared &X, int t) {
    if (t != 0) return;
    X.c_off = X.c_total = X.c_nseg = X.c_longest = 0;
    X.c_member = X.c_confirmed = 0;
    X.c_more = 0;
}
INF_FN void infs_ph_chain_member(InfsShared &X, const uint8_t *comp, int64_t comp_len, int t) {
    if (t != 0) return;
    X.c_member_comp = X.c_off;
    X.c_first = X.c_total;
    X.c_start = 1;
    infs_ph_member(X, comp, comp_len, 0);
}
INF_FN bool infs_lands(const InfsShared &X, const InfsRecord *rec, int64_t n_chunks, int64_t chunk_bytes, int64_t &k) {
    k = (int64_t)(X.bit / ((uint64_t)chunk_bytes * 8));
    return k < n_chunks && rec[k].s == X.bit;
}
// a segment begins at X.bit: with the record of its chunk when that starts here, else the wave walks
INF_FN void infs_ph_chain_land(InfsShared &X, const InfsRecord *rec, int64_t n_chunks, int64_t chunk_bytes, int t) {
    if (t != 0) return;
    X.c_seg_s = X.bit;
    int64_t k;
    X.c_landed = infs_lands(X, rec, n_chunks, chunk_bytes, k);
    X.c_guess = X.c_landed && k > 0;
    X.c_hit = 0;
    infs_ph_start(X, X.bit, 0);
    if (!X.c_landed) return;
    X.bit = rec[k].e;
    X.n = rec[k].n;
    if (rec[k].status != INF_OK)
        inf_refuse(X.S, rec[k].status);
    else if (rec[k].final)
        X.S.state = INF_END;
}
INF_FN void infs_ph_chain_probe(InfsShared &X, const InfsRecord *rec, int64_t n_chunks, int64_t chunk_bytes, int t) {
    if (t != 0) return;
    int64_t k;
    X.c_hit = infs_lands(X, rec, n_chunks, chunk_bytes, k);
}
INF_FN uint32_t infs_le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
// the segment [c_seg_s, X.bit) is listed; at a member's end the trailer, and whether another member follows (zlib's
// gzread: what does not begin with 1f 8b behind a member is ignored)
INF_FN void infs_ph_chain_emit(InfsShared &X, const uint8_t *comp, int64_t comp_len, InfsSegment *seg, int64_t seg_cap, int t) {
    if (t != 0 || X.S.state == INF_BAD) return;
    InfsSegment g;
    g.s = X.c_seg_s;
    g.e = X.bit;
    g.off = X.c_total;
    g.n = X.n;
    g.member_first = X.c_first;
    g.member_comp = X.c_member_comp;
    g.member = X.c_member;
    g.flags = (X.c_start ? INFS_F_START : 0) | (X.c_guess ? INFS_F_GUESS : 0);
    g.crc_want = g.isize_want = g.crc = 0;
    g.status = INF_OK;
    if (X.S.state == INF_END) {
        const uint64_t p = (X.bit + 7) >> 3;
        if (p + 8 > (uint64_t)comp_len) return inf_refuse(X.S, INF_E_INPUT);  // no trailer
        g.flags |= INFS_F_FINAL;
        g.crc_want = infs_le32(comp + p);
        g.isize_want = infs_le32(comp + p + 4);
        X.c_off = p + 8;
        X.c_more = (uint64_t)comp_len - X.c_off >= 2 && comp[X.c_off] == 0x1f && comp[X.c_off + 1] == 0x8b;
        X.c_member++;
    }
    if ((int64_t)X.c_nseg < seg_cap) seg[X.c_nseg] = g;
    X.c_nseg++;
    X.c_total += g.n;
    X.c_confirmed += X.c_guess;
    X.c_start = 0;
    const uint64_t bytes = ((g.e + 7) >> 3) - (g.s >> 3);
    if (bytes > X.c_longest) X.c_longest = bytes;
}
INF_FN void infs_ph_chain_result(InfsShared &X, const InfsRecord *rec, int64_t n_chunks, InfsResult *res, int t) {
    if (t != 0) return;
    res->total = X.c_total;
    res->n_seg = X.c_nseg;
    res->status = X.S.state == INF_BAD ? X.S.status : INF_OK;
    res->member = X.c_member;
    res->at = X.S.state == INF_BAD ? X.bit >> 3 : 0;
    int64_t cands = 0;
    for (int64_t k = 1; k < n_chunks; ++k) cands += rec[k].s != INFS_NONE;
    res->info[0] = X.c_member;
    res->info[1] = n_chunks;
    res->info[2] = X.c_confirmed;
    res->info[3] = cands - X.c_confirmed;
    res->info[4] = (n_chunks > 0 ? n_chunks - 1 : 0) - cands;
    res->info[5] = (int64_t)X.c_longest;
    res->info[6] = res->info[7] = 0;
}
// Called by all threads of ONE workgroup, after inf_ph_tables.  seg holds seg_cap entries; res->n_seg says how many there are.
INF_FN void infs_chain(InfsShared &X, const uint8_t *comp, int64_t comp_len, int64_t chunk_bytes, const InfsRecord *rec, int64_t n_chunks,
                       InfsSegment *seg, int64_t seg_cap, InfsResult *res) {
    INF_PHASE(infs_ph_chain_init(X, t))
    for (;;) {
        INF_PHASE(infs_ph_chain_member(X, comp, comp_len, t))
        while (X.S.state == INF_RUN) {
            INF_PHASE(infs_ph_chain_land(X, rec, n_chunks, chunk_bytes, t))
            while (!X.c_landed && !X.c_hit && X.S.state == INF_RUN) {
                infs_count_block(X, comp, comp_len);
                if (X.S.state != INF_RUN) break;
                INF_PHASE(infs_ph_chain_probe(X, rec, n_chunks, chunk_bytes, t))
            }
            INF_PHASE(infs_ph_chain_emit(X, comp, comp_len, seg, seg_cap, t))
        }
        if (X.S.state != INF_END || !X.c_more) break;
    }
    INF_PHASE(infs_ph_chain_result(X, rec, n_chunks, res, t))
}

// ---- decode: a segment -> the staging image ----
INF_FN void infs_ph_stage_stored(const InfsShared &X, const uint8_t *comp, uint16_t *stage, int t) {
    const uint8_t *src = comp + X.base + X.S.cp_src;
    for (uint32_t i = (uint32_t)t; i < X.S.cp_n; i += INF_THREADS) stage[X.cp_at + i] = src[i];
}
// `stage` is the segment's own image: byte j of the group goes to stage[g_at + j]
INF_FN void infs_ph_stage_place(const InfsShared &X, uint16_t *stage, int t) {
    const InfShared &S = X.S;
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
        uint16_t val;
        if (!(v & 0x8000u)) {
            val = (uint16_t)v;
        } else {
            const uint32_t d = (v & 0x7FFFu) + 1, i = j - S.tk_start[lo];
            const int64_t src = (int64_t)(X.g_at + S.tk_start[lo]) - (int64_t)d + (int64_t)(i < d ? i : i % d);
            val = src >= 0 ? stage[src] : (uint16_t)(0x8000 + (src + (int64_t)INFS_WINDOW));
        }
        stage[X.g_at + j] = val;
    }
}
INF_FN void infs_ph_stage_end(InfsShared &X, InfsSegment *g, int t) {
    if (t != 0) return;
    if (X.S.state == INF_BAD || X.bit != g->e || X.n != g->n) g->status = INFS_E_INTERNAL;
}
INF_FN void infs_decode_segment(InfsShared &X, const uint8_t *comp, int64_t comp_len, InfsSegment *g, uint16_t *stage_all) {
    uint16_t *stage = stage_all + g->off;
    const uint64_t end = g->e, cap = g->n;
    INF_PHASE(infs_ph_start(X, g->s, t))
    while (X.S.state == INF_RUN && X.bit < end) {
        INF_PHASE(infs_ph_block(X, comp, comp_len, cap, t))
        if (X.S.state == INF_BAD) break;
        if (X.S.kind == 0) {
            INF_PHASE(infs_ph_stage_stored(X, comp, stage, t))
            continue;
        }
        INF_PHASE(inf_ph_codes(X.S, t))
        if (X.S.state != INF_RUN) break;
        INF_PHASE(inf_ph_fill(X.S, t))
        bool more = true;
        while (more) {
            INF_PHASE(infs_ph_tokens(X, comp, comp_len, cap, t))
            INF_PHASE(infs_ph_stage_place(X, stage, t))
            more = X.S.state == INF_RUN && !X.S.eob;
        }
    }
    INF_PHASE(infs_ph_stage_end(X, g, t))
}

// ---- tails and rest: staged values -> final bytes ----
// staged value at plain position g.off + p -> its byte; the source of a marker is final already (a tail in front).
// hist (the windowed form, bdx_inflate_window_core.h; else NULL): the 32 KiB in front of out[0], hist[32767] the nearest
INF_FN void infs_resolve(InfsSegment *g, const uint16_t *stage, uint8_t *out, uint64_t p, const uint8_t *hist = nullptr) {
    const uint32_t v = stage[g->off + p];
    uint8_t byte = (uint8_t)v;
    if (v & 0x8000u) {
        const uint64_t back = INFS_WINDOW - (v & 0x7FFFu);  // 1 .. 32768 bytes in front of the segment
        if (g->off - g->member_first < back) {
            g->status = INF_E_DISTANCE;  // (every lane that finds one stores the same word)
            byte = 0;
        } else if (hist && back > g->off) {
            byte = hist[INFS_WINDOW - (back - g->off)];
        } else {
            byte = out[g->off - back];
        }
    }
    out[g->off + p] = byte;
}
INF_FN uint64_t infs_tail_from(const InfsSegment *g) { return g->n > INFS_WINDOW ? g->n - INFS_WINDOW : 0; }
// ONE workgroup, the segments in order
INF_FN void infs_tails(InfsSegment *seg, int64_t n_seg, const uint16_t *stage, uint8_t *out, const uint8_t *hist = nullptr) {
    for (int64_t i = 0; i < n_seg; ++i) {
        INFS_PHASE_WG(for (uint64_t p = infs_tail_from(seg + i) + (uint64_t)t; p < seg[i].n; p += (uint64_t)nt) infs_resolve(seg + i, stage, out, p, hist))
    }
}
INF_FN void infs_ph_rest(InfsSegment *g, const uint16_t *stage, uint8_t *out, const uint8_t *hist, int t) {
    const uint64_t to = infs_tail_from(g);
    for (uint64_t p = (uint64_t)t; p < to; p += INF_THREADS) infs_resolve(g, stage, out, p, hist);
}
INF_FN void infs_ph_crc_init(InfsShared &X, int t) {
    if (t == 0) X.crc = X.S.crc = 0;
}
// 64 slices of out[0, n), n <= 2^30, combined into S.crc
INF_FN void infs_ph_crc(InfsShared &X, const uint8_t *out, uint32_t n, int t) {
    InfShared &S = X.S;
    const uint32_t per = (n + INF_THREADS - 1) / INF_THREADS;
    const uint32_t a = (uint32_t)t * per < n ? (uint32_t)t * per : n;
    const uint32_t b = a + per < n ? a + per : n;
    if (a >= b) return;
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = a; i < b; ++i) c = S.crc_tab[(c ^ out[i]) & 0xFF] ^ (c >> 8);
    c ^= 0xFFFFFFFFu;
    INF_ATOMIC_XOR(&S.crc, bdx_crc_multmodp(bdx_crc_x8n(S.x2n, n - b), c));
}
INF_FN uint32_t infs_crc_shift(const uint32_t *x2n, uint32_t crc, uint64_t n) {  // crc of A -> its part in crc of A B, |B| = n
    while (n) {
        const uint32_t k = n < 0x40000000u ? (uint32_t)n : 0x40000000u;
        crc = bdx_crc_multmodp(bdx_crc_x8n(x2n, k), crc);
        n -= k;
    }
    return crc;
}
INF_FN void infs_ph_crc_piece(InfsShared &X, uint32_t n, int t) {
    if (t != 0) return;
    X.crc = infs_crc_shift(X.S.x2n, X.crc, n) ^ X.S.crc;
    X.S.crc = 0;
}
INF_FN void infs_ph_crc_store(const InfsShared &X, InfsSegment *g, int t) {
    if (t == 0) g->crc = X.crc;
}
// one wave per segment, after infs_tails
INF_FN void infs_rest_segment(InfsShared &X, InfsSegment *g, const uint16_t *stage, uint8_t *out, const uint8_t *hist = nullptr) {
    INF_PHASE(infs_ph_rest(g, stage, out, hist, t))
    INF_PHASE(infs_ph_crc_init(X, t))
    const uint64_t n = g->n;
    for (uint64_t at = 0; at < n; at += INFS_REBASE) {
        const uint32_t k = n - at < INFS_REBASE ? (uint32_t)(n - at) : INFS_REBASE;
        INF_PHASE(infs_ph_crc(X, out + g->off + at, k, t))
        INF_PHASE(infs_ph_crc_piece(X, k, t))
    }
    INF_PHASE(infs_ph_crc_store(X, g, t))
}

// ---- verdict: per member, the first refusal of a segment, then the CRC-32, then ISIZE ----
INF_FN void infs_ph_verdict(InfsShared &X, const InfsSegment *seg, int64_t n_seg, InfsResult *res, int t) {
    if (t != 0) return;
    uint32_t crc = 0, bad = INF_OK;
    res->status = INF_OK;
    for (int64_t i = 0; i < n_seg; ++i) {
        const InfsSegment &g = seg[i];
        if (g.flags & INFS_F_START) {
            crc = 0;
            bad = INF_OK;
        }
        crc = infs_crc_shift(X.S.x2n, crc, g.n) ^ g.crc;
        if (bad == INF_OK) bad = g.status;
        if (!(g.flags & INFS_F_FINAL)) continue;
        if (bad == INF_OK && crc != g.crc_want) bad = INF_E_CRC;
        if (bad == INF_OK && (uint32_t)(g.off + g.n - g.member_first) != g.isize_want) bad = INF_E_ISIZE;
        if (bad != INF_OK) {
            res->status = bad;
            res->member = g.member;
            res->at = g.member_comp;
            return;
        }
    }
}
