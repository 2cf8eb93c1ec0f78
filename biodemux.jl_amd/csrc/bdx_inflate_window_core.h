// bdx_inflate_window_core.h — the stream inflate of bdx_inflate_stream_core.h, one WINDOW of the file at a time: a call
// gets comp[0, comp_len), the file's bytes from the byte the call before stopped in, and the CARRIED STATE that call
// left; it inflates up to the last place the next call can resume from with the carried state alone.  Private; included
// by bdx_inflate_stream.hip.  The six steps are the whole-file ones: search, count, decode, the CRC and the token walk
// are called as they are; what is new is chunk 0's start, the chain's stop rule, the history in front of the window
// and a verdict that carries a member's CRC-32 and size across calls.
//
// Carried state (InfwCarry, device memory, owned by the window object, written by the verdict step alone and only when
// the whole call is good): where the position is — BETWEEN members (the next byte is a header, trailing bytes or the
// end of the file), INSIDE a member at a block start (bit 0..7 of the window's first byte), at a member's TRAILER (the
// final block ended at bit 0..7 of the first byte, its 8 bytes were not all there yet), or in trailing bytes that are
// IGNORED for good —; the member's index, the absolute byte it began at, its plain bytes and its CRC-32 so far; the
// absolute offsets of the window; the last 32 KiB of plain text (two copies' room: a call reads one and writes the
// other, so a call that ends in BDX_E_SPACE or that is refused has changed nothing).
//
// Stop rule (chain).  `last` says that comp ends with the file.  In a window that is not the last:
//   - a block that runs off the buffer (INF_E_INPUT; or "bad symbol" with fewer than 48 bits left, one token's most:
//     the bit reader pads with zeros, so a code that is cut may look like no code) is not a refusal: the window stops at
//     the end of the block before it.  Every other status is a refusal as in the whole-file decoder: all bits that
//     produced it lay inside the buffer.  A scan record that did not end well is never accepted as a unit: the scan
//     cuts it back to its last complete block end (infw_scan_count), and the chain walks the block behind that itself.
//   - a final block whose 8-byte trailer is not wholly in the buffer: the block is taken, the window stops AT THE
//     TRAILER; the next call checks the carried CRC-32 and size against it.
//   - a header (FEXTRA, FNAME, FCOMMENT, FHCRC) that runs off the buffer, or has no 8 bytes behind it: the window stops
//     BETWEEN members, in front of it.  A bad header whose bytes are all there is refused.
//   - a buffer that ends less than 2 bytes behind a trailer: stops BETWEEN members; whether 1f 8b follows is the next
//     call's to see.  Bytes there that do not begin with 1f 8b are trailing bytes: IGNORED from then on, as zlib's gzread.
//   In the last window: zero bytes (or one) BETWEEN members is a good end of the file; everything else above is what
//   the whole-file decoder says (input exhausted, bad header).
// A window that cannot get past its first block stops where it began: consumed 0, plain 0.  The caller feeds more.
//
// Invariants, as in bdx_inflate_stream_core.h:
//   - exactness never rests on a guess: a record is used only when a decoder that started from a confirmed position
//     (the carried one is confirmed: the call before arrived there) arrived exactly at its start bit, and only when it
//     ended well inside the buffer;
//   - no loop waits for another workgroup: ordering comes from the kernel boundaries;
//   - every loop consumes bits or output bytes: the chain's outer loop takes a member, its inner ones a block at least;
//   - no byte outside comp[0, comp_len) is read: every reader is bdx_inflate_core.h's with lim = comp_len - base, the
//     header test (infw_header_fits) and the trailer reads check their own ends;
//   - no byte outside out[0, total) or the carried state is written: segments tile [0, total), the history is read at
//     [32768 - back + off, 32768) only with back <= 32768 and back > off.
// Positions in a call are relative to the window (at most 2^28 bytes: no bit position reaches 2^31); absolute offsets
// are 64-bit and go into messages only.  member_first of a segment whose member began in an earlier window is
// "minus the carried size" in wrapping unsigned arithmetic: off - member_first is the member's bytes in front of it.
#pragma once
#include "bdx_inflate_stream_core.h"

#define INFW_MAX (1ll << 28)  // the longest window, bytes
#define INFW_BETWEEN 0u
#define INFW_INSIDE 1u
#define INFW_TRAILER 2u
#define INFW_IGNORE 3u

struct InfwCarry {
    uint32_t where, bit, member, crc, cur, pad;
    uint64_t member_comp, member_n;  // absolute byte the current member begins at; its plain bytes so far
    uint64_t comp_abs, plain_abs;    // absolute offsets of the next window's first byte and first plain byte
    uint8_t hist[2][INFS_WINDOW];    // hist[cur][32767] is the last plain byte
};
struct InfwResult {
    InfsResult r;                             // r.at is absolute
    uint64_t consumed, member_comp;           // whole bytes the next window does not begin with
    uint32_t where, bit, member;              // the next carried position
    uint32_t lead, lead_crc, lead_isize;      // the window began with the carried member's trailer
};
struct InfwShared {
    InfsShared X;
    uint64_t good_bit, good_n;
    uint32_t where, stop, last, pad;
};

// is the gzip header at p[0, rem) there whole, with 8 bytes behind it?  (A header that is bad in its first four bytes
// "fits": the parser refuses it on bytes that are all there.)
INF_FN bool infw_header_fits(const uint8_t *p, uint64_t rem) {
    if (rem < 18) return false;
    if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || (p[3] & 0xE0)) return true;
    const uint32_t flg = p[3];
    uint64_t q = 10;
    if (flg & 4) {
        if (q + 2 > rem) return false;
        q += 2 + ((uint64_t)p[q] | ((uint64_t)p[q + 1] << 8));
        if (q > rem) return false;
    }
    for (uint32_t bit = 8; bit <= 16; bit <<= 1) {
        if (!(flg & bit)) continue;
        while (q < rem && p[q]) ++q;
        if (q >= rem) return false;
        ++q;
    }
    if (flg & 2) q += 2;
    return q + 8 <= rem;
}

// ---- scan: chunk 0 begins at the carried position ----
INF_FN void infw_ph_first(InfsShared &X, const uint8_t *comp, int64_t comp_len, const InfwCarry *C, int t) {
    if (t != 0) return;
    X.found = INFS_NONE;
    if (C->where == INFW_INSIDE) {
        X.found = C->bit;
        return;
    }
    if (C->where == INFW_IGNORE) return;
    X.c_off = C->where == INFW_TRAILER ? ((C->bit + 7) >> 3) + 8 : 0;  // (a guess like any other: the chain decides)
    if (X.c_off + 18 > (uint64_t)comp_len) return;
    infs_ph_member(X, comp, comp_len, 0);
    if (X.S.state == INF_RUN) X.found = X.bit;
}
// The count of a window's chunk keeps its last complete block end: a record whose count ended badly (the last chunk's
// runs off the buffer in every window but the file's last) is cut back to the blocks that ended well and is a good
// record of those; the chain walks the one block behind it itself and says what it is.  (c_seg_s, c_first: the chain's
// fields, free in the scan.)
INF_FN void infw_ph_scan_good(InfsShared &X, int t) {
    if (t != 0) return;
    X.c_seg_s = X.bit;
    X.c_first = X.n;
}
INF_FN void infw_ph_scan_trim(InfsShared &X, int t) {
    if (t != 0 || X.S.state != INF_BAD || X.c_seg_s == X.found) return;
    X.bit = X.c_seg_s;
    X.n = X.c_first;
    X.S.state = INF_RUN;
    X.S.status = INF_OK;
}
INF_FN void infw_scan_count(InfsShared &X, const uint8_t *comp, int64_t comp_len, uint64_t next, InfsRecord *rec) {
    if (X.found != INFS_NONE) {
        INF_PHASE(infs_ph_start(X, X.found, t))
        for (;;) {
            INF_PHASE(infw_ph_scan_good(X, t))
            infs_count_block(X, comp, comp_len);
            if (X.S.state != INF_RUN || X.bit >= next) break;
        }
        INF_PHASE(infw_ph_scan_trim(X, t))
    }
    INF_PHASE(infs_ph_record(X, rec, t))
}
INF_FN void infw_scan_chunk(InfsShared &X, const uint8_t *comp, int64_t comp_len, int64_t chunk_bytes, int64_t k, const InfwCarry *C,
                            InfsRecord *rec) {
    const uint64_t from = (uint64_t)k * (uint64_t)chunk_bytes * 8, next = from + (uint64_t)chunk_bytes * 8;
    const uint64_t end = next < (uint64_t)comp_len * 8 ? next : (uint64_t)comp_len * 8;
    if (k == 0) {
        INF_PHASE(infw_ph_first(X, comp, comp_len, C, t))
    } else {
        infs_scan_search(X, comp, comp_len, from, end);
    }
    infw_scan_count(X, comp, comp_len, next, rec);
}

// ---- chain ----
INF_FN void infw_ph_chain_init(InfwShared &W, int last, const InfwCarry *C, InfwResult *res, int t) {
    if (t != 0) return;
    InfsShared &X = W.X;
    infs_ph_chain_init(X, 0);
    infs_ph_start(X, C->bit, 0);
    X.c_member = C->member;
    X.c_member_comp = C->member_comp;
    X.c_first = (uint64_t)0 - C->member_n;
    X.c_start = 0;
    X.c_landed = X.c_hit = X.c_guess = 0;
    X.c_seg_s = C->bit;
    W.where = C->where;
    W.stop = 0;
    W.last = last != 0;
    W.good_bit = C->bit;
    W.good_n = 0;
    res->lead = res->lead_crc = res->lead_isize = 0;
}
// the carried member's trailer at the window's front
INF_FN void infw_ph_lead_trailer(InfwShared &W, const uint8_t *comp, int64_t comp_len, InfwResult *res, int t) {
    if (t != 0) return;
    InfsShared &X = W.X;
    const uint64_t p = (X.bit + 7) >> 3;
    if (p + 8 > (uint64_t)comp_len) {
        if (W.last) return inf_refuse(X.S, INF_E_INPUT);  // no trailer
        W.stop = 1;
        return;
    }
    res->lead = 1;
    res->lead_crc = infs_le32(comp + p);
    res->lead_isize = infs_le32(comp + p + 4);
    X.c_off = p + 8;
    X.c_member++;
    W.where = INFW_BETWEEN;
}
// BETWEEN members at byte c_off: a header (-> INSIDE, or refused), trailing bytes, the end, or not known yet
INF_FN void infw_ph_between(InfwShared &W, const uint8_t *comp, int64_t comp_len, uint64_t comp_abs, int t) {
    if (t != 0) return;
    InfsShared &X = W.X;
    const uint64_t rem = (uint64_t)comp_len - X.c_off;
    if (X.c_member > 0) {  // (the file's first member has to be there: what is not a header is refused)
        if (rem < 2) {
            if (W.last)
                W.where = INFW_IGNORE;
            else
                W.stop = 1;
            return;
        }
        if (comp[X.c_off] != 0x1f || comp[X.c_off + 1] != 0x8b) {
            W.where = INFW_IGNORE;
            return;
        }
    }
    if (!W.last && !infw_header_fits(comp + X.c_off, rem)) {
        W.stop = 1;
        return;
    }
    const uint64_t at = X.c_off;
    infs_ph_chain_member(X, comp, comp_len, 0);
    X.c_member_comp = comp_abs + at;
    if (X.S.state == INF_RUN) W.where = INFW_INSIDE;
}
INF_FN bool infw_lands(const InfsShared &X, const InfsRecord *rec, int64_t n_chunks, int64_t chunk_bytes, int64_t &k) {
    return infs_lands(X, rec, n_chunks, chunk_bytes, k) && rec[k].status == INF_OK;
}
INF_FN void infw_ph_land(InfwShared &W, const InfsRecord *rec, int64_t n_chunks, int64_t chunk_bytes, int t) {
    if (t != 0) return;
    InfsShared &X = W.X;
    X.c_seg_s = X.bit;
    int64_t k;
    X.c_landed = infw_lands(X, rec, n_chunks, chunk_bytes, k);
    X.c_guess = X.c_landed && k > 0;
    X.c_hit = 0;
    infs_ph_start(X, X.bit, 0);
    if (!X.c_landed) return;
    X.bit = rec[k].e;
    X.n = rec[k].n;
    if (rec[k].final) X.S.state = INF_END;
}
INF_FN void infw_ph_good(InfwShared &W, int t) {
    if (t != 0) return;
    W.good_bit = W.X.bit;
    W.good_n = W.X.n;
}
// after a block the chain walked: ran off the buffer -> back to the block's start and stop; else a later record?
INF_FN void infw_ph_walked(InfwShared &W, int64_t comp_len, const InfsRecord *rec, int64_t n_chunks, int64_t chunk_bytes, int t) {
    if (t != 0) return;
    InfsShared &X = W.X;
    if (X.S.state == INF_BAD) {
        const bool ran_off = X.S.status == INF_E_INPUT || (X.S.status == INF_E_SYMBOL && (uint64_t)comp_len * 8 - X.bit < 48);
        if (W.last || !ran_off) return;
        X.bit = W.good_bit;
        X.n = W.good_n;
        X.S.state = INF_RUN;
        X.S.status = INF_OK;
        W.stop = 1;
        return;
    }
    if (X.S.state != INF_RUN) return;
    int64_t k;
    X.c_hit = infw_lands(X, rec, n_chunks, chunk_bytes, k);
}
// the segment [c_seg_s, X.bit) is listed (an empty one at a stop is not); at a member's end its trailer
INF_FN void infw_ph_emit(InfwShared &W, const uint8_t *comp, int64_t comp_len, InfsSegment *seg, int64_t seg_cap, int t) {
    InfsShared &X = W.X;
    if (t != 0 || X.S.state == INF_BAD) return;
    if (W.stop && X.bit == X.c_seg_s) return;
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
        if (p + 8 > (uint64_t)comp_len) {
            if (W.last) return inf_refuse(X.S, INF_E_INPUT);  // no trailer
            W.where = INFW_TRAILER;
            W.stop = 1;
        } else {
            g.flags |= INFS_F_FINAL;
            g.crc_want = infs_le32(comp + p);
            g.isize_want = infs_le32(comp + p + 4);
            X.c_off = p + 8;
            X.c_member++;
            W.where = INFW_BETWEEN;
        }
    }
    if ((int64_t)X.c_nseg < seg_cap) seg[X.c_nseg] = g;
    X.c_nseg++;
    X.c_total += g.n;
    X.c_confirmed += X.c_guess;
    X.c_start = 0;
    const uint64_t bytes = ((g.e + 7) >> 3) - (g.s >> 3);
    if (bytes > X.c_longest) X.c_longest = bytes;
}
INF_FN void infw_ph_chain_result(InfwShared &W, int64_t comp_len, const InfsRecord *rec, int64_t n_chunks, const InfwCarry *C, InfwResult *res,
                                 int t) {
    if (t != 0) return;
    InfsShared &X = W.X;
    infs_ph_chain_result(X, rec, n_chunks, &res->r, 0);
    res->r.info[0] = (int64_t)X.c_member - (int64_t)C->member;  // members that ended in this window
    if (X.S.state == INF_BAD) res->r.at = C->comp_abs + (X.bit >> 3);
    res->where = W.where;
    res->member = X.c_member;
    res->member_comp = X.c_member_comp;
    res->bit = 0;
    if (W.where == INFW_BETWEEN) {
        res->consumed = X.c_off;
    } else if (W.where == INFW_IGNORE) {
        res->consumed = (uint64_t)comp_len;
    } else {
        res->consumed = X.bit >> 3;
        res->bit = (uint32_t)(X.bit & 7);
    }
}
// Called by all threads of ONE workgroup, after inf_ph_tables.
INF_FN void infw_chain(InfwShared &W, const uint8_t *comp, int64_t comp_len, int last, int64_t chunk_bytes, const InfsRecord *rec, int64_t n_chunks,
                       InfsSegment *seg, int64_t seg_cap, const InfwCarry *C, InfwResult *res) {
    InfsShared &X = W.X;
    INF_PHASE(infw_ph_chain_init(W, last, C, res, t))
    if (W.where == INFW_TRAILER) INF_PHASE(infw_ph_lead_trailer(W, comp, comp_len, res, t))
    while (!W.stop && X.S.state != INF_BAD && W.where != INFW_IGNORE && W.where != INFW_TRAILER) {
        if (W.where == INFW_BETWEEN) {
            INF_PHASE(infw_ph_between(W, comp, comp_len, C->comp_abs, t))
            if (W.where != INFW_INSIDE) break;
        }
        while (X.S.state == INF_RUN && !W.stop) {
            INF_PHASE(infw_ph_land(W, rec, n_chunks, chunk_bytes, t))
            while (!X.c_landed && !X.c_hit && X.S.state == INF_RUN && !W.stop) {
                INF_PHASE(infw_ph_good(W, t))
                infs_count_block(X, comp, comp_len);
                INF_PHASE(infw_ph_walked(W, comp_len, rec, n_chunks, chunk_bytes, t))
            }
            INF_PHASE(infw_ph_emit(W, comp, comp_len, seg, seg_cap, t))
        }
    }
    INF_PHASE(infw_ph_chain_result(W, comp_len, rec, n_chunks, C, res, t))
}

// ---- verdict: the members that ended here against their trailers; then, all being well, the next carried state ----
INF_FN void infw_ph_verdict(InfsShared &X, const InfsSegment *seg, int64_t n_seg, const InfwCarry *C, InfwResult *res, int t) {
    if (t != 0) return;
    uint32_t crc = C->crc, bad = INF_OK;
    uint64_t size = C->member_n;
    uint32_t member = C->member;
    uint64_t member_comp = C->member_comp;
    X.v_bad = 0;
    res->r.status = INF_OK;
    if (res->lead) {
        if (crc != res->lead_crc)
            bad = INF_E_CRC;
        else if ((uint32_t)size != res->lead_isize)
            bad = INF_E_ISIZE;
        crc = 0;
        size = 0;
    }
    for (int64_t i = 0; i < n_seg && bad == INF_OK; ++i) {
        const InfsSegment &g = seg[i];
        member = g.member;
        member_comp = g.member_comp;
        if (g.flags & INFS_F_START) {
            crc = 0;
            size = 0;
        }
        crc = infs_crc_shift(X.S.x2n, crc, g.n) ^ g.crc;
        size += g.n;
        bad = g.status;
        if (bad != INF_OK) break;
        // a refusal found in a later segment of a member is found here or in a later window: the member fails either way
        if (!(g.flags & INFS_F_FINAL)) continue;
        if (crc != g.crc_want)
            bad = INF_E_CRC;
        else if ((uint32_t)size != g.isize_want)
            bad = INF_E_ISIZE;
        crc = 0;
        size = 0;
    }
    if (bad != INF_OK) {
        res->r.status = bad;
        res->r.member = member;
        res->r.at = member_comp;
        X.v_bad = 1;
        return;
    }
    X.crc = crc;
    X.c_total = size;
}
// the last 32 KiB of (old history, out[0, total)) -> the other copy
INF_FN void infw_ph_history(const InfsShared &X, const uint8_t *out, uint64_t total, InfwCarry *C, int t) {
    if (X.v_bad) return;
    const uint8_t *from = C->hist[C->cur & 1];
    uint8_t *to = C->hist[(C->cur & 1) ^ 1];
    const uint64_t keep = total < INFS_WINDOW ? INFS_WINDOW - total : 0;
    for (uint64_t i = (uint64_t)t; i < INFS_WINDOW; i += INF_THREADS) to[i] = i < keep ? from[i + total] : out[total - INFS_WINDOW + i];
}
INF_FN void infw_ph_carry(const InfsShared &X, uint64_t total, InfwCarry *C, const InfwResult *res, int t) {
    if (t != 0 || X.v_bad) return;
    C->cur = (C->cur & 1) ^ 1;
    C->where = res->where;
    C->bit = res->bit;
    C->member = res->member;
    C->member_comp = res->member_comp;
    C->crc = X.crc;
    C->member_n = X.c_total;
    C->comp_abs += res->consumed;
    C->plain_abs += total;
}
// Called by all threads of ONE workgroup, after inf_ph_tables.
INF_FN void infw_verdict(InfsShared &X, const InfsSegment *seg, int64_t n_seg, const uint8_t *out, uint64_t total, InfwCarry *C, InfwResult *res) {
    INF_PHASE(infw_ph_verdict(X, seg, n_seg, C, res, t))
    INF_PHASE(infw_ph_history(X, out, total, C, t))
    INF_PHASE(infw_ph_carry(X, total, C, res, t))
}
