// bdx_fastq.hip — the device FASTQ pipeline: FASTQ text in HBM -> line table -> packed reads (for bdx_classify_device)
// -> records partitioned by output class -> per-class FASTQ blocks.  Plain wave64 streaming kernels for gfx950 and the
// C-ABI entries that drive them on the context's stream.
//
// Every step has the contract of a host function of csrc/bdx_io.cpp (its test oracle):
//   bdx_fq_index_device  <-> bdx_fq_index / index_range   (line table of 4-line records, '\r' stripped, tail rules)
//   bdx_fq_pack_device   <-> bdx_fq_pack                  (sequence lines packed as the classify chunk layout)
//   bdx_fq_gather_device <-> the bytes demux_write_impl writes for one output stream of a batch, class by class
// Positions in line tables are byte offsets relative to the text pointer the caller passes.
#include <algorithm>
#include <cstring>

#include "bdx_ctx.h"

namespace {

constexpr int FQ_THREADS = 256;               // every kernel here: 4 waves per workgroup
constexpr int FQ_WAVES = FQ_THREADS / 64;
constexpr int FQ_LANE_BYTES = 16;             // text bytes a lane looks at per step (one 16-byte load when aligned)
constexpr int FQ_STEPS = 4;                   // steps per workgroup: a workgroup indexes 16 KiB of text
constexpr int64_t FQ_TILE = (int64_t)FQ_THREADS * FQ_LANE_BYTES * FQ_STEPS;
constexpr int FQ_SCAN_ITEMS = 4;              // items per thread of the generic scan (1024 per workgroup)
constexpr int64_t FQ_SCAN_BLOCK = (int64_t)FQ_THREADS * FQ_SCAN_ITEMS;

// scratch buffers of the context (bdx_ctx::fq)
enum {
    FQ_BLK = 0,   // index: newlines per workgroup, then their exclusive scan (+ total)
    FQ_NL,        // index: newline positions
    FQ_PART,      // generic scan: workgroup partials
    FQ_KEY_A,     // partition: class keys / record indices, ping-pong
    FQ_KEY_B,
    FQ_IDX_A,
    FQ_IDX_B,
    FQ_HIST,      // partition: per-tile digit histograms (digit-major) and their scan
    FQ_BASE,
    FQ_OFF,       // gather: output offset of every record in partition order (+ total)
    FQ_CLASS,     // gather: per-class start / end byte, then bytes per class
    FQ_SMALL,     // flags and values read back by the host
    FQ_NBUF
};
static_assert(FQ_NBUF <= BDX_FQ_SCRATCH, "bdx_ctx::fq holds the scratch buffers of the device FASTQ pipeline");

// ---- wave / workgroup primitives -------------------------------------------------------------------------------------
__device__ inline unsigned long long lanes_below() {
    const int lane = threadIdx.x & 63;
    return lane ? (~0ull >> (64 - lane)) : 0ull;
}

__device__ inline long long wave_incl_scan(long long v) {
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) {
        const long long u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

// Exclusive prefix of `v` over the workgroup (FQ_THREADS threads, every thread calls it); *total: the workgroup's sum.
__device__ inline long long block_excl_scan(long long v, long long *total) {
    __shared__ long long wsum[FQ_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long inc = wave_incl_scan(v);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    long long base = 0, tot = 0;
    for (int k = 0; k < FQ_WAVES; ++k) {
        if (k < w) base += wsum[k];
        tot += wsum[k];
    }
    __syncthreads();  // (wsum is reused by the next call)
    *total = tot;
    return base + inc - v;
}

// ---- generic exclusive scan: out[i] = sum_{k<i} get(k), out[n] = total ------------------------------------------------
template <class Get>
__global__ void __launch_bounds__(FQ_THREADS) scan_partials_kernel(Get get, int64_t n, long long *part) {
    const int64_t i0 = (int64_t)blockIdx.x * FQ_SCAN_BLOCK + (int64_t)threadIdx.x * FQ_SCAN_ITEMS;
    long long s = 0;
    for (int k = 0; k < FQ_SCAN_ITEMS; ++k)
        if (i0 + k < n) s += get(i0 + k);
    long long tot;
    (void)block_excl_scan(s, &tot);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// one workgroup: exclusive scan of v[0, n) in place, v[n] = total
__global__ void __launch_bounds__(FQ_THREADS) scan_small_kernel(long long *v, int64_t n) {
    long long carry = 0;
    for (int64_t b = 0; b < n; b += FQ_SCAN_BLOCK) {
        const int64_t i0 = b + (int64_t)threadIdx.x * FQ_SCAN_ITEMS;
        long long x[FQ_SCAN_ITEMS], s = 0;
        for (int k = 0; k < FQ_SCAN_ITEMS; ++k) {
            x[k] = i0 + k < n ? v[i0 + k] : 0;
            s += x[k];
        }
        long long tot;
        long long run = carry + block_excl_scan(s, &tot);
        for (int k = 0; k < FQ_SCAN_ITEMS; ++k) {
            if (i0 + k < n) v[i0 + k] = run;
            run += x[k];
        }
        carry += tot;
    }
    if (threadIdx.x == 0) v[n] = carry;
}

template <class Get>
__global__ void __launch_bounds__(FQ_THREADS) scan_apply_kernel(Get get, int64_t n, const long long *part, int64_t nparts,
                                                                long long *out) {
    const int64_t i0 = (int64_t)blockIdx.x * FQ_SCAN_BLOCK + (int64_t)threadIdx.x * FQ_SCAN_ITEMS;
    long long x[FQ_SCAN_ITEMS], s = 0;
    for (int k = 0; k < FQ_SCAN_ITEMS; ++k) {
        x[k] = i0 + k < n ? get(i0 + k) : 0;
        s += x[k];
    }
    long long tot;
    long long run = part[blockIdx.x] + block_excl_scan(s, &tot);
    for (int k = 0; k < FQ_SCAN_ITEMS; ++k) {
        if (i0 + k < n) out[i0 + k] = run;
        run += x[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = part[nparts];
}

template <class Get>
hipError_t exclusive_scan(bdx_ctx *ctx, Get get, int64_t n, long long *out) {
    const int64_t nb = (n + FQ_SCAN_BLOCK - 1) / FQ_SCAN_BLOCK;
    if (nb == 0) return hipMemsetAsync(out, 0, sizeof(long long), ctx->stream);
    hipError_t e = ctx->fq[FQ_PART].ensure((size_t)(nb + 1) * 8);
    if (e != hipSuccess) return e;
    long long *part = (long long *)ctx->fq[FQ_PART].p;
    scan_partials_kernel<<<dim3((unsigned)nb), dim3(FQ_THREADS), 0, ctx->stream>>>(get, n, part);
    scan_small_kernel<<<dim3(1), dim3(FQ_THREADS), 0, ctx->stream>>>(part, nb);
    scan_apply_kernel<<<dim3((unsigned)nb), dim3(FQ_THREADS), 0, ctx->stream>>>(get, n, part, nb, out);
    return hipGetLastError();
}

// ---- index --------------------------------------------------------------------------------------------------------------
// Bit j of the result: text[p + j] == '\n' (bytes at or beyond len do not count).
template <bool kAligned>
__device__ inline uint32_t newline_mask16(const uint8_t *t, int64_t len, int64_t p) {
    if (p >= len) return 0;
    uint32_t m = 0;
    if (kAligned && p + FQ_LANE_BYTES <= len) {
        const uint4 v = *reinterpret_cast<const uint4 *>(t + p);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t x = w[k] ^ 0x0A0A0A0Au;                                  // '\n' bytes -> 0
            const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);  // 0x80 exactly at the zero bytes
            m |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * k);
        }
    } else {
        const int e = (int)min<int64_t>(len - p, FQ_LANE_BYTES);
        for (int j = 0; j < e; ++j)
            if (t[p + j] == '\n') m |= 1u << j;
    }
    return m;
}

template <bool kAligned>
__global__ void __launch_bounds__(FQ_THREADS) nl_count_kernel(const uint8_t *t, int64_t len, long long *blk) {
    long long c = 0;
    for (int s = 0; s < FQ_STEPS; ++s) {
        const int64_t p = (int64_t)blockIdx.x * FQ_TILE + ((int64_t)s * FQ_THREADS + threadIdx.x) * FQ_LANE_BYTES;
        c += __popc(newline_mask16<kAligned>(t, len, p));
    }
    long long tot;
    (void)block_excl_scan(c, &tot);
    if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

// newline number k (in text order) -> nl[k], for k < cap; blk holds the workgroups' exclusive prefix
template <bool kAligned>
__global__ void __launch_bounds__(FQ_THREADS) nl_scatter_kernel(const uint8_t *t, int64_t len, const long long *blk,
                                                                long long *nl, int64_t cap) {
    long long base = blk[blockIdx.x];
    for (int s = 0; s < FQ_STEPS && base < cap; ++s) {
        const int64_t p = (int64_t)blockIdx.x * FQ_TILE + ((int64_t)s * FQ_THREADS + threadIdx.x) * FQ_LANE_BYTES;
        uint32_t m = newline_mask16<kAligned>(t, len, p);
        long long tot;
        long long k = base + block_excl_scan(__popc(m), &tot);
        while (m) {
            const int j = __ffs(m) - 1;
            m &= m - 1;
            if (k < cap) nl[k] = p + j;
            ++k;
        }
        base += tot;
    }
}

// line k ends at newline k: it starts after newline k-1 (or at 0); its length excludes a '\r' before the '\n'
__global__ void __launch_bounds__(FQ_THREADS) lines_kernel(const uint8_t *t, const long long *nl, int64_t nlines,
                                                           int64_t *line_off, int32_t *line_len) {
    for (int64_t k = (int64_t)blockIdx.x * FQ_THREADS + threadIdx.x; k < nlines; k += (int64_t)gridDim.x * FQ_THREADS) {
        const int64_t s = k ? nl[k - 1] + 1 : 0, e = nl[k];
        int64_t ln = e - s;
        if (ln > 0 && t[e - 1] == '\r') ln -= 1;
        line_off[k] = s;
        line_len[k] = (int32_t)ln;
    }
}

// one thread: the tail rules of index_range (unterminated last line when final, padding of a truncated record) and the
// record count / cursor for the host: res[0] = records, res[1] = cursor
__global__ void index_tail_kernel(const uint8_t *t, int64_t len, int32_t final, int64_t want, const long long *nl,
                                  int64_t nlines, int64_t *line_off, int32_t *line_len, long long *res) {
    int64_t cur = nlines ? nl[nlines - 1] + 1 : 0;
    if (final && nlines < want && cur < len) {  // data not terminated by '\n': the rest is one more line
        int64_t ln = len - cur;
        if (ln > 0 && t[len - 1] == '\r') ln -= 1;
        line_off[nlines] = cur;
        line_len[nlines] = (int32_t)ln;
        nlines += 1;
        cur = len;
    }
    const int64_t nrec = (nlines + 3) / 4;
    for (int64_t k = nlines; k < 4 * nrec; ++k) {  // a truncated last record: empty lines at the end of the text
        line_off[k] = len;
        line_len[k] = 0;
    }
    res[0] = nrec;
    res[1] = cur;
}

// ---- index of one span (bdx_fq_index_span_device) -------------------------------------------------------------------------
// per workgroup: newlines of its tile in t[0, len) -> blk, those of them in front of byte `lim` (<= len) -> blk_lim
template <bool kAligned>
__global__ void __launch_bounds__(FQ_THREADS) span_count_kernel(const uint8_t *t, int64_t len, int64_t lim, long long *blk,
                                                                long long *blk_lim) {
    long long c = 0, cl = 0;
    for (int s = 0; s < FQ_STEPS; ++s) {
        const int64_t p = (int64_t)blockIdx.x * FQ_TILE + ((int64_t)s * FQ_THREADS + threadIdx.x) * FQ_LANE_BYTES;
        const uint32_t m = newline_mask16<kAligned>(t, len, p);
        const int64_t room = lim - p;  // bytes of this lane's 16 that lie in front of lim
        c += __popc(m);
        cl += room >= FQ_LANE_BYTES ? __popc(m) : room > 0 ? __popc(m & ((1u << room) - 1u)) : 0;
    }
    long long tot, tot_lim;
    (void)block_excl_scan(c, &tot);
    (void)block_excl_scan(cl, &tot_lim);
    if (threadIdx.x == 0) {
        blk[blockIdx.x] = tot;
        blk_lim[blockIdx.x] = tot_lim;
    }
}

// Table entry k is line first + k of the window, line i being the bytes between newline i - 1 (or the window's start)
// and newline i.  Of the window's `total` newlines nl holds the first min(total, first + nlines).  Line `total` is the
// text's unterminated rest, the lines behind it pad a truncated record (the caller hands such lines out only with `final`).
__global__ void __launch_bounds__(FQ_THREADS) span_lines_kernel(const uint8_t *t, int64_t len, const long long *nl,
                                                                int64_t total, int64_t first, int64_t nlines,
                                                                int64_t *line_off, int32_t *line_len) {
    for (int64_t k = (int64_t)blockIdx.x * FQ_THREADS + threadIdx.x; k < nlines; k += (int64_t)gridDim.x * FQ_THREADS) {
        const int64_t i = first + k;
        int64_t s = len, ln = 0;
        if (i <= total) {
            s = i ? nl[i - 1] + 1 : 0;
            const int64_t e = i < total ? nl[i] : len;
            ln = e - s;
            if (ln > 0 && t[e - 1] == '\r') ln -= 1;
        }
        line_off[k] = s;
        line_len[k] = (int32_t)ln;
    }
}

// ---- pack -----------------------------------------------------------------------------------------------------------------
struct SeqLen {
    const int32_t *line_len;
    __device__ long long operator()(int64_t i) const { return max(line_len[4 * i + 1], 0); }  // (a negative length is refused by pack_kernel)
};

// a line of the table lies inside the text
__device__ inline bool line_ok(int64_t off, int32_t ln, int64_t text_len) {
    return off >= 0 && ln >= 0 && off + ln <= text_len;
}

// one wave per read: its sequence line -> seq[seq_off[i] ...]
__global__ void __launch_bounds__(FQ_THREADS) pack_kernel(const uint8_t *t, int64_t text_len, const int64_t *line_off,
                                                          const int32_t *line_len, int64_t n, uint8_t *seq,
                                                          const long long *seq_off, int *bad) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * FQ_WAVES;
    for (int64_t i = (int64_t)blockIdx.x * FQ_WAVES + (threadIdx.x >> 6); i < n; i += nw) {
        const int64_t so = line_off[4 * i + 1];
        const int32_t sl = line_len[4 * i + 1];
        if (!line_ok(so, sl, text_len)) {
            if (lane == 0) *bad = 1;
            continue;
        }
        uint8_t *o = seq + seq_off[i];
        for (int32_t j = lane; j < sl; j += 64) o[j] = t[so + j];
    }
}

// ---- classes and the stable partition -------------------------------------------------------------------------------------
// class of a read (nativeio.demux_native): 0 unknown, 1 ambiguous, else 2 + (bc1 - 1) * stride + (max(bc2, 1) - 1)
__global__ void __launch_bounds__(FQ_THREADS) class_kernel(const int32_t *bc1, const int32_t *bc2, int32_t stride,
                                                           int32_t n_classes, int64_t n, uint32_t *key, uint32_t *idx,
                                                           int *bad) {
    for (int64_t i = (int64_t)blockIdx.x * FQ_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * FQ_THREADS) {
        const int64_t b1 = bc1[i];
        int64_t c;
        if (b1 == 0)
            c = 0;
        else if (b1 < 0)
            c = 1;
        else
            c = 2 + (b1 - 1) * stride + (max(bc2[i], 1) - 1);
        if (c < 0 || c >= n_classes) {  // (never indexes a per-class table: reported, the record parks in class 0)
            *bad = 1;
            c = 0;
        }
        key[i] = (uint32_t)c;
        idx[i] = (uint32_t)i;
    }
}

// LSD counting sort, one 8-bit digit per pass.  Tile = one workgroup = FQ_THREADS records, one per thread.
// hist[d * ntiles + tile]: records of the tile with digit d (digit-major, so one exclusive scan gives every (digit, tile)
// its first output slot in stable order).
__global__ void __launch_bounds__(FQ_THREADS) digit_hist_kernel(const uint32_t *key, int64_t n, int shift,
                                                                int64_t ntiles, int32_t *hist) {
    __shared__ int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * FQ_THREADS + threadIdx.x;
    if (i < n) atomicAdd(&h[(key[i] >> shift) & 255u], 1);
    __syncthreads();
    hist[(int64_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

struct HistAt {
    const int32_t *h;
    __device__ long long operator()(int64_t i) const { return h[i]; }
};

__global__ void __launch_bounds__(FQ_THREADS) digit_scatter_kernel(const uint32_t *key_in, const uint32_t *idx_in, int64_t n,
                                                                   int shift, int64_t ntiles, const long long *base,
                                                                   uint32_t *key_out, uint32_t *idx_out) {
    __shared__ int wc[FQ_WAVES][256];  // records per (wave, digit) of this tile
    for (int w = 0; w < FQ_WAVES; ++w) wc[w][threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * FQ_THREADS + threadIdx.x;
    const bool valid = i < n;
    const uint32_t k = valid ? key_in[i] : 0u;
    const uint32_t d = (k >> shift) & 255u;
    // lanes of the wave with the same digit: match the 8 digit bits with ballots
    unsigned long long peers = __ballot(valid);
    for (int b = 0; b < 8; ++b) {
        const unsigned long long m = __ballot((d >> b) & 1u);
        peers &= ((d >> b) & 1u) ? m : ~m;
    }
    const int w = threadIdx.x >> 6;
    const int rank = __popcll(peers & lanes_below());
    if (valid && rank == 0) wc[w][d] = __popcll(peers);
    __syncthreads();
    if (!valid) return;
    long long pos = base[(int64_t)d * ntiles + blockIdx.x] + rank;
    for (int v = 0; v < w; ++v) pos += wc[v][d];
    key_out[pos] = k;
    idx_out[pos] = idx_in[i];
}

// ---- gather -----------------------------------------------------------------------------------------------------------------
// output of record i (demux_write_impl): header \n seq[a..b] \n plus \n qual[a..min(b, qual_len)] \n;
// untrimmed: a = 1, b = seq_len
struct RecordShape {
    const int64_t *line_off;
    const int32_t *line_len;
    const int32_t *keep_start, *keep_end;
    int32_t trim;
    // (a negative length is refused by gather_kernel; clamped here so that the offsets stay monotonic)
    __device__ int64_t len(int64_t k) const { return max(line_len[k], 0); }
    __device__ void slice(int64_t i, int64_t &a, int64_t &sl, int64_t &ql) const {
        sl = len(4 * i + 1);
        ql = len(4 * i + 3);
        a = 1;
        if (trim && keep_start[i] != -1) {
            a = max<int64_t>(keep_start[i], 1);
            const int64_t b = min<int64_t>(keep_end[i], sl);
            if (a > b) {
                sl = 0;
                ql = 0;
                return;
            }
            sl = b - a + 1;
            const int64_t qb = min<int64_t>(b, ql);  // the quality line is cut with the same range, clamped to its own length
            ql = qb >= a ? qb - a + 1 : 0;
        }
    }
    __device__ long long bytes(int64_t i) const {
        int64_t a, sl, ql;
        slice(i, a, sl, ql);
        return (long long)len(4 * i) + sl + len(4 * i + 2) + ql + 4;
    }
};

struct BytesAt {
    RecordShape r;
    const uint32_t *perm;
    __device__ long long operator()(int64_t j) const { return r.bytes(perm[j]); }
};

// first / last byte of every class that occurs (its records are consecutive in partition order)
__global__ void __launch_bounds__(FQ_THREADS) class_bounds_kernel(const uint32_t *skey, const long long *off, int64_t n,
                                                                  long long *cstart, long long *cend) {
    for (int64_t j = (int64_t)blockIdx.x * FQ_THREADS + threadIdx.x; j < n; j += (int64_t)gridDim.x * FQ_THREADS) {
        const uint32_t c = skey[j];
        if (j == 0 || skey[j - 1] != c) cstart[c] = off[j];
        if (j == n - 1 || skey[j + 1] != c) cend[c] = off[j + 1];
    }
}

__global__ void __launch_bounds__(FQ_THREADS) class_bytes_kernel(const long long *cstart, long long *cend, int64_t n_classes) {
    for (int64_t c = (int64_t)blockIdx.x * FQ_THREADS + threadIdx.x; c < n_classes; c += (int64_t)gridDim.x * FQ_THREADS)
        cend[c] -= cstart[c];
}

__device__ inline void copy_bytes(uint8_t *o, const uint8_t *s, int64_t len, int lane) {
    for (int64_t j = lane; j < len; j += 64) o[j] = s[j];
}

// one wave per record in partition order
__global__ void __launch_bounds__(FQ_THREADS) gather_kernel(const uint8_t *t, int64_t text_len, RecordShape r,
                                                            const uint32_t *perm, const long long *off, int64_t n,
                                                            uint8_t *out, int *bad) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * FQ_WAVES;
    for (int64_t j = (int64_t)blockIdx.x * FQ_WAVES + (threadIdx.x >> 6); j < n; j += nw) {
        const int64_t i = perm[j];
        bool ok = true;
        for (int l = 0; l < 4; ++l) ok = ok && line_ok(r.line_off[4 * i + l], r.line_len[4 * i + l], text_len);
        if (!ok) {
            if (lane == 0) *bad = 1;
            continue;
        }
        int64_t a, sl, ql;
        r.slice(i, a, sl, ql);
        const int64_t hl = r.len(4 * i), pl = r.len(4 * i + 2);
        uint8_t *o = out + off[j];
        copy_bytes(o, t + r.line_off[4 * i], hl, lane);
        o += hl + 1;
        copy_bytes(o, t + r.line_off[4 * i + 1] + a - 1, sl, lane);
        o += sl + 1;
        copy_bytes(o, t + r.line_off[4 * i + 2], pl, lane);
        o += pl + 1;
        copy_bytes(o, t + r.line_off[4 * i + 3] + a - 1, ql, lane);
        if (lane == 0) {
            out[off[j] + hl] = '\n';
            out[off[j] + hl + 1 + sl] = '\n';
            out[off[j] + hl + 1 + sl + 1 + pl] = '\n';
            out[off[j] + hl + 1 + sl + 1 + pl + 1 + ql] = '\n';
        }
    }
}

// ---- record and pair checks (bdx_fq_check_device, bdx_fq_check_pair_device) ---------------------------------------------
constexpr int FQ_CHECK_GRID = 2048;           // most workgroups of a check: 8 per CU, a grid-stride loop beyond
constexpr int FQ_NAME_LANES = 16;             // lanes that walk one pair of header lines together
constexpr int FQ_NAME_GROUPS = FQ_THREADS / FQ_NAME_LANES;
constexpr unsigned long long FQ_NO_KEY = ~0ull;

// The workgroup's smallest key, in thread 0 (every thread calls it): a wave minimum by shuffles, then one word per wave in LDS.
__device__ inline unsigned long long block_min_key(unsigned long long key) {
    __shared__ unsigned long long wmin[FQ_WAVES];
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(key, d, 64);
        key = o < key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < FQ_WAVES; ++k) key = wmin[k] < key ? wmin[k] : key;
    return key;
}

// the four table words of one kind of a record: two 16-byte loads (or one) when the table's address allows it
template <bool kVec>
__device__ inline void load_record_words(const int64_t *line_off, const int32_t *line_len, int64_t i, int64_t (&off)[4],
                                         int32_t (&len)[4]) {
    if (kVec) {
        const longlong2 a = *reinterpret_cast<const longlong2 *>(line_off + 4 * i);
        const longlong2 b = *reinterpret_cast<const longlong2 *>(line_off + 4 * i + 2);
        const int4 l = *reinterpret_cast<const int4 *>(line_len + 4 * i);
        off[0] = a.x, off[1] = a.y, off[2] = b.x, off[3] = b.y;
        len[0] = l.x, len[1] = l.y, len[2] = l.z, len[3] = l.w;
    } else {
        for (int k = 0; k < 4; ++k) {
            off[k] = line_off[4 * i + k];
            len[k] = line_len[4 * i + k];
        }
    }
}

// One lane per record: 48 bytes of table (consecutive lanes read consecutive records: whole cache lines), the first
// byte of lines 1 and 3.  key = (index << 8) | broken rules; the lowest key of a workgroup that holds a failure goes
// into *result with one atomicMin — a clean text costs no atomic at all.
template <bool kVec>
__global__ void __launch_bounds__(FQ_THREADS) check_kernel(const uint8_t *t, int64_t text_len, const int64_t *line_off,
                                                           const int32_t *line_len, int64_t n, int32_t rules,
                                                           unsigned long long *result, int *bad) {
    unsigned long long key = FQ_NO_KEY;
    for (int64_t i = (int64_t)blockIdx.x * FQ_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * FQ_THREADS) {
        int64_t off[4];
        int32_t len[4];
        load_record_words<kVec>(line_off, line_len, i, off, len);
        bool ok = true;
        for (int k = 0; k < 4; ++k) ok = ok && line_ok(off[k], len[k], text_len);
        if (!ok) {
            *bad = 1;
            continue;
        }
        int32_t m = 0;
        if ((rules & BDX_FQ_CHECK_HEADER) && (len[0] == 0 || t[off[0]] != '@')) m |= BDX_FQ_CHECK_HEADER;
        if ((rules & BDX_FQ_CHECK_PLUS) && (len[2] == 0 || t[off[2]] != '+')) m |= BDX_FQ_CHECK_PLUS;
        if ((rules & BDX_FQ_CHECK_LENGTH) && len[1] != len[3]) m |= BDX_FQ_CHECK_LENGTH;
        if (m && key == FQ_NO_KEY) key = ((unsigned long long)i << 8) | (unsigned)m;  // (a lane's records ascend)
    }
    key = block_min_key(key);
    if (threadIdx.x == 0 && key != FQ_NO_KEY) atomicMin(result, key);
}

// FQ_NAME_LANES lanes per record.  Lane j looks at byte 1 + 16 s + j of both header lines in step s (byte loads inside
// the lines only: nothing outside a text is read at any alignment); a byte at or behind a line's end counts as a blank.
// The group's ballots give each token's end (the first blank) and the first position at which the lines differ; the
// "/1" / "/2" suffix is judged from the two bytes in front of the token's end.  The names are equal when their lengths
// are and the first difference lies behind them.  key = index, reduced like check_kernel's.
__global__ void __launch_bounds__(FQ_THREADS) check_pair_kernel(const uint8_t *t1, int64_t text_len1, const int64_t *line_off1,
                                                                const int32_t *line_len1, const uint8_t *t2, int64_t text_len2,
                                                                const int64_t *line_off2, const int32_t *line_len2, int64_t n,
                                                                unsigned long long *result, int *bad) {
    const int j = threadIdx.x & (FQ_NAME_LANES - 1);
    const int shift = (threadIdx.x & 63) & ~(FQ_NAME_LANES - 1);  // the group's first lane in the wave
    unsigned long long key = FQ_NO_KEY;
    const int64_t stride = (int64_t)gridDim.x * FQ_NAME_GROUPS;
    // (every lane of a wave makes the same number of trips: the ballots below are wave-wide)
    const int64_t trips = (n + stride - 1) / stride;
    for (int64_t trip = 0; trip < trips; ++trip) {
        const int64_t i = trip * stride + (int64_t)blockIdx.x * FQ_NAME_GROUPS + threadIdx.x / FQ_NAME_LANES;
        bool live = i < n;
        int64_t o1 = 0, o2 = 0, h1 = 0, h2 = 0;
        if (live) {
            o1 = line_off1[4 * i], o2 = line_off2[4 * i];
            const int32_t l1 = line_len1[4 * i], l2 = line_len2[4 * i];
            if (!line_ok(o1, l1, text_len1) || !line_ok(o2, l2, text_len2)) {
                *bad = 1;
                live = false;
            }
            h1 = l1, h2 = l2;
        }
        int64_t end1 = -1, end2 = -1, diff = -1;  // not known yet
        bool open = live;
        for (int64_t p0 = 1; __ballot(open) != 0ull; p0 += FQ_NAME_LANES) {
            const int64_t p = p0 + j;
            const uint8_t b1 = open && p < h1 ? t1[o1 + p] : (uint8_t)' ';
            const uint8_t b2 = open && p < h2 ? t2[o2 + p] : (uint8_t)' ';
            const unsigned g1 = (unsigned)(__ballot(b1 == ' ' || b1 == '\t') >> shift) & 0xFFFFu;
            const unsigned g2 = (unsigned)(__ballot(b2 == ' ' || b2 == '\t') >> shift) & 0xFFFFu;
            const unsigned gd = (unsigned)(__ballot(b1 != b2) >> shift) & 0xFFFFu;
            if (open) {
                if (end1 < 0 && g1) end1 = p0 + (__ffs(g1) - 1);
                if (end2 < 0 && g2) end2 = p0 + (__ffs(g2) - 1);
                if (diff < 0 && gd) diff = p0 + (__ffs(gd) - 1);
                open = end1 < 0 || end2 < 0;
            }
        }
        if (live) {
            // token = bytes [1, end): the name drops one "/1" or "/2" the token ends in
            int64_t n1 = end1 - 1, n2 = end2 - 1;
            if (n1 >= 2 && t1[o1 + end1 - 2] == '/' && (t1[o1 + end1 - 1] == '1' || t1[o1 + end1 - 1] == '2')) n1 -= 2;
            if (n2 >= 2 && t2[o2 + end2 - 2] == '/' && (t2[o2 + end2 - 1] == '1' || t2[o2 + end2 - 1] == '2')) n2 -= 2;
            const bool same = n1 == n2 && (diff < 0 || diff >= 1 + n1);
            if (!same && key == FQ_NO_KEY) key = (unsigned long long)i;
        }
    }
    key = block_min_key(key);
    if (threadIdx.x == 0 && key != FQ_NO_KEY) atomicMin(result, key);
}

unsigned grid_for(int64_t items, int64_t per_block) {
    const int64_t g = (items + per_block - 1) / per_block;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(g, 1 << 20));
}

// 8 bytes -> host (synchronises the stream)
hipError_t read_back(bdx_ctx *ctx, const void *d, void *h, size_t bytes) {
    hipError_t e = hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return e;
}

hipError_t poison(bdx_ctx *ctx, void *p, size_t bytes) {
    return (ctx->tune.poison && p && bytes) ? hipMemsetAsync(p, 0xA5, bytes, ctx->stream) : hipSuccess;
}

}  // namespace

extern "C" {

int32_t bdx_fq_index_device(bdx_ctx *ctx, const uint8_t *d_text, int64_t text_len, int32_t final, int64_t max_reads,
                            int64_t *d_line_off, int32_t *d_line_len, int64_t *n_records, int64_t *next) {
    if (!ctx) return BDX_E_INVALID;
    if (!n_records || !next) return bdx_fail(ctx, BDX_E_INVALID, "n_records / next is NULL");
    *n_records = 0;
    *next = 0;
    if (text_len < 0 || max_reads < 0) return bdx_fail(ctx, BDX_E_INVALID, "text_len / max_reads is negative");
    if (max_reads > ((int64_t)1 << 40)) return bdx_fail(ctx, BDX_E_INVALID, "max_reads is too large");
    if (text_len == 0 || max_reads == 0) return BDX_OK;
    if (!d_text || !d_line_off || !d_line_len) return bdx_fail(ctx, BDX_E_INVALID, "NULL device pointer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t want = 4 * max_reads;
    HIP_TRY(ctx, poison(ctx, d_line_off, (size_t)want * 8));
    HIP_TRY(ctx, poison(ctx, d_line_len, (size_t)want * 4));
    const int64_t nb = (text_len + FQ_TILE - 1) / FQ_TILE;
    HIP_TRY(ctx, ctx->fq[FQ_BLK].ensure((size_t)(nb + 1) * 8));
    HIP_TRY(ctx, ctx->fq[FQ_SMALL].ensure(64));
    long long *blk = (long long *)ctx->fq[FQ_BLK].p;
    long long *small = (long long *)ctx->fq[FQ_SMALL].p;
    const bool aligned = ((uintptr_t)d_text & 15) == 0;
    if (aligned)
        nl_count_kernel<true><<<dim3((unsigned)nb), dim3(FQ_THREADS), 0, ctx->stream>>>(d_text, text_len, blk);
    else
        nl_count_kernel<false><<<dim3((unsigned)nb), dim3(FQ_THREADS), 0, ctx->stream>>>(d_text, text_len, blk);
    scan_small_kernel<<<dim3(1), dim3(FQ_THREADS), 0, ctx->stream>>>(blk, nb);
    HIP_TRY(ctx, hipGetLastError());
    long long total = 0;
    HIP_TRY(ctx, read_back(ctx, blk + nb, &total, 8));
    // lines terminated by a newline that this call hands out; without `final` only whole records
    int64_t nlines = std::min<int64_t>(total, want);
    if (!final) nlines -= nlines % 4;
    HIP_TRY(ctx, ctx->fq[FQ_NL].ensure((size_t)std::max<int64_t>(nlines, 1) * 8));
    long long *nl = (long long *)ctx->fq[FQ_NL].p;
    HIP_TRY(ctx, poison(ctx, nl, (size_t)nlines * 8));
    if (nlines > 0) {
        if (aligned)
            nl_scatter_kernel<true><<<dim3((unsigned)nb), dim3(FQ_THREADS), 0, ctx->stream>>>(d_text, text_len, blk, nl, nlines);
        else
            nl_scatter_kernel<false><<<dim3((unsigned)nb), dim3(FQ_THREADS), 0, ctx->stream>>>(d_text, text_len, blk, nl, nlines);
        lines_kernel<<<dim3(grid_for(nlines, FQ_THREADS)), dim3(FQ_THREADS), 0, ctx->stream>>>(d_text, nl, nlines, d_line_off,
                                                                                               d_line_len);
    }
    index_tail_kernel<<<dim3(1), dim3(1), 0, ctx->stream>>>(d_text, text_len, final, want, nl, nlines, d_line_off, d_line_len,
                                                             small);
    HIP_TRY(ctx, hipGetLastError());
    long long res[2] = {0, 0};
    HIP_TRY(ctx, read_back(ctx, small, res, 16));
    *n_records = res[0];
    *next = res[1];
    return BDX_OK;
}

int32_t bdx_fq_count_lines_device(bdx_ctx *ctx, const uint8_t *d_text, int64_t len, int64_t *n_newlines) {
    if (!ctx) return BDX_E_INVALID;
    if (!n_newlines) return bdx_fail(ctx, BDX_E_INVALID, "n_newlines is NULL");
    *n_newlines = 0;
    if (len < 0) return bdx_fail(ctx, BDX_E_INVALID, "len is negative");
    if (len == 0) return BDX_OK;
    if (!d_text) return bdx_fail(ctx, BDX_E_INVALID, "NULL device pointer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t nb = (len + FQ_TILE - 1) / FQ_TILE;
    HIP_TRY(ctx, ctx->fq[FQ_BLK].ensure((size_t)(nb + 1) * 8));
    long long *blk = (long long *)ctx->fq[FQ_BLK].p;
    if (((uintptr_t)d_text & 15) == 0)
        nl_count_kernel<true><<<dim3((unsigned)nb), dim3(FQ_THREADS), 0, ctx->stream>>>(d_text, len, blk);
    else
        nl_count_kernel<false><<<dim3((unsigned)nb), dim3(FQ_THREADS), 0, ctx->stream>>>(d_text, len, blk);
    scan_small_kernel<<<dim3(1), dim3(FQ_THREADS), 0, ctx->stream>>>(blk, nb);
    HIP_TRY(ctx, hipGetLastError());
    long long total = 0;
    HIP_TRY(ctx, read_back(ctx, blk + nb, &total, 8));
    *n_newlines = total;
    return BDX_OK;
}

int32_t bdx_fq_index_span_device(bdx_ctx *ctx, const uint8_t *d_text, int64_t text_len, int64_t span_len, int32_t phase,
                                 int32_t starts_line, int32_t final, int64_t max_reads, int64_t *d_line_off,
                                 int32_t *d_line_len, int64_t *n_records, int32_t *complete) {
    if (!ctx) return BDX_E_INVALID;
    if (!n_records || !complete) return bdx_fail(ctx, BDX_E_INVALID, "n_records / complete is NULL");
    *n_records = 0;
    *complete = 1;
    if (text_len < 0 || span_len < 0 || max_reads < 0)
        return bdx_fail(ctx, BDX_E_INVALID, "text_len / span_len / max_reads is negative");
    if (span_len > text_len)
        return bdx_fail(ctx, BDX_E_INVALID, "span_len (%lld) is larger than text_len (%lld)", (long long)span_len, (long long)text_len);
    if (phase < 0 || phase > 3) return bdx_fail(ctx, BDX_E_INVALID, "phase must be 0 .. 3 (got %d)", (int)phase);
    if (max_reads > ((int64_t)1 << 40)) return bdx_fail(ctx, BDX_E_INVALID, "max_reads is too large");
    if (span_len == 0) return BDX_OK;  // (no line starts in front of byte 0)
    if (!d_text || !d_line_off || !d_line_len) return bdx_fail(ctx, BDX_E_INVALID, "NULL device pointer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t nb = (text_len + FQ_TILE - 1) / FQ_TILE;
    HIP_TRY(ctx, ctx->fq[FQ_BLK].ensure((size_t)(nb + 1) * 8));
    HIP_TRY(ctx, ctx->fq[FQ_PART].ensure((size_t)(nb + 1) * 8));
    long long *blk = (long long *)ctx->fq[FQ_BLK].p;
    long long *blk_lim = (long long *)ctx->fq[FQ_PART].p;
    const bool aligned = ((uintptr_t)d_text & 15) == 0;
    // a line that starts in the span at byte s > 0 follows a newline in front of byte span_len - 1
    if (aligned)
        span_count_kernel<true><<<dim3((unsigned)nb), dim3(FQ_THREADS), 0, ctx->stream>>>(d_text, text_len, span_len - 1, blk, blk_lim);
    else
        span_count_kernel<false><<<dim3((unsigned)nb), dim3(FQ_THREADS), 0, ctx->stream>>>(d_text, text_len, span_len - 1, blk, blk_lim);
    scan_small_kernel<<<dim3(1), dim3(FQ_THREADS), 0, ctx->stream>>>(blk, nb);
    scan_small_kernel<<<dim3(1), dim3(FQ_THREADS), 0, ctx->stream>>>(blk_lim, nb);
    HIP_TRY(ctx, hipGetLastError());
    long long total = 0, in_span = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&in_span, blk_lim + nb, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, read_back(ctx, blk + nb, &total, 8));
    // window line i (i newlines in front of it) has the global number phase + i; lines 0 .. in_span start in the span,
    // line 0 only with starts_line
    int64_t first = (4 - phase) % 4;
    if (first == 0 && !starts_line) first = 4;
    if (first > in_span) return BDX_OK;
    const int64_t nrec = (in_span - first) / 4 + 1;
    *n_records = nrec;
    if (nrec > max_reads)
        return bdx_fail(ctx, BDX_E_SPACE, "%lld records start in the span, the line table holds %lld", (long long)nrec, (long long)max_reads);
    const int64_t nlines = 4 * nrec;
    if (first + nlines > total && !final) {  // the last record's fourth line ends behind the window
        *complete = 0;
        return BDX_OK;
    }
    const int64_t cap = std::min<int64_t>(total, first + nlines);
    HIP_TRY(ctx, ctx->fq[FQ_NL].ensure((size_t)std::max<int64_t>(cap, 1) * 8));
    long long *nl = (long long *)ctx->fq[FQ_NL].p;
    HIP_TRY(ctx, poison(ctx, nl, (size_t)cap * 8));
    HIP_TRY(ctx, poison(ctx, d_line_off, (size_t)nlines * 8));
    HIP_TRY(ctx, poison(ctx, d_line_len, (size_t)nlines * 4));
    if (cap > 0) {
        if (aligned)
            nl_scatter_kernel<true><<<dim3((unsigned)nb), dim3(FQ_THREADS), 0, ctx->stream>>>(d_text, text_len, blk, nl, cap);
        else
            nl_scatter_kernel<false><<<dim3((unsigned)nb), dim3(FQ_THREADS), 0, ctx->stream>>>(d_text, text_len, blk, nl, cap);
    }
    span_lines_kernel<<<dim3(grid_for(nlines, FQ_THREADS)), dim3(FQ_THREADS), 0, ctx->stream>>>(d_text, text_len, nl, total, first,
                                                                                                nlines, d_line_off, d_line_len);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return BDX_OK;
}

int32_t bdx_fq_pack_device(bdx_ctx *ctx, const uint8_t *d_text, int64_t text_len, const int64_t *d_line_off,
                           const int32_t *d_line_len, int64_t n, uint8_t *d_seq, int64_t seq_cap, int64_t *d_seq_off,
                           int64_t *seq_bytes) {
    if (!ctx) return BDX_E_INVALID;
    if (n < 0 || text_len < 0 || seq_cap < 0) return bdx_fail(ctx, BDX_E_INVALID, "n / text_len / seq_cap is negative");
    if (!d_seq_off) return bdx_fail(ctx, BDX_E_INVALID, "NULL device pointer");
    if (n > 0 && (!d_text || !d_line_off || !d_line_len || !d_seq)) return bdx_fail(ctx, BDX_E_INVALID, "NULL device pointer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, poison(ctx, d_seq_off, (size_t)(n + 1) * 8));
    HIP_TRY(ctx, exclusive_scan(ctx, SeqLen{d_line_len}, n, (long long *)d_seq_off));
    long long total = 0;
    HIP_TRY(ctx, read_back(ctx, d_seq_off + n, &total, 8));
    if (seq_bytes) *seq_bytes = total;
    if (total > seq_cap)
        return bdx_fail(ctx, BDX_E_INVALID, "packed reads need %lld bytes, d_seq holds %lld", (long long)total, (long long)seq_cap);
    if (n == 0) return BDX_OK;
    HIP_TRY(ctx, poison(ctx, d_seq, (size_t)total));
    HIP_TRY(ctx, ctx->fq[FQ_SMALL].ensure(64));
    int *bad = (int *)ctx->fq[FQ_SMALL].p;
    HIP_TRY(ctx, hipMemsetAsync(bad, 0, 4, ctx->stream));
    pack_kernel<<<dim3(grid_for(n, FQ_WAVES)), dim3(FQ_THREADS), 0, ctx->stream>>>(d_text, text_len, d_line_off, d_line_len, n,
                                                                                    d_seq, (const long long *)d_seq_off, bad);
    HIP_TRY(ctx, hipGetLastError());
    int flag = 0;
    HIP_TRY(ctx, read_back(ctx, bad, &flag, 4));
    if (flag) return bdx_fail(ctx, BDX_E_INVALID, "a sequence line of the line table lies outside the text");
    return BDX_OK;
}

int32_t bdx_fq_gather_device(bdx_ctx *ctx, const uint8_t *d_text, int64_t text_len, const int64_t *d_line_off,
                             const int32_t *d_line_len, int64_t n, const int32_t *d_bc1, const int32_t *d_bc2, int32_t stride,
                             int32_t n_classes, const int32_t *d_keep_start, const int32_t *d_keep_end, int32_t trim,
                             uint8_t *d_out, int64_t out_cap, int64_t *class_bytes) {
    if (!ctx) return BDX_E_INVALID;
    if (n < 0 || text_len < 0 || out_cap < 0) return bdx_fail(ctx, BDX_E_INVALID, "n / text_len / out_cap is negative");
    if (n > 0xFFFFFFFFLL) return bdx_fail(ctx, BDX_E_INVALID, "more than 2^32 - 1 records in one call");
    if (n_classes < 2 || stride < 1) return bdx_fail(ctx, BDX_E_INVALID, "n_classes must be >= 2 and stride >= 1");
    if (!class_bytes) return bdx_fail(ctx, BDX_E_INVALID, "class_bytes is NULL");
    std::fill(class_bytes, class_bytes + n_classes, (int64_t)0);
    if (n == 0) return BDX_OK;
    if (!d_text || !d_line_off || !d_line_len || !d_bc1 || !d_bc2 || !d_out || (trim && (!d_keep_start || !d_keep_end)))
        return bdx_fail(ctx, BDX_E_INVALID, "NULL device pointer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t ntiles = (n + FQ_THREADS - 1) / FQ_THREADS;
    HIP_TRY(ctx, ctx->fq[FQ_SMALL].ensure(64));
    for (int b : {FQ_KEY_A, FQ_KEY_B, FQ_IDX_A, FQ_IDX_B}) HIP_TRY(ctx, ctx->fq[b].ensure((size_t)n * 4));
    HIP_TRY(ctx, ctx->fq[FQ_HIST].ensure((size_t)ntiles * 256 * 4));
    HIP_TRY(ctx, ctx->fq[FQ_BASE].ensure(((size_t)ntiles * 256 + 1) * 8));
    HIP_TRY(ctx, ctx->fq[FQ_OFF].ensure(((size_t)n + 1) * 8));
    HIP_TRY(ctx, ctx->fq[FQ_CLASS].ensure((size_t)n_classes * 16));
    int *bad = (int *)ctx->fq[FQ_SMALL].p;
    uint32_t *key = (uint32_t *)ctx->fq[FQ_KEY_A].p, *key2 = (uint32_t *)ctx->fq[FQ_KEY_B].p;
    uint32_t *idx = (uint32_t *)ctx->fq[FQ_IDX_A].p, *idx2 = (uint32_t *)ctx->fq[FQ_IDX_B].p;
    int32_t *hist = (int32_t *)ctx->fq[FQ_HIST].p;
    long long *base = (long long *)ctx->fq[FQ_BASE].p, *off = (long long *)ctx->fq[FQ_OFF].p;
    long long *cstart = (long long *)ctx->fq[FQ_CLASS].p, *cend = cstart + n_classes;
    for (int b : {FQ_KEY_A, FQ_KEY_B, FQ_IDX_A, FQ_IDX_B}) HIP_TRY(ctx, poison(ctx, ctx->fq[b].p, (size_t)n * 4));
    HIP_TRY(ctx, poison(ctx, hist, (size_t)ntiles * 256 * 4));
    HIP_TRY(ctx, poison(ctx, base, ((size_t)ntiles * 256 + 1) * 8));
    HIP_TRY(ctx, poison(ctx, off, ((size_t)n + 1) * 8));
    HIP_TRY(ctx, hipMemsetAsync(bad, 0, 8, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(cstart, 0, (size_t)n_classes * 16, ctx->stream));  // classes without records: 0 bytes
    class_kernel<<<dim3(grid_for(n, FQ_THREADS)), dim3(FQ_THREADS), 0, ctx->stream>>>(d_bc1, d_bc2, stride, n_classes, n, key, idx,
                                                                                       bad);
    HIP_TRY(ctx, hipGetLastError());
    // stable partition by class: LSD counting sort over the bytes of the class id that can be non-zero
    for (int shift = 0; shift < 32 && ((uint32_t)(n_classes - 1) >> shift) != 0; shift += 8) {
        digit_hist_kernel<<<dim3((unsigned)ntiles), dim3(FQ_THREADS), 0, ctx->stream>>>(key, n, shift, ntiles, hist);
        HIP_TRY(ctx, exclusive_scan(ctx, HistAt{hist}, ntiles * 256, base));
        digit_scatter_kernel<<<dim3((unsigned)ntiles), dim3(FQ_THREADS), 0, ctx->stream>>>(key, idx, n, shift, ntiles, base, key2,
                                                                                           idx2);
        HIP_TRY(ctx, hipGetLastError());
        std::swap(key, key2);
        std::swap(idx, idx2);
    }
    const RecordShape shape{d_line_off, d_line_len, d_keep_start, d_keep_end, trim};
    HIP_TRY(ctx, exclusive_scan(ctx, BytesAt{shape, idx}, n, off));
    class_bounds_kernel<<<dim3(grid_for(n, FQ_THREADS)), dim3(FQ_THREADS), 0, ctx->stream>>>(key, off, n, cstart, cend);
    class_bytes_kernel<<<dim3(grid_for(n_classes, FQ_THREADS)), dim3(FQ_THREADS), 0, ctx->stream>>>(cstart, cend, n_classes);
    HIP_TRY(ctx, hipGetLastError());
    long long total = 0;
    int flag = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&flag, bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(class_bytes, cend, (size_t)n_classes * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, read_back(ctx, off + n, &total, 8));
    if (flag) return bdx_fail(ctx, BDX_E_INVALID, "class index out of range (bc1 / bc2 / stride / n_classes disagree)");
    if (total > out_cap)
        return bdx_fail(ctx, BDX_E_INVALID, "the blocks need %lld bytes, d_out holds %lld", (long long)total, (long long)out_cap);
    HIP_TRY(ctx, poison(ctx, d_out, (size_t)total));
    gather_kernel<<<dim3(grid_for(n, FQ_WAVES)), dim3(FQ_THREADS), 0, ctx->stream>>>(d_text, text_len, shape, idx, off, n, d_out,
                                                                                      bad + 1);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, read_back(ctx, bad + 1, &flag, 4));
    if (flag) return bdx_fail(ctx, BDX_E_INVALID, "a line of the line table lies outside the text");
    return BDX_OK;
}

// what both checks read back: the smallest key (8 bytes) and the line flag behind it
static int32_t check_result(bdx_ctx *ctx, unsigned long long *key) {
    struct {
        unsigned long long key;
        int flag, pad;
    } res = {FQ_NO_KEY, 0, 0};
    HIP_TRY(ctx, read_back(ctx, ctx->fq[FQ_SMALL].p, &res, 16));
    if (res.flag) return bdx_fail(ctx, BDX_E_INVALID, "a line of the line table lies outside the text");
    *key = res.key;
    return BDX_OK;
}

static hipError_t check_begin(bdx_ctx *ctx) {
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = ctx->fq[FQ_SMALL].ensure(64);
    if (e == hipSuccess) e = hipMemsetAsync(ctx->fq[FQ_SMALL].p, 0xFF, 8, ctx->stream);  // no key yet
    if (e == hipSuccess) e = hipMemsetAsync((char *)ctx->fq[FQ_SMALL].p + 8, 0, 8, ctx->stream);
    return e;
}

int32_t bdx_fq_check_device(bdx_ctx *ctx, const uint8_t *d_text, int64_t text_len, const int64_t *d_line_off,
                            const int32_t *d_line_len, int64_t n, int32_t rules, int64_t *first_bad, int32_t *broken) {
    if (!ctx) return BDX_E_INVALID;
    if (!first_bad || !broken) return bdx_fail(ctx, BDX_E_INVALID, "first_bad / broken is NULL");
    *first_bad = -1;
    *broken = 0;
    if (n < 0 || text_len < 0) return bdx_fail(ctx, BDX_E_INVALID, "n / text_len is negative");
    if (rules <= 0 || (rules & ~7) != 0) return bdx_fail(ctx, BDX_E_INVALID, "rules must be a mask of 1, 2 and 4 (got %d)", (int)rules);
    if (n > 0xFFFFFFFFLL) return bdx_fail(ctx, BDX_E_INVALID, "more than 2^32 - 1 records in one call");
    if (n == 0) return BDX_OK;
    if (!d_text || !d_line_off || !d_line_len) return bdx_fail(ctx, BDX_E_INVALID, "NULL device pointer");
    HIP_TRY(ctx, check_begin(ctx));
    unsigned long long *result = (unsigned long long *)ctx->fq[FQ_SMALL].p;
    int *bad = (int *)(result + 1);
    const dim3 grid((unsigned)std::min<int64_t>((n + FQ_THREADS - 1) / FQ_THREADS, FQ_CHECK_GRID));
    if ((((uintptr_t)d_line_off | (uintptr_t)d_line_len) & 15) == 0)
        check_kernel<true><<<grid, dim3(FQ_THREADS), 0, ctx->stream>>>(d_text, text_len, d_line_off, d_line_len, n, rules, result, bad);
    else
        check_kernel<false><<<grid, dim3(FQ_THREADS), 0, ctx->stream>>>(d_text, text_len, d_line_off, d_line_len, n, rules, result, bad);
    HIP_TRY(ctx, hipGetLastError());
    unsigned long long key = FQ_NO_KEY;
    const int32_t rc = check_result(ctx, &key);
    if (rc != BDX_OK) return rc;
    if (key != FQ_NO_KEY) {
        *first_bad = (int64_t)(key >> 8);
        *broken = (int32_t)(key & 0xFF);
    }
    return BDX_OK;
}

int32_t bdx_fq_check_pair_device(bdx_ctx *ctx, const uint8_t *d_text1, int64_t text_len1, const int64_t *d_line_off1,
                                 const int32_t *d_line_len1, const uint8_t *d_text2, int64_t text_len2,
                                 const int64_t *d_line_off2, const int32_t *d_line_len2, int64_t n, int64_t *first_bad) {
    if (!ctx) return BDX_E_INVALID;
    if (!first_bad) return bdx_fail(ctx, BDX_E_INVALID, "first_bad is NULL");
    *first_bad = -1;
    if (n < 0 || text_len1 < 0 || text_len2 < 0) return bdx_fail(ctx, BDX_E_INVALID, "n / text_len is negative");
    if (n > 0xFFFFFFFFLL) return bdx_fail(ctx, BDX_E_INVALID, "more than 2^32 - 1 records in one call");
    if (n == 0) return BDX_OK;
    if (!d_text1 || !d_line_off1 || !d_line_len1 || !d_text2 || !d_line_off2 || !d_line_len2)
        return bdx_fail(ctx, BDX_E_INVALID, "NULL device pointer");
    HIP_TRY(ctx, check_begin(ctx));
    unsigned long long *result = (unsigned long long *)ctx->fq[FQ_SMALL].p;
    const dim3 grid((unsigned)std::min<int64_t>((n + FQ_NAME_GROUPS - 1) / FQ_NAME_GROUPS, FQ_CHECK_GRID));
    check_pair_kernel<<<grid, dim3(FQ_THREADS), 0, ctx->stream>>>(d_text1, text_len1, d_line_off1, d_line_len1, d_text2, text_len2,
                                                                   d_line_off2, d_line_len2, n, result, (int *)(result + 1));
    HIP_TRY(ctx, hipGetLastError());
    unsigned long long key = FQ_NO_KEY;
    const int32_t rc = check_result(ctx, &key);
    if (rc != BDX_OK) return rc;
    if (key != FQ_NO_KEY) *first_bad = (int64_t)key;
    return BDX_OK;
}

}  // extern "C"
