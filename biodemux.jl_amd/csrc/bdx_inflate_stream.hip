// bdx_inflate_stream.hip — an ORDINARY .gz input of the device FASTQ pipeline inflated on the device: one gzip member (or
// a few) of any size, no size tags.  The whole compressed file is in device memory; it is cut into chunks, every chunk
// guesses a block start from the redundancy of a dynamic block's header and counts from there, one wave chains the
// guesses that a confirmed decoder arrives at, and the segments between them are decoded side by side into a 16-bit
// image whose references into the unknown window are resolved afterwards.  The steps are bdx_inflate_stream_core.h;
// this file holds one kernel per step and the C-ABI entries.  Ordering comes from the kernel boundaries on the
// context's stream: no workgroup waits for another one.
//
//   infs_scan_kernel     one chunk per workgroup of 64 threads, a persistent grid (search, then count)
//   infs_chain_kernel    one workgroup: records -> segment list, the plain size
//   infs_decode_kernel   one segment per workgroup, a persistent grid
//   infs_tails_kernel    ONE workgroup of INFS_TAIL_THREADS threads, the segments in order
//   infs_rest_kernel     one segment per workgroup: the rest of its bytes, its CRC-32
//   infs_verdict_kernel  one workgroup: CRC-32 and ISIZE of every member against its trailer
//
// The WINDOWED form (bdx_fq_inflate_window_*, bdx_inflate_window_core.h) takes the file a bounded window at a time from a
// carried state.  Decode, tails and rest are the kernels above (tails and rest get the 32 KiB in front of the window);
// scan, chain and verdict have a variant each that reads, and the verdict alone writes, the carried state:
//   infw_scan_kernel, infw_chain_kernel, infw_verdict_kernel
#include <algorithm>

#include "bdx_ctx.h"
#include "bdx_inflate_window_core.h"

namespace {

// bdx_ctx::inf[] behind the two buffers of bdx_inflate.hip
enum { INFS_BUF_RECORDS = 2, INFS_BUF_SEGMENTS, INFS_BUF_RESULT, INFS_BUF_STAGE, INFS_NBUF };
static_assert(INFS_NBUF <= BDX_INF_SCRATCH, "bdx_ctx::inf holds the scratch buffers of the stream inflate");
static_assert(sizeof(InfsShared) <= 20 * 1024, "at least 8 decoders resident per compute unit (160 KiB of LDS)");
static_assert(sizeof(InfwShared) <= 20 * 1024, "the windowed chain keeps that bound");

constexpr int INFS_WG_PER_CU = 16;

__global__ __launch_bounds__(INF_THREADS) void infs_scan_kernel(const uint8_t *__restrict__ d_comp, long long comp_len, long long chunk_bytes,
                                                                long long n_chunks, InfsRecord *rec) {
    __shared__ InfsShared X;
    INF_PHASE(inf_ph_tables(X.S, t))
    for (long long k = (long long)blockIdx.x; k < n_chunks; k += (long long)gridDim.x) infs_scan_chunk(X, d_comp, comp_len, chunk_bytes, k, rec + k);
}

__global__ __launch_bounds__(INF_THREADS) void infs_chain_kernel(const uint8_t *__restrict__ d_comp, long long comp_len, long long chunk_bytes,
                                                                 const InfsRecord *__restrict__ rec, long long n_chunks, InfsSegment *seg,
                                                                 long long seg_cap, InfsResult *res) {
    __shared__ InfsShared X;
    INF_PHASE(inf_ph_tables(X.S, t))
    infs_chain(X, d_comp, comp_len, chunk_bytes, rec, n_chunks, seg, seg_cap, res);
}

__global__ __launch_bounds__(INF_THREADS) void infs_decode_kernel(const uint8_t *__restrict__ d_comp, long long comp_len, InfsSegment *seg,
                                                                  long long n_seg, uint16_t *stage) {
    __shared__ InfsShared X;
    for (long long i = (long long)blockIdx.x; i < n_seg; i += (long long)gridDim.x) infs_decode_segment(X, d_comp, comp_len, seg + i, stage);
}

__global__ __launch_bounds__(INFS_TAIL_THREADS) void infs_tails_kernel(InfsSegment *seg, long long n_seg, const uint16_t *stage, uint8_t *out,
                                                                       const uint8_t *hist) {
    infs_tails(seg, n_seg, stage, out, hist);
}

__global__ __launch_bounds__(INF_THREADS) void infs_rest_kernel(InfsSegment *seg, long long n_seg, const uint16_t *stage, uint8_t *out,
                                                                const uint8_t *hist) {
    __shared__ InfsShared X;
    INF_PHASE(inf_ph_tables(X.S, t))
    for (long long i = (long long)blockIdx.x; i < n_seg; i += (long long)gridDim.x) infs_rest_segment(X, seg + i, stage, out, hist);
}

__global__ __launch_bounds__(INF_THREADS) void infs_verdict_kernel(const InfsSegment *seg, long long n_seg, InfsResult *res) {
    __shared__ InfsShared X;
    INF_PHASE(inf_ph_tables(X.S, t))
    INF_PHASE(infs_ph_verdict(X, seg, n_seg, res, t))
}

__global__ __launch_bounds__(INF_THREADS) void infw_scan_kernel(const uint8_t *__restrict__ d_comp, long long comp_len, long long chunk_bytes,
                                                                long long n_chunks, const InfwCarry *carry, InfsRecord *rec) {
    __shared__ InfsShared X;
    INF_PHASE(inf_ph_tables(X.S, t))
    for (long long k = (long long)blockIdx.x; k < n_chunks; k += (long long)gridDim.x)
        infw_scan_chunk(X, d_comp, comp_len, chunk_bytes, k, carry, rec + k);
}

__global__ __launch_bounds__(INF_THREADS) void infw_chain_kernel(const uint8_t *__restrict__ d_comp, long long comp_len, int last,
                                                                 long long chunk_bytes, const InfsRecord *__restrict__ rec, long long n_chunks,
                                                                 InfsSegment *seg, long long seg_cap, const InfwCarry *carry, InfwResult *res) {
    __shared__ InfwShared W;
    INF_PHASE(inf_ph_tables(W.X.S, t))
    infw_chain(W, d_comp, comp_len, last, chunk_bytes, rec, n_chunks, seg, seg_cap, carry, res);
}

__global__ __launch_bounds__(INF_THREADS) void infw_verdict_kernel(const InfsSegment *seg, long long n_seg, const uint8_t *out,
                                                                   unsigned long long total, InfwCarry *carry, InfwResult *res) {
    __shared__ InfsShared X;
    INF_PHASE(inf_ph_tables(X.S, t))
    infw_verdict(X, seg, n_seg, out, total, carry, res);
}

const char *infs_reason(uint32_t st) {
    static const char *const names[] = {"ok", "bad header", "bad block type", "bad stored lengths", "bad code set", "bad symbol",
                                        "distance too far", "output overrun", "output short", "input exhausted", "CRC mismatch",
                                        "ISIZE mismatch"};
    return st < sizeof names / sizeof names[0] ? names[st] : "a segment does not decode to what it counted to (internal)";
}

int32_t infs_refused(bdx_ctx *ctx, const InfsResult &r) {
    return bdx_fail(ctx, BDX_E_INVALID, "gzip member %u (near compressed byte %llu) is refused: %s (status %u)", r.member, (unsigned long long)r.at,
                    infs_reason(r.status), r.status);
}

}  // namespace

struct bdx_fq_inflate_window {
    bdx_ctx *ctx;
    int32_t chunk;
    int dead;
    uint32_t where;  // the host's copy of the carried position (all it needs of it)
    InfwCarry *d_carry;
    uint32_t cur = 0;  // which copy of the history the next call reads
};

extern "C" {

int32_t bdx_fq_inflate_stream_chunk(void) { return INFS_CHUNK_DEFAULT; }

int32_t bdx_fq_inflate_stream_device(bdx_ctx *ctx, const uint8_t *d_comp, int64_t comp_len, int32_t chunk_bytes, uint8_t *d_out, int64_t out_cap,
                                     int64_t *plain_len, int64_t *info) {
    if (comp_len < 0 || out_cap < 0) return bdx_fail(ctx, BDX_E_INVALID, "comp_len or out_cap negative");
    if (chunk_bytes != 0 && (chunk_bytes < INFS_CHUNK_MIN || chunk_bytes > INFS_CHUNK_MAX))
        return bdx_fail(ctx, BDX_E_INVALID, "chunk_bytes must be 0 (the default, %d) or %d .. %d, got %d", INFS_CHUNK_DEFAULT, INFS_CHUNK_MIN,
                        INFS_CHUNK_MAX, chunk_bytes);
    if (!plain_len) return bdx_fail(ctx, BDX_E_INVALID, "plain_len is NULL");
    if (!ctx) return bdx_fail(nullptr, BDX_E_INVALID, "ctx is NULL");
    if (comp_len > 0 && !d_comp) return bdx_fail(ctx, BDX_E_INVALID, "NULL device pointer (d_comp)");
    if (out_cap > 0 && !d_out) return bdx_fail(ctx, BDX_E_INVALID, "NULL device pointer (d_out)");
    if (info) std::fill(info, info + 8, (int64_t)0);
    *plain_len = 0;
    InfsResult res{};
    if (comp_len < 18) {  // (no room for a member: nothing to launch)
        res.status = INF_E_HEADER;
        return infs_refused(ctx, res);
    }
    const long long chunk = chunk_bytes ? chunk_bytes : INFS_CHUNK_DEFAULT;
    const long long n_chunks = (comp_len + chunk - 1) / chunk;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, ctx->inf[INFS_BUF_RECORDS].ensure((size_t)n_chunks * sizeof(InfsRecord)));
    HIP_TRY(ctx, ctx->inf[INFS_BUF_RESULT].ensure(sizeof(InfsResult)));
    InfsRecord *d_rec = (InfsRecord *)ctx->inf[INFS_BUF_RECORDS].p;
    InfsResult *d_res = (InfsResult *)ctx->inf[INFS_BUF_RESULT].p;
    const long long wide = (long long)std::max(1, ctx->n_cu) * INFS_WG_PER_CU;
    infs_scan_kernel<<<dim3((unsigned)std::min(n_chunks, wide)), dim3(INF_THREADS), 0, st>>>(d_comp, comp_len, chunk, n_chunks, d_rec);
    HIP_TRY(ctx, hipGetLastError());
    // the segment list: room for two per chunk; a file of very many members asks for more and the chain runs again
    long long seg_cap = 2 * n_chunks + 1024;
    for (int round = 0;; ++round) {
        HIP_TRY(ctx, ctx->inf[INFS_BUF_SEGMENTS].ensure((size_t)seg_cap * sizeof(InfsSegment)));
        infs_chain_kernel<<<dim3(1), dim3(INF_THREADS), 0, st>>>(d_comp, comp_len, chunk, d_rec, n_chunks, (InfsSegment *)ctx->inf[INFS_BUF_SEGMENTS].p,
                                                                  seg_cap, d_res);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (res.status != INF_OK) return infs_refused(ctx, res);
        if ((long long)res.n_seg <= seg_cap) break;
        if (round) return bdx_fail(ctx, BDX_E_STATE, "the segment list grew between two runs of the chain (internal)");
        seg_cap = (long long)res.n_seg;
    }
    *plain_len = (int64_t)res.total;
    if (info) std::copy(res.info, res.info + 8, info);
    if ((int64_t)res.total > out_cap)
        return bdx_fail(ctx, BDX_E_SPACE, "the file inflates to %llu bytes, d_out holds %lld", (unsigned long long)res.total, (long long)out_cap);
    const long long n_seg = (long long)res.n_seg;
    InfsSegment *d_seg = (InfsSegment *)ctx->inf[INFS_BUF_SEGMENTS].p;
    HIP_TRY(ctx, ctx->inf[INFS_BUF_STAGE].ensure((size_t)res.total * sizeof(uint16_t)));
    uint16_t *d_stage = (uint16_t *)ctx->inf[INFS_BUF_STAGE].p;
    const unsigned grid = (unsigned)std::min(n_seg, wide);
    infs_decode_kernel<<<dim3(grid), dim3(INF_THREADS), 0, st>>>(d_comp, comp_len, d_seg, n_seg, d_stage);
    HIP_TRY(ctx, hipGetLastError());
    infs_tails_kernel<<<dim3(1), dim3(INFS_TAIL_THREADS), 0, st>>>(d_seg, n_seg, d_stage, d_out, nullptr);
    HIP_TRY(ctx, hipGetLastError());
    infs_rest_kernel<<<dim3(grid), dim3(INF_THREADS), 0, st>>>(d_seg, n_seg, d_stage, d_out, nullptr);
    HIP_TRY(ctx, hipGetLastError());
    infs_verdict_kernel<<<dim3(1), dim3(INF_THREADS), 0, st>>>(d_seg, n_seg, d_res);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->inf[INFS_BUF_STAGE].release();  // (twice the plain text: not kept between calls)
    if (res.status != INF_OK) return infs_refused(ctx, res);
    return BDX_OK;
}

int32_t bdx_fq_inflate_window_open(bdx_ctx *ctx, int32_t chunk_bytes, bdx_fq_inflate_window **w) {
    if (!ctx) return bdx_fail(nullptr, BDX_E_INVALID, "ctx is NULL");
    if (!w) return bdx_fail(ctx, BDX_E_INVALID, "w is NULL");
    *w = nullptr;
    if (chunk_bytes != 0 && (chunk_bytes < INFS_CHUNK_MIN || chunk_bytes > INFS_CHUNK_MAX))
        return bdx_fail(ctx, BDX_E_INVALID, "chunk_bytes must be 0 (the default, %d) or %d .. %d, got %d", INFS_CHUNK_DEFAULT, INFS_CHUNK_MIN,
                        INFS_CHUNK_MAX, chunk_bytes);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void *p = nullptr;
    HIP_TRY(ctx, hipMalloc(&p, sizeof(InfwCarry)));
    // BETWEEN members, member 0, byte 0, an empty history; finished before open returns: the object may be fed on whatever
    // stream the context is given later (bdx_set_stream), which nothing orders behind this one
    hipError_t e = hipMemsetAsync(p, 0, sizeof(InfwCarry), ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return bdx_fail(ctx, BDX_E_DEVICE, "zeroing the carried state failed: %s", hipGetErrorString(e));
    }
    *w = new bdx_fq_inflate_window{ctx, chunk_bytes ? chunk_bytes : INFS_CHUNK_DEFAULT, 0, INFW_BETWEEN, (InfwCarry *)p};
    return BDX_OK;
}

int32_t bdx_fq_inflate_window_feed(bdx_fq_inflate_window *w, const uint8_t *d_comp, int64_t comp_len, int32_t last, uint8_t *d_out, int64_t out_cap,
                                   int64_t *consumed, int64_t *plain_len, int64_t *info) {
    if (!w) return bdx_fail(nullptr, BDX_E_INVALID, "w is NULL");
    bdx_ctx *ctx = w->ctx;
    if (comp_len < 0 || out_cap < 0) return bdx_fail(ctx, BDX_E_INVALID, "comp_len or out_cap negative");
    if (comp_len > INFW_MAX) return bdx_fail(ctx, BDX_E_INVALID, "a window holds at most %lld bytes, got %lld", INFW_MAX, (long long)comp_len);
    if (!consumed || !plain_len) return bdx_fail(ctx, BDX_E_INVALID, "consumed or plain_len is NULL");
    if (comp_len > 0 && !d_comp) return bdx_fail(ctx, BDX_E_INVALID, "NULL device pointer (d_comp)");
    if (out_cap > 0 && !d_out) return bdx_fail(ctx, BDX_E_INVALID, "NULL device pointer (d_out)");
    if (info) std::fill(info, info + 8, (int64_t)0);
    *consumed = *plain_len = 0;
    if (w->dead) return bdx_fail(ctx, BDX_E_STATE, "the window object has refused its file: no further feed");
    if (w->where == INFW_IGNORE) {  // trailing bytes
        *consumed = comp_len;
        return BDX_OK;
    }
    const long long chunk = w->chunk;
    const long long n_chunks = (comp_len + chunk - 1) / chunk;
    hipStream_t st = ctx->stream;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, ctx->inf[INFS_BUF_RECORDS].ensure((size_t)(n_chunks + 1) * sizeof(InfsRecord)));
    HIP_TRY(ctx, ctx->inf[INFS_BUF_RESULT].ensure(sizeof(InfwResult)));
    InfsRecord *d_rec = (InfsRecord *)ctx->inf[INFS_BUF_RECORDS].p;
    InfwResult *d_res = (InfwResult *)ctx->inf[INFS_BUF_RESULT].p;
    InfwResult res{};
    const long long wide = (long long)std::max(1, ctx->n_cu) * INFS_WG_PER_CU;
    if (n_chunks > 0) {
        infw_scan_kernel<<<dim3((unsigned)std::min(n_chunks, wide)), dim3(INF_THREADS), 0, st>>>(d_comp, comp_len, chunk, n_chunks, w->d_carry, d_rec);
        HIP_TRY(ctx, hipGetLastError());
    }
    long long seg_cap = 2 * n_chunks + 1024;
    for (int round = 0;; ++round) {
        HIP_TRY(ctx, ctx->inf[INFS_BUF_SEGMENTS].ensure((size_t)seg_cap * sizeof(InfsSegment)));
        infw_chain_kernel<<<dim3(1), dim3(INF_THREADS), 0, st>>>(d_comp, comp_len, last != 0, chunk, d_rec, n_chunks,
                                                                  (InfsSegment *)ctx->inf[INFS_BUF_SEGMENTS].p, seg_cap, w->d_carry, d_res);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        if (res.r.status != INF_OK) {
            w->dead = 1;
            return infs_refused(ctx, res.r);
        }
        if ((long long)res.r.n_seg <= seg_cap) break;
        if (round) return bdx_fail(ctx, BDX_E_STATE, "the segment list grew between two runs of the chain (internal)");
        seg_cap = (long long)res.r.n_seg;
    }
    *plain_len = (int64_t)res.r.total;
    if (info) std::copy(res.r.info, res.r.info + 8, info);
    if ((int64_t)res.r.total > out_cap)
        return bdx_fail(ctx, BDX_E_SPACE, "the window inflates to %llu bytes, d_out holds %lld", (unsigned long long)res.r.total, (long long)out_cap);
    if (last && res.where != INFW_IGNORE) return bdx_fail(ctx, BDX_E_STATE, "the last window did not end its file (internal)");
    const long long n_seg = (long long)res.r.n_seg;
    InfsSegment *d_seg = (InfsSegment *)ctx->inf[INFS_BUF_SEGMENTS].p;
    if (n_seg > 0) {
        HIP_TRY(ctx, ctx->inf[INFS_BUF_STAGE].ensure((size_t)res.r.total * sizeof(uint16_t)));
        uint16_t *d_stage = (uint16_t *)ctx->inf[INFS_BUF_STAGE].p;
        const uint8_t *d_hist = w->d_carry->hist[w->cur];
        const unsigned grid = (unsigned)std::min(n_seg, wide);
        infs_decode_kernel<<<dim3(grid), dim3(INF_THREADS), 0, st>>>(d_comp, comp_len, d_seg, n_seg, d_stage);
        HIP_TRY(ctx, hipGetLastError());
        infs_tails_kernel<<<dim3(1), dim3(INFS_TAIL_THREADS), 0, st>>>(d_seg, n_seg, d_stage, d_out, d_hist);
        HIP_TRY(ctx, hipGetLastError());
        infs_rest_kernel<<<dim3(grid), dim3(INF_THREADS), 0, st>>>(d_seg, n_seg, d_stage, d_out, d_hist);
        HIP_TRY(ctx, hipGetLastError());
    }
    infw_verdict_kernel<<<dim3(1), dim3(INF_THREADS), 0, st>>>(d_seg, n_seg, d_out, (unsigned long long)res.r.total, w->d_carry, d_res);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->inf[INFS_BUF_STAGE].release();  // (twice the window's text: not kept between calls)
    if (res.r.status != INF_OK) {
        w->dead = 1;
        return infs_refused(ctx, res.r);
    }
    w->where = res.where;
    w->cur ^= 1;
    *consumed = (int64_t)res.consumed;
    return BDX_OK;
}

int32_t bdx_fq_inflate_window_close(bdx_fq_inflate_window *w) {
    if (!w) return BDX_OK;
    bdx_ctx *ctx = w->ctx;
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = hipFree(w->d_carry);
    delete w;
    if (e != hipSuccess) return bdx_fail(ctx, BDX_E_DEVICE, "closing the window object failed: %s", hipGetErrorString(e));
    return BDX_OK;
}

}  // extern "C"
