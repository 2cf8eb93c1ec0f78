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
#include <algorithm>

#include "bdx_ctx.h"
#include "bdx_inflate_stream_core.h"

namespace {

// bdx_ctx::inf[] behind the two buffers of bdx_inflate.hip
enum { INFS_BUF_RECORDS = 2, INFS_BUF_SEGMENTS, INFS_BUF_RESULT, INFS_BUF_STAGE, INFS_NBUF };
static_assert(INFS_NBUF <= BDX_INF_SCRATCH, "bdx_ctx::inf holds the scratch buffers of the stream inflate");
static_assert(sizeof(InfsShared) <= 20 * 1024, "at least 8 decoders resident per compute unit (160 KiB of LDS)");

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

__global__ __launch_bounds__(INFS_TAIL_THREADS) void infs_tails_kernel(InfsSegment *seg, long long n_seg, const uint16_t *stage, uint8_t *out) {
    infs_tails(seg, n_seg, stage, out);
}

__global__ __launch_bounds__(INF_THREADS) void infs_rest_kernel(InfsSegment *seg, long long n_seg, const uint16_t *stage, uint8_t *out) {
    __shared__ InfsShared X;
    INF_PHASE(inf_ph_tables(X.S, t))
    for (long long i = (long long)blockIdx.x; i < n_seg; i += (long long)gridDim.x) infs_rest_segment(X, seg + i, stage, out);
}

__global__ __launch_bounds__(INF_THREADS) void infs_verdict_kernel(const InfsSegment *seg, long long n_seg, InfsResult *res) {
    __shared__ InfsShared X;
    INF_PHASE(inf_ph_tables(X.S, t))
    INF_PHASE(infs_ph_verdict(X, seg, n_seg, res, t))
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
    infs_tails_kernel<<<dim3(1), dim3(INFS_TAIL_THREADS), 0, st>>>(d_seg, n_seg, d_stage, d_out);
    HIP_TRY(ctx, hipGetLastError());
    infs_rest_kernel<<<dim3(grid), dim3(INF_THREADS), 0, st>>>(d_seg, n_seg, d_stage, d_out);
    HIP_TRY(ctx, hipGetLastError());
    infs_verdict_kernel<<<dim3(1), dim3(INF_THREADS), 0, st>>>(d_seg, n_seg, d_res);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    ctx->inf[INFS_BUF_STAGE].release();  // (twice the plain text: not kept between calls)
    if (res.status != INF_OK) return infs_refused(ctx, res);
    return BDX_OK;
}

}  // extern "C"
