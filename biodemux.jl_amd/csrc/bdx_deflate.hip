// bdx_deflate.hip — gzip output of the device FASTQ pipeline compressed on the device: the per-class blocks of
// bdx_fq_gather_device become chains of size-tagged gzip members (the layout of deflate_gz_members, bdx_io.cpp) that the
// host only appends (bdx_fq_write_blocks_raw).  The encoder itself is bdx_deflate_core.h (level 1) and
// bdx_deflate2_core.h (level 2: the same member, better matches, a run-length coded header); this file holds the
// kernels and the C-ABI entries.
//
//   dfl_encode_kernel   one workgroup of 256 threads per chunk of at most DFL_CHUNK bytes, a persistent grid of four
//                       workgroups per compute unit (41 KiB of LDS each); every chunk becomes one member in a slot of its own
//   dfl2_encode_kernel  the same for level 2: three workgroups per compute unit (42 KiB of LDS each)
//   dfl_scan_kernel     exclusive scan of the member sizes: where every member goes in the output
//   dfl_compact_kernel  copies the members there: each class's members contiguous, classes in order
#include <algorithm>
#include <vector>

#include "bdx_ctx.h"
#include "bdx_deflate2_core.h"

namespace {

struct DflChunk {
    long long in_off;    // first byte of the chunk in d_in
    long long slot_off;  // its slot in the slot buffer (64-byte aligned, n + 33 bytes rounded up)
    int n;
    int cls;
};

enum { DFL_BUF_CHUNKS = 0, DFL_BUF_SIZES, DFL_BUF_TOKENS, DFL_BUF_SLOTS, DFL_NBUF };
static_assert(DFL_NBUF <= BDX_DFL_SCRATCH, "bdx_ctx::dfl holds the scratch buffers of the device DEFLATE encoder");
static_assert(DFL_CHUNK >= 4096 && DFL_CHUNK <= 65535, "a chunk is one stored block at worst and positions fit 16 bits");

constexpr int DFL_WG_PER_CU = 4;
constexpr int DFL2_WG_PER_CU = 3;
constexpr int DFL_LEVELS = 2;
constexpr long long DFL_MAX_CHUNKS = 1ll << 26;
static_assert(sizeof(DflShared) * DFL_WG_PER_CU <= 160 * 1024 && sizeof(Dfl2Shared) * DFL2_WG_PER_CU <= 160 * 1024 &&
                  sizeof(Dfl2Shared) * (DFL2_WG_PER_CU + 1) > 160 * 1024,
              "the persistent grids are what the 160 KiB of LDS of a compute unit hold");

// (four waves per SIMD = four workgroups per CU: 128 VGPRs, what the 41 KiB of LDS allow as well)
__global__ __launch_bounds__(DFL_THREADS, DFL_WG_PER_CU) void dfl_encode_kernel(const uint8_t *__restrict__ d_in,
                                                                                const DflChunk *__restrict__ chunks, int nch,
                                                                                uint32_t *__restrict__ tokens,
                                                                                uint8_t *__restrict__ slots,
                                                                                uint32_t *__restrict__ msize) {
    __shared__ DflShared S;
    DFL_PHASE(dfl_ph_tables(S, t))
    uint32_t *tok = tokens + (size_t)blockIdx.x * DFL_CHUNK;
    for (int c = (int)blockIdx.x; c < nch; c += (int)gridDim.x) {
        const DflChunk ch = chunks[c];
        dfl_encode_chunk(S, d_in + ch.in_off, ch.n, tok, slots + ch.slot_off, msize + c);
    }
}

// (three waves per SIMD = three workgroups per CU, what the 42 KiB of LDS allow: 168 VGPRs)
__global__ __launch_bounds__(DFL_THREADS, DFL2_WG_PER_CU) void dfl2_encode_kernel(const uint8_t *__restrict__ d_in,
                                                                                  const DflChunk *__restrict__ chunks, int nch,
                                                                                  uint32_t *__restrict__ tokens,
                                                                                  uint8_t *__restrict__ slots,
                                                                                  uint32_t *__restrict__ msize) {
    __shared__ Dfl2Shared S;
    DFL_PHASE(dfl_ph_tables(S.B, t))
    uint32_t *tok = tokens + (size_t)blockIdx.x * DFL_CHUNK;
    for (int c = (int)blockIdx.x; c < nch; c += (int)gridDim.x) {
        const DflChunk ch = chunks[c];
        dfl2_encode_chunk(S, d_in + ch.in_off, ch.n, tok, slots + ch.slot_off, msize + c);
    }
}

// off[i] = msize[0] + .. + msize[i - 1], i = 0 .. nch (one workgroup; every thread sums a run of its own first)
__global__ __launch_bounds__(DFL_THREADS) void dfl_scan_kernel(const uint32_t *__restrict__ msize, int nch, long long *__restrict__ off) {
    __shared__ long long part[DFL_THREADS];
    const int t = (int)threadIdx.x;
    const int per = (nch + DFL_THREADS - 1) / DFL_THREADS;
    const int a = std::min(t * per, nch), b = std::min(a + per, nch);
    long long s = 0;
    for (int i = a; i < b; ++i) s += msize[i];
    part[t] = s;
    __syncthreads();
    long long before = 0;
    for (int j = 0; j < t; ++j) before += part[j];
    for (int i = a; i < b; ++i) {
        off[i] = before;
        before += msize[i];
    }
    if (t == DFL_THREADS - 1) off[nch] = before;
}

__global__ __launch_bounds__(DFL_THREADS) void dfl_compact_kernel(const DflChunk *__restrict__ chunks, const uint32_t *__restrict__ msize,
                                                                  const long long *__restrict__ off, const uint8_t *__restrict__ slots,
                                                                  uint8_t *__restrict__ d_out) {
    const int c = (int)blockIdx.x;
    const uint8_t *src = slots + chunks[c].slot_off;
    uint8_t *dst = d_out + off[c];
    const uint32_t n = msize[c];
    for (uint32_t i = threadIdx.x; i < n; i += DFL_THREADS) dst[i] = src[i];
}

int64_t chunks_of(int64_t len) { return (len + DFL_CHUNK - 1) / DFL_CHUNK; }

}  // namespace

extern "C" {

int32_t bdx_fq_deflate_chunk(void) { return DFL_CHUNK; }

int64_t bdx_fq_deflate_bound(const int64_t *class_bytes, int32_t n_classes) {
    if (n_classes < 0 || (n_classes > 0 && !class_bytes)) return BDX_E_INVALID;
    int64_t bound = 0;
    for (int32_t c = 0; c < n_classes; ++c) {
        const int64_t len = class_bytes[c];
        if (len < 0 || len > ((int64_t)1 << 46)) return BDX_E_INVALID;
        bound += len + (DFL_MEMBER_OVERHEAD + DFL_STORED_OVERHEAD) * chunks_of(len);
    }
    return bound;
}

int32_t bdx_fq_deflate_levels(void) { return DFL_LEVELS; }

int32_t bdx_fq_deflate_level_device(bdx_ctx *ctx, int32_t level, const uint8_t *d_in, const int64_t *class_bytes, int32_t n_classes,
                                    uint8_t *d_out, int64_t out_cap, int64_t *class_cbytes) {
    if (level < 1 || level > DFL_LEVELS) {  // (before anything else: refused without a context as well)
        if (class_cbytes && n_classes > 0) std::fill(class_cbytes, class_cbytes + n_classes, (int64_t)0);
        return bdx_fail(ctx, BDX_E_INVALID, "deflate level %d: the levels are 1 .. %d (bdx_fq_deflate_levels)", (int)level, DFL_LEVELS);
    }
    if (!ctx) return BDX_E_INVALID;
    if (n_classes < 0 || !class_bytes || !class_cbytes) return bdx_fail(ctx, BDX_E_INVALID, "class_bytes / class_cbytes is NULL or n_classes negative");
    std::fill(class_cbytes, class_cbytes + n_classes, (int64_t)0);
    const int64_t bound = bdx_fq_deflate_bound(class_bytes, n_classes);
    if (bound < 0) return bdx_fail(ctx, BDX_E_INVALID, "a class block has a negative (or absurd) size");
    if (out_cap < bound)
        return bdx_fail(ctx, BDX_E_INVALID, "the members may need %lld bytes (bdx_fq_deflate_bound), d_out holds %lld", (long long)bound,
                        (long long)out_cap);
    if (bound == 0) return BDX_OK;
    if (!d_in || !d_out) return bdx_fail(ctx, BDX_E_INVALID, "NULL device pointer");
    std::vector<DflChunk> chunks;
    std::vector<int64_t> first((size_t)n_classes + 1, 0);  // class c's chunks: [first[c], first[c + 1])
    long long in_off = 0, slot_off = 0;
    for (int32_t c = 0; c < n_classes; ++c) {
        first[(size_t)c] = (int64_t)chunks.size();
        if ((long long)chunks.size() + chunks_of(class_bytes[c]) > DFL_MAX_CHUNKS)
            return bdx_fail(ctx, BDX_E_INVALID, "more than 2^26 chunks in one call");
        for (int64_t o = 0; o < class_bytes[c]; o += DFL_CHUNK) {
            const int n = (int)std::min<int64_t>(DFL_CHUNK, class_bytes[c] - o);
            chunks.push_back(DflChunk{in_off + o, slot_off, n, c});
            slot_off += (n + DFL_MEMBER_OVERHEAD + DFL_STORED_OVERHEAD + 63) & ~63ll;
        }
        in_off += class_bytes[c];
    }
    const int nch = (int)chunks.size();
    first[(size_t)n_classes] = nch;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int grid = std::min(nch, std::max(1, ctx->n_cu) * (level == 1 ? DFL_WG_PER_CU : DFL2_WG_PER_CU));
    const size_t off_at = ((size_t)nch * 4 + 7) & ~(size_t)7;  // sizes buffer: uint32 msize[nch], then int64 off[nch + 1]
    HIP_TRY(ctx, ctx->dfl[DFL_BUF_CHUNKS].ensure((size_t)nch * sizeof(DflChunk)));
    HIP_TRY(ctx, ctx->dfl[DFL_BUF_SIZES].ensure(off_at + ((size_t)nch + 1) * 8));
    HIP_TRY(ctx, ctx->dfl[DFL_BUF_TOKENS].ensure((size_t)grid * DFL_CHUNK * 4));
    HIP_TRY(ctx, ctx->dfl[DFL_BUF_SLOTS].ensure((size_t)slot_off));
    DflChunk *d_chunks = (DflChunk *)ctx->dfl[DFL_BUF_CHUNKS].p;
    uint32_t *msize = (uint32_t *)ctx->dfl[DFL_BUF_SIZES].p;
    long long *off = (long long *)((uint8_t *)ctx->dfl[DFL_BUF_SIZES].p + off_at);
    HIP_TRY(ctx, hipMemcpyAsync(d_chunks, chunks.data(), (size_t)nch * sizeof(DflChunk), hipMemcpyHostToDevice, ctx->stream));
    if (level == 1)
        dfl_encode_kernel<<<dim3((unsigned)grid), dim3(DFL_THREADS), 0, ctx->stream>>>(d_in, d_chunks, nch, (uint32_t *)ctx->dfl[DFL_BUF_TOKENS].p,
                                                                                       (uint8_t *)ctx->dfl[DFL_BUF_SLOTS].p, msize);
    else
        dfl2_encode_kernel<<<dim3((unsigned)grid), dim3(DFL_THREADS), 0, ctx->stream>>>(d_in, d_chunks, nch, (uint32_t *)ctx->dfl[DFL_BUF_TOKENS].p,
                                                                                        (uint8_t *)ctx->dfl[DFL_BUF_SLOTS].p, msize);
    dfl_scan_kernel<<<dim3(1), dim3(DFL_THREADS), 0, ctx->stream>>>(msize, nch, off);
    dfl_compact_kernel<<<dim3((unsigned)nch), dim3(DFL_THREADS), 0, ctx->stream>>>(d_chunks, msize, off, (const uint8_t *)ctx->dfl[DFL_BUF_SLOTS].p,
                                                                                    d_out);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<long long> h_off((size_t)nch + 1);
    HIP_TRY(ctx, hipMemcpyAsync(h_off.data(), off, ((size_t)nch + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int32_t c = 0; c < n_classes; ++c) class_cbytes[c] = h_off[(size_t)first[(size_t)c + 1]] - h_off[(size_t)first[(size_t)c]];
    return BDX_OK;
}

int32_t bdx_fq_deflate_device(bdx_ctx *ctx, const uint8_t *d_in, const int64_t *class_bytes, int32_t n_classes, uint8_t *d_out,
                              int64_t out_cap, int64_t *class_cbytes) {
    return bdx_fq_deflate_level_device(ctx, 1, d_in, class_bytes, n_classes, d_out, out_cap, class_cbytes);
}

}  // extern "C"
