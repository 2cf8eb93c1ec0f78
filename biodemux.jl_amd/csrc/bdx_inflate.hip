// bdx_inflate.hip — .gz input of the device FASTQ pipeline inflated on the device: a batch's size-tagged gzip members
// (BGZF, or this library's own 'D','X' output) are uploaded compressed and every member is decoded into its place in
// the text window that bdx_fq_index_device takes; its CRC-32 and ISIZE are checked here as well.  The decoder itself is
// bdx_inflate_core.h; this file holds the kernel and the C-ABI entries.
//
//   inf_decode_kernel   one member per workgroup of 64 threads (one wavefront), a persistent grid of INF_WG_PER_CU
//                       workgroups per compute unit (6 KiB of LDS each: the 32 KiB window of a member is its own output
//                       in global memory / L2, not LDS)
#include <algorithm>
#include <vector>

#include "bdx_ctx.h"
#include "bdx_inflate_core.h"

namespace {

struct InfMember {
    long long comp_off;   // the member in d_comp
    long long plain_off;  // its slot in d_out
    int comp_len;
    int plain_len;
};

enum { INF_BUF_MEMBERS = 0, INF_BUF_STATUS, INF_NBUF };
static_assert(INF_NBUF <= BDX_INF_SCRATCH, "bdx_ctx::inf holds the scratch buffers of the device inflate");
static_assert(sizeof(InfShared) <= 20 * 1024, "at least 8 decoders resident per compute unit (160 KiB of LDS)");

constexpr int INF_WG_PER_CU = 16;  // four waves per SIMD

__global__ __launch_bounds__(INF_THREADS) void inf_decode_kernel(const uint8_t *__restrict__ d_comp, const InfMember *__restrict__ members,
                                                                 int n, uint8_t *d_out, int32_t *__restrict__ status) {
    __shared__ InfShared S;
    INF_PHASE(inf_ph_tables(S, t))
    for (int m = (int)blockIdx.x; m < n; m += (int)gridDim.x) {
        const InfMember mb = members[m];
        inf_decode_member(S, d_comp + mb.comp_off, mb.comp_len, d_out + mb.plain_off, mb.plain_len, status + m);
    }
}

const char *inf_reason(int32_t st) {
    static const char *const names[] = {"ok", "bad header", "bad block type", "bad stored lengths", "bad code set", "bad symbol",
                                        "distance too far", "output overrun", "output short", "input exhausted", "CRC mismatch",
                                        "ISIZE mismatch"};
    return st >= 0 && st < (int32_t)(sizeof names / sizeof names[0]) ? names[st] : "unknown status";
}

}  // namespace

extern "C" {

int32_t bdx_fq_inflate_member_max(void) { return INF_MEMBER_MAX; }

int32_t bdx_fq_inflate_device(bdx_ctx *ctx, const uint8_t *d_comp, const int64_t *comp_off, const int32_t *comp_len,
                              const int64_t *plain_off, const int32_t *plain_len, int32_t n_members, uint8_t *d_out, int64_t out_cap,
                              int32_t *status) {
    // the tables first: nothing is launched (and no context is needed to say so) when they are wrong
    if (n_members < 0 || out_cap < 0) return bdx_fail(ctx, BDX_E_INVALID, "n_members or out_cap negative");
    if (n_members > 0 && (!comp_off || !comp_len || !plain_off || !plain_len)) return bdx_fail(ctx, BDX_E_INVALID, "a member table is NULL");
    for (int32_t m = 0; m < n_members; ++m) {
        if (comp_off[m] < 0 || comp_len[m] < 0 || plain_off[m] < 0 || plain_len[m] < 0)
            return bdx_fail(ctx, BDX_E_INVALID, "member %d: a negative offset or length", m);
        if (plain_len[m] > INF_MEMBER_MAX)
            return bdx_fail(ctx, BDX_E_INVALID, "member %d: %d plain bytes, the device decoder takes %d at most (bdx_fq_inflate_member_max)", m,
                            plain_len[m], INF_MEMBER_MAX);
        if (plain_off[m] > out_cap - plain_len[m])
            return bdx_fail(ctx, BDX_E_INVALID, "member %d: its slot [%lld, +%d) is not inside d_out (%lld bytes)", m, (long long)plain_off[m],
                            plain_len[m], (long long)out_cap);
    }
    if (!ctx) return bdx_fail(nullptr, BDX_E_INVALID, "ctx is NULL");
    if (n_members == 0) return BDX_OK;
    if (!d_comp || !d_out) return bdx_fail(ctx, BDX_E_INVALID, "NULL device pointer");
    std::vector<InfMember> members((size_t)n_members);
    for (int32_t m = 0; m < n_members; ++m) members[(size_t)m] = InfMember{comp_off[m], plain_off[m], comp_len[m], plain_len[m]};
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, ctx->inf[INF_BUF_MEMBERS].ensure((size_t)n_members * sizeof(InfMember)));
    HIP_TRY(ctx, ctx->inf[INF_BUF_STATUS].ensure((size_t)n_members * sizeof(int32_t)));
    InfMember *d_members = (InfMember *)ctx->inf[INF_BUF_MEMBERS].p;
    int32_t *d_status = (int32_t *)ctx->inf[INF_BUF_STATUS].p;
    HIP_TRY(ctx, hipMemcpyAsync(d_members, members.data(), (size_t)n_members * sizeof(InfMember), hipMemcpyHostToDevice, ctx->stream));
    const int grid = std::min(n_members, std::max(1, ctx->n_cu) * INF_WG_PER_CU);
    inf_decode_kernel<<<dim3((unsigned)grid), dim3(INF_THREADS), 0, ctx->stream>>>(d_comp, d_members, n_members, d_out, d_status);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<int32_t> own;
    if (!status) {
        own.resize((size_t)n_members);
        status = own.data();
    }
    HIP_TRY(ctx, hipMemcpyAsync(status, d_status, (size_t)n_members * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int32_t m = 0; m < n_members; ++m)
        if (status[m] != INF_OK)
            return bdx_fail(ctx, BDX_E_INVALID, "member %d is refused: %s (status %d)", m, inf_reason(status[m]), status[m]);
    return BDX_OK;
}

}  // extern "C"
