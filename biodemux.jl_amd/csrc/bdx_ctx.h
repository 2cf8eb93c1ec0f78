// bdx_ctx.h — the context object behind the C-ABI (private; shared by bdx_abi.cpp, bdx_host.cpp and bdx_comm.cpp).
#pragma once
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "bdx_call.h"  // CallPlan, BdxSeedChoice; with it bdx_plan.h: BdxSetPlans, BdxPlanChoice and the planner's output (and bdx_internal.h)

#define BDX_FQ_SCRATCH 12  // scratch buffers of the device FASTQ pipeline (bdx_fastq.hip)
#define BDX_DFL_SCRATCH 4  // scratch buffers of the device DEFLATE encoder (bdx_deflate.hip)
#define BDX_INF_SCRATCH 6  // scratch buffers of the device inflate (bdx_inflate.hip: 2) and of the stream inflate (bdx_inflate_stream.hip: 4)

// An allocation that frees itself: move-only, so a block has one owner (the context, or a local that retires it).
template <hipError_t (*Free)(void *)>
struct OwnedBlock {
    void *p = nullptr;
    size_t cap = 0;
    OwnedBlock() = default;
    OwnedBlock(OwnedBlock &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    OwnedBlock &operator=(OwnedBlock &&o) noexcept {
        if (this != &o) {
            release();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    OwnedBlock(const OwnedBlock &) = delete;
    OwnedBlock &operator=(const OwnedBlock &) = delete;
    ~OwnedBlock() { release(); }
    void release() {
        if (p) (void)Free(p);
        p = nullptr;
        cap = 0;
    }
};

struct DevBuf : OwnedBlock<hipFree> {  // device memory
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap && p) return hipSuccess;
        release();
        size_t want = bytes < 256 ? 256 : bytes;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess)
            cap = want;
        else
            p = nullptr;
        return e;
    }
};

// Page-locked host twin of DevBuf: grows to `bytes` + `slack` (room for somewhat larger calls to come)
struct PinnedBuf : OwnedBlock<hipHostFree> {
    hipError_t ensure(size_t bytes, size_t slack) {
        if (bytes <= cap && p) return hipSuccess;
        release();
        hipError_t e = hipHostMalloc(&p, bytes + slack, hipHostMallocDefault);
        if (e == hipSuccess)
            cap = bytes + slack;
        else
            p = nullptr;
        return e;
    }
};

struct bdx_comm_state;  // bdx_comm.cpp

// One complete filter configuration of the fused kernel: sweep tables + seed tables + launch geometry.
// A context holds two: fs[0] filters at the config's full operation budgets; fs[1] — "tier 1" — at budgets
// capped so that single 8-base seeds stay selective (see bdx_plan.cpp, tiered budgets).  The plans come from the
// planner; bdx_create uploads its blobs into these buffers and binds the plans' pointers.
struct BdxFilterSet : BdxSetPlans {
    DevBuf bp_tables, seed_tables, seed_tables_alt, wave_tables, pair_tables;
};

struct bdx_ctx : BdxPlanChoice {  // (tiered, tier_q, tier_cap_fixed, pairs_tier, pair_mmin, band_roll_off, filter_used, path)
    bdx_config_t cfg{};
    BdxDevCfg dev{};
    BdxGenericPlan plan{};
    BdxFilterSet fs[2];
    BdxSeedChoice seed[2] = {BDX_SEED_MAIN, BDX_SEED_MAIN};  // per set: the seed plan in effect — the planning state that outlives a call
    CallPlan last;           // the last classify call's plan (bdx_launch_info reports from it)
    BdxTuning tune{};
    DevBuf d_maxlen;    // the scratch block: two BdxScratch halves (word 0: bdx_launch_maxlen's result)
    DevBuf d_tier;      // tiered budgets: reads handed from tier 1 to tier 0
    DevBuf d_carry;     // dual tiered known-class configs: the winning survivor of the pass tier 1 settled, per listed read (BdxWavePlan::d_carry)
    int user_len_hint = 0;  // 0 = measure every device batch
    int device = 0;
    int n_cu = 256;          // compute units of the device (hipDeviceAttributeMultiprocessorCount, read in bdx_create)
    int64_t wave_launches = 0;  // launches of the wave-autonomous kernel
    int64_t pair_launches = 0;  // launches of its pairs mode
    DevBuf d_dbg;            // [0] hand-over windows the exact kernel refused (not a window: defence in depth; must stay 0)
    DevBuf d_wlist;          // reads the wave kernel hands to the general kernel (plain configs; tiered ones use d_tier)
    hipStream_t own_stream = nullptr;
    hipStream_t copy_stream = nullptr;   // host entry point, large batches: chunk uploads beside the previous chunk's kernels
    hipEvent_t copy_events[8] = {};
    int64_t pipelined_calls = 0;
    int64_t staged_downloads = 0;  // large result downloads that went through the page-locked staging buffer (download_items)
    hipStream_t stream = nullptr;
    // device tables
    DevBuf bc_bytes[2], bc_off[2], bc_nn[2];
    DevBuf counts_own;
    unsigned long long *counts = nullptr;
    // staging for the host entry point
    DevBuf d_seq, d_off, d_out_i32, d_out_f64;
    // window upload (host entry point, long reads with short column windows): per-read true lengths / window starts
    DevBuf d_vlen, d_vlo;
    BdxScratchTurn turn;  // which half of the scratch block the next classify call uses, and which halves hold zeros
    // the half the next classify call uses (while it runs: this call's) / other: the half the last call used, which this call's last launch clears
    BdxScratch *scratch(bool other = false) const { return (BdxScratch *)d_maxlen.p + (other ? turn.other() : turn.mine()); }
    PinnedBuf h_stage;  // page-locked staging for the verdict vectors of small batches
    PinnedBuf h_in;     // page-locked staging for the bytes + offsets of small batches
    PinnedBuf h_back;   // page-locked staging for the result vectors of large batches handed over in pageable memory (download_items)
    hipEvent_t back_events[10] = {};
    bool back_events_made = false;
    int64_t window_uploads = 0;
    int64_t band_launches = 0;  // (pass, exact-kernel launch) pairs that ran with the diagonal-band DP enabled
    std::vector<uint8_t> h_win;    // host staging of the compacted windows
    std::vector<int64_t> h_coff;
    std::vector<int32_t> h_vlen, h_vlo;
    // candidate masks (filtered paths)
    DevBuf d_cand[2];
    DevBuf d_wins[2], d_wcnt[2];  // split mode: column windows for the exact kernel
    DevBuf d_exc;                 // known-score mode: reads handed over to the exact kernel
    // DemuxStats histograms (summary = true): [pass][pos | len | raw] int64 tables of st_rows (raw: st_raw_rows)
    // rows x n_barcodes, their all-reduced twins, and the overflow flag
    DevBuf st_tab[2][3], st_sum[2][3], st_flag;
    long long st_rows = 0, st_sum_rows = 0;
    int st_sum_len_rows = 0;  // height of the length table when the summed twins were last filled (its pitch follows from it)
    int st_raw_rows = 0, st_len_rows = 0;
    bool st_len_fixed = false;  // the length table has a height known from the config (else it grows with the reads)
    // multi-GPU: communicator + the reduced counter vector (bdx_comm.cpp)
    bdx_comm_state *comm = nullptr;
    DevBuf counts_sum;
    DevBuf fq[BDX_FQ_SCRATCH];  // scratch of the device FASTQ pipeline (bdx_fastq.hip)
    DevBuf dfl[BDX_DFL_SCRATCH];  // scratch of the device DEFLATE encoder (bdx_deflate.hip): chunk table, member sizes / offsets, tokens, slots
    DevBuf inf[BDX_INF_SCRATCH];  // scratch of the device inflate (bdx_inflate.hip): member table, member status; of the stream inflate
                                  // (bdx_inflate_stream.hip): chunk records, segment list, result, the 16-bit staging image
    std::string err;
    std::string launch_log;      // the classify kernels the last classify call enqueued (bdx_last_launches; a host call: all of its device calls)
    int64_t launches = 0;
    int64_t last_blocks = 0;
};

// One batch on the device with what its caller knows of it: the value behind bdx_classify_device (which knows nothing) and
// bdx_classify_host (bdx_host.cpp), whose facts hold for this call only.
struct BdxBatchIn {
    const uint8_t *d_seq = nullptr;
    const int64_t *d_off = nullptr;
    int64_t n_reads = 0;
    bdx_outputs_t out{};
    int known_maxlen = 0;  // the batch's longest read, clamped to [1, 2^30] (0: not known) — of the true reads when vlen is set
    // window upload: d_seq / d_off hold only each read's window; per read its true length and its window's first position
    // (BdxDevCfg::vlen / vlo of the call's launches).  Null: whole reads.
    const int32_t *vlen = nullptr, *vlo = nullptr;
    bool scratch_cleared = false;  // the copy kernel that brought the batch up already zeroed this call's scratch half
    bool append_log = false;       // the call continues the launch log of a host call
};
// arguments checked by the callers (n_reads > 0, no null pointer, device selected)
int bdx_classify_batch(bdx_ctx *ctx, const BdxBatchIn &in);

// records the message on ctx (or as the create error when ctx is NULL) and returns `code`
int bdx_fail(bdx_ctx *ctx, int code, const char *fmt, ...);
void bdx_comm_release(bdx_ctx *ctx);  // bdx_comm.cpp: frees ctx->comm (called by bdx_destroy)
// histogram tables: grow (append zero rows) to at least `rows` rows; synchronises the stream when it grows
int bdx_stats_reserve(bdx_ctx *ctx, long long rows, bool exact = false);  // exact: the height the ranks agreed on
// logical size of a table as bdx_get_stats hands it out: [keys][barcodes]
inline size_t bdx_stats_words(const bdx_ctx *ctx, int pass, int which, long long rows) {
    return (size_t)(which == 2 ? ctx->st_raw_rows : which == 1 ? ctx->st_len_rows : rows) * (size_t)ctx->dev.pass[pass].n_barcodes;
}
inline int bdx_stats_stride(const bdx_ctx *ctx, int which) {  // key stride of the transposed tables (len, raw)
    return ((which == 2 ? ctx->st_raw_rows : ctx->st_len_rows) + 15) & ~15;
}
// words a table occupies on the device (pos: [rows][barcodes]; len, raw: [barcode][key stride])
inline size_t bdx_stats_phys_words(const bdx_ctx *ctx, int pass, int which, long long rows) {
    if (which == 0) return (size_t)rows * (size_t)ctx->dev.pass[pass].n_barcodes;
    return (size_t)bdx_stats_stride(ctx, which) * (size_t)ctx->dev.pass[pass].n_barcodes;
}

#define HIP_TRY(ctx, call)                                                                      \
    do {                                                                                        \
        hipError_t e__ = (call);                                                                \
        if (e__ != hipSuccess)                                                                  \
            return bdx_fail(ctx, BDX_E_DEVICE, "%s failed: %s", #call, hipGetErrorString(e__)); \
    } while (0)
