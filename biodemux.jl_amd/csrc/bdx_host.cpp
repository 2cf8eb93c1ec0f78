// bdx_host.cpp — the host entry point of libbiodemux_hip.so (bdx_classify_host, bdx_host_alloc / bdx_host_free): what
// lies between a caller's host buffers and bdx_classify_device — the upload of the reads (small batches through one
// page-locked staging copy, large ones in chunks beside the kernels, long reads as their column windows only) and the
// download of the result vectors.  Host threads come from the one worker pool of bdx_pool.h.
#include <array>
#include <cstring>
#include <thread>

#include "bdx_ctx.h"
#include "bdx_pool.h"

namespace {

// ---- the device outputs of a host call ----------------------------------------------------------------------------
// d_out_i32 holds bc1 | bc2 | keep_start | keep_end (n each), then pass_start | pass_end | pass_raw | pass_bc (2n each);
// d_out_f64 pass_score | pass_delta (2n each).  The small path's mapped h_stage holds the first four only (the caller
// wants no other).  `r0`: the slots of reads r0.. (a chunk of the pipelined upload).  bc1 is always handed to the
// kernels, whether or not the caller wants it back.
bdx_outputs_t out_slots(const bdx_outputs_t &want, int32_t *i32, double *f64, size_t n, size_t r0 = 0) {
    bdx_outputs_t d{};
    d.bc1 = i32 + r0;
    d.bc2 = want.bc2 ? i32 + n + r0 : nullptr;
    d.keep_start = want.keep_start ? i32 + 2 * n + r0 : nullptr;
    d.keep_end = want.keep_end ? i32 + 3 * n + r0 : nullptr;
    d.pass_start = want.pass_start ? i32 + 4 * n + 2 * r0 : nullptr;
    d.pass_end = want.pass_end ? i32 + 6 * n + 2 * r0 : nullptr;
    d.pass_raw = want.pass_raw ? i32 + 8 * n + 2 * r0 : nullptr;
    d.pass_bc = want.pass_bc ? i32 + 10 * n + 2 * r0 : nullptr;
    d.pass_score = want.pass_score ? f64 + 2 * r0 : nullptr;
    d.pass_delta = want.pass_delta ? f64 + 2 * n + 2 * r0 : nullptr;
    return d;
}

// ---- host entry point: result vectors back to the caller -------------------------------------------------------------
// A device-to-host copy into PAGEABLE memory is staged by the runtime and, when the caller's arrays are fresh (the usual
// case: a result vector allocated per call), page-faulted in by that one copying thread: 13 of the 40 ms of a 10 M-read
// call.  Large downloads into pageable memory therefore go through a page-locked staging buffer of the context's own —
// one asynchronous DMA per vector at PCIe speed — and a few host threads copy each vector out (and fault the caller's
// pages in, in parallel) while the next one is still in flight.  Page-locked destinations (bdx_host_alloc) and small
// downloads keep the direct copies.  (Measured and dropped: populating the caller's pages with MADV_POPULATE_WRITE from a few
// threads while the reads go up — it slows the runtime's pageable upload down by more than the download gains: 293 -> 251 M reads/s.)
struct BackItem {
    void *h;
    const void *d;
    size_t bytes;
};
using BackItems = std::array<BackItem, 10>;

// every output the caller wants, from its slot `d` (out_slots of the whole batch)
BackItems back_items(const bdx_outputs_t &out, const bdx_outputs_t &d, size_t n) {
    return {{{out.bc1, d.bc1, n * 4},
             {out.bc2, d.bc2, n * 4},
             {out.keep_start, d.keep_start, n * 4},
             {out.keep_end, d.keep_end, n * 4},
             {out.pass_start, d.pass_start, n * 8},
             {out.pass_end, d.pass_end, n * 8},
             {out.pass_raw, d.pass_raw, n * 8},
             {out.pass_bc, d.pass_bc, n * 8},
             {out.pass_score, d.pass_score, n * 16},
             {out.pass_delta, d.pass_delta, n * 16}}};
}

bool host_is_page_locked(const void *p) {
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof(a));
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // (an unregistered pointer is an error for older runtimes: not sticky)
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

int enqueue_and_copy_out(bdx_ctx *ctx, const BackItems &items) {
    size_t total = 0;
    const void *first = nullptr;
    for (const BackItem &it : items)
        if (it.h && it.d && it.bytes) {
            total += (it.bytes + 255) & ~(size_t)255;
            if (!first) first = it.h;
        }
    bool staged = total >= ((size_t)16 << 20) && !ctx->tune.no_staged_download && first && !host_is_page_locked(first);
    if (staged && ctx->h_back.ensure(total, total >> 3) != hipSuccess) {
        (void)hipGetLastError();  // (page-locked memory is a limited resource: fall back to the direct copies)
        staged = false;
    }
    if (!staged) {
        for (const BackItem &it : items)
            if (it.h && it.d && it.bytes) HIP_TRY(ctx, hipMemcpyAsync(it.h, it.d, it.bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        return BDX_OK;
    }
    if (!ctx->back_events_made) {
        for (hipEvent_t &e : ctx->back_events) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->back_events_made = true;
    }
    size_t offs[10];
    size_t off = 0;
    for (int k = 0; k < 10; ++k) {
        offs[k] = off;
        if (!(items[k].h && items[k].d && items[k].bytes)) continue;
        HIP_TRY(ctx, hipMemcpyAsync((char *)ctx->h_back.p + off, items[k].d, items[k].bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(ctx->back_events[k], ctx->stream));
        off += (items[k].bytes + 255) & ~(size_t)255;
    }
    // every vector is cut into T page-aligned slices, copied out by the pool as soon as its DMA is done
    int T = (int)std::thread::hardware_concurrency();
    T = T < 1 ? 1 : (T > 8 ? 8 : T);
    for (int k = 0; k < 10; ++k) {
        if (!(items[k].h && items[k].d && items[k].bytes)) continue;
        HIP_TRY(ctx, hipEventSynchronize(ctx->back_events[k]));
        const size_t per = ((items[k].bytes + (size_t)T - 1) / (size_t)T + 4095) & ~(size_t)4095;
        parallel_for(T, [&](const int sl) {
            const size_t a = per * (size_t)sl, b = a + per < items[k].bytes ? a + per : items[k].bytes;
            if (a < b) memcpy((char *)items[k].h + a, (const char *)ctx->h_back.p + offs[k] + a, b - a);
        });
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->staged_downloads += 1;
    return BDX_OK;
}

// (every return waits for the stream: copies already enqueued may still be writing into h_back and the caller's arrays)
int download_items(bdx_ctx *ctx, const BackItems &items) {
    const int rc = enqueue_and_copy_out(ctx, items);
    if (rc != BDX_OK) (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

// ---- host entry point: shared tail (device outputs, launch, download) and the window upload ----------
// in: the batch on the device and what the host has seen of it; its outputs are set here
int run_and_download(bdx_ctx *ctx, BdxBatchIn in, const bdx_outputs_t *out, const bool mapped_outputs = false) {
    const size_t n = (size_t)in.n_reads;
    // Small batches (the reference hands over chunks of 4000 reads, core.jl:5-10) that want the four verdict vectors
    // only: they come back through h_stage, side by side
    const bool verdicts_only = n <= (size_t)(256 * 1024) && !out->pass_start && !out->pass_end && !out->pass_raw &&
                               !out->pass_bc && !out->pass_score && !out->pass_delta;
    if (verdicts_only) HIP_TRY(ctx, ctx->h_stage.ensure(n * 16, 4096));
    const bool mapped = mapped_outputs && verdicts_only;
    int32_t *i32;
    double *f64 = nullptr;
    if (mapped) {
        // the kernels write the four verdict vectors straight into page-locked host memory (posted writes over PCIe,
        // 16 bytes per read) — no device-to-host copy call at all
        void *hs_dev = nullptr;
        HIP_TRY(ctx, hipHostGetDevicePointer(&hs_dev, ctx->h_stage.p, 0));
        i32 = (int32_t *)hs_dev;
    } else {
        HIP_TRY(ctx, ctx->d_out_i32.ensure(n * 4 * 12));
        HIP_TRY(ctx, ctx->d_out_f64.ensure(n * 8 * 4));
        if (ctx->tune.poison) {  // test switch: an output element no kernel writes comes back as garbage, never as a stale right answer
            HIP_TRY(ctx, hipMemsetAsync(ctx->d_out_i32.p, 0xA5, n * 4 * 12, ctx->stream));
            HIP_TRY(ctx, hipMemsetAsync(ctx->d_out_f64.p, 0xA5, n * 8 * 4, ctx->stream));
        }
        i32 = (int32_t *)ctx->d_out_i32.p;
        f64 = (double *)ctx->d_out_f64.p;
    }
    const bdx_outputs_t d = in.out = out_slots(*out, i32, f64, n);
    const int rc = bdx_classify_batch(ctx, in);
    if (rc != BDX_OK) return rc;
    if (!verdicts_only) return download_items(ctx, back_items(*out, d, n));
    // not mapped: ONE copy into h_stage and four host memcpys instead of four pageable copies with their fixed cost each
    if (!mapped) HIP_TRY(ctx, hipMemcpyAsync(ctx->h_stage.p, i32, n * 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const int32_t *hs = (const int32_t *)ctx->h_stage.p;
    if (out->bc1) memcpy(out->bc1, hs, n * 4);
    if (out->bc2) memcpy(out->bc2, hs + n, n * 4);
    if (out->keep_start) memcpy(out->keep_start, hs + 2 * n, n * 4);
    if (out->keep_end) memcpy(out->keep_end, hs + 3 * n, n * 4);
    return BDX_OK;
}

// Large batches through the host entry point: the reads go up in a few chunks on a copy stream of the context's own
// while the kernels of the previous chunk run (one classify call per chunk on the context's stream, tied to its copy
// by an event); the verdict vectors come back once at the end.  With pageable host memory hipMemcpyAsync returns when
// the chunk is staged, so the launch of chunk i's kernels falls exactly between the copies of chunks i and i + 1.
// (The longest read is known, `facts` holds it: bdx_classify_host has scanned the offsets — a device-side measurement per
// chunk would synchronise the stream and undo the overlap.)
int classify_host_pipelined(bdx_ctx *ctx, const uint8_t *seq_bytes, const int64_t *seq_off, int64_t n_reads,
                            const bdx_outputs_t *out, int n_chunks, BdxBatchIn facts) {
    const size_t n = (size_t)n_reads;
    const int64_t base = seq_off[0];
    const int64_t total = seq_off[n_reads] - base;
    if (!ctx->copy_stream) {
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
        for (hipEvent_t &e : ctx->copy_events) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    HIP_TRY(ctx, ctx->d_seq.ensure((size_t)total + 64));
    HIP_TRY(ctx, ctx->d_off.ensure((n + 1) * 8));
    HIP_TRY(ctx, ctx->d_out_i32.ensure(n * 4 * 12));
    HIP_TRY(ctx, ctx->d_out_f64.ensure(n * 8 * 4));
    int32_t *bi = (int32_t *)ctx->d_out_i32.p;
    double *bf = (double *)ctx->d_out_f64.p;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_off.p, seq_off, (n + 1) * 8, hipMemcpyHostToDevice, ctx->copy_stream));
    facts.d_seq = (const uint8_t *)ctx->d_seq.p - base;
    for (int c = 0; c < n_chunks; ++c) {
        // (earlier chunks take the remainder: no work buffer has to grow while kernels run)
        const size_t r0 = n / n_chunks * c + ((size_t)c < n % n_chunks ? c : n % n_chunks);
        const size_t r1 = r0 + n / n_chunks + ((size_t)c < n % n_chunks ? 1 : 0);
        const int64_t b0 = seq_off[r0], b1 = seq_off[r1];
        if (b1 > b0)
            HIP_TRY(ctx, hipMemcpyAsync((uint8_t *)ctx->d_seq.p + (b0 - base), seq_bytes + b0, (size_t)(b1 - b0), hipMemcpyHostToDevice, ctx->copy_stream));
        HIP_TRY(ctx, hipEventRecord(ctx->copy_events[c], ctx->copy_stream));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->copy_events[c], 0));
        facts.d_off = (const int64_t *)ctx->d_off.p + r0;
        facts.n_reads = (int64_t)(r1 - r0);
        facts.out = out_slots(*out, bi, bf, n, r0);
        const int rc = bdx_classify_batch(ctx, facts);
        if (rc != BDX_OK) {
            (void)hipStreamSynchronize(ctx->copy_stream);
            return rc;
        }
    }
    const int rcd = download_items(ctx, back_items(*out, out_slots(*out, bi, bf, n), n));
    if (rcd != BDX_OK) return rcd;
    ctx->pipelined_calls += 1;
    return BDX_OK;
}

// Longest read and monotonicity of a host offset vector (8 threads for large batches: the pass is memory-bound).
void scan_offsets(const int64_t *seq_off, int64_t n_reads, int64_t &mx_out, bool &monotone_out) {
    const int nt = n_reads > 262144 ? 8 : 1;
    int64_t mx[8] = {};
    bool bad[8] = {};
    parallel_for(nt, [&](const int t) {
        const int64_t lo = n_reads * t / nt, hi = n_reads * (t + 1) / nt;
        int64_t m = 0;
        bool neg = false;
        for (int64_t i = lo; i < hi; ++i) {
            const int64_t d = seq_off[i + 1] - seq_off[i];
            neg |= d < 0;
            m = d > m ? d : m;
        }
        mx[t] = m;
        bad[t] = neg;
    });
    mx_out = 0;
    monotone_out = true;
    for (int t = 0; t < nt; ++t) {
        mx_out = mx[t] > mx_out ? mx[t] : mx_out;
        monotone_out = monotone_out && !bad[t];
    }
}

// Host mirror of the device's per-read window arithmetic (bdx_core.h resolve_range / pass_window and the per-read
// setup of bdx_bitpar.hip): the 0-based half-open byte range [ulo, uhi) of a read of n code units that ANY pass may
// touch — final_search_range first:last per pass (classification.jl:795-809), + max_m - 1 beyond the last start
// position for :hamming / :exact.
void host_union_window(const BdxDevCfg &cfg, long long n_ll, long long &ulo, long long &uhi) {
    const long long n = n_ll > (1LL << 30) ? (1LL << 30) : n_ll;
    const auto resolve = [&](const BdxDevRange &dr, long long &first, long long &last) { bdx_resolve_range(dr, n, first, last); };
    ulo = (1LL << 40);
    uhi = 0;
    const bool sgm = cfg.algorithm == BDX_ALG_SEMIGLOBAL;
    for (int p = 0; p < (cfg.is_dual ? 2 : 1); ++p) {
        const BdxDevPass &P = cfg.pass[p];
        long long first, last;
        bool ok = true;
        if (P.explicit_window) {
            first = P.win_first > 1 ? P.win_first : 1;
            last = P.win_last < n ? P.win_last : n;
        } else {
            long long rf, rl, bf, bl, ef, el;
            resolve(P.ref_search, rf, rl);
            resolve(P.bc_start, bf, bl);
            resolve(P.bc_end, ef, el);
            first = rf > bf ? rf : bf;
            if (first < 1) first = 1;
            last = rl < el ? rl : el;
            if (n < last) last = n;
            if (first > last || first > bl || last < ef) ok = false;  // :805-807
        }
        const long long f = ok ? (first > 1 ? first : 1) : 1;
        const long long l = ok ? (last < n ? last : n) : 0;
        if (l >= f) {
            long long h = sgm ? l : l + cfg.max_m - 1;
            if (h > n) h = n;
            if (f - 1 < ulo) ulo = f - 1;
            if (h > uhi) uhi = h;
        }
    }
    if (uhi <= ulo) ulo = uhi = 0;
}

// 1: not worth it (the caller uploads the whole reads); 0: classified through the window upload; < 0: error
int classify_host_windows(bdx_ctx *ctx, const uint8_t *seq_bytes, const int64_t *seq_off, int64_t n_reads,
                          const bdx_outputs_t *out, BdxBatchIn facts) {
    if (ctx->tune.no_window_upload) return 1;
    const int64_t total = seq_off[n_reads] - seq_off[0];
    if (total < (int64_t)n_reads * 512) return 1;  // short reads: nothing to save
    const size_t n = (size_t)n_reads;
    ctx->h_coff.resize(n + 1);
    ctx->h_vlen.resize(n);
    ctx->h_vlo.resize(n);
    // two passes over the reads, both on a few host threads (the gather touches one cache line or two of every
    // 10 kbp read: latency-bound on one core): windows, a serial prefix sum of their sizes, gather
    const unsigned hw = std::thread::hardware_concurrency();
    const int nthr = n < 65536 ? 1 : (hw >= 8 ? 8 : (hw >= 2 ? (int)hw : 1));
    long long t_max[8] = {};
    bool t_bad[8] = {};
    parallel_for(nthr, [&](const int t) {
        long long mx = 0;
        for (size_t i = n * t / nthr; i < n * (t + 1) / nthr; ++i) {
            const long long len = seq_off[i + 1] - seq_off[i];
            if (len < 0) {
                t_bad[t] = true;
                return;
            }
            long long ulo, uhi;
            host_union_window(ctx->dev, len, ulo, uhi);
            ctx->h_coff[i + 1] = uhi - ulo;  // (sizes now, offsets after the prefix sum)
            ctx->h_vlen[i] = (int32_t)(len > (1LL << 30) ? (1LL << 30) : len);
            ctx->h_vlo[i] = (int32_t)ulo;
            if (len > mx) mx = len;
        }
        t_max[t] = mx;
    });
    long long maxlen = 0;
    for (int t = 0; t < nthr; ++t) {
        if (t_bad[t]) return bdx_fail(ctx, BDX_E_INVALID, "seq_off is not non-decreasing");
        if (t_max[t] > maxlen) maxlen = t_max[t];
    }
    ctx->h_coff[0] = 0;
    for (size_t i = 0; i < n; ++i) ctx->h_coff[i + 1] += ctx->h_coff[i];
    const int64_t wbytes = ctx->h_coff[n];
    if (wbytes * 2 + (int64_t)n_reads * 16 > total) return 1;  // the windows are most of the reads anyway
    ctx->h_win.resize((size_t)wbytes + 64);
    parallel_for(nthr, [&](const int t) {
        for (size_t i = n * t / nthr; i < n * (t + 1) / nthr; ++i) {
            const int64_t len_w = ctx->h_coff[i + 1] - ctx->h_coff[i];
            if (len_w > 0) memcpy(ctx->h_win.data() + ctx->h_coff[i], seq_bytes + seq_off[i] + ctx->h_vlo[i], (size_t)len_w);
        }
    });
    HIP_TRY(ctx, ctx->d_seq.ensure((size_t)wbytes + 64));
    HIP_TRY(ctx, ctx->d_off.ensure((n + 1) * 8));
    HIP_TRY(ctx, ctx->d_vlen.ensure(n * 4));
    HIP_TRY(ctx, ctx->d_vlo.ensure(n * 4));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_seq.p, ctx->h_win.data(), (size_t)wbytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_off.p, ctx->h_coff.data(), (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_vlen.p, ctx->h_vlen.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_vlo.p, ctx->h_vlo.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
    facts.d_seq = (const uint8_t *)ctx->d_seq.p;
    facts.d_off = (const int64_t *)ctx->d_off.p;
    facts.vlen = (const int32_t *)ctx->d_vlen.p;
    facts.vlo = (const int32_t *)ctx->d_vlo.p;
    facts.known_maxlen = (int)(maxlen > (1LL << 30) ? (1LL << 30) : (maxlen < 1 ? 1 : maxlen));  // (of the true reads)
    const int rc = run_and_download(ctx, facts, out);
    if (rc == BDX_OK) ctx->window_uploads += 1;
    return rc == BDX_OK ? 0 : rc;
}

}  // namespace

extern "C" {

int32_t bdx_classify_host(bdx_ctx *ctx, const uint8_t *seq_bytes, const int64_t *seq_off, int64_t n_reads,
                          const bdx_outputs_t *out) {
    if (!ctx) return BDX_E_INVALID;
    if (n_reads < 0) return bdx_fail(ctx, BDX_E_INVALID, "n_reads is negative");
    if (n_reads == 0) return BDX_OK;
    if (!seq_bytes || !seq_off || !out) return bdx_fail(ctx, BDX_E_INVALID, "NULL pointer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t base = seq_off[0];
    const int64_t total = seq_off[n_reads] - base;
    if (total < 0) return bdx_fail(ctx, BDX_E_INVALID, "seq_off is not non-decreasing");
    // what the host has seen of this batch (the longest read; the window upload's per-read windows) goes to the launch plan
    // as a value, with the batch; the launch log (bdx_last_launches) spans all of this call's device calls
    ctx->launch_log.clear();
    BdxBatchIn facts;
    facts.n_reads = n_reads;
    facts.append_log = true;
    {
        // Window upload: when the passes only look at a short column window of long reads (ONT-style reads with the
        // barcodes at an end, C5), copy just each read's window — the union over the passes of final_search_range
        // (+ m - 1 for :hamming / :exact), resolved exactly like the device does — instead of the whole read:
        // 10 kbp reads with "1:200" move 212 B per read over PCIe instead of 10 KB.
        int rcw = classify_host_windows(ctx, seq_bytes, seq_off, n_reads, out, facts);
        if (rcw != 1) return rcw;  // 0 done, < 0 error, 1: ordinary upload below
    }
    // The batch's longest read, for the launch plan and the statistics tables: the offsets are on the host anyway
    // (saves the device-side measurement — a tiny kernel, a 4-byte copy and a stream synchronisation per call, which
    // matters at the reference's chunk size of 4000 reads)
    {
        // one pass over the offsets: they must be non-decreasing (a negative length would reach the kernels' address
        // arithmetic), and the longest read comes out of the same pass; large batches are scanned by a few threads
        int64_t mx = 0;
        bool monotone = true;
        scan_offsets(seq_off, n_reads, mx, monotone);
        if (!monotone) return bdx_fail(ctx, BDX_E_INVALID, "seq_off is not non-decreasing");
        facts.known_maxlen = (int)(mx > (1LL << 30) ? (1LL << 30) : (mx < 1 ? 1 : mx));
    }
    if ((size_t)total + (size_t)(n_reads + 1) * 8 <= ((size_t)2 << 20)) {  // (beyond ~2 MB the extra host copy costs more than the second transfer)
        // small batches: bytes and offsets through ONE page-locked staging buffer and ONE asynchronous copy
        const size_t o_off = ((size_t)total + 64 + 255) & ~(size_t)255;
        const size_t bytes = o_off + (size_t)(n_reads + 1) * 8;
        HIP_TRY(ctx, ctx->h_in.ensure(bytes, 1 << 16));
        memcpy(ctx->h_in.p, seq_bytes + base, (size_t)total);
        memcpy((char *)ctx->h_in.p + o_off, seq_off, (size_t)(n_reads + 1) * 8);
        HIP_TRY(ctx, ctx->d_seq.ensure(bytes + 64));
        void *h_in_dev = nullptr;  // the staging buffer as the device sees it
        HIP_TRY(ctx, hipHostGetDevicePointer(&h_in_dev, ctx->h_in.p, 0));
        const bool zero_scratch = ctx->d_maxlen.p != nullptr;  // (allocated at bdx_create when a filter is in use)
        HIP_TRY(ctx, bdx_launch_copy(ctx->d_seq.p, h_in_dev, bytes, ctx->stream, zero_scratch ? ctx->scratch()->tile_queue : nullptr, 4 * BDX_SCRATCH_WORDS));
        facts.scratch_cleared = zero_scratch;  // (a credit for the one call below, whatever path it takes)
        facts.d_seq = (const uint8_t *)ctx->d_seq.p - base;
        facts.d_off = (const int64_t *)((const char *)ctx->d_seq.p + o_off);
        return run_and_download(ctx, facts, out, /*mapped_outputs=*/true);
    }
    // (worth it when the kernels take a noticeable part of the call — tiered budgets, split mode, no filter; the
    // single fused launch of a plain known-score config is 3 ms per 10 M reads, chunking it costs more than it hides:
    // measured C4 202 -> 242 M reads/s from pageable and 235 -> 295 M from page-locked buffers, C2 299 -> 260 M)
    bool heavy = ctx->tiered || !ctx->fs[0].bplan.enabled;
    for (int k = 0; k < (ctx->dev.is_dual ? 2 : 1); ++k) heavy = heavy || !ctx->fs[0].bplan.known_ok[k];
    if (heavy && total >= ((int64_t)96 << 20) && n_reads >= 8 * 65536 && !ctx->tune.no_pipeline) {
        int k = (int)(total / ((int64_t)48 << 20));
        k = k < 2 ? 2 : (k > 8 ? 8 : k);
        return classify_host_pipelined(ctx, seq_bytes, seq_off, n_reads, out, k, facts);
    }
    // The offsets are uploaded as given; the byte pointer is rebased so that off[0] indexes it.
    HIP_TRY(ctx, ctx->d_seq.ensure((size_t)total + 64));
    HIP_TRY(ctx, ctx->d_off.ensure((size_t)(n_reads + 1) * 8));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_seq.p, seq_bytes + base, (size_t)total, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_off.p, seq_off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    // kernel sees the byte base shifted by -base so that off[i] addresses read i
    facts.d_seq = (const uint8_t *)ctx->d_seq.p - base;
    facts.d_off = (const int64_t *)ctx->d_off.p;
    return run_and_download(ctx, facts, out);
}

// Page-locked host memory for the buffers handed to bdx_classify_host (reads, offsets, outputs): the
// copies then run as asynchronous DMA at PCIe speed instead of being staged through the driver.
void *bdx_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (bytes == 0) bytes = 1;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void bdx_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

}  // extern "C"
