// Both levels of the chunk encoder (csrc/bdx_deflate_core.h, csrc/bdx_deflate2_core.h) compiled as plain C++ behind one
// entry that takes the level, the way bdx_fq_deflate_level_device does: tests/test_device_gzip_level_cpu.py holds the
// members it makes to zlib and to the named edges of tests/deflate2_cases.py, and tests/test_device_gzip_level_gpu.py
// holds the device to these very bytes.  Built with -DDFL2_K / -DDFL2_INBLOCK / -DDFL2_LAZY / -DDFL2_RLE for the
// ablation of deflate2_cases.ratio_report.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../biodemux.jl_amd/csrc/bdx_deflate2_core.h"

static Dfl2Shared S;  // one for every call and both levels, like a persistent workgroup's

extern "C" int32_t dfl2_host_chunk(void) { return DFL_CHUNK; }
extern "C" int32_t dfl2_host_k(void) { return DFL2_K; }
extern "C" int32_t dfl2_host_hash_bits(void) { return DFL2_HASH_BITS; }
extern "C" void dfl2_host_reset(void) { std::memset(&S, 0, sizeof S); }

// members of in[0, n) back to back into out (cap >= n + 33 per chunk, + 64); returns their bytes, -1 when cap is short
// or the level is none.  Tokens and slot are exact-size for every chunk.
extern "C" int64_t dfl2_host_encode(int32_t level, const uint8_t *in, int64_t n, uint8_t *out, int64_t cap) {
    if (level != 1 && level != 2) return -1;
    DFL_PHASE(dfl_ph_tables(S.B, t))
    int64_t pos = 0;
    for (int64_t o = 0; o < n; o += DFL_CHUNK) {
        const int len = (int)(n - o < DFL_CHUNK ? n - o : DFL_CHUNK);
        std::vector<uint32_t> tok((size_t)len);
        std::vector<uint8_t> slot(((size_t)len + 33 + 63) & ~(size_t)63);
        uint32_t ms = 0;
        if (level == 1)
            dfl_encode_chunk(S.B, in + o, len, tok.data(), slot.data(), &ms);
        else
            dfl2_encode_chunk(S, in + o, len, tok.data(), slot.data(), &ms);
        if (ms > (uint32_t)len + 33 || pos + ms > cap) return -1;
        for (uint32_t i = 0; i < ms; ++i) out[pos + i] = slot[i];
        pos += ms;
    }
    return pos;
}

// what the last level-2 chunk's dynamic block takes or would have taken, in bytes, from the state the encoder left
extern "C" int64_t dfl2_host_last_dynamic_bytes(void) {
    uint64_t bits = S.hdr_bits;
    for (int s = 0; s < DFL_NLL; ++s) bits += (uint64_t)S.B.hist[s] * (S.B.clen[s] + (s > 256 ? dfl_len_extra(s) : 0u));
    for (int s = 0; s < DFL_ND; ++s) bits += (uint64_t)S.B.hist[DFL_NLL + s] * (S.B.clen[DFL_NLL + s] + dfl_dist_extra(s));
    return (int64_t)((bits + 7) >> 3);
}

// the code-length code's lengths of the last level-2 chunk (19, by symbol)
extern "C" void dfl2_host_last_cl_lengths(uint8_t *out19) {
    for (int s = 0; s < DFL2_NCL; ++s) out19[s] = S.cl_len[s];
}

// every position's best match BEFORE the walk (what dfl2_ph_find leaves) of one chunk: the predicates on lazy steps
// need to see the match that gave way
extern "C" void dfl2_host_records(const uint8_t *in, int32_t n, uint16_t *len, uint16_t *dist) {
    std::vector<uint32_t> tok((size_t)n);
    DFL_PHASE(dfl2_ph_init(S, t))
    for (int base = 0; base < n; base += DFL_THREADS) {
        DFL_PHASE(dfl2_ph_hash(S, in, n, base, t))
        DFL_PHASE(dfl2_ph_find(S, in, n, base, t))
        for (int t = 0; t < DFL_THREADS && base + t < n; ++t) len[base + t] = S.B.mlen[t], dist[base + t] = S.B.mdist[t];
        DFL_PHASE(dfl2_ph_insert_walk(S, in, n, base, tok.data(), t))
        DFL_PHASE(dfl_ph_emit(S.B, in, base, tok.data(), t))
    }
}
