// The chunk encoder of csrc/bdx_deflate_core.h compiled as plain C++ (its phases run as loops over the thread index):
// tests/test_device_gzip_cpu.py holds the members it makes to the same checks as the device's, and
// tests/test_device_gzip_bytes_gpu.py holds the device to these very bytes.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../biodemux.jl_amd/csrc/bdx_deflate_core.h"

static DflShared S;  // one for every call, like a persistent workgroup's: dfl_host_reset makes it a fresh one

extern "C" int32_t dfl_host_chunk(void) { return DFL_CHUNK; }

// the state a workgroup starts with: everything zero (the harshest "uninitialised" a test can name), tables not built
extern "C" void dfl_host_reset(void) { std::memset(&S, 0, sizeof S); }

// members of in[0, n) back to back into out (cap >= n + 33 per chunk, + 64); returns their bytes, -1 when cap is short.
// Tokens and slot are exact-size for every chunk: n words, n + 33 bytes rounded up to the slot's 64.
extern "C" int64_t dfl_host_encode(const uint8_t *in, int64_t n, uint8_t *out, int64_t cap) {
    DFL_PHASE(dfl_ph_tables(S, t))
    int64_t pos = 0;
    for (int64_t o = 0; o < n; o += DFL_CHUNK) {
        const int len = (int)(n - o < DFL_CHUNK ? n - o : DFL_CHUNK);
        std::vector<uint32_t> tok((size_t)len);
        std::vector<uint8_t> slot(((size_t)len + 33 + 63) & ~(size_t)63);
        uint32_t ms = 0;
        dfl_encode_chunk(S, in + o, len, tok.data(), slot.data(), &ms);
        if (ms > (uint32_t)len + 33 || pos + ms > cap) return -1;
        for (uint32_t i = 0; i < ms; ++i) out[pos + i] = slot[i];
        pos += ms;
    }
    return pos;
}

// What the last chunk's dynamic block takes (or would have taken: a stored member does not show how close it came), in
// bytes, recomputed from what the encoder left in its shared state: the histograms, the code lengths, HLIT and HDIST.
extern "C" int64_t dfl_host_last_dynamic_bytes(void) {
    uint64_t bits = DFL_HDR_FIXED_BITS + 4u * (S.hlit + S.hdist);
    for (int s = 0; s < DFL_NLL; ++s) bits += (uint64_t)S.hist[s] * (S.clen[s] + (s > 256 ? dfl_len_extra(s) : 0u));
    for (int s = 0; s < DFL_ND; ++s) bits += (uint64_t)S.hist[DFL_NLL + s] * (S.clen[DFL_NLL + s] + dfl_dist_extra(s));
    return (int64_t)((bits + 7) >> 3);
}
