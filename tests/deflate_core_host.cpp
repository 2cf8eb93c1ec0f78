// The chunk encoder of csrc/bdx_deflate_core.h compiled as plain C++ (its phases run as loops over the thread index):
// tests/test_device_gzip_cpu.py holds the members it makes to the same checks as the device's.
#include <cstdint>
#include <vector>

#include "../biodemux.jl_amd/csrc/bdx_deflate_core.h"

extern "C" int32_t dfl_host_chunk(void) { return DFL_CHUNK; }

// members of in[0, n) back to back into out (cap >= n + 33 per chunk, + 64); returns their bytes, -1 when cap is short
extern "C" int64_t dfl_host_encode(const uint8_t *in, int64_t n, uint8_t *out, int64_t cap) {
    static DflShared S;
    std::vector<uint32_t> tok(DFL_CHUNK);
    std::vector<uint8_t> slot(DFL_CHUNK + 64);
    DFL_PHASE(dfl_ph_tables(S, t))
    int64_t pos = 0;
    for (int64_t o = 0; o < n; o += DFL_CHUNK) {
        const int len = (int)(n - o < DFL_CHUNK ? n - o : DFL_CHUNK);
        uint32_t ms = 0;
        dfl_encode_chunk(S, in + o, len, tok.data(), slot.data(), &ms);
        if (ms > (uint32_t)len + 33 || pos + ms > cap) return -1;
        for (uint32_t i = 0; i < ms; ++i) out[pos + i] = slot[i];
        pos += ms;
    }
    return pos;
}
