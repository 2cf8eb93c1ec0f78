// The member decoder of csrc/bdx_inflate_core.h compiled as plain C++ (its phases run as loops over the thread index):
// tests/test_device_gunzip_cpu.py holds it to the cases of tests/inflate_cases.py, the ones the GPU tests hold the
// device to.
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../biodemux.jl_amd/csrc/bdx_inflate_core.h"

static InfShared S;  // one for every call, like a persistent workgroup's: inf_host_reset makes it a fresh one
static const int CANARY = 64;

extern "C" int32_t inf_host_member_max(void) { return INF_MEMBER_MAX; }
extern "C" int32_t inf_host_shared_bytes(void) { return (int32_t)sizeof(InfShared); }

// the state a workgroup starts with: everything zero, tables not built
extern "C" void inf_host_reset(void) { std::memset(&S, 0, sizeof S); }

// One member comp[0, clen) into out[0, plen); returns its status, or -1 when a byte beside the slot was touched.  The
// member is decoded from an exact-size copy that ends its allocation and into a slot with canaries on both sides.
extern "C" int32_t inf_host_decode(const uint8_t *comp, int32_t clen, uint8_t *out, int32_t plen) {
    INF_PHASE(inf_ph_tables(S, t))
    const size_t cbytes = clen > 0 ? (size_t)clen : 0, pbytes = plen > 0 ? (size_t)plen : 0;
    uint8_t *in = (uint8_t *)malloc(cbytes ? cbytes : 1);
    uint8_t *slot = (uint8_t *)malloc(pbytes + 2 * CANARY);
    if (cbytes) memcpy(in, comp, cbytes);
    memset(slot, 0xC5, pbytes + 2 * CANARY);
    int32_t status = -2;
    inf_decode_member(S, in, clen, slot + CANARY, plen, &status);
    for (int i = 0; i < CANARY; ++i)
        if (slot[i] != 0xC5 || slot[CANARY + pbytes + i] != 0xC5) status = -1;
    if (pbytes) memcpy(out, slot + CANARY, pbytes);
    free(slot);
    free(in);
    return status;
}
