// bdx_crc32_core.h — the CRC-32 arithmetic the device DEFLATE encoder (bdx_deflate_core.h) and the device inflate
// (bdx_inflate_core.h) share: a byte table, and the combination of slice CRCs as polynomials over GF(2) modulo P,
// reflected (bit 31 is x^0).  Plain functions of their arguments: they compile for the device and as plain C++.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BDX_CRC_FN __device__ inline
#else
#define BDX_CRC_FN inline
#endif

#define BDX_CRC_POLY 0xedb88320u

BDX_CRC_FN uint32_t bdx_crc_multmodp(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1) ? (b >> 1) ^ BDX_CRC_POLY : b >> 1;
    }
    return p;
}
// x2n[k] = x^(2^k) mod P, k = 0 .. 31
BDX_CRC_FN void bdx_crc_x2n_init(uint32_t *x2n) {
    uint32_t p = 0x40000000u;  // x^1
    x2n[0] = p;
    for (int k = 1; k < 32; ++k) x2n[k] = p = bdx_crc_multmodp(p, p);
}
// x^(8 n) mod P
BDX_CRC_FN uint32_t bdx_crc_x8n(const uint32_t *x2n, uint32_t n) {
    uint32_t p = 0x80000000u;
    for (int k = 3; n; n >>= 1, ++k)
        if (n & 1) p = bdx_crc_multmodp(x2n[k & 31], p);
    return p;
}
// entry t of the byte table
BDX_CRC_FN uint32_t bdx_crc_table_entry(int t) {
    uint32_t c = (uint32_t)t;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? BDX_CRC_POLY ^ (c >> 1) : c >> 1;
    return c;
}
