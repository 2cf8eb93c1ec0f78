// bdx_read_index.h — the wave kernel's hit -> read mapping for a tile of equal-length reads (bdx_wave_kernel.h, resolve):
// read t = floor(x / len) of the flat position x counted from the tile's first base, as one multiply-high.  Plain functions
// of their arguments: they compile for the device and as plain C++ (tests/read_index_host.cpp checks them against x / len).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BDX_RIX_FN __host__ __device__ __forceinline__
#else
#define BDX_RIX_FN inline
#endif

// The multiplier of a read length.  With 2^32 = q len + r (0 <= r < len) and m = q + 1 = floor(2^32 / len) + 1:
//     m len = 2^32 + e,  e = len - r in [1, len],   so   x m / 2^32 = x / len + x e / (len 2^32).
// x = a len + b with b <= len - 1 leaves x / len at most (len - 1) / len above a, and the second term stays below 1 / len
// whenever x e < 2^32, for which x len < 2^32 is enough:  floor(x m / 2^32) = floor(x / len)  for every x with x len < 2^32.
// (The kernel's x is below 10 x 1024 + 16 and its len at most that: x len < 2^27.)
// The value is formed in 32 bits as floor((2^32 - 1) / len) + 1.  That is the m above unless len divides 2^32; for such a
// power of two it is 2^32 / len itself (e = 0), and the multiply-high is the exact shift, for every x.
// len = 1: m would be 2^32 + 1, which no 32-bit multiplier holds; the sum wraps to 0, and 0 stands for "no multiplier" (so
// does len = 0): bdx_read_index returns x itself then, the kernel sends such a tile down its path for mixed lengths.
BDX_RIX_FN uint32_t bdx_read_index_mul(const uint32_t len) { return len ? 0xFFFFFFFFu / len + 1u : 0u; }

// floor(x m / 2^32)
BDX_RIX_FN uint32_t bdx_mul_hi(const uint32_t x, const uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(x, m);
#else
    return (uint32_t)(((uint64_t)x * m) >> 32);
#endif
}

// floor(x / len), m = bdx_read_index_mul(len), for x len < 2^32.
// A position in front of the tile's first base (the head padding: the caller's difference is -1 .. -15) arrives as
// x >= 2^32 - 16.  It then comes out as at least floor(x / len) >= (2^32 - 16) / 10256 > 400 000, far beyond any tile's read
// count: the caller's UNSIGNED test t < nr rejects it together with the positions behind the last read (x >= nr len).
BDX_RIX_FN uint32_t bdx_read_index(const uint32_t x, const uint32_t m) { return m ? bdx_mul_hi(x, m) : x; }
