// Stand-alone driver for csrc/bdx_read_index.h, the wave kernel's hit -> read mapping for tiles of equal-length reads
// (test_read_index_cpu.py builds it with the host compiler under ASan / UBSan and runs it as a program):
//   1. bdx_read_index(x, bdx_read_index_mul(len)) == x / len for every len = 1 .. 5136 and x = 0 .. 5135 (a LEAN tile holds at
//      most 5 x 1024 + 16 flat positions);
//   2. for len = 2 .. 400 and a spread of larger ones up to 65 535: the same at the largest x with x len < 2^32, at the few x
//      below it and at every multiple of len next to it (the places a too small or too large multiplier shows first);
//   3. x = (uint32_t)-1 .. (uint32_t)-16, a position in the head padding in front of the tile's first base: the index is at
//      least 32 for every len = 1 .. 10256, so the kernel's unsigned test against the tile's read count (<= 32) rejects it;
//   4. the multiplier is floor(2^32 / len) + 1 unless len is a power of two (then 2^32 / len), and 0 for len = 0 and len = 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "bdx_read_index.h"

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            fprintf(stderr, "FAILED %s: ", #cond);        \
            fprintf(stderr, __VA_ARGS__);                  \
            fprintf(stderr, "\n");                        \
            exit(1);                                       \
        }                                                  \
    } while (0)

int main() {
    long exhaustive = 0, edges = 0, heads = 0;
    for (uint32_t len = 1; len <= 5136u; ++len) {
        const uint32_t m = bdx_read_index_mul(len);
        for (uint32_t x = 0; x < 5136u; ++x, ++exhaustive) {
            const uint32_t t = bdx_read_index(x, m);
            CHECK(t == x / len, "len %u x %u: %u", len, x, t);
        }
    }
    long lens = 0;
    for (uint32_t len = 2; len <= 65535u; len += (len < 400u ? 1u : 97u + len / 64u), ++lens) {
        const uint32_t m = bdx_read_index_mul(len);
        const uint64_t expect = (len & (len - 1u)) == 0u ? (1ull << 32) / len : (1ull << 32) / len + 1ull;
        CHECK((uint64_t)m == expect, "multiplier of %u: %u", len, m);
        const uint32_t xmax = (uint32_t)(((1ull << 32) - 1ull) / len);  // the largest x with x len < 2^32
        CHECK((uint64_t)xmax * len < (1ull << 32) && (uint64_t)(xmax + 1ull) * len >= (1ull << 32), "xmax of %u", len);
        for (uint32_t d = 0; d < 64u && d <= xmax; ++d, ++edges) {
            const uint32_t x = xmax - d;
            CHECK(bdx_read_index(x, m) == x / len, "len %u x %u: %u", len, x, bdx_read_index(x, m));
        }
        const uint32_t top = xmax / len * len;  // the last multiple of len and its neighbours
        for (int d = -2; d <= 2; ++d) {
            const uint64_t x = (uint64_t)top + (uint64_t)(int64_t)d;
            if (x > xmax) continue;
            CHECK(bdx_read_index((uint32_t)x, m) == (uint32_t)x / len, "len %u x %llu", len, (unsigned long long)x);
            ++edges;
        }
    }
    CHECK(lens >= 300, "%ld lengths", lens);
    CHECK(bdx_read_index_mul(0u) == 0u && bdx_read_index_mul(1u) == 0u, "no multiplier for len 0 / 1");
    for (uint32_t len = 1; len <= 10256u; ++len) {
        const uint32_t m = bdx_read_index_mul(len);
        for (uint32_t d = 1; d <= 16u; ++d, ++heads) {
            const uint32_t t = bdx_read_index(0u - d, m);
            CHECK(t >= 32u, "len %u x -%u: %u", len, d, t);
        }
    }
    printf("read index driver ok: %ld exhaustive, %ld lengths, %ld edge positions, %ld head positions\n", exhaustive, lens, edges, heads);
    return 0;
}
