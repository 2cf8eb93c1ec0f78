// Stand-alone driver for the sweep set-up helpers of csrc/bdx_sweep_col.h (test_sweep_setup_cpu.py builds it with the host
// compiler under ASan / UBSan and runs it as a program).  The helpers replace expressions the wave kernel's LEAN forms used
// to spell out; every other form still does, so the old expressions are written out here as the kernel has them:
//   1. bdx_col_junk_word(rem, u) against bdx_col_junk(rem - 8 u) for every rem in -40 .. 72 and every word u = 0 .. 3, and
//      the "one word" shortcut of the sweep: with rem >= 24 the words 0 .. 2 carry no junk at all;
//   2. bdx_col_pv0(m) against  m >= 32 ? ~0 : ((1 << m) - 1) << (32 - m)  for m = 1 .. 32.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "bdx_sweep_col.h"

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            fprintf(stderr, "FAILED %s: ", #cond);        \
            fprintf(stderr, __VA_ARGS__);                  \
            fprintf(stderr, "\n");                        \
            exit(1);                                       \
        }                                                  \
    } while (0)

static uint32_t old_junk(const int rem, const int u) {  // the sweep's loop body, every form but LEAN
    const int nv = rem - 8 * u;
    return nv >= 8 ? 0u : (nv <= 0 ? 0x44444444u : (0x44444444u << (4 * nv)));
}

static uint32_t old_pv0(const int mm) { return mm >= 32 ? 0xFFFFFFFFu : (((1u << mm) - 1u) << (32 - mm)); }

int main() {
    long masks = 0, shortcuts = 0, pvs = 0;
    for (int rem = -40; rem <= 72; ++rem) {
        for (int u = 0; u < 4; ++u) {
            const uint32_t want = old_junk(rem, u);
            CHECK(want == bdx_col_junk(rem - 8 * u), "rem %d word %d: the driver's copy of the old expression", rem, u);
            CHECK(bdx_col_junk_word(rem, u) == want, "rem %d word %d: %08x, expected %08x", rem, u, bdx_col_junk_word(rem, u), want);
            // a junk nibble is code 4 exactly in the columns at or behind the window's end
            for (int c = 0; c < 8; ++c) CHECK(((bdx_col_junk_word(rem, u) >> (4 * c)) & 15u) == (8 * u + c >= rem ? 4u : 0u), "rem %d word %d column %d", rem, u, c);
            ++masks;
        }
        if (rem >= 24) {
            for (int u = 0; u < 3; ++u) CHECK(old_junk(rem, u) == 0u, "rem %d: word %d has junk although the window ends in word 3", rem, u);
            ++shortcuts;
        }
    }
    for (int m = 1; m <= 32; ++m) {
        CHECK(bdx_col_pv0(m) == old_pv0(m), "m %d: %08x, expected %08x", m, bdx_col_pv0(m), old_pv0(m));
        CHECK(__builtin_popcount(bdx_col_pv0(m)) == m && (bdx_col_pv0(m) >> 31) == 1u, "m %d: not the top m bits", m);
        ++pvs;
    }
    printf("sweep setup driver ok: %ld masks, %ld shortcuts, %ld start values\n", masks, shortcuts, pvs);
    return 0;
}
