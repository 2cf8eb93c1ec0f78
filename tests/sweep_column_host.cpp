// Stand-alone driver for csrc/bdx_sweep_col.h, the column code of the wave kernel's sweeps (test_sweep_column_cpu.py builds it
// with the host compiler under ASan / UBSan and runs it as a program):
//   1. every dword of eight codes 0..4: byte field k of the expansion is 4 x code k — and equals the bit-field address;
//   2. the same with the junk nibbles of nv = -1 .. 9 live columns OR-ed in: live columns keep their field, junk columns get
//      a field of 16 .. 28, the rows of the peq table that no barcode has a base in;
//   3. 10^6 random (Ph, Mh) with never both top bits set, and the corner pairs: the add-with-carry score update equals the
//      carry-free one written out here (score + (Ph >> 31) + ((int)Mh >> 31): the form DESIGN.md section 4 measured and dropped),
//      and the doubling helper equals the doubled words the carry form returns;
//   4. 2 000 random (barcode of 16 .. 32 bases, 64-column text over A, C, G, T, N): both forms of the column step — tracked
//      (score by carry-out) and untracked (doublings through the add helper, score by popcount) — give the per-column scores
//      of a plain semi-global DP and the same state.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bdx_sweep_col.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            fprintf(stderr, "FAILED %s: ", #cond);        \
            fprintf(stderr, __VA_ARGS__);                  \
            fprintf(stderr, "\n");                        \
            exit(1);                                       \
        }                                                  \
    } while (0)

static long check_fields() {
    long words = 0;
    for (uint32_t w = 0; w < 390625u; ++w) {  // 5^8
        uint32_t A = 0, x = w;
        int code[8];
        for (int k = 0; k < 8; ++k) {
            code[k] = (int)(x % 5u);
            x /= 5u;
            A |= (uint32_t)code[k] << (4 * k);
        }
        for (int nv = -1; nv <= 9; ++nv) {  // (9 = no junk, as 8; -1 = all junk, as 0)
            const uint32_t J = A | bdx_col_junk(nv);
            uint32_t ev, od;
            bdx_col_fields(J, BDX_COL_FIELD_MASK, ev, od);
            CHECK((ev & ~BDX_COL_FIELD_MASK) == 0 && (od & ~BDX_COL_FIELD_MASK) == 0, "stray bits, word %08x nv %d", A, nv);
            for (int k = 0; k < 8; ++k) {
                const uint32_t f = bdx_col_field(ev, od, k);
                const uint32_t old = ((J >> (4 * k)) & 7u) << 2;  // the bit-field address: 3 bits of nibble k, times 4
                CHECK(f == old, "field %d of %08x (nv %d): %u, bit-field address %u", k, A, nv, f, old);
                if (k < nv)
                    CHECK(f == 4u * (uint32_t)code[k], "live field %d of %08x (nv %d): %u", k, A, nv, f);
                else
                    CHECK(f == 4u * (uint32_t)(code[k] | 4) && f >= 16u && f <= 28u, "junk field %d of %08x (nv %d): %u", k, A, nv, f);
            }
        }
        ++words;
    }
    return words;
}

static void check_score_pair(const uint32_t Ph, const uint32_t Mh, const int score) {
    uint32_t p = Ph, m = Mh;
    const int carry = bdx_col_score_carry(p, m, score);
    const int top = score + (int)(Ph >> 31) + ((int)Mh >> 31);
    CHECK(carry == top, "Ph %08x Mh %08x score %d: carry %d, carry-free %d", Ph, Mh, score, carry, top);
    CHECK(carry == score + (int)(Ph >> 31) - (int)(Mh >> 31), "Ph %08x Mh %08x: %d", Ph, Mh, carry);
    CHECK(p == bdx_col_dbl(Ph) && m == bdx_col_dbl(Mh) && p == Ph << 1 && m == Mh << 1, "doubling of %08x / %08x", Ph, Mh);
}

static long check_scores() {
    const uint32_t corners[][2] = {{0u, 0u}, {0xFFFFFFFFu, 0u}, {0u, 0xFFFFFFFFu}, {0x80000000u, 0x7FFFFFFFu}, {0x7FFFFFFFu, 0x80000000u}};
    long n = 0;
    for (const auto &c : corners)
        for (const int s : {0, 1, 32, -1}) check_score_pair(c[0], c[1], s), ++n;
    for (int i = 0; i < 1000000; ++i) {
        uint32_t Ph = (uint32_t)rnd(), Mh = (uint32_t)rnd();
        const uint64_t r = rnd();
        if ((Ph & Mh) >> 31) (r & 1 ? Ph : Mh) &= 0x7FFFFFFFu;  // never both top bits: a delta is +1 or -1
        check_score_pair(Ph, Mh, (int)((r >> 8) % 65u) - 16);
        ++n;
    }
    return n;
}

static long check_columns() {
    static const char SYM[5] = {'A', 'C', 'T', 'G', 'N'};  // codes 0..3 = (byte >> 1) & 3, 4 = other
    long cols = 0;
    for (int it = 0; it < 2000; ++it) {
        const int m = 16 + (int)(rnd() % 17u), n = 64, shift = 32 - m;
        int bc[32], text[64];
        for (int i = 0; i < m; ++i) bc[i] = (int)(rnd() % 4u);
        for (int j = 0; j < n; ++j) {
            const uint64_t r = rnd();
            // (half of the cases carry a noisy copy of the barcode, so that the scores fall well below m)
            text[j] = (it & 1) && j >= 10 && j < 10 + m && r % 8u ? bc[j - 10] : (int)((r >> 8) % 5u);
        }
        // the peq words of the kernel's table (bdx_plan.cpp peq8_rows): top-aligned rows, the virtual rows below match everything
        const uint32_t rows = m == 32 ? 0xFFFFFFFFu : (((1u << m) - 1u) << shift);
        uint32_t peq[8];
        for (int code = 0; code < 8; ++code) {
            peq[code] = ~rows;
            if (code < 4)
                for (int i = 0; i < m; ++i)
                    if (bc[i] == code) peq[code] |= 1u << (shift + i);
        }
        // plain DP: D[0][j] = 0 (free start), D[i][0] = i, unit costs; score of column j = D[m][j]
        std::vector<int> prev(m + 1), cur(m + 1);
        for (int i = 0; i <= m; ++i) prev[i] = i;
        uint32_t Pv[2] = {rows, rows}, Mv[2] = {0u, 0u};
        int score[2] = {m, m}, best[2] = {0x7FFFFFFF, 0x7FFFFFFF}, dp_best = 0x7FFFFFFF;
        for (int j = 0; j < n; ++j) {
            cur[0] = 0;
            for (int i = 1; i <= m; ++i) {
                const int sub = prev[i - 1] + (text[j] < 4 && text[j] == bc[i - 1] ? 0 : 1);
                const int del = prev[i] + 1, ins = cur[i - 1] + 1;
                cur[i] = sub < del ? (sub < ins ? sub : ins) : (del < ins ? del : ins);
            }
            prev.swap(cur);
            dp_best = prev[m] < dp_best ? prev[m] : dp_best;
            const uint32_t ep0 = sweep_step<true, false>(peq[text[j]], Pv[0], Mv[0], score[0], best[0]);
            // (the untracked step, doublings through the add helper: its score is popcount(Pv) - popcount(Mv), the sum of the
            // vertical deltas — what the kernel takes at its first tracked column)
            int unused_score = 0, unused_best = 0;
            const uint32_t ep1 = sweep_step<false, true>(peq[text[j]], Pv[1], Mv[1], unused_score, unused_best);
            score[1] = __builtin_popcount(Pv[1]) - __builtin_popcount(Mv[1]);
            best[1] = score[1] < best[1] ? score[1] : best[1];
            CHECK(score[0] == prev[m] && score[1] == prev[m], "case %d (m %d) column %d '%c': DP %d, tracked %d, untracked + popcount %d", it, m, j,
                  SYM[text[j]], prev[m], score[0], score[1]);
            CHECK(best[0] == dp_best && best[1] == dp_best && ep0 == ep1 && Pv[0] == Pv[1] && Mv[0] == Mv[1], "case %d column %d: state", it, j);
            ++cols;
        }
    }
    return cols;
}

int main() {
    const long words = check_fields();
    const long pairs = check_scores();
    const long cols = check_columns();
    printf("sweep column driver ok: %ld words, %ld pairs, %ld columns\n", words, pairs, cols);
    return 0;
}
