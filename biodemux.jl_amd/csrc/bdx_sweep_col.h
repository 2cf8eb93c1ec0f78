// bdx_sweep_col.h — one column of the wave kernel's sweeps (bdx_wave_kernel.h): the address fields of a group of eight
// columns and Myers' recurrence with the tracked score update.  Plain functions of their arguments: they
// compile for the device and as plain C++ (tests/sweep_column_host.cpp checks them against each other and a plain DP).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BDX_COL_FN __host__ __device__ __forceinline__
#else
#define BDX_COL_FN inline
#endif

#define BDX_COL_FIELD_MASK 0x1C1C1C1Cu

// Nibbles of a group of eight columns of which only the first nv lie inside the window: the others become code 4 ("other":
// matches no barcode row), OR-ed onto the group's dword of 4-bit codes.
BDX_COL_FN uint32_t bdx_col_junk(const int nv) { return nv >= 8 ? 0u : (nv <= 0 ? 0x44444444u : (0x44444444u << (4 * nv))); }

// bdx_col_junk for word u (0..3) of a block of 32 columns of which `rem` (any value) lie inside the window: the count of
// the word's valid columns clamped to 0..8, and the low word of a 64-bit shift (eight valid columns shift everything out).
BDX_COL_FN uint32_t bdx_col_junk_word(const int rem, const int u) {
    int nv = rem - 8 * u;
    nv = nv < 0 ? 0 : (nv > 8 ? 8 : nv);
    return (uint32_t)(0x44444444ull << (4 * nv));
}

// Pv in front of a sweep's first column for a top-aligned barcode of m rows, 1 <= m <= 32 (the planner admits no other
// length): ones in the top m bits, which is ((1 << m) - 1) << (32 - m) without the special case for m = 32.
BDX_COL_FN uint32_t bdx_col_pv0(const int m) { return 0xFFFFFFFFu << ((32 - m) & 31); }

// A dword of eight 4-bit codes 0..4 (column k in nibble k) -> two words of byte fields, each 4 x code = the byte offset of
// the code's word in a barcode's peq row: ev holds columns 0, 2, 4, 6 and od columns 1, 3, 5, 7, column k in byte k >> 1.
// `mask` is BDX_COL_FIELD_MASK (an argument: the kernel keeps it in a register).
BDX_COL_FN void bdx_col_fields(const uint32_t A, const uint32_t mask, uint32_t &ev, uint32_t &od) {
    ev = (A << 2) & mask;
    od = (A >> 2) & mask;
}
BDX_COL_FN uint32_t bdx_col_field(const uint32_t ev, const uint32_t od, const int k) { return (((k & 1) ? od : ev) >> (8 * (k >> 1))) & 0xFFu; }

// The score after a tracked column, from the horizontal deltas Ph / Mh BEFORE their shift.  The pattern is top-aligned: bit 31
// is the barcode's last row, its delta is +1 (Ph), -1 (Mh) or 0 (never both), and it is the carry-out of the doubling, which
// is done here too.
BDX_COL_FN int bdx_col_score_carry(uint32_t &Ph, uint32_t &Mh, int score) {
#if defined(__has_builtin) && __has_builtin(__builtin_addc)
    uint32_t cp, cm;
    Ph = __builtin_addc(Ph, Ph, 0u, &cp);
    Mh = __builtin_addc(Mh, Mh, 0u, &cm);
#else
    const uint64_t p2 = (uint64_t)Ph + Ph, m2 = (uint64_t)Mh + Mh;
    const uint32_t cp = (uint32_t)(p2 >> 32), cm = (uint32_t)(m2 >> 32);
    Ph = (uint32_t)p2;
    Mh = (uint32_t)m2;
#endif
    score += (int)cp;
    score -= (int)cm;
    return score;
}

// x + x as an add (the compiler turns the C expression into a shift, which is the dearer instruction class on gfx950)
BDX_COL_FN uint32_t bdx_col_dbl(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_add_u32 %0, %0, %0" : "+v"(x));
    return x;
#else
    return x + x;
#endif
}

// One column of Myers' recurrence on a top-aligned pattern (bdx_bitpar.hip `step`); TRACK: the horizontal delta of the
// barcode's last row is the carry-out of the doubling and updates the score and the running minimum.  ADD (the LEAN forms'
// untracked columns): the doublings reach the assembler as adds.
template <bool TRACK, bool ADD = false>
BDX_COL_FN uint32_t sweep_step(const uint32_t Eq, uint32_t &Pv, uint32_t &Mv, int &score, int &best) {
    const uint32_t Xv = Eq | Mv;
    const uint32_t ep = Eq & Pv;  // (returned: its top bit is the known-start class's "the diagonal move into the last row is optimal")
    const uint32_t Xh = ((ep + Pv) ^ Pv) | Eq;
    uint32_t Ph = Mv | ~(Xh | Pv);
    uint32_t Mh = Pv & Xh;
    if (TRACK) {
        score = bdx_col_score_carry(Ph, Mh, score);
    } else {
        Ph = ADD ? bdx_col_dbl(Ph) : Ph + Ph;
        Mh = ADD ? bdx_col_dbl(Mh) : Mh + Mh;
    }
    Pv = Mh | ~(Xv | Ph);
    Mv = Ph & Xv;
    if (TRACK) best = score < best ? score : best;
    return ep;
}
