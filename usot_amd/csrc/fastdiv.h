// Division by a run-time divisor that is known when the launch is prepared: the host turns the divisor into a multiplier and a
// shift once (fastdiv_make), the kernel forms the quotient as the high part of one 32 x 32 -> 64-bit product (fastdiv_div:
// s_mul_hi_u32 + s_mul_i32 + a 64-bit shift, or v_mad_u64_u32 + a shift) instead of the ~40-instruction reciprocal expansion
// hipcc emits for `/` by a run-time value.  No branch and no special case, d = 1 included.
//
// Scheme (Granlund & Montgomery, "Division by invariant integers using multiplication", PLDI 1994, Theorem 4.2 with N = 31; the
// multiplier CUTLASS' FastDivmod uses).  For a divisor d >= 1 let s = ceil(log2 d) (2^(s-1) < d <= 2^s; s = 0 for d = 1) and
//     mul = ceil(2^(31+s) / d),   shr = 31 + s,   q(n) = (n * mul) >> shr = floor(n * mul / 2^(31+s)),  the product in 64 bits.
// mul fits 32 bits: 2^(31+s) / d < 2^(31+s) / 2^(s-1) = 2^32 for d > 2^(s-1), and mul = 2^31 for d = 2^s (d = 1: mul = 2^31,
// shr = 31).  The product fits 64 bits: n < 2^31 and mul < 2^32.
// RANGE, with proof.  q(n) == n / d for every dividend 0 <= n <= FASTDIV_MAX_DIVIDEND = 2^31 - 1 and every divisor
// 1 <= d <= 2^31 - 1:
//   write mul * d = 2^(31+s) + e with 0 <= e < d.  Then n * mul / 2^(31+s) = n / d + n * e / (d * 2^(31+s)), and with e < d <= 2^s
//   and n < 2^31 the second term is below 2^31 * 2^s / (d * 2^(31+s)) = 1 / d.  n / d = floor(n / d) + r / d with r <= d - 1, so
//   the sum stays below floor(n / d) + 1 and its floor is floor(n / d).  Dividends of 2^31 and more are outside the proof: every
//   caller keeps its dividends - block indices, output rows, k-tile and tap counts - below 2^31, and the conv launcher answers
//   USOT_EINVAL for a problem that could not (tests/test_fastdiv.py checks the bound itself).
// The remainder is n - q * d: fastdiv_divmod.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define USOT_FD_HD __host__ __device__ __forceinline__
#else
#define USOT_FD_HD inline
#endif

#define FASTDIV_MAX_DIVIDEND 0x7fffffffu     // the scheme is exact for dividends 0 .. 2^31 - 1
#define FASTDIV_MAX_DIVISOR  0x7fffffffu     // and divisors 1 .. 2^31 - 1

struct FastDiv {
    uint32_t mul;
    uint32_t shr;      // 31 .. 62
};

// the constants of divisor d (1 <= d <= FASTDIV_MAX_DIVISOR; 0 is answered like 1: no caller divides by it)
USOT_FD_HD FastDiv fastdiv_make(uint32_t d)
{
    uint32_t s = 0;
    while (s < 31u && ((uint32_t)1 << s) < d) ++s;              // s = ceil(log2 d), 0 .. 31
    if (d == 0u) d = 1u;
    const uint64_t p = (uint64_t)1 << (31u + s);
    FastDiv f;
    f.mul = (uint32_t)((p + d - 1u) / d);
    f.shr = 31u + s;
    return f;
}

// n / d for the FastDiv of d, 0 <= n <= FASTDIV_MAX_DIVIDEND
USOT_FD_HD uint32_t fastdiv_div(uint32_t n, FastDiv f)
{
    return (uint32_t)(((uint64_t)n * f.mul) >> f.shr);
}

// quotient returned, remainder through *rem (d: the divisor the constants were made from)
USOT_FD_HD uint32_t fastdiv_divmod(uint32_t n, FastDiv f, uint32_t d, uint32_t *rem)
{
    const uint32_t q = fastdiv_div(n, f);
    *rem = n - q * d;
    return q;
}
