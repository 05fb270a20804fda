// Stand-alone host check of usot_amd/csrc/fastdiv.h against `/` and `%` (tests/test_fastdiv.py builds and runs it; it may also be
// built with -fsanitize=address,undefined and run on its own).  Prints one line per part and exits non-zero on the first mismatch.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <thread>
#include <vector>
#include <atomic>
#include "fastdiv.h"

static std::atomic<int> g_bad{0};

static inline void check(uint32_t n, uint32_t d, FastDiv f)
{
    uint32_t r;
    const uint32_t q = fastdiv_divmod(n, f, d, &r);
    if (q != n / d || r != n % d) {
        if (g_bad.fetch_add(1) < 8) fprintf(stderr, "MISMATCH n=%u d=%u: got q=%u r=%u, want q=%u r=%u\n", n, d, q, r, n / d, n % d);
    }
}

// every dividend in [lo, hi) for one divisor, quotient and remainder against `/` and `%`
static void sweep(uint32_t d, uint32_t lo, uint32_t hi)
{
    const FastDiv f = fastdiv_make(d);
    uint32_t bad = 0;
    for (uint32_t n = lo; n < hi; ++n) {
        const uint32_t q = fastdiv_div(n, f);
        bad |= (q ^ (n / d)) | ((n - q * d) ^ (n % d));
    }
    if (bad)
        for (uint32_t n = lo; n < hi; ++n) check(n, d, f);     // name the offenders
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

int main(int argc, char **argv)
{
    const uint32_t MAXN = FASTDIV_MAX_DIVIDEND, MAXD = FASTDIV_MAX_DIVISOR;
    unsigned nthreads = std::thread::hardware_concurrency();
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 16) nthreads = 16;
    if (argc > 1) nthreads = (unsigned)atoi(argv[1]);

    // 1. exhaustive: every dividend below 2^22, every divisor 1 .. 4096
    {
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < nthreads; ++t)
            pool.emplace_back([t, nthreads] { for (uint32_t d = 1 + t; d <= 4096; d += nthreads) sweep(d, 0, 1u << 22); });
        for (auto &th : pool) th.join();
        printf("exhaustive n < 2^22, d = 1 .. 4096: %s\n", g_bad ? "FAILED" : "ok");
        if (g_bad) return 1;
    }
    // 2. the divisors the frame plans produce (search crops of 255 and of 271): every dividend below 2^24, the top 2^20 dividends of
    //    the documented range, and around every 4 099th multiple of the divisor up to the bound
    {
        const uint32_t plan[] = {961, 625, 31, 25, 29, 27, 3, 124, 248, 632,          // 255
                                 1089, 729, 33, 35, 140, 280, 1, 2, 4, 8, 9, 16, 18, 36, 64, 72, 256};      // 271 and the small k-walk counts
        for (uint32_t d : plan) {
            const FastDiv f = fastdiv_make(d);
            sweep(d, 0, 1u << 24);
            sweep(d, MAXN - (1u << 20), MAXN);
            check(MAXN, d, f);
            for (uint64_t m = d; m <= MAXN; m += (uint64_t)d * 4099) {
                check((uint32_t)m - 1, d, f); check((uint32_t)m, d, f);
                if (m + 1 <= MAXN) check((uint32_t)m + 1, d, f);
            }
        }
        printf("plan divisors: %s\n", g_bad ? "FAILED" : "ok");
        if (g_bad) return 1;
    }
    // 3. random pairs up to the documented bound (dividend <= 2^31 - 1, divisor 1 .. 2^31 - 1), divisors of every magnitude
    {
        for (int i = 0; i < 6000000; ++i) {
            const uint64_t a = rng(), b = rng();
            const uint32_t n = (uint32_t)(a & MAXN);
            uint32_t d = (uint32_t)((b & MAXD) >> (b >> 59));           // 0 .. 31 bits shorter
            if (d == 0) d = 1;
            check(n, d, fastdiv_make(d));
        }
        printf("6 000 000 random pairs: %s\n", g_bad ? "FAILED" : "ok");
        if (g_bad) return 1;
    }
    // 4. the bound itself: the largest dividend against small, large and extreme divisors; the largest divisor; powers of two and
    //    their neighbours
    {
        for (uint32_t d = 1; d <= 100000; ++d) check(MAXN, d, fastdiv_make(d));
        for (uint32_t d = MAXD; d > MAXD - 100000; --d) { const FastDiv f = fastdiv_make(d); check(MAXN, d, f); check(d - 1, d, f); check(d, d, f); check(0, d, f); }
        for (int s = 0; s < 31; ++s)
            for (int k = -2; k <= 2; ++k) {
                const int64_t d = ((int64_t)1 << s) + k;
                if (d < 1 || d > (int64_t)MAXD) continue;
                const FastDiv f = fastdiv_make((uint32_t)d);
                for (int64_t n = (int64_t)MAXN - (4 * d + 2 < 5000 ? 4 * d + 2 : 5000); n <= (int64_t)MAXN; ++n)      // the last multiples of d below the bound
                    if (n >= 0) check((uint32_t)n, (uint32_t)d, f);
                for (int j = 0; j < 31; ++j)
                    for (int e = -1; e <= 1; ++e) {
                        const int64_t n = ((int64_t)1 << j) + e;
                        if (n >= 0 && n <= (int64_t)MAXN) check((uint32_t)n, (uint32_t)d, f);
                    }
            }
        printf("the bound 2^31 - 1: %s\n", g_bad ? "FAILED" : "ok");
        if (g_bad) return 1;
    }
    printf("fastdiv: all parts ok\n");
    return 0;
}
