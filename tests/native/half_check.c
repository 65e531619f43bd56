/* half_check.c -- host check of the mini-host's plain-C binary16
 * (zhpe-ompi_amd/mca/host/mx_host.c: mxh_half_to_float, mxh_float_to_half,
 * mxh_short_float_reduce).  Built together with mx_host.c by the host
 * compiler under AddressSanitizer and UBSan and run on the CPU
 * (tests/test_short_float_native.py).  The operand arrays are heap blocks of
 * the exact size, so a function that reads or writes past `n` elements is
 * caught; the conversions are checked for properties that need no binary16
 * type in the compiler: exactness of half -> float, round trip, monotonic
 * rounding with ties to even.  Exits non-zero on the first violated class. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "host/mx_host.h"

static int g_fail;
#define CHECK(cond, ...)                                               \
    do {                                                               \
        if (!(cond)) {                                                 \
            if (g_fail++ < 20) {                                       \
                fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
                fprintf(stderr, __VA_ARGS__);                          \
                fprintf(stderr, "\n");                                 \
            }                                                          \
        }                                                              \
    } while (0)

static int is_nan16(uint16_t h) { return (h & 0x7c00) == 0x7c00 && (h & 0x3ff); }

int main(void)
{
    /* half -> float is exact: the value is sign * m * 2^(e - 25) (normal: m
     * has the hidden bit), computed here with ldexp */
    for (uint32_t h = 0; h < 65536; h++) {
        const float f = mxh_half_to_float((uint16_t)h);
        const int e = (h >> 10) & 0x1f, m = h & 0x3ff;
        if (e == 0x1f) {
            CHECK(m ? isnan(f) : (isinf(f) && (f < 0) == !!(h & 0x8000)), "pattern %#x", h);
            if (m) continue;
        } else {
            const double v = e ? ldexp((double)(m | 0x400), e - 25) : ldexp((double)m, -24);
            CHECK((double)f == ((h & 0x8000) ? -v : v) && !!signbit(f) == !!(h & 0x8000), "pattern %#x", h);
        }
        CHECK(mxh_float_to_half(f) == h, "round trip of %#x gives %#x", h, mxh_float_to_half(f));
    }
    /* float -> half rounds to nearest, ties to even: between neighbours lo <
     * hi, everything below the midpoint gives lo, above it hi, the midpoint
     * the one with the even significand; past the largest value, infinity */
    for (uint32_t h = 0; h < 0x7c00; h++) {
        const double lo = mxh_half_to_float((uint16_t)h);
        const double hi = h + 1 < 0x7c00 ? mxh_half_to_float((uint16_t)(h + 1)) : 65536.0;
        const float mid = (float)((lo + hi) / 2);      /* exact: 12 significand bits */
        const uint16_t even = (h & 1) ? (uint16_t)(h + 1) : (uint16_t)h;
        CHECK(mxh_float_to_half(mid) == even, "tie above %#x gives %#x", h, mxh_float_to_half(mid));
        CHECK(mxh_float_to_half(nextafterf(mid, 0.0f)) == h, "below the tie above %#x", h);
        CHECK(mxh_float_to_half(nextafterf(mid, 1e30f)) == h + 1, "above the tie above %#x", h);
        CHECK(mxh_float_to_half(-mid) == (even | 0x8000), "negative tie above %#x", h);
    }
    CHECK(mxh_float_to_half(1e30f) == 0x7c00 && mxh_float_to_half(-1e30f) == 0xfc00, "overflow");
    CHECK(mxh_float_to_half(1e-30f) == 0 && mxh_float_to_half(-1e-30f) == 0x8000, "underflow");
    CHECK(is_nan16(mxh_float_to_half(NAN)), "NaN");

    /* the base functions on exact-size heap blocks, 2- and 3-buffer form */
    const int pairs[6][2] = {{1, 14}, {2, 14}, {3, 14}, {4, 14}, {3, 26}, {4, 26}};
    const size_t counts[4] = {0, 1, 7, 1000};
    uint32_t s = 12345;
    for (int p = 0; p < 6; p++)
        for (int c = 0; c < 4; c++) {
            const size_t n = counts[c], w = pairs[p][1] == 26 ? 2 : 1, nb = n * w * sizeof(uint16_t);
            uint16_t *a = malloc(nb ? nb : 1), *b = malloc(nb ? nb : 1), *o = malloc(nb ? nb : 1);
            for (size_t i = 0; i < n * w; i++) {
                s = s * 1664525u + 1013904223u;
                a[i] = (uint16_t)(s >> 16);
                s = s * 1664525u + 1013904223u;
                b[i] = (uint16_t)(s >> 16);
            }
            CHECK(mxh_short_float_reduce(pairs[p][0], pairs[p][1], a, b, o, n) == 0, "3-buffer rc");
            if (pairs[p][0] <= 2)   /* MAX / MIN give one of the operands, bit for bit */
                for (size_t i = 0; i < n; i++) CHECK(o[i] == a[i] || o[i] == b[i], "select");
            CHECK(mxh_short_float_reduce(pairs[p][0], pairs[p][1], a, NULL, b, n) == 0, "2-buffer rc");
            free(a);
            free(b);
            free(o);
        }
    CHECK(mxh_short_float_reduce(6, 14, NULL, NULL, NULL, 0) == -1, "BAND has no binary16 slot");
    /* the distinguishing complex product */
    {
        const uint16_t a[2] = {0x3c01, 0x4203}, b[2] = {0x3bff, 0xc101};
        uint16_t o[2];
        mxh_short_float_reduce(4, 26, a, b, o, 1);
        CHECK(o[0] == 0x4842 && o[1] == 0x3800, "complex product %#x %#x", o[0], o[1]);
    }
    printf("half_check: %d failures\n", g_fail);
    return g_fail ? 1 : 0;
}
