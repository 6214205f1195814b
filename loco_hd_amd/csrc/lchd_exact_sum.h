/* lchd_exact_sum.h -- an exact, order-free sum of doubles as a signed fixed-point number (host + device, C99 / C++ / HIP from one text).
 *
 * One sum lives in LCHD_GRAD_LIMBS = 8 little-endian limbs of int64.  Limb k carries the 32-bit chunk of weight 2^(32 k - 192) of every
 * value added; the upper bits of a limb are headroom, so up to 2^31 values are added without carry propagation.  The unit of the number
 * is the quantum q = 2^LCHD_GRAD_QUANTUM_LOG2 = 2^-192, and a value must be smaller than 2^LCHD_GRAD_LIMIT_LOG2 = 2^63 in magnitude.
 *
 *   lchd_xs_add(limbs, s, flag)   t = trunc(s / q) toward zero; the (at most three) non-zero 32-bit chunks of |t| go, with the sign of
 *                                 s, to their limbs -- one 64-bit integer add each (device: one atomic add without a return value).
 *                                 Integer addition is associative: the limbs after any number of adds do not depend on their order.
 *                                 A non-finite s or |s| >= 2^63 adds nothing and ORs LCHD_XS_OUT_OF_RANGE into *flag.
 *   lchd_xs_add_parts(limbs, r)   the adds of lchd_xs_add for a value already split (lchd_xs_split, r.ok): for a caller that ORs the flag itself.
 *   lchd_xs_finish(limbs)         propagates the carries and returns THE correctly rounded (to nearest, ties to even) double of
 *                                 q * sum t; a sum of exactly 0 is +0.0.
 *
 * A double below 2^63 has its lowest bit at 2^-1074 at the least; everything below q = 2^-192 is cut off (toward zero) by the add.
 * For a value with no bits below q the add is exact, and the finished sum is then the correctly rounded exact sum (math.fsum).
 */
#ifndef LCHD_EXACT_SUM_H
#define LCHD_EXACT_SUM_H

#include <stdint.h>
#include <string.h>

#ifndef LCHD_GRAD_LIMBS
#define LCHD_GRAD_LIMBS 8
#define LCHD_GRAD_QUANTUM_LOG2 (-192)
#define LCHD_GRAD_LIMIT_LOG2 63
#endif
#define LCHD_XS_OUT_OF_RANGE 1u

#if defined(__HIPCC__)
#define LCHD_XS_FN __host__ __device__ static inline
#else
#define LCHD_XS_FN static inline
#endif

/* One value cut into chunks: chunk[j] (32 bits each) belongs to limb first + j; limbs beyond LCHD_GRAD_LIMBS - 1 only ever get a zero
 * chunk (|s| < 2^63).  negative: the sign of s.  ok == 0: s is not finite or too large, nothing is to be added. */
typedef struct lchd_xs_parts {
    uint32_t chunk[3];
    int32_t first;
    int32_t negative;
    int32_t ok;
} lchd_xs_parts;

LCHD_XS_FN lchd_xs_parts lchd_xs_split(double s) {
    lchd_xs_parts r;
    uint64_t bits;
    memcpy(&bits, &s, 8);
    const int ef = (int)((bits >> 52) & 0x7FF);
    uint64_t m = bits & 0xFFFFFFFFFFFFFull;
    r.negative = (int32_t)(bits >> 63);
    r.first = 0;
    r.chunk[0] = r.chunk[1] = r.chunk[2] = 0u;
    /* |s| = m 2^e; finite and below 2^63: the exponent field is at most 1023 + 62 */
    r.ok = ef <= 1023 + LCHD_GRAD_LIMIT_LOG2 - 1;
    if (!r.ok || ef == 0) return r; /* (a subnormal is far below q: t = 0) */
    m |= (uint64_t)1 << 52;
    const int sh = ef - 1075 - LCHD_GRAD_QUANTUM_LOG2; /* t = m 2^sh, cut off below bit 0 */
    int o = 0;
    if (sh < 0) {
        if (sh <= -53) return r;
        m >>= -sh;
    } else {
        r.first = sh >> 5;
        o = sh & 31;
    }
    r.chunk[0] = (uint32_t)(m << o);
    r.chunk[1] = (uint32_t)(m >> (32 - o));
    r.chunk[2] = o ? (uint32_t)(m >> (64 - o)) : 0u;
    return r;
}

/* limb += v: the one place that touches memory.  Device: a 64-bit integer atomic add at agent scope, no return value. */
LCHD_XS_FN void lchd_xs_limb_add(int64_t *limb, int64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)__hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(limb), (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    *limb = (int64_t)((uint64_t)*limb + (uint64_t)v);
#endif
}
LCHD_XS_FN void lchd_xs_flag_or(uint32_t *flag, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)__hip_atomic_fetch_or(flag, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    *flag |= v;
#endif
}

/* limbs += the chunks of one split value (r.ok): at most three limb adds, zero chunks skipped.  For a caller that raises the flag itself. */
LCHD_XS_FN void lchd_xs_add_parts(int64_t *limbs, const lchd_xs_parts r) {
    int j;
    for (j = 0; j < 3; ++j) {
        const int k = r.first + j;
        if (r.chunk[j] && k < LCHD_GRAD_LIMBS) lchd_xs_limb_add(limbs + k, r.negative ? -(int64_t)r.chunk[j] : (int64_t)r.chunk[j]);
    }
}

LCHD_XS_FN void lchd_xs_add(int64_t *limbs, double s, uint32_t *flag) {
    const lchd_xs_parts r = lchd_xs_split(s);
    if (!r.ok) {
        lchd_xs_flag_or(flag, LCHD_XS_OUT_OF_RANGE);
        return;
    }
    lchd_xs_add_parts(limbs, r);
}

/* The correctly rounded double of q * (sum of the limbs' chunks); the limbs are read, not changed. */
LCHD_XS_FN double lchd_xs_finish(const int64_t *limbs) {
    /* the sum as sign and magnitude in 32-bit words: 8 chunks, the 64 bits of the last carry, two words of zero padding */
    uint32_t w[LCHD_GRAD_LIMBS + 4];
    int64_t carry = 0;
    int k, h = -1, negative;
    for (k = 0; k < LCHD_GRAD_LIMBS; ++k) {
        const uint64_t v = (uint64_t)limbs[k] + (uint64_t)carry; /* (|limb| <= 2^62 and |carry| < 2^31: no overflow) */
        w[k] = (uint32_t)v;
        carry = (int64_t)v >> 32; /* arithmetic shift: floor */
    }
    w[LCHD_GRAD_LIMBS] = (uint32_t)(uint64_t)carry;
    w[LCHD_GRAD_LIMBS + 1] = (uint32_t)((uint64_t)carry >> 32);
    w[LCHD_GRAD_LIMBS + 2] = w[LCHD_GRAD_LIMBS + 3] = 0u;
    negative = carry < 0;
    if (negative) { /* two's complement over the ten words */
        uint64_t c = 1;
        for (k = 0; k < LCHD_GRAD_LIMBS + 2; ++k) {
            c += (uint64_t)(uint32_t)~w[k];
            w[k] = (uint32_t)c;
            c >>= 32;
        }
    }
    for (k = LCHD_GRAD_LIMBS + 1; k >= 0 && h < 0; --k)
        if (w[k]) {
            int b = 31;
            while (!((w[k] >> b) & 1u)) --b;
            h = 32 * k + b;
        }
    if (h < 0) return 0.0;
    /* the 53 bits from the highest set bit down, then round to nearest, ties to even, on what lies below them */
    const int low = h > 52 ? h - 52 : 0;
    const int wi = low >> 5, o = low & 31;
    const uint64_t lo64 = (uint64_t)w[wi] | (uint64_t)w[wi + 1] << 32;
    uint64_t mant = ((lo64 >> o) | (o ? (uint64_t)w[wi + 2] << (64 - o) : 0)) & (((uint64_t)1 << 53) - 1);
    if (low > 0) {
        const int rb = low - 1;
        const int round = (int)((w[rb >> 5] >> (rb & 31)) & 1u);
        int sticky = (w[rb >> 5] & (((uint32_t)1 << (rb & 31)) - 1u)) != 0u;
        for (k = 0; k < (rb >> 5); ++k) sticky |= w[k] != 0u;
        if (round && (sticky || (mant & 1))) ++mant; /* (2^53 is a double too) */
    }
    /* mant 2^(low - 192): both factors are exact doubles and so is the product (its exponent is far inside the normal range) */
    const uint64_t scale_bits = (uint64_t)(1023 + low + LCHD_GRAD_QUANTUM_LOG2) << 52;
    double scale;
    memcpy(&scale, &scale_bits, 8);
    const double r = (double)mant * scale;
    return negative ? -r : r;
}

#endif /* LCHD_EXACT_SUM_H */
