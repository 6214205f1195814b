/* lchd_strain_sum.h -- the strain derivative W of a native gradient call as six exact sums (host + device, C99 / C++ / HIP from one text).
 *
 * W[i][j] = sum over the used slots of step_i * disp_j, i <= j, with step_c = coef * disp_c and coef = (v * g) / dist: the rule of
 * include/loco_hd_hip.h ("native coordinate gradients", "the strain derivative").  Every product is one IEEE float64 operation (the
 * translation unit is built without contraction).  The six sums of a side live in LCHD_STRAIN_COMPONENTS accumulators of lchd_exact_sum.h,
 * component order (0,0) (0,1) (0,2) (1,1) (1,2) (2,2).
 *
 *   lchd_strain_terms      the six terms of one slot
 *   lchd_strain_part_add   partial sums += the chunks of one term: no memory is touched, the partial sums are plain integers (on the
 *                          device: registers of one lane).  A partial sum takes 2^31 terms, as a limb of lchd_exact_sum.h does.
 *   lchd_strain_slot       one slot of a list into the partial sums; returns 0 if a term was out of range (that term adds nothing)
 *   lchd_strain_finish     the six sums rounded once into the symmetric double[9]; the limbs are read, not changed
 */
#ifndef LCHD_STRAIN_SUM_H
#define LCHD_STRAIN_SUM_H

#include "lchd_exact_sum.h"

#define LCHD_STRAIN_COMPONENTS 6
#define LCHD_STRAIN_LIMBS (LCHD_STRAIN_COMPONENTS * LCHD_GRAD_LIMBS)

/* component of W[i][j], i <= j */
LCHD_XS_FN int lchd_strain_component(int i, int j) { return i == 0 ? j : (i == 1 ? 2 + j : 5); }

LCHD_XS_FN void lchd_strain_terms(double coef, const double *disp, double *term) {
    const double s0 = coef * disp[0], s1 = coef * disp[1], s2 = coef * disp[2];
    term[0] = s0 * disp[0];
    term[1] = s0 * disp[1];
    term[2] = s0 * disp[2];
    term[3] = s1 * disp[1];
    term[4] = s1 * disp[2];
    term[5] = s2 * disp[2];
}

/* selects, no indexed access to `limb` once the loop is unrolled */
LCHD_XS_FN void lchd_strain_part_add(int64_t *limb, const lchd_xs_parts r) {
    int k;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (k = 0; k < LCHD_GRAD_LIMBS; ++k) {
        const int j = k - r.first;
        const uint32_t c = j == 0 ? r.chunk[0] : (j == 1 ? r.chunk[1] : (j == 2 ? r.chunk[2] : 0u));
        limb[k] += r.negative ? -(int64_t)c : (int64_t)c;
    }
}

/* the use rule is the caller's; part: [LCHD_STRAIN_COMPONENTS][LCHD_GRAD_LIMBS] */
LCHD_XS_FN int lchd_strain_slot(int64_t (*part)[LCHD_GRAD_LIMBS], double v, double g, double dist, const double *disp) {
    double term[LCHD_STRAIN_COMPONENTS];
    int c, ok = 1;
    lchd_strain_terms((v * g) / dist, disp, term);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (c = 0; c < LCHD_STRAIN_COMPONENTS; ++c) {
        const lchd_xs_parts r = lchd_xs_split(term[c]);
        if (!r.ok) {
            ok = 0;
            continue;
        }
        lchd_strain_part_add(part[c], r);
    }
    return ok;
}

LCHD_XS_FN void lchd_strain_finish(const int64_t *limbs, double *w) {
    int i, j;
    for (i = 0; i < 3; ++i)
        for (j = i; j < 3; ++j) w[3 * i + j] = w[3 * j + i] = lchd_xs_finish(limbs + lchd_strain_component(i, j) * LCHD_GRAD_LIMBS);
}

#endif /* LCHD_STRAIN_SUM_H */
