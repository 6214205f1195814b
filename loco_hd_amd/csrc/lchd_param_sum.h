/* lchd_param_sum.h -- reduced parameter gradients: out[b][k] = sum_p v_p row[p][k] over the rows of a per-pair parameter-gradient call,
 * as exact sums (host + device, C99 / C++ / HIP from one text).
 *
 * The rule of include/loco_hd_hip.h ("reduced parameter gradients"), in IEEE float64 with no contraction:
 *     use    = !isnan(row[p][0])          (an unusable pair's row is NaN in every column)
 *     term_k = v_p * row[p][k]            (one multiplication; v_p = 1.0 without pair weights)
 *     acc[b][k] += term_k                 exact (lchd_exact_sum.h), b = the pair's bucket
 *     out[b][k] = lchd_xs_finish(acc[b][k])
 *
 *   lchd_param_use        the use test on a row's first column
 *   lchd_param_slot       one (row, column) into the column's partial sums: no memory is touched, the partial sums are plain integers (on
 *                         the device: registers of one lane).  A partial sum takes 2^31 terms, as a limb of lchd_exact_sum.h does.
 *                         Returns 0 if the term was out of range (it adds nothing).
 *   lchd_param_sum_rows   the host path: n rows of w columns (leading dimension ld) into acc[n_buckets][w][LCHD_GRAD_LIMBS]
 *   lchd_param_finish     every accumulator rounded once; the limbs are read, not changed
 */
#ifndef LCHD_PARAM_SUM_H
#define LCHD_PARAM_SUM_H

#include "lchd_exact_sum.h"
#include "lchd_strain_sum.h"

LCHD_XS_FN int lchd_param_use(double row0) { return row0 == row0; }

LCHD_XS_FN int lchd_param_slot(int64_t *part, double v, double x) {
    const lchd_xs_parts r = lchd_xs_split(v * x);
    if (!r.ok) return 0;
    lchd_strain_part_add(part, r);
    return 1;
}

/* rows: [n][ld], the first w columns of a row are its terms; v: [n] or NULL; bucket: [n] or NULL (bucket 0).  A usable row whose bucket
 * lies outside 0 .. n_buckets - 1 is skipped (the per-pair call gives such a pair a NaN row).  Returns 0 if a term was out of range. */
LCHD_XS_FN int lchd_param_sum_rows(const double *rows, int64_t n, int w, int64_t ld, const double *v, const int32_t *bucket, int n_buckets,
                                   int64_t *acc) {
    int64_t p;
    int k, ok = 1;
    for (p = 0; p < n; ++p) {
        const double *row = rows + p * ld;
        const int b = bucket ? bucket[p] : 0;
        if (!lchd_param_use(row[0]) || b < 0 || b >= n_buckets) continue;
        for (k = 0; k < w; ++k)
            if (!lchd_param_slot(acc + ((int64_t)b * w + k) * LCHD_GRAD_LIMBS, v ? v[p] : 1.0, row[k])) ok = 0;
    }
    return ok;
}

LCHD_XS_FN void lchd_param_finish(const int64_t *acc, int64_t n, double *out) {
    int64_t i;
    for (i = 0; i < n; ++i) out[i] = lchd_xs_finish(acc + i * LCHD_GRAD_LIMBS);
}

#endif /* LCHD_PARAM_SUM_H */
