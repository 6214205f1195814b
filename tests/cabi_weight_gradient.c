/* A plain-C client of the host leaf of the weight-function gradient, lchd_wf_cdf_grad, and of the width query, through
 * include/loco_hd_hip.h alone; needs no GPU.  Checks by itself what needs no reference: the closed form of uniform [3, 10], the zeros at
 * +inf and outside the support, the Euler identity of hyper_exp, finite outputs for a steep kumaraswamy, the error paths, and that
 * lchd_weight_gradient_width is 0 without a context.  Prints every table as hexadecimal floating-point numbers (exact bits) for
 * tests/test_cabi_weight_gradient.py.  The wrapper builds it with -fsanitize=address,undefined as well. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "loco_hd_hip.h"

#define CHECK(call)                                                          \
    do {                                                                     \
        int rc_ = (call);                                                    \
        if (rc_ != LCHD_OK) {                                                \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, lchd_last_error()); \
            return 1;                                                        \
        }                                                                    \
    } while (0)
#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); return 1; } while (0)

enum { NX = 9 };

static int table(const char *name, int32_t kind, const double *params, int32_t np, const double *x, double *out) {
    CHECK(lchd_wf_cdf_grad(kind, params, np, x, NX, out));
    for (int i = 0; i < NX; ++i) {
        printf("%s %d", name, i);
        for (int k = 0; k < np; ++k) {
            if (!isfinite(out[i * np + k])) FAIL("%s: x = %g, parameter %d is not finite\n", name, x[i], k);
            printf(" %a", out[i * np + k]);
        }
        printf("\n");
    }
    for (int k = 0; k < np; ++k)
        if (out[(NX - 1) * np + k] != 0.0) FAIL("%s: not 0 at +inf\n", name);
    return 0;
}

int main(void) {
    const double x[NX] = {0.0, 1.0, 2.0, 3.0, 6.5, 10.0, 11.0, 12.5, INFINITY};
    /* exactly-sized heap blocks: an access past n_params * NX doubles is the sanitizer's to find */
    double *out = malloc(sizeof(double) * NX * 4);
    if (!out) return 1;

    const double uni[2] = {3.0, 10.0};
    if (table("uniform", LCHD_WF_UNIFORM, uni, 2, x, out)) return 1;
    if (out[2 * 4 + 0] != (6.5 - 10.0) / 49.0 || out[2 * 4 + 1] != -(6.5 - 3.0) / 49.0) FAIL("uniform at 6.5: %g %g\n", out[8], out[9]);
    for (int i = 0; i < NX; ++i)
        if ((x[i] < 3.0 || x[i] > 10.0) && (out[2 * i] != 0.0 || out[2 * i + 1] != 0.0)) FAIL("uniform outside the support at %g\n", x[i]);

    const double kum[4] = {2.0, 11.0, 0.5, 0.5}; /* alpha, beta < 1: infinite limits on both bounds, 0 by convention */
    if (table("kumaraswamy", LCHD_WF_KUMARASWAMY, kum, 4, x, out)) return 1;
    const double dag[3] = {4.0, 6.0, 1.5};
    if (table("dagum", LCHD_WF_DAGUM, dag, 3, x, out)) return 1;
    if (out[0] != 0.0 || out[1] != 0.0 || out[2] != 0.0) FAIL("dagum at 0\n");
    const double hyp[4] = {1.0, 0.5, 0.2, 0.05};
    if (table("hyper_exp", LCHD_WF_HYPER_EXP, hyp, 4, x, out)) return 1;
    for (int i = 0; i < NX; ++i) {
        const double euler = hyp[0] * out[4 * i] + hyp[1] * out[4 * i + 1];
        if (!(fabs(euler) <= 1e-15)) FAIL("hyper_exp at %g: sum_i a_i dF/da_i = %g\n", x[i], euler);
    }
    free(out);

    /* one point, one block of exactly n_params doubles */
    double *one = malloc(sizeof(double) * 3);
    const double at = 7.0;
    if (!one) return 1;
    CHECK(lchd_wf_cdf_grad(LCHD_WF_DAGUM, dag, 3, &at, 1, one));
    free(one);

    /* error paths: a negative point, invalid parameters, null pointers; nothing is read or written with n = 0 */
    const double neg = -1.0, bad[2] = {10.0, 3.0};
    double sink[2];
    if (lchd_wf_cdf_grad(LCHD_WF_UNIFORM, uni, 2, &neg, 1, sink) != LCHD_EVALUE) FAIL("a negative point was taken\n");
    if (lchd_wf_cdf_grad(LCHD_WF_UNIFORM, bad, 2, &at, 1, sink) != LCHD_EVALUE) FAIL("a > b was taken\n");
    if (lchd_wf_cdf_grad(LCHD_WF_UNIFORM, uni, 2, NULL, 1, sink) != LCHD_EVALUE) FAIL("a null x was taken\n");
    CHECK(lchd_wf_cdf_grad(LCHD_WF_UNIFORM, uni, 2, NULL, 0, NULL));
    if (lchd_weight_gradient_width(NULL) != 0) FAIL("a width without a context\n");

    printf("cabi weight gradient ok\n");
    return 0;
}
