/* A plain-C client of the category-weight gradient entry points of include/loco_hd_hip.h that take host arrays: one thresholded call
 * (lchd_category_gradient_primitives) and one dense call (lchd_category_gradient_coords) on 48 atoms, through the header alone.  Checks
 * by itself what needs no reference: sum_c w_c G[p][c] = 0 to 1e-12 for every row, the error paths.  Prints every table as hexadecimal
 * floating-point numbers (exact bits) for tests/test_cabi_category_gradient.py. */
#include <math.h>
#include <stdio.h>

#include "loco_hd_hip.h"

#define CHECK(call)                                                          \
    do {                                                                     \
        int rc_ = (call);                                                    \
        if (rc_ != LCHD_OK) {                                                \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, lchd_last_error()); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

enum { N = 48, NP = 20, C = 5 };

static int print_table(const char *name, const double *t, const double *w, int rows) {
    for (int r = 0; r < rows; ++r) {
        double euler = 0.0;
        printf("%s %d", name, r);
        for (int k = 0; k < C; ++k) {
            printf(" %a", t[r * C + k]);
            euler += w[k] * t[r * C + k];
        }
        printf("\n");
        if (!(fabs(euler) <= 1e-12)) { fprintf(stderr, "%s row %d: sum_c w_c G_c = %g\n", name, r, euler); return 1; }
    }
    return 0;
}

int main(void) {
    lchd_ctx *ctx = NULL;
    CHECK(lchd_ctx_create(-1, &ctx));

    double wf_params[2] = {3.0, 10.0};
    lchd_weight_function wf = {LCHD_WF_UNIFORM, 2, wf_params};
    double weights[C] = {1.0, 2.0, 0.5, 1.0, 1.5};
    lchd_config cfg = {0};
    cfg.n_categories = C;
    cfg.category_weights = weights;
    cfg.n_weight_functions = 1;
    cfg.weight_functions = &wf;
    cfg.sd_kind = LCHD_SD_HELLINGER;
    cfg.sd_n_params = 1;
    cfg.sd_params[0] = 2.0;
    cfg.tag_mode = 0;
    cfg.tag_accept_same = 1;

    double xa[N][3], xb[N][3];
    static double tab[N * C];
    int32_t cat_a[N], cat_b[N], tag[N];
    int64_t anchors[NP][2];
    for (int i = 0; i < N; ++i) {
        xa[i][0] = fmod(7.31 * i, 11.0) + 0.5; xa[i][1] = fmod(3.77 * i, 11.0) + 0.5; xa[i][2] = fmod(5.13 * i, 11.0) + 0.5;
        xb[i][0] = fmod(2.91 * i, 11.0) + 0.5; xb[i][1] = fmod(6.43 * i, 11.0) + 0.5; xb[i][2] = fmod(4.57 * i, 11.0) + 0.5;
        cat_a[i] = (3 * i + 1) % C;
        cat_b[i] = (2 * i + 3) % C;
        tag[i] = i % 3;
    }
    for (int k = 0; k < NP; ++k) { anchors[k][0] = (7 * k) % N; anchors[k][1] = (11 * k + 5) % N; }

    for (int pass = 0; pass < 2; ++pass) { /* Hellinger 2, then Kullback-Leibler 1e-3 */
        const char *names[2][2] = {{"prims", "coords"}, {"prims_kl", "coords_kl"}};
        cfg.sd_kind = pass ? LCHD_SD_KULLBACK_LEIBLER : LCHD_SD_HELLINGER;
        cfg.sd_params[0] = pass ? 1e-3 : 2.0;
        CHECK(lchd_category_gradient_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 6.5, NULL,
                                                NULL, NULL, NULL, tab));
        if (print_table(names[pass][0], tab, weights, NP)) return 2;
        CHECK(lchd_category_gradient_coords(ctx, &cfg, cat_a, N, cat_b, N, &xa[0][0], N, &xb[0][0], N, NULL, NULL, NULL, tab));
        if (print_table(names[pass][1], tab, weights, N)) return 2;
    }

    /* error paths: a distance without a gradient, an anchor outside its structure */
    cfg.sd_kind = LCHD_SD_KOLMOGOROV_SMIRNOV;
    cfg.sd_n_params = 0;
    if (lchd_category_gradient_coords(ctx, &cfg, cat_a, N, cat_b, N, &xa[0][0], N, &xb[0][0], N, NULL, NULL, NULL, tab) != LCHD_EUNSUPPORTED ||
        lchd_category_gradient_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 6.5, NULL, NULL,
                                          NULL, NULL, tab) != LCHD_EUNSUPPORTED) {
        fprintf(stderr, "expected LCHD_EUNSUPPORTED under Kolmogorov-Smirnov\n");
        return 3;
    }
    cfg.sd_kind = LCHD_SD_HELLINGER;
    cfg.sd_n_params = 1;
    cfg.sd_params[0] = 2.0;
    anchors[3][1] = N;
    if (lchd_category_gradient_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 6.5, NULL, NULL,
                                          NULL, NULL, tab) != LCHD_EPANIC) {
        fprintf(stderr, "expected LCHD_EPANIC for an anchor outside the structure\n");
        return 5;
    }

    lchd_ctx_destroy(ctx);
    printf("cabi category gradient ok\n");
    return 0;
}
