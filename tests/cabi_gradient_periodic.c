/* A plain-C client of the periodic native gradient entry points of include/loco_hd_hip.h: lchd_gradient_primitives_periodic (40 atoms a
 * side in a box against a triclinic cell, 12 anchor pairs with weights, tile_pairs 0 and 5, with and without strain) and
 * lchd_gradient_coords_periodic (dense rows, a triclinic cell against an open side), lchd_gradient_plan_periodic and the argument errors.
 * The expected values are made here: the lists of lchd_sensitivity_primitives_periodic / lchd_sensitivity_coords_periodic on the same
 * inputs, reduced by the header's rule in long double.  A float64 term carries at most three roundings against the long double one, the
 * exact sum one more, so every output must lie within 8 DBL_EPSILON of the largest sum of |terms| of its array.  Both strain tensors
 * must be symmetric in every bit, the scores the sensitivity call's in every bit.  No HIP call is made from here. */
#include <float.h>
#include <inttypes.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

enum { N = 40, NP = 12, C = 5, K = 256 };

/* One side's lists reduced in long double: grad [n][3], W [3][3] (full, no mirroring), and the largest sum of |terms| of either array.
 * dense: the anchor of row p is atom p, else idx[p][0]. */
static long double reduce(int n_pairs, int width, int n_atoms, int dense, const double *v, const int32_t *idx, const double *dist, const double *g,
                          const double *disp, long double *grad, long double *w) {
    long double *mag = calloc((size_t)3 * n_atoms + 9, sizeof *mag), most = 0.0L;
    if (!mag) return -1.0L;
    for (int i = 0; i < 3 * n_atoms; ++i) grad[i] = 0.0L;
    for (int i = 0; i < 9; ++i) w[i] = 0.0L;
    for (int p = 0; p < n_pairs; ++p) {
        const int a = dense ? p : idx[(size_t)p * width];
        for (int k = 1; k < width; ++k) {
            const size_t s = (size_t)p * width + k;
            const int m = idx[s];
            if (m < 0 || !(dist[s] > 0.0) || !isfinite(g[s])) continue;
            const long double coef = (long double)v[p] * g[s] / dist[s];
            for (int c = 0; c < 3; ++c) {
                const long double step = coef * disp[3 * s + c];
                grad[3 * m + c] += step;
                grad[3 * a + c] -= step;
                mag[3 * m + c] += fabsl(step);
                mag[3 * a + c] += fabsl(step);
                for (int j = 0; j < 3; ++j) {
                    w[3 * c + j] += step * disp[3 * s + j];
                    mag[3 * n_atoms + 3 * c + j] += fabsl(step * disp[3 * s + j]);
                }
            }
        }
    }
    for (int i = 0; i < 3 * n_atoms + 9; ++i) most = mag[i] > most ? mag[i] : most;
    free(mag);
    return most;
}

static int close_to(const char *what, const double *got, const long double *want, int n, long double scale) {
    const long double tol = 8.0L * DBL_EPSILON * scale;
    for (int i = 0; i < n; ++i)
        if (!(fabsl((long double)got[i] - want[i]) <= tol))
            FAIL("%s: element %d is %.17g, the long double sum %.21Lg (tolerance %.3Lg)\n", what, i, got[i], want[i], tol);
    return 0;
}
static int symmetric(const char *what, const double *w) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < i; ++j)
            if (memcmp(&w[3 * i + j], &w[3 * j + i], 8)) FAIL("%s: W[%d][%d] and W[%d][%d] differ in their bits\n", what, i, j, j, i);
    return 0;
}
static int same_bits(const char *what, const double *x, const double *y, int n) {
    if (memcmp(x, y, sizeof(double) * (size_t)n)) FAIL("%s: the bits differ\n", what);
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

    static double xa[N][3], xb[N][3], v[NP], vd[N];
    static int32_t cat_a[N], cat_b[N], tag[N];
    static int64_t anchors[NP][2];
    double box[3] = {13.0, 11.5, 12.25};
    double cell[9] = {14.0, 0.0, 0.0, 3.5, 12.0, 0.0, -2.0, 4.0, 13.0}; /* perpendicular widths above the threshold of 10 */
    for (int i = 0; i < N; ++i) {
        xa[i][0] = fmod(7.31 * i, 9.0) + 0.5; xa[i][1] = fmod(3.77 * i, 9.0) + 0.5; xa[i][2] = fmod(5.13 * i, 9.0) + 0.5;
        xb[i][0] = fmod(2.91 * i, 9.0) + 0.5; xb[i][1] = fmod(6.43 * i, 9.0) + 0.5; xb[i][2] = fmod(4.57 * i, 9.0) + 0.5;
        cat_a[i] = (3 * i + 1) % C;
        cat_b[i] = (2 * i + 3) % C;
        tag[i] = 0;
        vd[i] = 0.75 + 0.03125 * i;
    }
    for (int k = 0; k < NP; ++k) { anchors[k][0] = (7 * k) % N; anchors[k][1] = (11 * k + 5) % N; v[k] = 0.5 + 0.125 * k; }

    /* the plan: rows of 88 width + 16 bytes with displacements, 8 ceil(width / 4) more with image codes; the slot rule; bad modes */
    int64_t tile = -1;
    CHECK(lchd_gradient_plan_periodic(NP, 128, LCHD_GRAD_MIN_IMAGE, (int64_t)5 * (88 * 128 + 16), &tile));
    if (tile != 5) FAIL("lchd_gradient_plan_periodic (min image): %lld, expected 5\n", (long long)tile);
    CHECK(lchd_gradient_plan_periodic(NP, 128, LCHD_GRAD_IMAGES, (int64_t)5 * (88 * 128 + 16 + 8 * 32), &tile));
    if (tile != 5) FAIL("lchd_gradient_plan_periodic (images): %lld, expected 5\n", (long long)tile);
    if (lchd_gradient_plan_periodic(NP, 128, 3, 1000, &tile) != LCHD_EVALUE || tile != 0) FAIL("a plan with resolve 3 accepted\n");
    if (lchd_gradient_plan_periodic((int64_t)1 << 24, 128, LCHD_GRAD_IMAGES, 1000, &tile) != LCHD_EUNSUPPORTED) FAIL("2^31 slots planned\n");

    /* ---- thresholded: side A in a box, side B in a triclinic cell ---- */
    static double s_scores[NP], s_dist[2][NP * K], s_g[2][NP * K], s_disp[2][NP * K * 3];
    static int32_t s_count[2][NP], s_idx[2][NP * K];
    static int8_t s_image[2][NP * K];
    CHECK(lchd_sensitivity_primitives_periodic(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 10.0, K, box,
                                               NULL, NULL, cell, s_scores, s_count[0], s_idx[0], s_image[0], s_dist[0], s_g[0], s_disp[0],
                                               s_count[1], s_idx[1], s_image[1], s_dist[1], s_g[1], s_disp[1]));
    static long double want_g[2][3 * N], want_w[2][9];
    long double scale[2];
    int images = 0;
    for (int k = 0; k < 2; ++k) {
        scale[k] = reduce(NP, K, N, 0, v, s_idx[k], s_dist[k], s_g[k], s_disp[k], want_g[k], want_w[k]);
        if (!(scale[k] > 0.0L)) FAIL("side %d of the thresholded case has no term\n", k);
        for (int i = 0; i < NP * K; ++i) images += s_image[k][i] != 0;
    }
    if (!images) FAIL("no member of the thresholded case arrives through an image\n");

    static double scores[NP], ga[N][3], gb[N][3], wa[9], wb[9], scores2[NP], ga2[N][3], gb2[N][3], wa2[9], wb2[9];
    CHECK(lchd_gradient_primitives_periodic(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 10.0, box, NULL,
                                            NULL, cell, v, 0, scores, &ga[0][0], &gb[0][0], wa, wb));
    if (same_bits("thresholded: scores", scores, s_scores, NP)) return 1;
    if (close_to("thresholded: grad_a", &ga[0][0], want_g[0], 3 * N, scale[0]) || close_to("thresholded: grad_b", &gb[0][0], want_g[1], 3 * N, scale[1]) ||
        close_to("thresholded: strain_a", wa, want_w[0], 9, scale[0]) || close_to("thresholded: strain_b", wb, want_w[1], 9, scale[1]))
        return 1;
    if (symmetric("thresholded: strain_a", wa) || symmetric("thresholded: strain_b", wb)) return 1;
    if (wa[0] == 0.0 || wb[4] == 0.0) FAIL("a strain tensor of the thresholded case is empty\n");
    /* tiles of five pairs: the same bits; without strain: the same scores and gradients */
    CHECK(lchd_gradient_primitives_periodic(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 10.0, box, NULL,
                                            NULL, cell, v, 5, scores2, &ga2[0][0], &gb2[0][0], wa2, wb2));
    if (same_bits("tiles of 5: scores", scores2, scores, NP) || same_bits("tiles of 5: grad_a", &ga2[0][0], &ga[0][0], 3 * N) ||
        same_bits("tiles of 5: grad_b", &gb2[0][0], &gb[0][0], 3 * N) || same_bits("tiles of 5: strain_a", wa2, wa, 9) ||
        same_bits("tiles of 5: strain_b", wb2, wb, 9))
        return 1;
    memset(ga2, 0xFF, sizeof ga2); memset(gb2, 0xFF, sizeof gb2);
    CHECK(lchd_gradient_primitives_periodic(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 10.0, box, NULL,
                                            NULL, cell, v, 0, scores2, &ga2[0][0], &gb2[0][0], NULL, NULL));
    if (same_bits("no strain: grad_a", &ga2[0][0], &ga[0][0], 3 * N) || same_bits("no strain: grad_b", &gb2[0][0], &gb[0][0], 3 * N)) return 1;
    /* argument errors */
    if (lchd_gradient_primitives_periodic(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 10.0, box, NULL,
                                          NULL, cell, v, 0, scores2, &ga2[0][0], &gb2[0][0], wa2, NULL) != LCHD_EVALUE)
        FAIL("one strain pointer alone accepted\n");
    if (lchd_gradient_primitives_periodic(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 10.0, box, cell,
                                          NULL, NULL, v, 0, scores2, &ga2[0][0], &gb2[0][0], NULL, NULL) != LCHD_EVALUE)
        FAIL("a box and a cell on one side accepted\n");
    if (lchd_gradient_primitives_periodic(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 10.0, box, NULL,
                                          NULL, cell, v, -1, scores2, &ga2[0][0], &gb2[0][0], NULL, NULL) != LCHD_EVALUE)
        FAIL("tile_pairs -1 accepted\n");
    /* a weight that takes a term out of range fails behind valid scores; the next call is clean */
    v[3] = ldexp(1.0, 200);
    memset(scores2, 0xFF, sizeof scores2);
    if (lchd_gradient_primitives_periodic(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 10.0, box, NULL,
                                          NULL, cell, v, 0, scores2, &ga2[0][0], &gb2[0][0], wa2, wb2) != LCHD_EVALUE ||
        !strstr(lchd_last_error(), "gradient contribution not finite or >= 2^63"))
        FAIL("a weight of 2^200 did not fail as out of range: %s\n", lchd_last_error());
    if (same_bits("scores of the failed call", scores2, scores, NP)) return 1;
    v[3] = 0.5 + 0.125 * 3;
    CHECK(lchd_gradient_primitives_periodic(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 10.0, box, NULL,
                                            NULL, cell, v, 0, scores2, &ga2[0][0], &gb2[0][0], wa2, wb2));
    if (same_bits("after a failed call: grad_a", &ga2[0][0], &ga[0][0], 3 * N) || same_bits("after a failed call: strain_a", wa2, wa, 9) ||
        same_bits("after a failed call: strain_b", wb2, wb, 9))
        return 1;

    /* ---- dense rows: side A in the triclinic cell (minimum image), side B open ---- */
    static double d_scores[N], d_dist[2][N * N], d_g[2][N * N], d_disp[2][N * N * 3];
    static int32_t d_count[2][N], d_idx[2][N * N];
    CHECK(lchd_sensitivity_coords_periodic(ctx, &cfg, cat_a, N, cat_b, N, &xa[0][0], &xb[0][0], N, NULL, cell, NULL, N, d_scores, d_count[0], d_idx[0],
                                           d_dist[0], d_g[0], d_count[1], d_idx[1], d_dist[1], d_g[1], d_disp[0], d_disp[1]));
    for (int k = 0; k < 2; ++k) {
        scale[k] = reduce(N, N, N, 1, vd, d_idx[k], d_dist[k], d_g[k], d_disp[k], want_g[k], want_w[k]);
        if (!(scale[k] > 0.0L)) FAIL("side %d of the dense case has no term\n", k);
    }
    static double scores3[N];
    CHECK(lchd_gradient_coords_periodic(ctx, &cfg, cat_a, N, cat_b, N, &xa[0][0], &xb[0][0], N, NULL, cell, NULL, vd, scores3, &ga[0][0], &gb[0][0], wa,
                                        wb));
    if (same_bits("dense: scores", scores3, d_scores, N)) return 1;
    if (close_to("dense: grad_a", &ga[0][0], want_g[0], 3 * N, scale[0]) || close_to("dense: grad_b", &gb[0][0], want_g[1], 3 * N, scale[1]) ||
        close_to("dense: strain_a", wa, want_w[0], 9, scale[0]) || close_to("dense: strain_b", wb, want_w[1], 9, scale[1]))
        return 1;
    if (symmetric("dense: strain_a", wa) || symmetric("dense: strain_b", wb)) return 1;
    if (wa[0] == 0.0 || wb[0] == 0.0) FAIL("a strain tensor of the dense case is empty\n");
    CHECK(lchd_gradient_coords_periodic(ctx, &cfg, cat_a, N, cat_b, N, &xa[0][0], &xb[0][0], N, NULL, cell, NULL, vd, scores3, &ga2[0][0], &gb2[0][0],
                                        NULL, NULL));
    if (same_bits("dense, no strain: grad_a", &ga2[0][0], &ga[0][0], 3 * N) || same_bits("dense, no strain: grad_b", &gb2[0][0], &gb[0][0], 3 * N))
        return 1;
    if (lchd_gradient_coords_periodic(ctx, &cfg, cat_a, N, cat_b, N, &xa[0][0], &xb[0][0], N, NULL, cell, NULL, vd, scores3, &ga2[0][0], &gb2[0][0], NULL,
                                      wb2) != LCHD_EVALUE)
        FAIL("dense: one strain pointer alone accepted\n");

    lchd_ctx_destroy(ctx);
    printf("cabi gradient periodic ok\n");
    return 0;
}
