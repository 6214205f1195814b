/* A plain-C client of the periodic sensitivity entry points of include/loco_hd_hip.h: lchd_sensitivity_primitives_periodic (host arrays),
 * lchd_cloud_image_origin and lchd_cloud_home_size, on three atoms in the box (10, 10, 10) with threshold 4.5:
 *   atom 0 (1, 5, 5)   has its +x image (11, 5, 5), code 1
 *   atom 1 (9, 5, 5)   has its -x image (-1, 5, 5), code 2
 *   atom 2 (5, 5, 5)   has none
 * so the image cloud holds 5 slots with origin 0 1 2 0 1 and code 0 0 0 1 2, and the environments are known by hand:
 *   anchor 0: atom 1 through image 2 at (-2, 0, 0), atom 2 at (4, 0, 0)
 *   anchor 1: atom 0 through image 1 at (2, 0, 0), atom 2 at (-4, 0, 0)
 *   anchor 2: atoms 0 and 1, both home, tied at distance 4: (-4, 0, 0) then (4, 0, 0)
 * Scores are compared with lchd_from_primitives_periodic on the same input. */
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
#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); return 1; } while (0)

enum { N = 3, NP = 3, K = 4 };

static int check_row(const char *name, int p, int count, const int32_t *idx, const int8_t *image, const double *dist, const double *g,
                     const double *disp, const int *want_idx, const int *want_image, const double *want_dx) {
    if (count != 3) FAIL("%s row %d: count %d\n", name, p, count);
    for (int t = 0; t < K; ++t) {
        const int real = t < count;
        if (idx[t] != (real ? want_idx[t] : -1) || image[t] != (real ? want_image[t] : 0)) FAIL("%s row %d slot %d: idx %d image %d\n", name, p, t, (int)idx[t], (int)image[t]);
        if (disp[3 * t] != (real ? want_dx[t] : 0.0) || disp[3 * t + 1] != 0.0 || disp[3 * t + 2] != 0.0) FAIL("%s row %d slot %d: disp\n", name, p, t);
        if (dist[t] != fabs(real ? want_dx[t] : 0.0)) FAIL("%s row %d slot %d: dist %.17g\n", name, p, t, dist[t]);
        if ((t == 0 || !real) && g[t] != 0.0) FAIL("%s row %d slot %d: g %.17g\n", name, p, t, g[t]);
        if (!(g[t] == g[t])) FAIL("%s row %d slot %d: g is NaN\n", name, p, t);
    }
    return 0;
}

int main(void) {
    lchd_ctx *ctx = NULL;
    CHECK(lchd_ctx_create(-1, &ctx));
    double wf_params[2] = {1.0, 4.5};
    lchd_weight_function wf = {LCHD_WF_UNIFORM, 2, wf_params};
    double weights[2] = {1.0, 1.0};
    lchd_config cfg = {0};
    cfg.n_categories = 2;
    cfg.category_weights = weights;
    cfg.n_weight_functions = 1;
    cfg.weight_functions = &wf;
    cfg.sd_kind = LCHD_SD_HELLINGER;
    cfg.sd_n_params = 1;
    cfg.sd_params[0] = 2.0;
    cfg.tag_mode = 0;
    cfg.tag_accept_same = 1;

    const double xyz[N][3] = {{1.0, 5.0, 5.0}, {9.0, 5.0, 5.0}, {5.0, 5.0, 5.0}};
    const int32_t cat_a[N] = {0, 1, 0}, cat_b[N] = {1, 1, 0}, tag[N] = {0, 0, 0};
    const int64_t anchors[NP][2] = {{0, 0}, {1, 1}, {2, 2}};
    const double box[3] = {10.0, 10.0, 10.0}, thr = 4.5;

    /* the origin map of the image cloud */
    lchd_cloud *src = NULL, *img = NULL;
    CHECK(lchd_ctx_set_config(ctx, &cfg));
    CHECK(lchd_cloud_create(ctx, &xyz[0][0], cat_a, tag, N, &src));
    CHECK(lchd_cloud_create_images(ctx, src, box, 1, thr, &img));
    if (lchd_cloud_size(img) != 5 || lchd_cloud_home_size(img) != 3 || lchd_cloud_home_size(src) != 3) FAIL("sizes: %lld %lld\n", (long long)lchd_cloud_size(img), (long long)lchd_cloud_home_size(img));
    int32_t origin[5];
    int8_t code[5];
    CHECK(lchd_cloud_image_origin(ctx, img, origin, code, 5));
    const int want_origin[5] = {0, 1, 2, 0, 1}, want_code[5] = {0, 0, 0, 1, 2};
    for (int o = 0; o < 5; ++o)
        if (origin[o] != want_origin[o] || code[o] != want_code[o]) FAIL("slot %d: origin %d code %d\n", o, (int)origin[o], (int)code[o]);
    if (lchd_cloud_image_origin(ctx, img, origin, code, 4) != LCHD_EVALUE) FAIL("a wrong size accepted\n");
    if (lchd_cloud_image_origin(ctx, src, origin, code, 3) != LCHD_EVALUE) FAIL("a cloud that is no image cloud accepted\n");
    lchd_cloud_destroy(ctx, img);
    lchd_cloud_destroy(ctx, src);

    /* the host call: side A in the box, side B the same atoms (other categories) in the same box */
    double scores[NP], ref[NP], dist_a[NP * K], dist_b[NP * K], g_a[NP * K], g_b[NP * K], disp_a[NP * K * 3], disp_b[NP * K * 3];
    int32_t count_a[NP], count_b[NP], idx_a[NP * K], idx_b[NP * K];
    int8_t image_a[NP * K], image_b[NP * K];
    int rc = lchd_sensitivity_primitives_periodic(ctx, &cfg, &xyz[0][0], cat_a, tag, N, &xyz[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, thr, 2, box,
                                                  NULL, box, NULL, scores, count_a, idx_a, image_a, dist_a, g_a, disp_a, count_b, idx_b, image_b,
                                                  dist_b, g_b, disp_b);
    if (rc != LCHD_EVALUE || lchd_sensitivity_needed_width(ctx) != 3) FAIL("narrow rows: rc %d, needed width %d\n", rc, (int)lchd_sensitivity_needed_width(ctx));
    CHECK(lchd_sensitivity_primitives_periodic(ctx, &cfg, &xyz[0][0], cat_a, tag, N, &xyz[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, thr, K, box, NULL,
                                               box, NULL, scores, count_a, idx_a, image_a, dist_a, g_a, disp_a, count_b, idx_b, image_b, dist_b, g_b,
                                               disp_b));
    CHECK(lchd_from_primitives_periodic(ctx, &cfg, &xyz[0][0], cat_a, tag, N, &xyz[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, thr, box, box, ref));
    const int want_idx[NP][3] = {{0, 1, 2}, {1, 0, 2}, {2, 0, 1}}, want_image[NP][3] = {{0, 2, 0}, {0, 1, 0}, {0, 0, 0}};
    const double want_dx[NP][3] = {{0.0, -2.0, 4.0}, {0.0, 2.0, -4.0}, {0.0, -4.0, 4.0}};
    int moved = 0;
    for (int p = 0; p < NP; ++p) {
        if (!(fabs(scores[p] - ref[p]) <= 1e-11)) FAIL("pair %d: score %.17g, lchd_from_primitives_periodic %.17g\n", p, scores[p], ref[p]);
        if (check_row("a", p, count_a[p], idx_a + p * K, image_a + p * K, dist_a + p * K, g_a + p * K, disp_a + p * K * 3, want_idx[p], want_image[p], want_dx[p])) return 1;
        if (check_row("b", p, count_b[p], idx_b + p * K, image_b + p * K, dist_b + p * K, g_b + p * K, disp_b + p * K * 3, want_idx[p], want_image[p], want_dx[p])) return 1;
        for (int t = 1; t < 3; ++t) moved += g_a[p * K + t] != 0.0 || g_b[p * K + t] != 0.0;
    }
    if (!moved) FAIL("every sensitivity is 0\n");
    /* errors: a box and a cell on one side, an anchor outside its structure (it would name a ghost), a null output */
    const double cell[9] = {10.0, 0.0, 0.0, 0.0, 10.0, 0.0, 0.0, 0.0, 10.0};
    if (lchd_sensitivity_primitives_periodic(ctx, &cfg, &xyz[0][0], cat_a, tag, N, &xyz[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, thr, K, box, cell,
                                             NULL, NULL, scores, count_a, idx_a, image_a, dist_a, g_a, disp_a, count_b, idx_b, image_b, dist_b, g_b,
                                             disp_b) != LCHD_EVALUE) FAIL("a box and a cell on one side accepted\n");
    const int64_t beyond[1][2] = {{3, 0}};
    if (lchd_sensitivity_primitives_periodic(ctx, &cfg, &xyz[0][0], cat_a, tag, N, &xyz[0][0], cat_b, tag, N, &beyond[0][0], NULL, 1, thr, K, box, NULL,
                                             box, NULL, scores, count_a, idx_a, image_a, dist_a, g_a, disp_a, count_b, idx_b, image_b, dist_b, g_b,
                                             disp_b) == LCHD_OK) FAIL("an anchor that names a ghost accepted\n");
    if (lchd_sensitivity_primitives_periodic(ctx, &cfg, &xyz[0][0], cat_a, tag, N, &xyz[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, thr, K, box, NULL,
                                             box, NULL, scores, count_a, idx_a, NULL, dist_a, g_a, disp_a, count_b, idx_b, image_b, dist_b, g_b,
                                             disp_b) != LCHD_EVALUE) FAIL("null image output accepted\n");
    lchd_ctx_destroy(ctx);
    printf("cabi sensitivity periodic ok\n");
    return 0;
}
