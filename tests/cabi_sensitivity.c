/* A plain-C client of the sensitivity entry points of include/loco_hd_hip.h: lchd_sensitivity_primitives (host arrays) and
 * lchd_sensitivity_needed_width, on 48 atoms.  Checks by itself what needs no reference: a row width that is too small fails with
 * LCHD_EVALUE and names the width to use; with that width every score equals lchd_from_primitives on the same input to 1e-12, slot 0 is
 * the anchor with g == 0, the lists ascend in (distance, index), the padding is (-1, 0, 0); lchd_wf_pdf is 1/7 inside [3, 10).  Prints
 * every row for tests/test_cabi_sensitivity.py. */
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

enum { N = 48, NP = 20, C = 5, KMAX = N };

static int check_side(const char *name, int p, int64_t anchor, int k, int count, const int32_t *idx, const double *dist, const double *g) {
    if (count < 1 || count > k || idx[0] != anchor || dist[0] != 0.0 || g[0] != 0.0) FAIL("%s row %d: bad head\n", name, p);
    printf("%s %d %d", name, p, count);
    for (int t = 0; t < k; ++t) {
        if (t >= count && (idx[t] != -1 || dist[t] != 0.0 || g[t] != 0.0)) FAIL("%s row %d: padding at slot %d\n", name, p, t);
        if (t >= 2 && t < count && (dist[t] < dist[t - 1] || (dist[t] == dist[t - 1] && idx[t] < idx[t - 1]))) FAIL("%s row %d: order at slot %d\n", name, p, t);
        if (t < count) printf(" %d %.17g %.17g", (int)idx[t], dist[t], g[t]);
    }
    printf("\n");
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

    const double x[3] = {2.0, 3.0, 10.0};
    double w[3];
    CHECK(lchd_wf_pdf(LCHD_WF_UNIFORM, wf_params, 2, x, 3, w));
    if (w[0] != 0.0 || w[1] != 1.0 / 7.0 || w[2] != 0.0) FAIL("lchd_wf_pdf: %g %g %g\n", w[0], w[1], w[2]);

    double xa[N][3], xb[N][3];
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

    static double scores[NP], ref[NP], dist_a[NP * KMAX], dist_b[NP * KMAX], g_a[NP * KMAX], g_b[NP * KMAX];
    static int32_t count_a[NP], count_b[NP], idx_a[NP * KMAX], idx_b[NP * KMAX];
    /* a row of two slots is too narrow: LCHD_EVALUE, and the width the pairs take */
    int rc = lchd_sensitivity_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 6.5, 2, scores,
                                         count_a, idx_a, dist_a, g_a, count_b, idx_b, dist_b, g_b);
    const int k = (int)lchd_sensitivity_needed_width(ctx);
    if (rc != LCHD_EVALUE || k <= 2 || k > KMAX) FAIL("narrow rows: rc %d, needed width %d: %s\n", rc, k, lchd_last_error());
    CHECK(lchd_sensitivity_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 6.5, k, scores, count_a,
                                      idx_a, dist_a, g_a, count_b, idx_b, dist_b, g_b));
    if (lchd_sensitivity_needed_width(ctx) != k) FAIL("needed width moved\n");
    CHECK(lchd_from_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 6.5, ref));
    for (int p = 0; p < NP; ++p) {
        if (!(fabs(scores[p] - ref[p]) <= 1e-12)) FAIL("pair %d: score %.17g, lchd_from_primitives %.17g\n", p, scores[p], ref[p]);
        printf("score %d %.17g\n", p, scores[p]);
        if (check_side("a", p, anchors[p][0], k, count_a[p], idx_a + p * k, dist_a + p * k, g_a + p * k)) return 1;
        if (check_side("b", p, anchors[p][1], k, count_b[p], idx_b + p * k, dist_b + p * k, g_b + p * k)) return 1;
    }
    /* errors: a null output, a width of 0, an anchor outside its structure */
    if (lchd_sensitivity_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 6.5, k, NULL, count_a, idx_a,
                                    dist_a, g_a, count_b, idx_b, dist_b, g_b) != LCHD_EVALUE) FAIL("null scores accepted\n");
    if (lchd_sensitivity_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 6.5, 0, scores, count_a, idx_a,
                                    dist_a, g_a, count_b, idx_b, dist_b, g_b) != LCHD_EVALUE) FAIL("width 0 accepted\n");
    anchors[3][1] = N;
    if (lchd_sensitivity_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 6.5, k, scores, count_a, idx_a,
                                    dist_a, g_a, count_b, idx_b, dist_b, g_b) != LCHD_EPANIC) FAIL("anchor outside its structure accepted\n");
    lchd_ctx_destroy(ctx);
    printf("cabi sensitivity ok\n");
    return 0;
}
