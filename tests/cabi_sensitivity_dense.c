/* A plain-C client of the dense sensitivity entry points of include/loco_hd_hip.h: lchd_sensitivity_dmxs on 2 rows x 5 columns (side B:
 * 3 columns) with the order and the counts worked out by hand.  Checks by itself what needs no reference: a width below the longer
 * side's columns fails with LCHD_EVALUE and lchd_sensitivity_needed_width names the width to use; with it every list is the row in
 * (distance, column) order -- ties in column order, slot 0 the lowest column among the zeros, no forced anchor -- dist are the entries,
 * g is 0 in slot 0 and outside the support of uniform [3, 10), the padding is (-1, 0, 0), and the scores equal lchd_from_dmxs to 1e-12.
 * Prints every row for tests/test_cabi_sensitivity_dense.py. */
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

enum { ROWS = 2, CA = 5, CB = 3, C = 2, K = 6 };

static int check_side(const char *name, int r, int cols, int count, const int32_t *idx, const double *dist, const double *g, const int *order,
                      const double *row) {
    if (count != cols || g[0] != 0.0) FAIL("%s row %d: count %d, g[0] %g\n", name, r, count, g[0]);
    printf("%s %d %d", name, r, count);
    for (int t = 0; t < K; ++t) {
        if (t >= count && (idx[t] != -1 || dist[t] != 0.0 || g[t] != 0.0)) FAIL("%s row %d: padding at slot %d\n", name, r, t);
        if (t < count && (idx[t] != order[t] || dist[t] != row[order[t]])) FAIL("%s row %d: slot %d holds column %d at %g\n", name, r, t, (int)idx[t], dist[t]);
        if (t < count && !(dist[t] >= 3.0 && dist[t] < 10.0) && g[t] != 0.0) FAIL("%s row %d: g %g outside the support\n", name, r, g[t]);
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
    double weights[C] = {1.0, 1.0};
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

    /* row 0 of A: two zeros (columns 1 and 3) and a tie at 4.5 (columns 0 and 2); row 1: the zero in the last column */
    const double dmx_a[ROWS][CA] = {{4.5, 0.0, 4.5, 0.0, 7.25}, {9.0, 3.5, 12.0, 6.0, 0.0}};
    const double dmx_b[ROWS][CB] = {{0.0, 8.0, 5.0}, {6.5, 0.0, 6.5}};
    const int order_a[ROWS][CA] = {{1, 3, 0, 2, 4}, {4, 1, 3, 0, 2}};
    const int order_b[ROWS][CB] = {{0, 2, 1}, {1, 0, 2}};
    const int32_t seq_a[CA] = {0, 1, 1, 0, 1}, seq_b[CB] = {1, 0, 0};

    static double scores[ROWS], ref[ROWS], dist_a[ROWS * K], dist_b[ROWS * K], g_a[ROWS * K], g_b[ROWS * K];
    static int32_t count_a[ROWS], count_b[ROWS], idx_a[ROWS * K], idx_b[ROWS * K];
    /* rows of four slots are too narrow for five columns: LCHD_EVALUE before any pass, and the width the rows take */
    int rc = lchd_sensitivity_dmxs(ctx, &cfg, seq_a, CA, seq_b, CB, &dmx_a[0][0], &dmx_b[0][0], ROWS, CA, CB, NULL, 4, scores, count_a, idx_a, dist_a,
                                   g_a, count_b, idx_b, dist_b, g_b);
    if (rc != LCHD_EVALUE || lchd_sensitivity_needed_width(ctx) != CA) FAIL("narrow rows: rc %d, needed width %d: %s\n", rc, (int)lchd_sensitivity_needed_width(ctx), lchd_last_error());
    CHECK(lchd_sensitivity_dmxs(ctx, &cfg, seq_a, CA, seq_b, CB, &dmx_a[0][0], &dmx_b[0][0], ROWS, CA, CB, NULL, K, scores, count_a, idx_a, dist_a, g_a,
                                count_b, idx_b, dist_b, g_b));
    if (lchd_sensitivity_needed_width(ctx) != CA) FAIL("needed width moved\n");
    CHECK(lchd_from_dmxs(ctx, &cfg, seq_a, CA, seq_b, CB, &dmx_a[0][0], ROWS, CA, &dmx_b[0][0], ROWS, CB, NULL, ref));
    int moved = 0;
    for (int r = 0; r < ROWS; ++r) {
        if (!(fabs(scores[r] - ref[r]) <= 1e-12)) FAIL("row %d: score %.17g, lchd_from_dmxs %.17g\n", r, scores[r], ref[r]);
        printf("score %d %.17g\n", r, scores[r]);
        if (check_side("a", r, CA, count_a[r], idx_a + r * K, dist_a + r * K, g_a + r * K, order_a[r], dmx_a[r])) return 1;
        if (check_side("b", r, CB, count_b[r], idx_b + r * K, dist_b + r * K, g_b + r * K, order_b[r], dmx_b[r])) return 1;
        for (int t = 0; t < K; ++t) moved += g_a[r * K + t] != 0.0 || g_b[r * K + t] != 0.0;
    }
    if (!moved) FAIL("every g is 0\n");
    /* errors: a null output, a width of 0, a negative entry (what lchd_from_dmxs answers), a row without a zero */
    if (lchd_sensitivity_dmxs(ctx, &cfg, seq_a, CA, seq_b, CB, &dmx_a[0][0], &dmx_b[0][0], ROWS, CA, CB, NULL, K, NULL, count_a, idx_a, dist_a, g_a,
                              count_b, idx_b, dist_b, g_b) != LCHD_EVALUE) FAIL("null scores accepted\n");
    if (lchd_sensitivity_dmxs(ctx, &cfg, seq_a, CA, seq_b, CB, &dmx_a[0][0], &dmx_b[0][0], ROWS, CA, CB, NULL, 0, scores, count_a, idx_a, dist_a, g_a,
                              count_b, idx_b, dist_b, g_b) != LCHD_EVALUE) FAIL("width 0 accepted\n");
    double bad[ROWS][CB] = {{0.0, 8.0, 5.0}, {6.5, 0.0, -6.5}};
    const int want = lchd_from_dmxs(ctx, &cfg, seq_a, CA, seq_b, CB, &dmx_a[0][0], ROWS, CA, &bad[0][0], ROWS, CB, NULL, ref);
    rc = lchd_sensitivity_dmxs(ctx, &cfg, seq_a, CA, seq_b, CB, &dmx_a[0][0], &bad[0][0], ROWS, CA, CB, NULL, K, scores, count_a, idx_a, dist_a, g_a,
                               count_b, idx_b, dist_b, g_b);
    if (want == LCHD_OK || rc != want) FAIL("a negative entry: lchd_from_dmxs %d, lchd_sensitivity_dmxs %d\n", want, rc);
    bad[1][2] = 6.5;
    bad[1][1] = 0.5;
    if (lchd_sensitivity_dmxs(ctx, &cfg, seq_a, CA, seq_b, CB, &dmx_a[0][0], &bad[0][0], ROWS, CA, CB, NULL, K, scores, count_a, idx_a, dist_a, g_a,
                              count_b, idx_b, dist_b, g_b) != LCHD_EVALUE) FAIL("a row without a zero accepted\n");
    lchd_ctx_destroy(ctx);
    printf("cabi sensitivity dense ok\n");
    return 0;
}
