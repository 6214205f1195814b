/* A plain-C client of lchd_sensitivity_coords_periodic of include/loco_hd_hip.h: 6 atoms a side, side A in an orthorhombic box given as
 * its diagonal cell, side B open (a NULL cell).  Checks by itself what needs no reference: a width below n fails with LCHD_EVALUE and
 * lchd_sensitivity_needed_width names n; with width n + 1 every list holds all n atoms in ascending distance with the row's atom in
 * slot 0 (row 2 of side A: atom 0, the lower index of the two atoms at distance 0); sqrt((dx dx + dy dy) + dz dz) of disp is dist bit
 * for bit on both sides; side B's disp is x[member] - x[row atom]; atom 1 of side A -- exactly half an edge from atom 0 -- is seen from
 * atom 0 at +L/2 (rint(-0.5) is -0: no wrap) and atom 2, a whole edge from atom 0, at distance 0; the padding is (-1, 0, 0, 0 0 0); the
 * scores equal lchd_from_coords_periodic to 1e-12; a singular cell is LCHD_EVALUE.  Prints every row for
 * tests/test_cabi_sensitivity_coords_periodic.py. */
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

enum { N = 6, C = 2, K = 7 };

static int check_side(const char *name, int r, int first, int count, const int32_t *idx, const double *dist, const double *g, const double *disp,
                      const double *open_xyz) {
    if (count != N || idx[0] != first || dist[0] != 0.0 || g[0] != 0.0) FAIL("%s row %d: count %d, slot 0 holds %d at %g, g %g\n", name, r, count, (int)idx[0], dist[0], g[0]);
    printf("%s %d %d", name, r, count);
    for (int t = 0; t < K; ++t) {
        const double *d = disp + 3 * t;
        if (t >= count) {
            if (idx[t] != -1 || dist[t] != 0.0 || g[t] != 0.0 || d[0] != 0.0 || d[1] != 0.0 || d[2] != 0.0) FAIL("%s row %d: padding at slot %d\n", name, r, t);
            continue;
        }
        if (t && dist[t] < dist[t - 1]) FAIL("%s row %d: slot %d descends\n", name, r, t);
        if (sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) != dist[t]) FAIL("%s row %d: |disp| is not dist at slot %d\n", name, r, t);
        if (open_xyz)
            for (int k = 0; k < 3; ++k)
                if (d[k] != open_xyz[3 * idx[t] + k] - open_xyz[3 * r + k]) FAIL("%s row %d: slot %d is not x[member] - x[row atom]\n", name, r, t);
        printf(" %d %.17g %.17g %.17g %.17g %.17g", (int)idx[t], dist[t], g[t], d[0], d[1], d[2]);
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

    /* a box of 16 x 12 x 20; atom 1 half an edge from atom 0 along x, atom 2 a whole edge from atom 0 along y, atom 5 outside the box */
    const double cell_a[9] = {16.0, 0.0, 0.0, 0.0, 12.0, 0.0, 0.0, 0.0, 20.0};
    const double xyz_a[N][3] = {{1.5, 2.25, 3.0}, {9.5, 2.25, 3.0}, {1.5, 14.25, 3.0}, {6.0, 7.5, 11.25}, {13.0, 1.0, 17.5}, {-20.5, 30.0, 4.75}};
    const double xyz_b[N][3] = {{0.0, 0.0, 0.0}, {4.0, 1.0, 0.5}, {2.5, 6.0, 3.25}, {9.0, 2.0, 7.5}, {1.0, 11.0, 2.0}, {5.5, 5.5, 12.0}};
    const int32_t seq_a[N] = {0, 1, 1, 0, 1, 0}, seq_b[N] = {1, 0, 0, 1, 1, 0};

    static double scores[N], ref[N], dist_a[N * K], dist_b[N * K], g_a[N * K], g_b[N * K], disp_a[N * K * 3], disp_b[N * K * 3];
    static int32_t count_a[N], count_b[N], idx_a[N * K], idx_b[N * K];
    int rc = lchd_sensitivity_coords_periodic(ctx, &cfg, seq_a, N, seq_b, N, &xyz_a[0][0], &xyz_b[0][0], N, NULL, cell_a, NULL, N - 1, scores, count_a,
                                              idx_a, dist_a, g_a, count_b, idx_b, dist_b, g_b, disp_a, disp_b);
    if (rc != LCHD_EVALUE || lchd_sensitivity_needed_width(ctx) != N) FAIL("narrow rows: rc %d, needed width %d: %s\n", rc, (int)lchd_sensitivity_needed_width(ctx), lchd_last_error());
    CHECK(lchd_sensitivity_coords_periodic(ctx, &cfg, seq_a, N, seq_b, N, &xyz_a[0][0], &xyz_b[0][0], N, NULL, cell_a, NULL, K, scores, count_a, idx_a,
                                           dist_a, g_a, count_b, idx_b, dist_b, g_b, disp_a, disp_b));
    CHECK(lchd_from_coords_periodic(ctx, &cfg, seq_a, N, seq_b, N, &xyz_a[0][0], N, &xyz_b[0][0], N, NULL, cell_a, NULL, ref));
    int moved = 0;
    for (int r = 0; r < N; ++r) {
        if (!(fabs(scores[r] - ref[r]) <= 1e-12)) FAIL("row %d: score %.17g, lchd_from_coords_periodic %.17g\n", r, scores[r], ref[r]);
        printf("score %d %.17g\n", r, scores[r]);
        if (check_side("a", r, r == 2 ? 0 : r, count_a[r], idx_a + r * K, dist_a + r * K, g_a + r * K, disp_a + r * K * 3, NULL)) return 1;
        if (check_side("b", r, r, count_b[r], idx_b + r * K, dist_b + r * K, g_b + r * K, disp_b + r * K * 3, &xyz_b[0][0])) return 1;
        for (int t = 0; t < K; ++t) moved += g_a[r * K + t] != 0.0 || g_b[r * K + t] != 0.0;
    }
    if (!moved) FAIL("every g is 0\n");
    /* row 0 of A: slot 1 is atom 2 at distance 0 (a whole edge away), and atom 1 sits at +L/2 */
    if (idx_a[1] != 2 || dist_a[1] != 0.0) FAIL("row 0: the atom a whole edge away is not at distance 0 in slot 1\n");
    int seen = 0;
    for (int t = 0; t < N; ++t)
        if (idx_a[t] == 1) {
            seen = 1;
            if (dist_a[t] != 8.0 || disp_a[3 * t] != 8.0 || disp_a[3 * t + 1] != 0.0 || disp_a[3 * t + 2] != 0.0) FAIL("row 0: the atom half an edge away is at (%g %g %g)\n", disp_a[3 * t], disp_a[3 * t + 1], disp_a[3 * t + 2]);
        }
    if (!seen) FAIL("row 0: atom 1 is missing\n");
    /* errors: a null disp output, a singular cell */
    if (lchd_sensitivity_coords_periodic(ctx, &cfg, seq_a, N, seq_b, N, &xyz_a[0][0], &xyz_b[0][0], N, NULL, cell_a, NULL, K, scores, count_a, idx_a, dist_a,
                                         g_a, count_b, idx_b, dist_b, g_b, NULL, disp_b) != LCHD_EVALUE) FAIL("null disp accepted\n");
    const double flat[9] = {16.0, 0.0, 0.0, 0.0, 12.0, 0.0, 16.0, 12.0, 0.0};
    if (lchd_sensitivity_coords_periodic(ctx, &cfg, seq_a, N, seq_b, N, &xyz_a[0][0], &xyz_b[0][0], N, NULL, flat, NULL, K, scores, count_a, idx_a, dist_a,
                                         g_a, count_b, idx_b, dist_b, g_b, disp_a, disp_b) != LCHD_EVALUE) FAIL("a singular cell accepted\n");
    lchd_ctx_destroy(ctx);
    printf("cabi sensitivity coords periodic ok\n");
    return 0;
}
