/* A plain-C client of the attribution entry points of include/loco_hd_hip.h that take host arrays: lchd_attribution_primitives (open and
 * with a box on side A), lchd_attribution_coords and lchd_attribution_dmxs, on 48 atoms.  Checks by itself what needs no reference: every
 * row sums to the score of lchd_from_primitives / lchd_from_primitives_periodic / lchd_from_coords / lchd_from_dmxs on the same input to
 * 1e-12, no entry is negative, the error paths.  Prints every table for tests/test_cabi_attribution.py. */
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

static int print_table(const char *name, const double *t, const double *score, int rows) {
    for (int r = 0; r < rows; ++r) {
        double sum = 0.0;
        printf("%s %d", name, r);
        for (int k = 0; k < C; ++k) {
            printf(" %.17g", t[r * C + k]);
            sum += t[r * C + k];
            if (!(t[r * C + k] >= 0.0)) { fprintf(stderr, "%s row %d: entry %d is %g\n", name, r, k, t[r * C + k]); return 1; }
        }
        printf("\n");
        if (!(fabs(sum - score[r]) <= 1e-12)) { fprintf(stderr, "%s row %d sums to %.17g, the score is %.17g\n", name, r, sum, score[r]); return 1; }
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

    const double box[3] = {12.0, 14.0, 13.0};
    double xa[N][3], xb[N][3], ma[N][N], mb[N][N - 7];
    static double tab[N * C], score[N];
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
    for (int i = 0; i < N; ++i) {
        for (int j = 0; j < N; ++j) {
            const double dx = xa[i][0] - xa[j][0], dy = xa[i][1] - xa[j][1], dz = xa[i][2] - xa[j][2];
            ma[i][j] = (i != j && i / 4 == j / 4) ? INFINITY : sqrt((dx * dx + dy * dy) + dz * dz);
        }
        for (int j = 0; j < N - 7; ++j) { /* side B: shorter rows, the zero in column i % (N - 7) */
            const int q = (j + N - 7 - i % (N - 7)) % (N - 7);
            const double dx = xb[i][0] - xb[q][0], dy = xb[i][1] - xb[q][1], dz = xb[i][2] - xb[q][2];
            mb[i][j] = q == 0 ? 0.0 : sqrt((dx * dx + dy * dy) + dz * dz) + 0.125;
        }
    }

    for (int pass = 0; pass < 2; ++pass) { /* exponent 2 with category weights, then exponent 3.5 */
        const char *names[2][4] = {{"prims", "box", "coords", "dmxs"}, {"prims3.5", "box3.5", "coords3.5", "dmxs3.5"}};
        cfg.sd_params[0] = pass ? 3.5 : 2.0;
        CHECK(lchd_from_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 6.5, score));
        CHECK(lchd_attribution_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 6.5, NULL, NULL,
                                          NULL, NULL, tab));
        if (print_table(names[pass][0], tab, score, NP)) return 2;
        CHECK(lchd_from_primitives_periodic(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 6.5, box, NULL,
                                            score));
        CHECK(lchd_attribution_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 6.5, box, NULL,
                                          NULL, NULL, tab));
        if (print_table(names[pass][1], tab, score, NP)) return 2;
        CHECK(lchd_from_coords(ctx, &cfg, cat_a, N, cat_b, N, &xa[0][0], N, &xb[0][0], N, NULL, score));
        CHECK(lchd_attribution_coords(ctx, &cfg, cat_a, N, cat_b, N, &xa[0][0], N, &xb[0][0], N, NULL, NULL, NULL, tab));
        if (print_table(names[pass][2], tab, score, N)) return 2;
        CHECK(lchd_from_dmxs(ctx, &cfg, cat_a, N, cat_b, N, &ma[0][0], N, N, &mb[0][0], N, N - 7, NULL, score));
        CHECK(lchd_attribution_dmxs(ctx, &cfg, cat_a, N, cat_b, N, &ma[0][0], &mb[0][0], N, N, N - 7, NULL, tab));
        if (print_table(names[pass][3], tab, score, N)) return 2;
    }

    /* error paths: a distance that does not decompose, an anchor outside its structure, a box and a cell on one side */
    cfg.sd_kind = LCHD_SD_KOLMOGOROV_SMIRNOV;
    cfg.sd_n_params = 0;
    if (lchd_attribution_dmxs(ctx, &cfg, cat_a, N, cat_b, N, &ma[0][0], &mb[0][0], N, N, N - 7, NULL, tab) != LCHD_EUNSUPPORTED ||
        lchd_attribution_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 6.5, NULL, NULL, NULL,
                                    NULL, tab) != LCHD_EUNSUPPORTED) {
        fprintf(stderr, "expected LCHD_EUNSUPPORTED under Kolmogorov-Smirnov\n");
        return 3;
    }
    CHECK(lchd_from_dmxs(ctx, &cfg, cat_a, N, cat_b, N, &ma[0][0], N, N, &mb[0][0], N, N - 7, NULL, score)); /* the scoring call is untouched */
    cfg.sd_kind = LCHD_SD_HELLINGER;
    cfg.sd_n_params = 1;
    cfg.sd_params[0] = 2.0;
    anchors[3][1] = N;
    if (lchd_attribution_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 6.5, NULL, NULL, NULL,
                                    NULL, tab) != LCHD_EPANIC) {
        fprintf(stderr, "expected LCHD_EPANIC for an anchor outside the structure\n");
        return 5;
    }
    anchors[3][1] = 0;
    const double cell[9] = {13.0, 0.0, 0.0, 4.0, 12.0, 0.0, -3.0, 5.0, 14.0};
    if (lchd_attribution_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 6.5, box, cell, NULL,
                                    NULL, tab) != LCHD_EVALUE) {
        fprintf(stderr, "expected LCHD_EVALUE for a box and a cell\n");
        return 6;
    }

    lchd_ctx_destroy(ctx);
    printf("cabi attribution ok\n");
    return 0;
}
