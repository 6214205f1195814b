/* A plain-C client of the dense periodic entry point of include/loco_hd_hip.h: lchd_from_coords_periodic on 40 atoms scattered over
 * several cells, side A in an orthorhombic box (a diagonal cell), side B in a sheared cell.  Prints one score per row for the test that
 * compiled it (tests/test_cabi_dense_periodic.py compares them with the Python call) and checks by itself what needs no reference. */
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

int main(void) {
    lchd_ctx *ctx = NULL;
    CHECK(lchd_ctx_create(-1, &ctx));

    double wf_params[2] = {3.0, 10.0};
    lchd_weight_function wf = {LCHD_WF_UNIFORM, 2, wf_params};
    double weights[5] = {1.0, 1.0, 1.0, 1.0, 1.0};
    lchd_config cfg = {0};
    cfg.n_categories = 5;
    cfg.category_weights = weights;
    cfg.n_weight_functions = 1;
    cfg.weight_functions = &wf;
    cfg.sd_kind = LCHD_SD_HELLINGER;
    cfg.sd_n_params = 1;
    cfg.sd_params[0] = 2.0;

    enum { N = 40 };
    const double box[9] = {12.0, 0.0, 0.0, 0.0, 14.0, 0.0, 0.0, 0.0, 13.0};
    const double cell[9] = {20.0, 0.0, 0.0, 15.0, 18.0, 0.0, -9.0, 7.0, 16.0};
    double xa[N][3], xb[N][3], out[N], self[N], open[N];
    int32_t seq_a[N], seq_b[N];
    for (int i = 0; i < N; ++i) { /* (a fixed scatter: multiples of irrational-looking steps, several cells wide) */
        xa[i][0] = fmod(7.31 * i, 30.0) - 15.0; xa[i][1] = fmod(3.77 * i, 33.0) - 12.0; xa[i][2] = fmod(5.13 * i, 29.0) - 20.0;
        xb[i][0] = fmod(4.91 * i, 47.0) - 25.0; xb[i][1] = fmod(6.07 * i, 41.0) - 17.0; xb[i][2] = fmod(2.89 * i, 37.0) - 11.0;
        seq_a[i] = i % 5; seq_b[i] = (3 * i + 1) % 5;
    }
    CHECK(lchd_from_coords_periodic(ctx, &cfg, seq_a, N, seq_b, N, &xa[0][0], N, &xb[0][0], N, NULL, box, cell, out));
    for (int i = 0; i < N; ++i) {
        if (!(out[i] >= 0.0 && out[i] <= 1.0)) { fprintf(stderr, "score %d is %.17g\n", i, out[i]); return 2; }
        printf("score %d %.17g\n", i, out[i]);
    }

    /* the same periodic structure on both sides: identical rows */
    CHECK(lchd_from_coords_periodic(ctx, &cfg, seq_a, N, seq_a, N, &xa[0][0], N, &xa[0][0], N, NULL, cell, cell, self));
    for (int i = 0; i < N; ++i)
        if (!(fabs(self[i]) <= 1e-12)) { fprintf(stderr, "a periodic structure against itself scored %.17g\n", self[i]); return 3; }

    /* no cell on either side: the call is lchd_from_coords */
    CHECK(lchd_from_coords_periodic(ctx, &cfg, seq_a, N, seq_b, N, &xa[0][0], N, &xb[0][0], N, NULL, NULL, NULL, self));
    CHECK(lchd_from_coords(ctx, &cfg, seq_a, N, seq_b, N, &xa[0][0], N, &xb[0][0], N, NULL, open));
    double far = 0.0;
    for (int i = 0; i < N; ++i) {
        if (self[i] != open[i]) { fprintf(stderr, "row %d: %.17g without cells, %.17g from lchd_from_coords\n", i, self[i], open[i]); return 4; }
        far = fmax(far, fabs(out[i] - open[i]));
    }
    if (!(far > 1e-3)) { fprintf(stderr, "the cells made no difference\n"); return 5; }

    /* lchd_cell_reduce: a diagonal cell comes back as it is; error paths: a singular cell, a non-finite coordinate */
    double reduced[9], inverse[9];
    CHECK(lchd_cell_reduce(box, reduced, inverse));
    for (int k = 0; k < 9; ++k)
        if (reduced[k] != box[k]) { fprintf(stderr, "lchd_cell_reduce changed a diagonal cell\n"); return 6; }
    const double flat[9] = {20.0, 0.0, 0.0, 15.0, 18.0, 0.0, 35.0, 18.0, 0.0};
    if (lchd_cell_reduce(flat, reduced, inverse) != LCHD_EVALUE) { fprintf(stderr, "expected LCHD_EVALUE for a singular cell\n"); return 7; }
    if (lchd_from_coords_periodic(ctx, &cfg, seq_a, N, seq_b, N, &xa[0][0], N, &xb[0][0], N, NULL, flat, NULL, self) != LCHD_EVALUE) {
        fprintf(stderr, "expected LCHD_EVALUE for a singular cell_a\n");
        return 8;
    }
    xb[7][1] = NAN;
    if (lchd_from_coords_periodic(ctx, &cfg, seq_a, N, seq_b, N, &xa[0][0], N, &xb[0][0], N, NULL, box, cell, self) != LCHD_EVALUE) {
        fprintf(stderr, "expected LCHD_EVALUE for a non-finite coordinate\n");
        return 9;
    }

    lchd_ctx_destroy(ctx);
    printf("cabi dense periodic ok\n");
    return 0;
}
