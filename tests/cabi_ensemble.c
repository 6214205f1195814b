/* A plain-C client of the dense ensemble entry point: three 40-point structures of one topology, every pair i < j through
 * lchd_ensemble_from_coords, each row checked against lchd_from_coords of the same pair. */
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

enum { M = 3, N = 40, P = M * (M - 1) / 2 };

int main(void) {
    lchd_ctx *ctx = NULL;
    CHECK(lchd_ctx_create(-1, &ctx));
    double wf_params[2] = {3.0, 10.0};
    lchd_weight_function wf = {LCHD_WF_UNIFORM, 2, wf_params};
    double weights[4] = {1.0, 1.0, 1.0, 1.0};
    lchd_config cfg = {0};
    cfg.n_categories = 4;
    cfg.category_weights = weights;
    cfg.n_weight_functions = 1;
    cfg.weight_functions = &wf;
    cfg.sd_kind = LCHD_SD_HELLINGER;
    cfg.sd_n_params = 1;
    cfg.sd_params[0] = 2.0;
    cfg.tag_accept_same = 1;

    static double xyz[M][N][3], out[P][N], row[N];
    int32_t seq[N];
    unsigned s = 12345u;
    for (int i = 0; i < N; ++i) {
        seq[i] = i % 4;
        for (int k = 0; k < 3; ++k) {
            s = s * 1103515245u + 12345u;
            const double base = (double)(s >> 8) / (double)(1u << 24) * 12.0;
            for (int m = 0; m < M; ++m) xyz[m][i][k] = base + 0.3 * m * ((i + k + m) % 3 - 1);
        }
    }
    CHECK(lchd_ensemble_from_coords(ctx, &cfg, seq, N, &xyz[0][0][0], M, NULL, P, NULL, NULL, NULL, &out[0][0]));
    int p = 0;
    double worst = 0.0;
    for (int i = 0; i < M; ++i)
        for (int j = i + 1; j < M; ++j, ++p) {
            CHECK(lchd_from_coords(ctx, &cfg, seq, N, seq, N, &xyz[i][0][0], N, &xyz[j][0][0], N, NULL, row));
            for (int r = 0; r < N; ++r) worst = fmax(worst, fabs(out[p][r] - row[r]));
        }
    printf("ensemble max |diff| %.3g, out[0][0] %.17g\n", worst, out[0][0]);
    if (!(worst < 1e-12) || !(out[0][0] > 0.0)) { fprintf(stderr, "ensemble rows differ from from_coords\n"); return 2; }
    int32_t bad[2] = {0, M};
    if (lchd_ensemble_from_coords(ctx, &cfg, seq, N, &xyz[0][0][0], M, bad, 1, NULL, NULL, NULL, &out[0][0]) != LCHD_EVALUE) {
        fprintf(stderr, "expected LCHD_EVALUE for a pair outside the ensemble\n");
        return 3;
    }
    lchd_ctx_destroy(ctx);
    printf("cabi ensemble ok\n");
    return 0;
}
