/* A plain-C client of the cross-scoring entry points of include/loco_hd_hip.h: lchd_cross_plan, lchd_cross_primitives and
 * lchd_nearest_primitives (host arrays), 7 anchors against 70 on 48 atoms, on a deterministic context.  Checks by itself what needs no
 * reference: every entry of the cross matrix equals lchd_from_primitives on the explicit pair list to 1e-12, whatever tile_rows; the
 * nearest rows are the K smallest (score, column) of that matrix, exactly; the error codes.  Prints the matrix and the nearest rows for
 * tests/test_cabi_cross.py. */
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

enum { N = 48, NA = 7, NB = 70, C = 5, K = 5 };

int main(void) {
    lchd_ctx *ctx = NULL;
    CHECK(lchd_ctx_create(-1, &ctx));
    CHECK(lchd_ctx_set_deterministic(ctx, 1));
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

    int64_t rows = -1;
    CHECK(lchd_cross_plan(NA, NB, 3 * NB * 28, &rows));
    if (rows != 3) FAIL("lchd_cross_plan: %lld rows for a budget of three\n", (long long)rows);
    if (lchd_cross_plan(NA, NB, NB * 28 - 1, &rows) != LCHD_EUNSUPPORTED || rows != 0) FAIL("lchd_cross_plan: a budget below one row accepted\n");

    double xa[N][3], xb[N][3];
    int32_t cat_a[N], cat_b[N], tag[N];
    int64_t anchors_a[NA], anchors_b[NB], pairs[NA * NB][2];
    for (int i = 0; i < N; ++i) {
        xa[i][0] = fmod(7.31 * i, 11.0) + 0.5; xa[i][1] = fmod(3.77 * i, 11.0) + 0.5; xa[i][2] = fmod(5.13 * i, 11.0) + 0.5;
        xb[i][0] = fmod(2.91 * i, 11.0) + 0.5; xb[i][1] = fmod(6.43 * i, 11.0) + 0.5; xb[i][2] = fmod(4.57 * i, 11.0) + 0.5;
        cat_a[i] = (3 * i + 1) % C;
        cat_b[i] = (2 * i + 3) % C;
        tag[i] = i % 3;
    }
    for (int i = 0; i < NA; ++i) anchors_a[i] = (7 * i) % N;
    for (int j = 0; j < NB; ++j) anchors_b[j] = (11 * j + 5) % N;  /* 70 anchors on 48 atoms: 22 columns repeat an earlier one */
    for (int i = 0; i < NA; ++i)
        for (int j = 0; j < NB; ++j) { pairs[i * NB + j][0] = anchors_a[i]; pairs[i * NB + j][1] = anchors_b[j]; }

    static double ref[NA * NB], m[NA * NB], m3[NA * NB], scores[NA * K];
    static int32_t cols[NA * K];
    CHECK(lchd_from_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &pairs[0][0], NULL, NA * NB, 6.5, ref));
    CHECK(lchd_cross_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, anchors_a, NA, anchors_b, NB, -1, 6.5, 0, m));
    CHECK(lchd_cross_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, anchors_a, NA, anchors_b, NB, 0, 6.5, 3, m3));
    for (int p = 0; p < NA * NB; ++p) {
        if (!(fabs(m[p] - ref[p]) <= 1e-12)) FAIL("entry %d: cross %.17g, lchd_from_primitives %.17g\n", p, m[p], ref[p]);
        if (m3[p] != m[p]) FAIL("entry %d: tile_rows 3 gives %.17g, one tile %.17g\n", p, m3[p], m[p]);
    }
    for (int i = 0; i < NA; ++i) {
        printf("cross %d", i);
        for (int j = 0; j < NB; ++j) printf(" %.17g", m[i * NB + j]);
        printf("\n");
    }
    for (int tile = 0; tile <= 2; tile += 2) {
        CHECK(lchd_nearest_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, anchors_a, NA, anchors_b, NB, -1, 6.5, tile, K,
                                      scores, cols));
        for (int i = 0; i < NA; ++i) {
            unsigned char taken[NB] = {0};
            for (int t = 0; t < K; ++t) {  /* selection by hand: the smallest (score, column) not taken yet */
                int best = -1;
                for (int j = 0; j < NB; ++j)
                    if (!taken[j] && (best < 0 || m[i * NB + j] < m[i * NB + best])) best = j;
                taken[best] = 1;
                if (cols[i * K + t] != best || scores[i * K + t] != m[i * NB + best])
                    FAIL("tile_rows %d, row %d, place %d: column %d (%.17g), expected %d (%.17g)\n", tile, i, t, (int)cols[i * K + t],
                         scores[i * K + t], best, m[i * NB + best]);
            }
        }
    }
    for (int i = 0; i < NA; ++i) {
        printf("nearest %d", i);
        for (int t = 0; t < K; ++t) printf(" %d %.17g", (int)cols[i * K + t], scores[i * K + t]);
        printf("\n");
    }
    /* errors: k outside 1 .. min(n_b, 64), a negative tile_rows, a weight-function index the configuration lacks, a null output, an
     * anchor outside its structure */
    const int bad_k[3] = {0, 65, NB + 1};
    for (int q = 0; q < 3; ++q)
        if (lchd_nearest_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, anchors_a, NA, anchors_b, NB, -1, 6.5, 0, bad_k[q],
                                    scores, cols) != LCHD_EVALUE) FAIL("k = %d accepted\n", bad_k[q]);
    if (lchd_nearest_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, anchors_a, NA, anchors_b, 3, -1, 6.5, 0, 4, scores,
                                cols) != LCHD_EVALUE) FAIL("k = 4 of 3 columns accepted\n");
    if (lchd_cross_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, anchors_a, NA, anchors_b, NB, -1, 6.5, -1, m3) !=
        LCHD_EVALUE) FAIL("tile_rows = -1 accepted\n");
    if (lchd_cross_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, anchors_a, NA, anchors_b, NB, 1, 6.5, 0, m3) !=
        LCHD_EVALUE) FAIL("weight-function index 1 of 1 accepted\n");
    if (lchd_cross_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, anchors_a, NA, anchors_b, NB, -1, 6.5, 0, NULL) !=
        LCHD_EVALUE) FAIL("null output accepted\n");
    anchors_b[NB - 1] = N;
    if (lchd_cross_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, anchors_a, NA, anchors_b, NB, -1, 6.5, 2, m3) !=
        LCHD_EPANIC) FAIL("anchor outside its structure accepted\n");
    lchd_ctx_destroy(ctx);
    printf("cabi cross ok\n");
    return 0;
}
