/* A plain-C client of the native gradient entry points of include/loco_hd_hip.h on two 40-atom structures with 12 anchor pairs and pair
 * weights: lchd_gradient_primitives (host arrays) with tile_pairs 0 and 5, lchd_gradient_primitives_dev on clouds and device buffers,
 * lchd_gradient_plan, and the error paths.  argv[1] names a file with the expected bits (hex, one per line: 12 scores, 120 of grad_a,
 * 120 of grad_b) that tests/test_cabi_gradient.py computed from the sensitivity call and the model accumulator; every form must give
 * exactly those.  HIP runtime only. */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <inttypes.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
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
#define HIP(call)                                                                    \
    do {                                                                             \
        hipError_t e_ = (call);                                                      \
        if (e_ != hipSuccess) {                                                      \
            fprintf(stderr, "%s -> %d (%s)\n", #call, (int)e_, hipGetErrorName(e_)); \
            return 1;                                                                \
        }                                                                            \
    } while (0)
#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); return 1; } while (0)

enum { N = 40, NP = 12, C = 5, NOUT = NP + 6 * N };

static uint64_t want[NOUT];

static int same(const char *what, const double *scores, const double *ga, const double *gb) {
    const double *part[3] = {scores, ga, gb};
    const int len[3] = {NP, 3 * N, 3 * N};
    int at = 0;
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < len[k]; ++i, ++at) {
            uint64_t b;
            memcpy(&b, &part[k][i], 8);
            if (b != want[at]) FAIL("%s: output %d of array %d is %016" PRIx64 ", expected %016" PRIx64 "\n", what, i, k, b, want[at]);
        }
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) FAIL("usage: %s expected.txt\n", argv[0]);
    FILE *f = fopen(argv[1], "r");
    if (!f) FAIL("cannot open %s\n", argv[1]);
    for (int i = 0; i < NOUT; ++i)
        if (fscanf(f, "%" SCNx64, &want[i]) != 1) FAIL("short file of expected values\n");
    fclose(f);

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

    static double xa[N][3], xb[N][3], v[NP], scores[NP], ga[N][3], gb[N][3];
    static int32_t cat_a[N], cat_b[N], tag[N];
    static int64_t anchors[NP][2];
    for (int i = 0; i < N; ++i) {
        xa[i][0] = fmod(7.31 * i, 9.0) + 0.5; xa[i][1] = fmod(3.77 * i, 9.0) + 0.5; xa[i][2] = fmod(5.13 * i, 9.0) + 0.5;
        xb[i][0] = fmod(2.91 * i, 9.0) + 0.5; xb[i][1] = fmod(6.43 * i, 9.0) + 0.5; xb[i][2] = fmod(4.57 * i, 9.0) + 0.5;
        cat_a[i] = (3 * i + 1) % C;
        cat_b[i] = (2 * i + 3) % C;
        tag[i] = 0;
    }
    for (int k = 0; k < NP; ++k) { anchors[k][0] = (7 * k) % N; anchors[k][1] = (11 * k + 5) % N; v[k] = 0.5 + 0.125 * k; }

    int64_t tile = -1;
    CHECK(lchd_gradient_plan(NP, 128, (int64_t)5 * (40 * 128 + 16), &tile));
    if (tile != 5) FAIL("lchd_gradient_plan: %lld, expected 5\n", (long long)tile);
    if (lchd_gradient_plan(NP, 0, 1000, &tile) != LCHD_EVALUE || tile != 0) FAIL("a plan with width 0 accepted\n");

    /* host arrays: planned tiles, then tiles of five pairs -- the same bits */
    CHECK(lchd_gradient_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 10.0, v, 0, scores,
                                   &ga[0][0], &gb[0][0]));
    if (same("host arrays, planned tiles", scores, &ga[0][0], &gb[0][0])) return 1;
    memset(ga, 0xFF, sizeof ga); memset(gb, 0xFF, sizeof gb); memset(scores, 0xFF, sizeof scores);
    CHECK(lchd_gradient_primitives(ctx, &cfg, &xa[0][0], cat_a, tag, N, &xb[0][0], cat_b, tag, N, &anchors[0][0], NULL, NP, 10.0, v, 5, scores,
                                   &ga[0][0], &gb[0][0]));
    if (same("host arrays, tiles of 5", scores, &ga[0][0], &gb[0][0])) return 1;

    /* the device form on clouds */
    lchd_cloud *a = NULL, *b = NULL;
    CHECK(lchd_cloud_create(ctx, &xa[0][0], cat_a, tag, N, &a));
    CHECK(lchd_cloud_create(ctx, &xb[0][0], cat_b, tag, N, &b));
    int64_t *d_anchors = NULL;
    double *d_v = NULL, *d_scores = NULL, *d_ga = NULL, *d_gb = NULL;
    HIP(hipMalloc((void **)&d_anchors, sizeof anchors));
    HIP(hipMalloc((void **)&d_v, sizeof v));
    HIP(hipMalloc((void **)&d_scores, sizeof scores));
    HIP(hipMalloc((void **)&d_ga, sizeof ga));
    HIP(hipMalloc((void **)&d_gb, sizeof gb));
    HIP(hipMemcpy(d_anchors, anchors, sizeof anchors, hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_v, v, sizeof v, hipMemcpyHostToDevice));
    CHECK(lchd_gradient_primitives_dev(ctx, a, b, d_anchors, NULL, NP, 10.0, d_v, 1, d_scores, d_ga, d_gb));
    HIP(hipMemcpy(scores, d_scores, sizeof scores, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(ga, d_ga, sizeof ga, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(gb, d_gb, sizeof gb, hipMemcpyDeviceToHost));
    if (same("device form, tiles of 1", scores, &ga[0][0], &gb[0][0])) return 1;

    /* errors: a negative tile, a null output, a weight that takes a contribution out of range -- and clean accumulators behind it */
    if (lchd_gradient_primitives_dev(ctx, a, b, d_anchors, NULL, NP, 10.0, d_v, -1, d_scores, d_ga, d_gb) != LCHD_EVALUE) FAIL("tile_pairs -1 accepted\n");
    if (lchd_gradient_primitives_dev(ctx, a, b, d_anchors, NULL, NP, 10.0, d_v, 0, d_scores, NULL, d_gb) != LCHD_EVALUE) FAIL("null grad_a accepted\n");
    v[3] = ldexp(1.0, 200);
    HIP(hipMemcpy(d_v, v, sizeof v, hipMemcpyHostToDevice));
    if (lchd_gradient_primitives_dev(ctx, a, b, d_anchors, NULL, NP, 10.0, d_v, 0, d_scores, d_ga, d_gb) != LCHD_EVALUE ||
        !strstr(lchd_last_error(), "gradient contribution not finite or >= 2^63"))
        FAIL("a weight of 2^200 did not fail as out of range: %s\n", lchd_last_error());
    v[3] = 0.5 + 0.125 * 3;
    HIP(hipMemcpy(d_v, v, sizeof v, hipMemcpyHostToDevice));
    CHECK(lchd_gradient_primitives_dev(ctx, a, b, d_anchors, NULL, NP, 10.0, d_v, 0, d_scores, d_ga, d_gb));
    HIP(hipMemcpy(scores, d_scores, sizeof scores, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(ga, d_ga, sizeof ga, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(gb, d_gb, sizeof gb, hipMemcpyDeviceToHost));
    if (same("device form after a failed call", scores, &ga[0][0], &gb[0][0])) return 1;

    HIP(hipFree(d_anchors)); HIP(hipFree(d_v)); HIP(hipFree(d_scores)); HIP(hipFree(d_ga)); HIP(hipFree(d_gb));
    lchd_cloud_destroy(ctx, a);
    lchd_cloud_destroy(ctx, b);
    lchd_ctx_destroy(ctx);
    printf("cabi gradient ok\n");
    return 0;
}
