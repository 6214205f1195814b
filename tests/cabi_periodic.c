/* A plain-C client of the periodic entry point of include/loco_hd_hip.h: lchd_from_primitives_periodic on a 3 x 3 x 3 lattice that
 * fills its box (spacing L / 3, threshold = L: every atom has all 26 images and every distance is tied many times over).
 * Prints one score per anchor pair for the test that compiled it (tests/test_gpu_periodic.py compares them with the CPU oracle on
 * the replicated system) and checks by itself what needs no oracle. */
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
    double weights[7] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0};
    lchd_config cfg = {0};
    cfg.n_categories = 7;
    cfg.category_weights = weights;
    cfg.n_weight_functions = 1;
    cfg.weight_functions = &wf;
    cfg.sd_kind = LCHD_SD_HELLINGER;
    cfg.sd_n_params = 1;
    cfg.sd_params[0] = 2.0;
    cfg.tag_mode = 0;
    cfg.tag_accept_same = 0;

    enum { N = 27 };
    const double box[3] = {12.0, 12.0, 12.0};
    double xyz[N][3], out[N], self[N];
    int32_t cat_a[N], cat_b[N], tag[N];
    int64_t anchors[N][2];
    for (int i = 0; i < N; ++i) {
        xyz[i][0] = (i % 3) * 4.0; xyz[i][1] = ((i / 3) % 3) * 4.0; xyz[i][2] = (i / 9) * 4.0;
        cat_a[i] = i % 7; cat_b[i] = (3 * i + 1) % 7; tag[i] = i / 3;
        anchors[i][0] = i; anchors[i][1] = (i + 5) % N;
    }
    CHECK(lchd_from_primitives_periodic(ctx, &cfg, &xyz[0][0], cat_a, tag, N, &xyz[0][0], cat_b, tag, N, &anchors[0][0], NULL, N, 12.0,
                                        box, box, out));
    for (int i = 0; i < N; ++i) printf("score %d %.17g\n", i, out[i]);

    /* the same periodic structure on both sides, pair (i, i): identical environments */
    for (int i = 0; i < N; ++i) anchors[i][1] = i;
    CHECK(lchd_from_primitives_periodic(ctx, &cfg, &xyz[0][0], cat_a, tag, N, &xyz[0][0], cat_a, tag, N, &anchors[0][0], NULL, N, 12.0,
                                        box, box, self));
    for (int i = 0; i < N; ++i)
        if (!(fabs(self[i]) <= 1e-12)) { fprintf(stderr, "a periodic structure against itself scored %.17g\n", self[i]); return 2; }

    /* one side periodic, the other open (NULL box): the call runs and the open side differs from the periodic one */
    CHECK(lchd_from_primitives_periodic(ctx, &cfg, &xyz[0][0], cat_a, tag, N, &xyz[0][0], cat_a, tag, N, &anchors[0][0], NULL, N, 12.0,
                                        box, NULL, self));
    double far = 0.0;
    for (int i = 0; i < N; ++i) far = fmax(far, fabs(self[i]));
    printf("open-vs-periodic %.17g\n", far);
    if (!(far > 1e-3)) { fprintf(stderr, "the box made no difference\n"); return 3; }

    /* error paths: a threshold beyond the smallest edge, a bad edge, an anchor outside its structure */
    const double thin[3] = {12.0, 11.0, 12.0}, bad[3] = {12.0, 0.0, 12.0};
    if (lchd_from_primitives_periodic(ctx, &cfg, &xyz[0][0], cat_a, tag, N, &xyz[0][0], cat_a, tag, N, &anchors[0][0], NULL, N, 12.0, thin,
                                      box, self) != LCHD_EVALUE) { fprintf(stderr, "expected LCHD_EVALUE for a thin box\n"); return 4; }
    if (lchd_box_validate(bad, 1, 1.0) != LCHD_EVALUE || lchd_box_validate(box, 1, 12.0) != LCHD_OK) { fprintf(stderr, "lchd_box_validate\n"); return 5; }
    anchors[3][1] = N; /* a ghost atom of the image cloud, not an atom of the structure */
    if (lchd_from_primitives_periodic(ctx, &cfg, &xyz[0][0], cat_a, tag, N, &xyz[0][0], cat_a, tag, N, &anchors[0][0], NULL, N, 12.0, box,
                                      box, self) != LCHD_EPANIC) { fprintf(stderr, "expected LCHD_EPANIC for an anchor beyond the structure\n"); return 6; }

    lchd_ctx_destroy(ctx);
    printf("cabi periodic ok\n");
    return 0;
}
