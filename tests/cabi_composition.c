/* A plain-C client of the composition entry points of include/loco_hd_hip.h that take host arrays: lchd_composition_primitives (and its
 * periodic form with a box and with a cell), lchd_composition_coords (open and in a cell) and lchd_composition_dmx, on 48 atoms.  Prints
 * every table for the test that compiled it (tests/test_cabi_composition.py compares them with the Python calls) and checks by itself
 * what needs no reference: every row sums to F(inf) - F(0) = 1, a repeated anchor repeats its row, the error paths. */
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

enum { N = 48, NA = 20, C = 5 };

static int print_table(const char *name, const double *t, int rows) {
    for (int r = 0; r < rows; ++r) {
        double sum = 0.0;
        printf("%s %d", name, r);
        for (int c = 0; c < C; ++c) {
            printf(" %.17g", t[r * C + c]);
            sum += t[r * C + c];
        }
        printf("\n");
        if (!(fabs(sum - 1.0) <= 1e-11)) { fprintf(stderr, "%s row %d sums to %.17g\n", name, r, sum); return 1; }
    }
    return 0;
}

int main(void) {
    lchd_ctx *ctx = NULL;
    CHECK(lchd_ctx_create(-1, &ctx));

    double wf_params[2] = {1.0, 0.2};
    lchd_weight_function wf = {LCHD_WF_HYPER_EXP, 2, wf_params};
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
    const double cell[9] = {13.0, 0.0, 0.0, 4.0, 12.0, 0.0, -3.0, 5.0, 14.0};
    double xyz[N][3], dmx[N][N];
    static double tab[N * C];
    int32_t cat[N], tag[N];
    int64_t anchors[NA];
    for (int i = 0; i < N; ++i) { /* (a fixed scatter inside the box and the cell's inscribed region) */
        xyz[i][0] = fmod(7.31 * i, 11.0) + 0.5; xyz[i][1] = fmod(3.77 * i, 11.0) + 0.5; xyz[i][2] = fmod(5.13 * i, 11.0) + 0.5;
        cat[i] = (3 * i + 1) % C;
        tag[i] = i % 3;
    }
    for (int k = 0; k < NA; ++k) anchors[k] = (7 * k) % N;
    anchors[NA - 1] = anchors[0]; /* a repeated anchor */
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) {
            const double dx = xyz[i][0] - xyz[j][0], dy = xyz[i][1] - xyz[j][1], dz = xyz[i][2] - xyz[j][2];
            dmx[i][j] = (i != j && i / 4 == j / 4) ? INFINITY : sqrt((dx * dx + dy * dy) + dz * dz);
        }

    CHECK(lchd_composition_primitives(ctx, &cfg, &xyz[0][0], cat, tag, N, anchors, NULL, NA, 6.0, tab));
    if (print_table("prims", tab, NA)) return 2;
    for (int c = 0; c < C; ++c)
        if (tab[c] != tab[(NA - 1) * C + c]) { fprintf(stderr, "a repeated anchor did not repeat its row\n"); return 3; }
    CHECK(lchd_composition_primitives_periodic(ctx, &cfg, &xyz[0][0], cat, tag, N, anchors, NULL, NA, 6.0, box, NULL, tab));
    if (print_table("box", tab, NA)) return 2;
    CHECK(lchd_composition_primitives_periodic(ctx, &cfg, &xyz[0][0], cat, tag, N, anchors, NULL, NA, 6.0, NULL, cell, tab));
    if (print_table("cell", tab, NA)) return 2;
    CHECK(lchd_composition_coords(ctx, &cfg, cat, N, &xyz[0][0], N, NULL, NULL, tab));
    if (print_table("coords", tab, N)) return 2;
    CHECK(lchd_composition_coords(ctx, &cfg, cat, N, &xyz[0][0], N, NULL, cell, tab));
    if (print_table("coordscell", tab, N)) return 2;
    CHECK(lchd_composition_dmx(ctx, &cfg, cat, N, &dmx[0][0], N, N, NULL, tab));
    if (print_table("dmx", tab, N)) return 2;

    /* error paths: an anchor outside the structure, a box and a cell at once, a threshold beyond the box, a row without a zero */
    anchors[3] = N;
    if (lchd_composition_primitives(ctx, &cfg, &xyz[0][0], cat, tag, N, anchors, NULL, NA, 6.0, tab) != LCHD_EPANIC) {
        fprintf(stderr, "expected LCHD_EPANIC for an anchor outside the structure\n");
        return 4;
    }
    anchors[3] = 0;
    if (lchd_composition_primitives_periodic(ctx, &cfg, &xyz[0][0], cat, tag, N, anchors, NULL, NA, 6.0, box, cell, tab) != LCHD_EVALUE) {
        fprintf(stderr, "expected LCHD_EVALUE for a box and a cell\n");
        return 5;
    }
    if (lchd_composition_primitives_periodic(ctx, &cfg, &xyz[0][0], cat, tag, N, anchors, NULL, NA, 12.5, box, NULL, tab) != LCHD_EVALUE) {
        fprintf(stderr, "expected LCHD_EVALUE for a threshold beyond the smallest edge\n");
        return 6;
    }
    dmx[5][5] = 0.25;
    if (lchd_composition_dmx(ctx, &cfg, cat, N, &dmx[0][0], N, N, NULL, tab) != LCHD_EVALUE) {
        fprintf(stderr, "expected LCHD_EVALUE for a distance row that does not start at 0\n");
        return 7;
    }
    cat[9] = -1; /* not in the category map */
    if (lchd_composition_coords(ctx, &cfg, cat, N, &xyz[0][0], N, NULL, NULL, tab) != LCHD_EVALUE) {
        fprintf(stderr, "expected LCHD_EVALUE for an atom outside the category map\n");
        return 8;
    }

    lchd_ctx_destroy(ctx);
    printf("cabi composition ok\n");
    return 0;
}
