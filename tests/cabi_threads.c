/* A plain-C client that shares one deterministic context between four POSIX threads and one {0, 0} device group between two.
 * Every thread makes host-pointer calls (lchd_from_primitives, lchd_from_coords, lchd_from_dmxs_ragged, lchd_from_anchors) in
 * its own order; each output must equal, byte for byte, the serial output of the same context (the group's: within 1e-13, a
 * group picks kernels per share).  Thread 0 also makes calls with an out-of-range anchor and must get LCHD_EPANIC with its own
 * lchd_last_error() every time. */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
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

enum { NA = 1500, NP = 3000, NC = 400, ROWS = 100, COLS = 150, LD = 300, THREADS = 4, CALLS = 100, KINDS = 4, GCALLS = 30 };

static lchd_ctx *ctx;
static lchd_group *grp;
static lchd_config cfg;
static double xyz_a[NA][3], xyz_b[NA][3], coords_a[NC][3], coords_b[NC][3], dmx_a[ROWS][COLS], dmx_b[ROWS][COLS], dist_a[LD], dist_b[LD];
static int32_t cat_a[NA], cat_b[NA], tag_a[NA], seq_c[NC], seq_d[COLS], seq_l[LD], len_a[ROWS], len_b[ROWS];
static int64_t anchors[NP][2], bad_anchors[2][2];
static double want_prims[NP], want_coords[NC], want_dmxs[ROWS], want_anchors[1], want_group[NP];
static const char *bad_msg = "anchor index is outside its structure";

static unsigned lcg(unsigned *s) { return *s = *s * 1103515245u + 12345u; }
static double unif(unsigned *s, double hi) { return (double)(lcg(s) >> 8) / (double)(1u << 24) * hi; }

static int call_kind(int kind, double *out) {
    switch (kind) {
    case 0:
        return lchd_from_primitives(ctx, &cfg, &xyz_a[0][0], cat_a, tag_a, NA, &xyz_b[0][0], cat_b, tag_a, NA, &anchors[0][0], NULL, NP, 9.0, out);
    case 1:
        return lchd_from_coords(ctx, &cfg, seq_c, NC, seq_c, NC, &coords_a[0][0], NC, &coords_b[0][0], NC, NULL, out);
    case 2:
        return lchd_from_dmxs_ragged(ctx, &cfg, seq_d, COLS, seq_d, COLS, &dmx_a[0][0], ROWS, COLS, len_a, &dmx_b[0][0], ROWS, COLS, len_b, NULL, out);
    default:
        return lchd_from_anchors(ctx, &cfg, seq_l, LD, dist_a, LD, seq_l, LD, dist_b, LD, 0, out);
    }
}

static const double *want_of(int kind, size_t *bytes) {
    static const size_t n[KINDS] = {NP, NC, ROWS, 1};
    *bytes = n[kind] * sizeof(double);
    return kind == 0 ? want_prims : kind == 1 ? want_coords : kind == 2 ? want_dmxs : want_anchors;
}

struct job { int id; int failed; char why[256]; };

static void *ctx_worker(void *arg) {
    struct job *j = (struct job *)arg;
    static double outs[THREADS][NP];
    double *out = outs[j->id];
    unsigned s = 777u + 31u * (unsigned)j->id;
    for (int k = 0; k < CALLS; ++k) {
        const int kind = (int)((lcg(&s) >> 16) % KINDS);
        if (j->id == 0 && k % 10 == 0) {
            double junk[2];
            const int rc = lchd_from_primitives(ctx, &cfg, &xyz_a[0][0], cat_a, tag_a, NA, &xyz_b[0][0], cat_b, tag_a, NA, &bad_anchors[0][0],
                                                NULL, 2, 9.0, junk);
            if (rc != LCHD_EPANIC || !strstr(lchd_last_error(), bad_msg)) {
                j->failed = 1;
                snprintf(j->why, sizeof j->why, "bad anchor call %d -> %d: %s", k, rc, lchd_last_error());
                return NULL;
            }
        }
        const int rc = call_kind(kind, out);
        size_t bytes;
        const double *want = want_of(kind, &bytes);
        if (rc != LCHD_OK || memcmp(out, want, bytes) != 0) {
            j->failed = 1;
            snprintf(j->why, sizeof j->why, "call %d (kind %d) -> %d (%s): %s", k, kind, rc, lchd_last_error(),
                     rc == LCHD_OK ? "differs from the serial output" : "failed");
            return NULL;
        }
    }
    return NULL;
}

static void *group_worker(void *arg) {
    struct job *j = (struct job *)arg;
    static double outs[2][NP];
    double *out = outs[j->id];
    for (int k = 0; k < GCALLS; ++k) {
        const int rc = lchd_group_from_primitives(grp, &cfg, &xyz_a[0][0], cat_a, tag_a, NA, &xyz_b[0][0], cat_b, tag_a, NA, &anchors[0][0], NULL,
                                                  NP, 9.0, out);
        double worst = 0.0;
        for (int p = 0; p < NP && rc == LCHD_OK; ++p) worst = fmax(worst, fabs(out[p] - want_group[p]));
        if (rc != LCHD_OK || !(worst <= 1e-13)) {
            j->failed = 1;
            snprintf(j->why, sizeof j->why, "group call %d -> %d (%s), max |diff| %g", k, rc, lchd_last_error(), worst);
            return NULL;
        }
    }
    return NULL;
}

int main(void) {
    CHECK(lchd_ctx_create(-1, &ctx));
    CHECK(lchd_ctx_set_deterministic(ctx, 1));
    static double wf_params[2] = {1.0, 0.15};
    static lchd_weight_function wf = {LCHD_WF_HYPER_EXP, 2, wf_params};
    static double weights[5] = {1.0, 1.0, 1.0, 1.0, 1.0};
    cfg.n_categories = 5;
    cfg.category_weights = weights;
    cfg.n_weight_functions = 1;
    cfg.weight_functions = &wf;
    cfg.sd_kind = LCHD_SD_HELLINGER;
    cfg.sd_n_params = 1;
    cfg.sd_params[0] = 2.0;
    cfg.tag_accept_same = 1;

    unsigned s = 2024u;
    for (int i = 0; i < NA; ++i) {
        cat_a[i] = (int32_t)(lcg(&s) >> 16) % 5;
        cat_b[i] = (int32_t)(lcg(&s) >> 16) % 5;
        tag_a[i] = i / 3;
        for (int k = 0; k < 3; ++k) {
            xyz_a[i][k] = unif(&s, 31.0);
            xyz_b[i][k] = unif(&s, 31.0);
        }
    }
    for (int p = 0; p < NP; ++p) {
        anchors[p][0] = (int64_t)((lcg(&s) >> 8) % NA);
        anchors[p][1] = (int64_t)((lcg(&s) >> 8) % NA);
    }
    bad_anchors[0][0] = bad_anchors[0][1] = 0;
    bad_anchors[1][0] = NA + 5;
    bad_anchors[1][1] = 1;
    for (int i = 0; i < NC; ++i) {
        seq_c[i] = (int32_t)(lcg(&s) >> 16) % 5;
        for (int k = 0; k < 3; ++k) {
            coords_a[i][k] = unif(&s, 18.0);
            coords_b[i][k] = coords_a[i][k] + unif(&s, 1.0) - 0.5;
        }
    }
    for (int c = 0; c < COLS; ++c) seq_d[c] = (int32_t)(lcg(&s) >> 16) % 5;
    for (int r = 0; r < ROWS; ++r) {
        len_a[r] = 40 + (int32_t)((lcg(&s) >> 8) % (COLS - 40 + 1));
        if (len_a[r] < r + 1) len_a[r] = r + 1;
        len_b[r] = COLS;
        for (int c = 0; c < COLS; ++c) {
            dmx_a[r][c] = c == r ? 0.0 : ((lcg(&s) >> 8) % 10 == 0 ? INFINITY : unif(&s, 15.0) + 0.01);
            dmx_b[r][c] = c == r ? 0.0 : ((lcg(&s) >> 8) % 10 == 0 ? INFINITY : unif(&s, 15.0) + 0.01);
        }
    }
    dist_a[0] = dist_b[0] = 0.0;
    for (int i = 1; i < LD; ++i) {
        dist_a[i] = dist_a[i - 1] + unif(&s, 0.1);
        dist_b[i] = dist_b[i - 1] + unif(&s, 0.1);
        seq_l[i] = (int32_t)(lcg(&s) >> 16) % 5;
    }
    seq_l[0] = 0;

    /* serial outputs of the same context, each repeated once */
    static double again[NP];
    for (int kind = 0; kind < KINDS; ++kind) {
        size_t bytes;
        double *want = (double *)want_of(kind, &bytes);
        CHECK(call_kind(kind, want));
        CHECK(call_kind(kind, again));
        if (memcmp(again, want, bytes) != 0) { fprintf(stderr, "serial repeat of kind %d differs\n", kind); return 2; }
    }
    const int32_t devs[2] = {0, 0};
    CHECK(lchd_group_create(devs, 2, &grp));
    CHECK(lchd_group_from_primitives(grp, &cfg, &xyz_a[0][0], cat_a, tag_a, NA, &xyz_b[0][0], cat_b, tag_a, NA, &anchors[0][0], NULL, NP, 9.0,
                                     want_group));
    double worst = 0.0;
    for (int p = 0; p < NP; ++p) worst = fmax(worst, fabs(want_group[p] - want_prims[p]));
    if (!(worst <= 1e-13)) { fprintf(stderr, "group and context differ by %g\n", worst); return 3; }

    pthread_t th[THREADS + 2];
    struct job jobs[THREADS + 2];
    memset(jobs, 0, sizeof jobs);
    for (int t = 0; t < THREADS + 2; ++t) {
        jobs[t].id = t < THREADS ? t : t - THREADS;
        if (pthread_create(&th[t], NULL, t < THREADS ? ctx_worker : group_worker, &jobs[t]) != 0) { fprintf(stderr, "pthread_create\n"); return 4; }
    }
    int failed = 0;
    for (int t = 0; t < THREADS + 2; ++t) {
        pthread_join(th[t], NULL);
        if (jobs[t].failed) {
            fprintf(stderr, "%s thread %d: %s\n", t < THREADS ? "context" : "group", jobs[t].id, jobs[t].why);
            failed = 1;
        }
    }
    lchd_group_destroy(grp);
    lchd_ctx_destroy(ctx);
    if (failed) return 5;
    printf("cabi threads ok: prims[0] %.17g coords[0] %.17g dmxs[0] %.17g anchors %.17g\n", want_prims[0], want_coords[0], want_dmxs[0],
           want_anchors[0]);
    return 0;
}
