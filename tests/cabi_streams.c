/* A plain-C client of the stream contract (include/loco_hd_hip.h, "Streams"), HIP runtime only, no torch:
 *   - the context is moved to a hipStreamNonBlocking stream; the anchor pairs are copied to the device with hipMemcpyAsync ON THAT
 *     STREAM from pinned memory and lchd_from_primitives_dev follows with no synchronise in between (d_anchors is read in stream
 *     order; d_out is complete on return);
 *   - trajectory frames are loaded on a SECOND non-blocking stream and scored with lchd_from_primitives_dev_async /
 *     lchd_ctx_finish (the pass is ordered behind the load by the library);
 *   - every output equals, byte for byte (deterministic mode), the output of the same calls made on the NULL stream with
 *     complete inputs. */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
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
#define HIP(call)                                                                          \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            fprintf(stderr, "%s -> %d (%s)\n", #call, (int)e_, hipGetErrorName(e_));       \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

enum { NA = 1500, NP = 3000, NT = 300, NF = 4, NPF = 250, ROUNDS = 20 };

static double xyz_a[NA][3], xyz_b[NA][3], tmpl_xyz[NT][3], frames_x[NF][NT][3], frames_y[NF][NT][3];
static int32_t cat_a[NA], cat_b[NA], tag_a[NA], tmpl_cat[NT];
static int64_t anchors[NP][2], other_anchors[NP][2], frame_anchors[NF * NPF][2];
static double want_prims[NP], want_other[NP], want_x[NF * NPF], want_y[NF * NPF], got[NP];

static unsigned lcg(unsigned *s) { return *s = *s * 1103515245u + 12345u; }
static double unif(unsigned *s, double hi) { return (double)(lcg(s) >> 8) / (double)(1u << 24) * hi; }

int main(void) {
    lchd_ctx *ctx;
    lchd_config cfg;
    memset(&cfg, 0, sizeof cfg);
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

    unsigned s = 4242u;
    for (int i = 0; i < NA; ++i) {
        cat_a[i] = (int32_t)(lcg(&s) >> 16) % 5;
        cat_b[i] = (int32_t)(lcg(&s) >> 16) % 5;
        tag_a[i] = 0;
        for (int k = 0; k < 3; ++k) {
            xyz_a[i][k] = unif(&s, 31.0);
            xyz_b[i][k] = unif(&s, 31.0);
        }
    }
    for (int p = 0; p < NP; ++p)
        for (int k = 0; k < 2; ++k) {
            anchors[p][k] = (int64_t)((lcg(&s) >> 8) % NA);
            other_anchors[p][k] = (int64_t)((lcg(&s) >> 8) % NA);
        }
    for (int i = 0; i < NT; ++i) {
        tmpl_cat[i] = (int32_t)(lcg(&s) >> 16) % 5;
        for (int k = 0; k < 3; ++k) tmpl_xyz[i][k] = unif(&s, 20.0);
    }
    for (int f = 0; f < NF; ++f)
        for (int i = 0; i < NT; ++i)
            for (int k = 0; k < 3; ++k) {  /* atoms 0 and 1 pin the bounding box of every frame set */
                frames_x[f][i][k] = i == 0 ? 0.0 : i == 1 ? 20.0 : unif(&s, 20.0);
                frames_y[f][i][k] = i == 0 ? 0.0 : i == 1 ? 20.0 : unif(&s, 20.0);
            }
    for (int f = 0; f < NF; ++f)
        for (int p = 0; p < NPF; ++p) {
            frame_anchors[f * NPF + p][0] = (int64_t)((lcg(&s) >> 8) % NT);
            frame_anchors[f * NPF + p][1] = (int64_t)f * NT + (int64_t)((lcg(&s) >> 8) % NT);
        }

    CHECK(lchd_ctx_create(-1, &ctx));
    CHECK(lchd_ctx_set_deterministic(ctx, 1));
    CHECK(lchd_ctx_set_config(ctx, &cfg));
    lchd_cloud *a, *b, *tmpl, *frames;
    CHECK(lchd_cloud_create(ctx, &xyz_a[0][0], cat_a, tag_a, NA, &a));
    CHECK(lchd_cloud_create(ctx, &xyz_b[0][0], cat_b, tag_a, NA, &b));
    CHECK(lchd_cloud_create(ctx, &tmpl_xyz[0][0], tmpl_cat, tag_a, NT, &tmpl));
    CHECK(lchd_frames_create(ctx, tmpl, NF, &frames));

    int64_t *d_anchors, *d_frame_anchors, *h_anchors, *h_other;
    double *d_out, *d_out2;
    HIP(hipMalloc((void **)&d_anchors, sizeof anchors));
    HIP(hipMalloc((void **)&d_frame_anchors, sizeof frame_anchors));
    HIP(hipMalloc((void **)&d_out, sizeof(double) * NP));
    HIP(hipMalloc((void **)&d_out2, sizeof(double) * NP));
    HIP(hipHostMalloc((void **)&h_anchors, sizeof anchors, 0));
    HIP(hipHostMalloc((void **)&h_other, sizeof anchors, 0));
    memcpy(h_anchors, anchors, sizeof anchors);
    memcpy(h_other, other_anchors, sizeof anchors);

    /* ---- the NULL stream, complete inputs: what every later call must reproduce ---- */
    HIP(hipMemcpy(d_frame_anchors, frame_anchors, sizeof frame_anchors, hipMemcpyHostToDevice));
    HIP(hipMemcpy(d_anchors, other_anchors, sizeof anchors, hipMemcpyHostToDevice));
    CHECK(lchd_from_primitives_dev(ctx, a, b, d_anchors, NULL, NP, 9.0, d_out));
    HIP(hipMemcpy(want_other, d_out, sizeof want_other, hipMemcpyDeviceToHost));
    HIP(hipMemcpy(d_anchors, anchors, sizeof anchors, hipMemcpyHostToDevice));
    CHECK(lchd_from_primitives_dev(ctx, a, b, d_anchors, NULL, NP, 9.0, d_out));
    HIP(hipMemcpy(want_prims, d_out, sizeof want_prims, hipMemcpyDeviceToHost));
    if (memcmp(want_prims, want_other, sizeof want_prims) == 0) { fprintf(stderr, "the two pair lists score alike\n"); return 2; }
    CHECK(lchd_frames_load(ctx, frames, &frames_x[0][0][0], NF, NULL));
    CHECK(lchd_from_primitives_dev(ctx, tmpl, frames, d_frame_anchors, NULL, NF * NPF, 8.0, d_out));
    HIP(hipMemcpy(want_x, d_out, sizeof want_x, hipMemcpyDeviceToHost));
    CHECK(lchd_frames_load(ctx, frames, &frames_y[0][0][0], NF, NULL));
    CHECK(lchd_from_primitives_dev(ctx, tmpl, frames, d_frame_anchors, NULL, NF * NPF, 8.0, d_out));
    HIP(hipMemcpy(want_y, d_out, sizeof want_y, hipMemcpyDeviceToHost));
    if (memcmp(want_x, want_y, sizeof want_x) == 0) { fprintf(stderr, "the two frame sets score alike\n"); return 2; }

    /* ---- non-blocking streams ---- */
    hipStream_t st, copy_st;
    HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    HIP(hipStreamCreateWithFlags(&copy_st, hipStreamNonBlocking));
    CHECK(lchd_ctx_set_stream(ctx, (void *)st));
    for (int r = 0; r < ROUNDS; ++r) {
        /* the pair list alternates; its copy and the sentinel fill of the output are queued on the stream, the call follows at once */
        const int odd = r & 1;
        HIP(hipMemcpyAsync(d_anchors, odd ? h_other : h_anchors, sizeof anchors, hipMemcpyHostToDevice, st));
        HIP(hipMemsetAsync(d_out, 0xFF, sizeof(double) * NP, st));
        CHECK(lchd_from_primitives_dev(ctx, a, b, d_anchors, NULL, NP, 9.0, d_out));
        HIP(hipMemcpyAsync(got, d_out, sizeof(double) * NP, hipMemcpyDeviceToHost, st)); /* d_out is complete on return: stream order is enough */
        HIP(hipStreamSynchronize(st));
        if (memcmp(got, odd ? want_other : want_prims, sizeof(double) * NP) != 0) {
            fprintf(stderr, "round %d: lchd_from_primitives_dev behind hipMemcpyAsync differs from the NULL-stream output\n", r);
            return 3;
        }
        /* frames: loaded on the copy stream, scored on the context's stream by the split call */
        CHECK(lchd_frames_load(ctx, frames, odd ? &frames_x[0][0][0] : &frames_y[0][0][0], NF, (void *)copy_st));
        HIP(hipMemsetAsync(d_out2, 0xFF, sizeof(double) * NP, st));
        CHECK(lchd_from_primitives_dev_async(ctx, tmpl, frames, d_frame_anchors, NULL, NF * NPF, 8.0, d_out2));
        if (lchd_frames_load(ctx, frames, &frames_x[0][0][0], NF, (void *)copy_st) != LCHD_EVALUE) {
            fprintf(stderr, "round %d: a frames buffer was reloaded under a pending pass\n", r);
            return 4;
        }
        if (lchd_ctx_set_stream(ctx, NULL) != LCHD_EVALUE) {
            fprintf(stderr, "round %d: the stream was switched under a pending pass\n", r);
            return 4;
        }
        CHECK(lchd_ctx_finish(ctx));
        HIP(hipMemcpy(got, d_out2, sizeof(double) * NF * NPF, hipMemcpyDeviceToHost));
        if (memcmp(got, odd ? want_x : want_y, sizeof(double) * NF * NPF) != 0) {
            fprintf(stderr, "round %d: the pass on frames loaded on a second stream differs from the NULL-stream output\n", r);
            return 5;
        }
    }
    /* back to the NULL stream: lchd_ctx_set_stream waits for the stream it leaves */
    CHECK(lchd_ctx_set_stream(ctx, NULL));
    HIP(hipMemcpy(d_anchors, anchors, sizeof anchors, hipMemcpyHostToDevice));
    CHECK(lchd_from_primitives_dev(ctx, a, b, d_anchors, NULL, NP, 9.0, d_out));
    HIP(hipMemcpy(got, d_out, sizeof(double) * NP, hipMemcpyDeviceToHost));
    if (memcmp(got, want_prims, sizeof want_prims) != 0) { fprintf(stderr, "after the switch back to the NULL stream the output differs\n"); return 6; }

    lchd_cloud_destroy(ctx, frames);
    lchd_cloud_destroy(ctx, tmpl);
    lchd_cloud_destroy(ctx, a);
    lchd_cloud_destroy(ctx, b);
    lchd_ctx_destroy(ctx);
    HIP(hipStreamDestroy(st));
    HIP(hipStreamDestroy(copy_st));
    HIP(hipFree(d_anchors));
    HIP(hipFree(d_frame_anchors));
    HIP(hipFree(d_out));
    HIP(hipFree(d_out2));
    HIP(hipHostFree(h_anchors));
    HIP(hipHostFree(h_other));
    printf("cabi streams ok: prims[0] %.17g frames[0] %.17g / %.17g\n", want_prims[0], want_x[0], want_y[0]);
    return 0;
}
