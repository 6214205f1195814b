/* A C99 client of the host path of loco_hd_amd/csrc/lchd_param_sum.h and, built with -DWITH_LIBRARY and linked with the library, of
 * lchd_param_sum_plan (tests/test_cabi_param_sum.py).  No GPU is needed.
 *
 *   cabi_param_sum CASES     replays every case of the text file CASES and prints its sums with exact bits:
 *       file:    case NAME P W HAS_WEIGHTS HAS_BUCKETS N_BUCKETS, then P lines of W row values [weight] [bucket]
 *       stdout:  sum NAME FLAG v[0][0] ... v[N_BUCKETS - 1][W - 1]      (flag 1: a term was out of range)
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#ifdef WITH_LIBRARY
#include "loco_hd_hip.h"
#endif
#include "lchd_param_sum.h"

#ifdef WITH_LIBRARY

static int check_plan(void) {
    static const int64_t budgets[3] = {0, 1000, (int64_t)1 << 40};
    static const int32_t rows[3] = {5, 17, 64};
    const int64_t n = 1000000;
    int64_t tile = -1;
    int b, r;
    for (b = 0; b < 3; ++b)
        for (r = 0; r < 3; ++r) {
            /* the documented formula: the largest tile in 1 .. n with tile * (8 row_doubles + 20) <= budget */
            int64_t want = budgets[b] / (8 * (int64_t)rows[r] + 20);
            if (want > n) want = n;
            if (want < 1) want = 1;
            if (lchd_param_sum_plan(n, rows[r], budgets[b], &tile) != LCHD_OK || tile != want) {
                fprintf(stderr, "plan(%lld, %d, %lld) = %lld, expected %lld\n", (long long)n, rows[r], (long long)budgets[b], (long long)tile,
                        (long long)want);
                return 1;
            }
        }
    if (lchd_param_sum_plan(3, 5, (int64_t)1 << 40, &tile) != LCHD_OK || tile != 3) return 1; /* clamped to n_pairs */
    if (lchd_param_sum_plan(0, 5, 1000, &tile) != LCHD_EVALUE || tile != 0) return 1;
    if (lchd_param_sum_plan(-1, 5, 1000, &tile) != LCHD_EVALUE) return 1;
    if (lchd_param_sum_plan(10, 0, 1000, &tile) != LCHD_EVALUE) return 1;
    if (lchd_param_sum_plan(10, 66, 1000, &tile) != LCHD_EVALUE) return 1;
    if (lchd_param_sum_plan(10, 5, -1, &tile) != LCHD_EVALUE) return 1;
    if (lchd_param_sum_plan(10, 5, 1000, NULL) != LCHD_EVALUE) return 1;
    if (strlen(lchd_last_error()) == 0) return 1;
    printf("plan ok\n");
    return 0;
}
#endif

static int replay(const char *path) {
    FILE *f = fopen(path, "r");
    char name[64];
    long long P, W, has_w, has_b, nb;
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        return 1;
    }
    while (fscanf(f, " case %63s %lld %lld %lld %lld %lld", name, &P, &W, &has_w, &has_b, &nb) == 6) {
        double *rows = (double *)malloc(sizeof(double) * (size_t)(P * W));
        double *v = has_w ? (double *)malloc(sizeof(double) * (size_t)P) : NULL;
        int32_t *bucket = has_b ? (int32_t *)malloc(sizeof(int32_t) * (size_t)P) : NULL;
        int64_t *acc = (int64_t *)calloc((size_t)(nb * W) * LCHD_GRAD_LIMBS, sizeof(int64_t));
        double *out = (double *)malloc(sizeof(double) * (size_t)(nb * W));
        long long p, k;
        int ok;
        if (!rows || (has_w && !v) || (has_b && !bucket) || !acc || !out) return 1;
        for (p = 0; p < P; ++p) {
            char tok[64];
            for (k = 0; k < W; ++k) {
                if (fscanf(f, " %63s", tok) != 1) return 1;
                rows[p * W + k] = strtod(tok, NULL);
            }
            if (has_w) {
                if (fscanf(f, " %63s", tok) != 1) return 1;
                v[p] = strtod(tok, NULL);
            }
            if (has_b) {
                int b;
                if (fscanf(f, " %d", &b) != 1) return 1;
                bucket[p] = b;
            }
        }
        ok = lchd_param_sum_rows(rows, P, (int)W, W, v, bucket, (int)nb, acc);
        lchd_param_finish(acc, nb * W, out);
        printf("sum %s %d", name, ok ? 0 : 1);
        for (k = 0; k < nb * W; ++k) printf(" %a", out[k]);
        printf("\n");
        free(rows);
        free(v);
        free(bucket);
        free(acc);
        free(out);
    }
    fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s CASES\n", argv[0]);
        return 2;
    }
    if (replay(argv[1])) return 1;
#ifdef WITH_LIBRARY
    if (check_plan()) return 1;
#endif
    printf("cabi param sum ok\n");
    return 0;
}
