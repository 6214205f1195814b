/* A stand-alone C99 client of the HOST path of loco_hd_amd/csrc/lchd_exact_sum.h, built by tests/test_exact_sum_host.py with
 * -fsanitize=address,undefined and run as a child process.  Replays the vectors of the file named on the command line -- per vector a
 * line with the count n, then n lines with the bits of one double each (hex) -- through lchd_xs_add and lchd_xs_finish, and prints per
 * vector:   the eight limbs (decimal)  the status flag  the bits of the finished double (hex). */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include "lchd_exact_sum.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s vectors.txt\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    long n;
    while (fscanf(f, "%ld", &n) == 1) {
        int64_t *limbs = (int64_t *)calloc(LCHD_GRAD_LIMBS, sizeof(int64_t)); /* (heap: the sanitizer sees an access beyond limb 7) */
        uint32_t flag = 0;
        if (!limbs) return 2;
        for (long i = 0; i < n; ++i) {
            uint64_t b;
            double s;
            if (fscanf(f, "%" SCNx64, &b) != 1) { fprintf(stderr, "short vector\n"); return 2; }
            memcpy(&s, &b, 8);
            lchd_xs_add(limbs, s, &flag);
        }
        const double r = lchd_xs_finish(limbs);
        uint64_t rb;
        memcpy(&rb, &r, 8);
        for (int k = 0; k < LCHD_GRAD_LIMBS; ++k) printf("%" PRId64 " ", limbs[k]);
        printf("%u %016" PRIx64 "\n", flag, rb);
        free(limbs);
    }
    fclose(f);
    return 0;
}
