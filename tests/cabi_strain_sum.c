/* cabi_strain_sum.c -- the host path of loco_hd_amd/csrc/lchd_strain_sum.h, replayed on slot lists from a file.
 *
 * Input (text): per case one line "n", then n lines of six hexadecimal float64 bit patterns: v g dist disp0 disp1 disp2.  The caller has
 * applied the use rule; every line is a used slot.  The slots are dealt round-robin to LANES sets of partial sums, as the lanes of a
 * wavefront take the slots of a row, added with lchd_strain_part_add, and the sets are summed limb by limb (the wavefront's reduction).
 * Output per case: the 48 limbs, the flag, and the nine finished doubles as bit patterns.
 * The same terms also go through lchd_xs_add, the memory path of lchd_exact_sum.h; both must give the same limbs (exit status 2 if not).
 */
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include "lchd_strain_sum.h"

#define LANES 7

static double from_bits(uint64_t b) {
    double d;
    memcpy(&d, &b, 8);
    return d;
}

int main(int argc, char **argv) {
    FILE *f;
    long n;
    if (argc != 2 || !(f = fopen(argv[1], "r"))) return 1;
    while (fscanf(f, "%ld", &n) == 1) {
        int64_t(*part)[LCHD_STRAIN_COMPONENTS][LCHD_GRAD_LIMBS] = calloc(LANES, sizeof *part);
        int64_t total[LCHD_STRAIN_LIMBS] = {0}, memory[LCHD_STRAIN_LIMBS] = {0};
        uint32_t flag = 0, flag_memory = 0;
        double w[9];
        long s;
        int c, k, lane;
        if (!part) return 1;
        for (s = 0; s < n; ++s) {
            uint64_t b[6];
            double disp[3], term[LCHD_STRAIN_COMPONENTS];
            if (fscanf(f, "%" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64, b, b + 1, b + 2, b + 3, b + 4, b + 5) != 6) return 1;
            disp[0] = from_bits(b[3]);
            disp[1] = from_bits(b[4]);
            disp[2] = from_bits(b[5]);
            if (!lchd_strain_slot(part[s % LANES], from_bits(b[0]), from_bits(b[1]), from_bits(b[2]), disp)) flag |= LCHD_XS_OUT_OF_RANGE;
            lchd_strain_terms((from_bits(b[0]) * from_bits(b[1])) / from_bits(b[2]), disp, term);
            for (c = 0; c < LCHD_STRAIN_COMPONENTS; ++c) lchd_xs_add(memory + c * LCHD_GRAD_LIMBS, term[c], &flag_memory);
        }
        for (lane = 0; lane < LANES; ++lane)
            for (c = 0; c < LCHD_STRAIN_COMPONENTS; ++c)
                for (k = 0; k < LCHD_GRAD_LIMBS; ++k) total[c * LCHD_GRAD_LIMBS + k] += part[lane][c][k];
        free(part);
        if (memcmp(total, memory, sizeof total) || flag != flag_memory) return 2;
        lchd_strain_finish(total, w);
        for (k = 0; k < LCHD_STRAIN_LIMBS; ++k) printf("%" PRId64 " ", total[k]);
        printf("%u", flag);
        for (k = 0; k < 9; ++k) {
            uint64_t bits;
            memcpy(&bits, &w[k], 8);
            printf(" %" PRIx64, bits);
        }
        printf("\n");
    }
    fclose(f);
    return 0;
}
