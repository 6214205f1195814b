// The tile planner of the cross-scoring calls (loco_hd_amd/csrc/lchd_cross_plan.h: cross_plan_rows) over a table of cases at every limit
// of its two rules, one line per case: "name: rows=R".  A stand-alone host program: no HIP, no device.  tests/test_cross_host.py builds
// it with -fsanitize=address,undefined, runs it and compares with expectations written out by hand.
#include <cstdint>
#include <cstdio>

#include "lchd_cross_plan.h"

using namespace lchd;

static void show(const char* name, int64_t n_a, int64_t n_b, int64_t budget) {
    printf("%s: rows=%lld\n", name, (long long)cross_plan_rows(n_a, n_b, budget));
}

int main() {
    printf("constants: pair_bytes=%lld max_tile_pairs=%lld max_k=%d\n", (long long)kCrossPairBytes, (long long)kCrossMaxTilePairs, kNearestMaxK);
    const int64_t P = kCrossPairBytes, CAP = kCrossMaxTilePairs, I64 = INT64_MAX;
    // the budget rule: 7 rows of 130 pairs
    show("fits_exactly", 100, 130, 7 * 130 * P);
    show("one_byte_below", 100, 130, 7 * 130 * P - 1);
    show("one_row_exactly", 100, 130, 130 * P);
    show("one_row_one_byte_below", 100, 130, 130 * P - 1);
    show("no_budget", 100, 130, 0);
    // never above n_a
    show("clamped_to_n_a", 37, 130, I64);
    show("single_anchor", 1, 130, I64);
    show("single_anchor_tight", 1, 130, 130 * P);
    show("single_column", 5, 1, 3 * P);
    // the pair cap of one pass
    show("cap_row_at_limit", 10, CAP, I64);
    show("cap_row_above_limit", 10, CAP + 1, I64);
    show("cap_two_rows", 10, CAP / 2, I64);
    show("cap_two_rows_plus_1", 10, CAP / 2 + 1, I64);
    show("cap_65536", 1 << 20, 65536, I64);  // 32 767 rows: 32 768 * 65 536 == 2^31
    // nothing overflows at the largest arguments
    show("largest_arguments", I64, I64, I64);
    show("largest_rows", I64, 1, I64);
    return 0;
}
