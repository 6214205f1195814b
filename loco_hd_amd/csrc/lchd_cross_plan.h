// lchd_cross_plan.h -- the tile size of a cross-scoring call (lchd_cross_plan, include/loco_hd_hip.h) as a pure host function: no HIP,
// no device, compiled by the host compiler alone in tests/cross_plan_cases.cpp.
#pragma once
#include <cstdint>

namespace lchd {

constexpr int64_t kCrossPairBytes = 16 + 4 + 8;          // per pair of a tile: its [2] int64 record, its wf index, its score scratch
constexpr int64_t kCrossMaxTilePairs = 0x7FFFFFFF;       // what one pass takes (lchd_from_primitives_dev)
constexpr int kNearestMaxK = 64;                         // one result per lane of k_nearest_rows' wavefront

// The largest tile_rows in 1 .. n_a with tile_rows * n_b * kCrossPairBytes <= budget_bytes and tile_rows * n_b <= kCrossMaxTilePairs;
// 0: not even one row fits.  n_a >= 1, n_b >= 1, budget_bytes >= 0 (the entry point checks).  Divisions only: no product can overflow.
inline int64_t cross_plan_rows(int64_t n_a, int64_t n_b, int64_t budget_bytes) {
    const int64_t by_budget = budget_bytes / kCrossPairBytes / n_b;  // floor(floor(x / p) / q) == floor(x / (p q)) for positive integers
    const int64_t by_pairs = kCrossMaxTilePairs / n_b;
    const int64_t rows = by_budget < by_pairs ? by_budget : by_pairs;
    return rows < n_a ? rows : n_a;
}

}  // namespace lchd
