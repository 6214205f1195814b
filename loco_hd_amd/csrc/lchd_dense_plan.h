// lchd_dense_plan.h -- which kernel sorts the dense rows of a from_coords / from_dmxs / dense-ensemble call, as ONE pure host function
// (plan_dense; exported as lchd_plan_dense, include/loco_hd_hip.h).  dense_pass and ensemble_core (lchd_capi.hip) ask it once per attempt
// and hand the answer to launch_dense_fused, launch_env_rows2 and launch_env_rows, which switch on it and compare no length themselves.
// Every row-length, category-width and capacity limit of the three kernels is a constant of this file; the kernels' static_asserts and
// tests/test_dense_plan.py hold them against the template parameters.  No context, no device, no HIP header.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/loco_hd_hip.h"
#include "lchd_pass_plan.h"

#if defined(__HIPCC__)
#define LCHD_PLAN_HD __host__ __device__
#else
#define LCHD_PLAN_HD
#endif

namespace lchd {

// ---- k_dense_fused (lchd_dense_fused.hip) --------------------------------------------------------------------------------------
// Hellinger-2 with unit category weights, at most kDenseFusedMaxCat categories, rows of kDenseFusedMinRow < n <= kDenseFusedMaxRow points
constexpr int kDenseFusedMinRow = 1024, kDenseFusedMaxRow = 20480, kDenseFusedMaxCat = 16;
constexpr int kDenseFusedSegCap = 6144;  // events of one distance segment (keys + values in LDS)
constexpr int kDenseFusedSample = 4;     // the coarse CDF of a row pair is estimated from every 4th point of either row
constexpr int kDenseFusedMaxSeg = 16;    // segments of a row pair's scratch region
constexpr int kDenseFusedGrid = 512;     // workgroups of a launch
// events a segment may be PLANNED to hold: the plan sees a sample, the segment must hold the real thing (six standard deviations of the
// count that a sample of one in kDenseFusedSample predicts, and a coarse bin's worth)
LCHD_PLAN_HD inline int dense_fused_seg_margin(int est) { return 6 * (int)sqrtf((float)(est * kDenseFusedSample)) + 70; }
// Segments of a workgroup's scratch region for row pairs of `total` events: the plan starts at ceil(total / cap) segments and adds some
// until the sample's estimates fit with their margin; two more than the balanced plan needs cover every row pair whose sample is not
// grossly off (otherwise: ST_ROW_RETRY).
inline int dense_fused_segments(int64_t total) {
    int S = (int)std::max<int64_t>(1, (total + kDenseFusedSegCap - 1) / kDenseFusedSegCap);
    while (S < kDenseFusedMaxSeg && (int)(total / S) + dense_fused_seg_margin((int)(total / S)) > kDenseFusedSegCap) ++S;
    return std::min(kDenseFusedMaxSeg, S + 2);
}

// ---- k_env_rows2 (lchd_env_rows.hip) -------------------------------------------------------------------------------------------
// One launch for both sides; <NT, EPT, 1> holds a row of NT * EPT points in registers, <1024, kRows2SegEpt, 2> sorts a longer row in two
// distance segments (and gives up -- ST_ROW_RETRY -- on a row whose segments come out unbalanced or whose buckets overflow).
constexpr int kRows2OneSeg = 16384;   // longest row of the one-segment instantiations (= the key array, n2)
constexpr int kRows2MaxRow = 20480;   // longest row of the two-segment instantiation (1024 threads x kRowLongEpt points)
constexpr int kRows2SegEpt = 12;
struct Rows2Inst { int nt, ept, upto; };  // rows of at most `upto` points (NT * EPT == upto: sized to fit exactly at its limit)
inline constexpr Rows2Inst kRows2Ladder[] = {{64, 16, 1024}, {256, 16, 4096}, {1024, 8, 8192}, {1024, 10, 10240}, {1024, 16, 16384}};

// ---- k_env_rows (lchd_env_rows.hip) --------------------------------------------------------------------------------------------
constexpr int kRowBucketsSmall = 2048;   // distance buckets of the dense-row sort (rows <= 16384 points)
constexpr int kRowBucketsMax = 8192;     // ... of k_env_rows2 when the row leaves room for them
constexpr int kRowBucketsBig = 16384;    // ... for rows of up to 65536 points (keys stay in global memory)
constexpr int kRowBucketsHuge = 32768;   // ... for longer rows
constexpr int kRowsLdsCap = 16384;       // largest slot whose keys and 8-bit categories are sorted in LDS (9 bytes per point)
constexpr int kRowsLdsCap16 = 8192;      // ... with 16-bit categories (10 bytes per point)
constexpr int kRowsBigCap = 65536;       // largest slot of the kRowBucketsBig form; beyond it kRowBucketsHuge, 8-bit categories only
constexpr int kRowsMaxCap = 1 << 23;     // largest slot at all
constexpr int kRowsMaxPoints16 = 65535;  // longest dense row with 16-bit categories (the sweep's 64-bit-count form has 8-bit ids only)

// One side of the k_env_rows path: rows of at most row_len points in slots of `cap` points.  false: no instantiation.
inline bool plan_dense_rows_side(int64_t cap, int64_t row_len, bool cat16, lchd_dense_rows_side& p) {
    p = lchd_dense_rows_side{};
    if (row_len < 1 || row_len > cap || cap > kRowsMaxCap) return false;
    if (cat16 && cap > kRowsBigCap) return false;
    p.cap = (int32_t)cap;
    p.cat_bytes = cat16 ? 2 : 1;
    const int lds_cap = cat16 ? kRowsLdsCap16 : kRowsLdsCap;
    if (cap > lds_cap) {  // keys in global memory, the histogram alone in LDS
        p.nt = 1024;
        p.globalkv = 1;
        p.buckets = cap > kRowsBigCap ? kRowBucketsHuge : kRowBucketsBig;
        return true;
    }
    p.globalkv = 0;
    p.buckets = kRowBucketsSmall;
    // (16-bit categories: no 256-thread instantiation)
    p.nt = cap <= 1024 ? 64 : ((cap <= 4096 && !cat16) ? 256 : 1024);
    return true;
}

inline bool dense_query_ok(const lchd_dense_query& q) {
    return q.n_categories >= 1 && q.attempt >= 0 && q.attempt <= 1 && !(q.hooks & ~(uint32_t)(LCHD_DENSE_HOOK_OLD_ROWS | LCHD_DENSE_HOOK_NO_FUSED));
}

// The plan of one attempt of a dense call.  Exactly one path for every supported query.
inline lchd_dense_plan plan_dense(const lchd_dense_query& q) {
    lchd_dense_plan p{};
    const int64_t longest = std::max(q.cols_a, q.cols_b), shortest = std::min(q.cols_a, q.cols_b);
    const bool cat16 = q.cat16 != 0;
    if (shortest < 1 || longest > kRowsMaxCap || (cat16 && longest > kRowsMaxPoints16)) {
        p.unsupported = 1;
        return p;
    }
    // the second attempt, like LCHD_OLD_ROWS: the kernel that never gives up on a row
    const bool old_rows = (q.hooks & LCHD_DENSE_HOOK_OLD_ROWS) || q.attempt > 0;
    // The common configuration: sort and sweep in ONE kernel per row pair, nothing but the score is written.
    if (!old_rows && !(q.hooks & LCHD_DENSE_HOOK_NO_FUSED) && !q.single_attempt && !cat16 && q.hellinger2 && q.unit_weights &&
        q.n_categories <= kDenseFusedMaxCat && longest > kDenseFusedMinRow && longest <= kDenseFusedMaxRow) {
        p.path = LCHD_DENSE_FUSED;
        p.fused_slots = q.n_categories <= 8 ? 8 : (q.n_categories <= 12 ? 12 : 16);
        p.fused_dmx = q.given_rows ? 1 : 0;
        p.scr_segs = dense_fused_segments(q.cols_a + q.cols_b);
        return p;
    }
    // Both sides in one launch of the register-resident sort.  Two segments: one launch has one segment count, so both sides must be
    // long and no row may be short (ragged rows), and the caller must be able to repeat the call.
    const bool two_seg = longest > kRows2OneSeg;
    if (!old_rows && !cat16 && longest <= kRows2MaxRow && !(two_seg && (shortest <= kRows2OneSeg || q.ragged || q.single_attempt))) {
        p.path = LCHD_DENSE_ROWS2;
        p.n2 = (int32_t)std::min<int64_t>(next_pow2_host(longest), kRows2OneSeg);
        if (two_seg) {
            p.nt = 1024; p.ept = kRows2SegEpt; p.seg = 2;
            return p;
        }
        p.seg = 1;
        for (const Rows2Inst& inst : kRows2Ladder)
            if (longest <= inst.upto) { p.nt = inst.nt; p.ept = inst.ept; break; }
        return p;
    }
    // One launch per side of the three-pass sort (any length up to kRowsMaxCap, 16-bit categories).
    p.path = LCHD_DENSE_ROWS;
    if (!plan_dense_rows_side(next_pow2_host(q.cols_a), q.cols_a, cat16, p.rows[0]) ||
        !plan_dense_rows_side(next_pow2_host(q.cols_b), q.cols_b, cat16, p.rows[1])) {
        p = lchd_dense_plan{};
        p.unsupported = 1;
    }
    return p;
}

}  // namespace lchd
