// lchd_pair_columns.h -- the column-tile skeleton of the per-pair profile kernels (k_radial, k_attribution, k_category_gradient,
// k_sensitivity).  One pair per wavefront, grid-stride over pairs; tiles of kSweepTile merged events from the keys and category ids of
// both stores; lane l owns ceil(T / 64) consecutive events of a tile (merge path); the category counts at a lane's first event come
// from a wave scan of the per-lane histograms (LDS columns, count_A | count_B << 16); the lane then walks its events.  A lane's
// intervals are: lane 0, the interval the previous tile (or the anchors) left open; then event to event; then from its last event to
// the FIRST event of the next lane.  The last lane with events leaves its interval open for the next tile; the tail to F(inf) is
// lane 0's, on the counts of the whole pair.
//   pair_head_load         the pair record of k_pair_meta, the weight-function index and the "unusable pair" verdict
//   column_carve           the LDS of one wavefront; column_wave_bytes its size
//   column_seed_anchors    the two anchors in the carry row and in every lane's column (the walk below seeds them in the loop that
//                          empties its accumulators: two loops in place of that one cost it 120 instructions)
//   column_tile_stage      one tile into LDS and its merge-path split across the lanes
//   column_histogram_scan  pass 1: the counts in front of every lane's first event
//   walk_category_columns  the whole walk of the kernels whose events only end intervals: per interval a caller's add_interval on
//                          the lane's counts, per pair one row of per-category sums reduced in lane order
//   launch_most_waves, raise_dynamic_lds    the launchers' choice of pairs per workgroup and the dynamic-LDS attribute
// The event loops of k_radial and k_sensitivity carry per-event state (bins; per-slot stores and H handed from lane to lane) and stay
// in their files.
#pragma once
#include <initializer_list>

#include "lchd_sweep_common.h"

namespace lchd {

constexpr uint32_t kOneA = 1u, kOneB = 1u << 16, kMaskA = 0xFFFFu;  // a count column's entry: count_A | count_B << 16
constexpr int kColumnDynMax = 150 * 1024;  // dynamic LDS the instantiations are allowed (+ the static tables: below the 160 KB of a CU)

// ---- the pair record --------------------------------------------------------------------------------------------------------------------
struct PairHead {
    int64_t ea, eb;  // the pair's environments in the two stores
    int nA, nB;      // their points, anchors included
    int c0a, c0b;    // the anchors' categories
    int wfi;         // the pair's weight function
    bool usable;     // false: anchor out of range / overflowed or empty environment (flagged where it happened), or an index outside the dictionary
};
// Wave-uniform.  CAT16: the 16-bit-category pair record.  n_sets: weight functions the stores have keys for.
template <bool CAT16>
__device__ __forceinline__ PairHead pair_head_load(const SweepArgs& args, int64_t p, int n_sets, int lane) {
    const int4 m = args.meta[p];
    const int mx = __builtin_amdgcn_readfirstlane(m.x), my = __builtin_amdgcn_readfirstlane(m.y);
    const int mz = __builtin_amdgcn_readfirstlane(m.z), mw = __builtin_amdgcn_readfirstlane(m.w);
    PairHead h;
    h.nA = CAT16 ? (mz & 0xFFFF) : (mz & 0xFFFFFF);
    h.nB = CAT16 ? (mw & 0xFFFF) : (mw & 0xFFFFFF);
    h.wfi = __builtin_amdgcn_readfirstlane(args.wf_index ? args.wf_index[p] : 0);
    const bool bad_wf = h.wfi < 0 || h.wfi >= n_sets;
    h.usable = !(h.nA <= 0 || h.nB <= 0 || h.nA > kRadialMaxPoints || h.nB > kRadialMaxPoints || bad_wf);
    if (bad_wf && lane == 0) sweep_report(args.hst, ST_BAD_WF);
    h.ea = mx;
    h.eb = my;
    h.c0a = CAT16 ? ((mz >> 16) & 0xFFFF) : ((mz >> 24) & 255);
    h.c0b = CAT16 ? ((mw >> 16) & 0xFFFF) : ((mw >> 24) & 255);
    return h;
}

// ---- the LDS of one wavefront -------------------------------------------------------------------------------------------------------------
// two key tiles | `front` bytes of the kernel's own (a multiple of 8) | count columns [C][64] | carry row [C] | two category tiles
struct ColumnLds {
    uint64_t *sA, *sB;
    unsigned char* front;
    uint32_t *cnt0, *carry;  // lane l's count column is cnt0 + l: cnt[c * 64]; carry[c]: the counts before the current tile
    uint16_t *cA, *cB;
};
constexpr size_t column_wave_bytes(int C, size_t front) {
    return ((size_t)kSweepTile * 16 + front + (size_t)C * 260 + (size_t)kSweepTile * 4 + 15) & ~(size_t)15;
}
__device__ __forceinline__ ColumnLds column_carve(unsigned char* base, int C, size_t front) {
    ColumnLds l;
    l.sA = reinterpret_cast<uint64_t*>(base);
    l.sB = l.sA + kSweepTile;
    l.front = reinterpret_cast<unsigned char*>(l.sB + kSweepTile);
    l.cnt0 = reinterpret_cast<uint32_t*>(l.front + front);
    l.carry = l.cnt0 + (size_t)C * 64;
    l.cA = reinterpret_cast<uint16_t*>(l.carry + C);
    l.cB = l.cA + kSweepTile;
    return l;
}
// The byte counts of the four kernels, spelled out per kernel: 7 680 bytes of tiles, 260 per category, and in front of the count columns
// radial's bounds and bins (65 + 64 doubles), the k = 1 .. 3 f64 columns [C][64] of the attribution / category-gradient modes, nothing
// for the sensitivities.
constexpr bool column_wave_bytes_hold() {
    auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
    for (int C = 1; C <= kWideCategories; ++C)
        if (column_wave_bytes(C, (65 + 64) * 8) != up16(7680 + 1032 + 260 * (size_t)C)) return false;
    for (int C = 1; C <= 64; ++C) {
        for (int k = 1; k <= 3; ++k)
            if (column_wave_bytes(C, (size_t)k * C * 512) != up16(7680 + (size_t)C * (260 + 512 * k))) return false;
        if (column_wave_bytes(C, 0) != up16(7680 + 260 * (size_t)C)) return false;
    }
    return true;
}
static_assert(kSweepTile == 384 && column_wave_bytes_hold(), "per-wavefront LDS of the profile kernels");

__device__ __forceinline__ void column_seed_anchors(const ColumnLds& l, uint32_t* cnt, int C, int c0a, int c0b, int lane) {
    for (int c = lane; c < C; c += 64) l.carry[c] = (c == c0a ? kOneA : 0u) | (c == c0b ? kOneB : 0u);
    for (int c = 0; c < C; ++c) cnt[c * 64] = (c == c0a ? kOneA : 0u) | (c == c0b ? kOneB : 0u);
}

// StatisticalDistance::run on one lane's count column (cnt[c * 64] = count_A | count_B << 16), normalised like pmf.rs:65-83; out of line:
// the library's pow / log stay out of the event loop's code (k_sensitivity, k_weight_gradient).
static __device__ __noinline__ double sens_sd(int kind, double p0, double p1, const uint32_t* cnt, const double* __restrict__ w, int C, double ia,
                                              double ib) {
    return sd_eval<0>(kind, p0, p1, [&](int c) { return (w[c] * (double)(cnt[c * 64] & 0xFFFFu)) * ia; },
                      [&](int c) { return (w[c] * (double)(cnt[c * 64] >> 16)) * ib; }, C);
}

// ---- one tile -----------------------------------------------------------------------------------------------------------------------------
struct ColumnTile {
    int T;               // events of the tile
    int d0, d1;          // this lane's events [d0, d1) of the tile, [i0, i1) of the staged A run and [j0, j1) of the B run
    int i0, i1, j0, j1;
    int iend;            // A events of the whole tile
    int last;            // the last lane with events (wave-uniform)
    bool has;            // this lane has events
};
// Stages the tile that starts ia / ib non-anchor points into the two lists (kA / kB keys, tA / tB categories; mA / mB non-anchor points,
// k0 of M = mA + mB merged events done) and splits it.
template <typename CT>
__device__ __forceinline__ ColumnTile column_tile_stage(const ColumnLds& l, const uint64_t* kA, const uint64_t* kB, const CT* tA, const CT* tB, int mA, int mB,
                                                        int M, int k0, int ia, int ib, int lane) {
    constexpr int TILE = kSweepTile;
    ColumnTile t;
    t.T = min(TILE, M - k0);
    const int nAt = min(TILE, mA - ia), nBt = min(TILE, mB - ib);
    wave_sync_lds();  // previous tile fully consumed
    for (int q = lane; q < nAt; q += 64) { l.sA[q] = kA[1 + ia + q]; l.cA[q] = tA[1 + ia + q]; }
    for (int q = lane; q < nBt; q += 64) { l.sB[q] = kB[1 + ib + q]; l.cB[q] = tB[1 + ib + q]; }
    wave_sync_lds();
    const int epl = (t.T + 63) >> 6;
    t.d0 = min(lane * epl, t.T);
    t.d1 = min(t.d0 + epl, t.T);
    t.i1 = merge_path(l.sA, nAt, l.sB, nBt, t.d1);
    t.i0 = __shfl_up(t.i1, 1);
    if (lane == 0) t.i0 = 0;
    t.iend = __builtin_amdgcn_readlane(t.i1, 63);
    t.j0 = t.d0 - t.i0;
    t.j1 = t.d1 - t.i1;
    t.last = (t.T - 1) / epl;
    t.has = t.d0 < t.d1;
    return t;
}

// pass 1: histogram of this lane's chunk into its column, wave scan per category with the carry; the column then holds the counts in
// front of the lane's first event, which also go to per_category(excl).  True: the chunk has a category outside the configuration.
template <typename PerCategory>
__device__ __forceinline__ bool column_histogram_scan(const ColumnLds& l, uint32_t* cnt, const ColumnTile& t, int C, int lane, PerCategory&& per_category) {
    bool bad_cat = false;
    for (int c = 0; c < C; ++c) cnt[c * 64] = 0u;
    for (int i = t.i0; i < t.i1; ++i) {
        const int ct = l.cA[i];
        if (ct >= C) bad_cat = true; else cnt[ct * 64] += kOneA;
    }
    for (int j = t.j0; j < t.j1; ++j) {
        const int ct = l.cB[j];
        if (ct >= C) bad_cat = true; else cnt[ct * 64] += kOneB;
    }
    for (int c = 0; c < C; ++c) {
        const uint32_t own = cnt[c * 64];
        const uint32_t incl = wave_incl_scan_u32(own + (lane == 0 ? l.carry[c] : 0u));
        const uint32_t excl = incl - own;
        cnt[c * 64] = excl;
        if (lane == 63) l.carry[c] = incl;
        per_category(excl);
    }
    return bad_cat;
}

// ---- the walk of k_attribution and k_category_gradient --------------------------------------------------------------------------------------
// What add_interval sees of the walk besides the lane's count column.
struct ColumnWalk {
    int totA, totB;  // points per side in the lane's counts (incl. the anchor)
    bool zero_norm;  // set by add_interval: a side's weighted counts sum to 0
};
// Every pair of this wavefront (WPB wavefronts per workgroup, this one wv): out[p][c] = finish(c, sum over the pair's intervals of what
// add_interval(dF, walk) added to acc[c * 64], the lane's accumulator column (LDS, in ColumnLds::front)), lanes summed in lane order --
// no floating-point atomics, no cross-wave traffic, one fixed summation shape for a stored pair.  A row is NaN for an unusable pair, a
// category outside the configuration (ST_BAD_CATEGORY) or a zero norm (ST_ZERO_NORM).
template <int WPB, typename AddInterval, typename Finish>
__device__ __forceinline__ void walk_category_columns(const SweepArgs& args, double* rows, const ColumnLds& l, double* acc, int lane, int wv,
                                                      AddInterval&& add_interval, Finish&& finish) {
    const DevConfig* __restrict__ cfgp = args.cfg;
    const int C = cfgp->n_categories;
    uint32_t* const cnt = l.cnt0 + lane;
    const int n_sets = args.env_a.cdf_keys;
    const double* __restrict__ finf_tab = cfgp->wf_finf;
    const int64_t pstride = (int64_t)gridDim.x * WPB;
    for (int64_t p = (int64_t)blockIdx.x * WPB + wv; p < args.n_pairs; p += pstride) {
        double* const out = rows + p * (int64_t)C;
        const PairHead h = pair_head_load<false>(args, p, n_sets, lane);
        if (!h.usable) {
            for (int c = lane; c < C; c += 64) out[c] = nan("");
            continue;
        }
        const uint64_t* __restrict__ kA = args.env_a.key + h.ea * args.env_a.stride + (int64_t)h.wfi * args.env_a.set_stride;
        const uint64_t* __restrict__ kB = args.env_b.key + h.eb * args.env_b.stride + (int64_t)h.wfi * args.env_b.set_stride;
        const uint8_t* __restrict__ tA = args.env_a.cat + h.ea * args.env_a.stride;
        const uint8_t* __restrict__ tB = args.env_b.cat + h.eb * args.env_b.stride;
        const double Finf = finf_tab[h.wfi];

        bool bad_cat = h.c0a >= C || h.c0b >= C;
        ColumnWalk w{1, 1, false};
        // empty accumulators, the two anchors (src/locohd.rs:82-84)
        wave_sync_lds();
        for (int c = lane; c < C; c += 64) l.carry[c] = (c == h.c0a ? kOneA : 0u) | (c == h.c0b ? kOneB : 0u);
        for (int c = 0; c < C; ++c) {
            cnt[c * 64] = (c == h.c0a ? kOneA : 0u) | (c == h.c0b ? kOneB : 0u);
            acc[c * 64] = 0.0;
        }
        wave_sync_lds();
        double F_carry = u2d(kA[0]);  // F(0): both anchors sit at distance 0

        const int mA = h.nA - 1, mB = h.nB - 1, M = mA + mB;  // non-anchor events
        int ia = 0, ib = 0;
        for (int k0 = 0; k0 < M; k0 += kSweepTile) {
            const ColumnTile t = column_tile_stage(l, kA, kB, tA, tB, mA, mB, M, k0, ia, ib, lane);
            if (column_histogram_scan(l, cnt, t, C, lane, [](uint32_t) {})) bad_cat = true;
            w.totA = 1 + ia + t.i0;
            w.totB = 1 + ib + t.j0;

            // pass 2: this lane's events, one after the other; every interval is added on the counts in front of the event that ends it
            int i = t.i0, j = t.j0;
            uint64_t ka = (i < t.i1) ? l.sA[i] : kPadKey, kb = (j < t.j1) ? l.sB[j] : kPadKey;
            const double firstF = t.has ? u2d(ka <= kb ? ka : kb) : 0.0;
            const double nextF = shfl_f64(firstF, min(lane + 1, 63));  // the first event of the next lane's chunk
            double Fp = F_carry;
            bool open = lane == 0;  // lane 0 closes the interval the previous tile (or the anchors) left open
            for (int e = t.d0; e < t.d1; ++e) {
                const bool takeA = (ka <= kb);  // an exhausted run shows the pad key (> every real key)
                const uint64_t key = takeA ? ka : kb;
                const int ct = takeA ? l.cA[i] : l.cB[j];
                if (takeA) { ++i; ka = (i < t.i1) ? l.sA[i] : kPadKey; } else { ++j; kb = (j < t.j1) ? l.sB[j] : kPadKey; }
                const double F = u2d(key);
                if (open && !bad_cat) add_interval(F - Fp, w);
                open = true;
                // pmf.rs:47-63: one more point of category ct on one side
                if (ct < C) cnt[ct * 64] += takeA ? kOneA : kOneB;
                else bad_cat = true;
                w.totA += takeA ? 1 : 0;
                w.totB += takeA ? 0 : 1;
                Fp = F;
            }
            if (t.has && lane < t.last && !bad_cat) add_interval(nextF - Fp, w);
            F_carry = readlane_f64(Fp, t.last);
            ia += t.iend;
            ib += t.T - t.iend;
        }
        // the last interval to +inf (:165-171,204-210,212-221) on the counts of the whole pair, by lane 0
        wave_sync_lds();
        const unsigned long long anybad = __ballot(bad_cat);
        if (lane == 0 && !anybad) {
            for (int c = 0; c < C; ++c) cnt[c * 64] = l.carry[c];
            w.totA = h.nA;
            w.totB = h.nB;
            add_interval(Finf - F_carry, w);
        }
        wave_sync_lds();
        const unsigned long long anyzero = __ballot(w.zero_norm);
        if (lane == 0) {
            if (anybad) sweep_report(args.hst, ST_BAD_CATEGORY);
            if (anyzero) sweep_report(args.hst, ST_ZERO_NORM);
        }
        // the row: one wave reduction per category, in lane order
        for (int c = 0; c < C; ++c) {
            const double s = wave_sum_f64(acc[c * 64]);
            if (lane == 0) out[c] = (anybad || anyzero) ? nan("") : finish(c, s);
        }
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------------
// go(pairs per workgroup as an integral_constant, workgroups) with the most pairs per workgroup (4, 2 or 1) whose LDS fits dyn_max;
// false if one pair's does not.
template <typename Go>
bool launch_most_waves(size_t dyn_max, size_t wave_bytes, int64_t n_pairs, Go&& go) {
    auto run = [&](auto wpb) {
        constexpr int WPB = decltype(wpb)::value;
        const int64_t blocks = (n_pairs + WPB - 1) / WPB;
        go(wpb, (unsigned)(blocks < 8192 ? blocks : 8192));
    };
    if (wave_bytes * 4 <= dyn_max) run(std::integral_constant<int, 4>{});
    else if (wave_bytes * 2 <= dyn_max) run(std::integral_constant<int, 2>{});
    else if (wave_bytes <= dyn_max) run(std::integral_constant<int, 1>{});
    else return false;
    return true;
}
template <typename K>
const void* kernel_ptr(K* k) { return reinterpret_cast<const void*>(k); }
inline void raise_dynamic_lds(std::initializer_list<const void*> kernels, int bytes) {
    for (const void* fn : kernels) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

}  // namespace lchd
