// lchd_attribution.hip -- score attribution by category (additive, not in the reference): which primitive types carry a pair's score.
//
//   t_c(r) = |a_c^(1/e) - b_c^(1/e)|^e      T(r) = sum_c t_c(r)      H(r) = (T / 2)^(1/e)
//   out[p][c] = sum_j (F(u_{j+1}) - F(u_j)) * H_j * t_{c,j} / T_j          (a piece with T_j = 0 adds 0 to every column)
//
// over the merged breakpoints u_0 = 0 <= u_1 <= ... <= u_J of the pair's two environments (u_{J+1} = +inf), a / b the weighted,
// normalised PMFs between u_j and u_{j+1} -- exactly what the sweeps integrate, the anchors included.  Only the Hellinger distance
// is a sum of one term per category, so only it decomposes; a row sums to the pair's score.
//
// Shape: k_radial's (lchd_radial.hip) without the bins.  One pair per wavefront; tiles of kSweepTile merged events read from the F
// keys of both stores (EnvStore::cdf_keys >= 1) and the pair records of k_pair_meta; lane l owns ceil(T / 64) consecutive events of a
// tile (merge path); the category counts at a lane's first event come from a wave scan of the per-lane histograms (LDS columns,
// count_A | count_B << 16); the lane then walks its events.  A lane's intervals are: lane 0, the interval the previous tile (or the
// anchors) left open; then event to event; then from its last event to the FIRST event of the next lane.  The last lane with events
// leaves its interval open for the next tile; the tail to F(inf) is lane 0's, on the counts of the whole pair.
// Sums: every interval adds dF * H * t_c / T for all C categories to the lane's accumulator column acc[c][lane] (LDS, next to its
// count column).  After the last tile one wave reduction per category in lane order writes the row: no floating-point atomics, no
// cross-wave traffic, one fixed summation shape for a stored pair.
// Terms: always the literal per-category form.  Exponent 2: (sqrt a_c - sqrt b_c)^2, H * t_c / T = t_c / (2 H); with unit weights the
// roots come from the sqrt / rsqrt tables of the counts.  Every other exponent goes through attribution_terms_pow, out of line: the
// library's pow stays out of the exponent-2 instantiations.
#include "lchd_sweep_common.h"

namespace lchd {

constexpr int kAttrTab = kSqrtTab + 8;   // LDS square-root tables: counts 0 .. kSqrtTab (stores of at most kSqrtTab points per slot)
constexpr int kAttrDynMax = 150 * 1024;  // dynamic LDS the instantiations are allowed (+ the static tables: below the 160 KB of a CU)
enum { ATTR_H2U = 0, ATTR_H2W = 1, ATTR_POW = 2 };  // Hellinger-2 with unit weights / with category weights / any other exponent

// The terms of one lane's count column (cnt[c * 64] = count_A | count_B << 16) for a general exponent e (statistical_distances.rs:4-10
// on pmf.rs:65-83's normalised vectors): term[c * 64] = t_c, *H = (T / 2)^(1/e), returns T.
static __device__ __noinline__ double attribution_terms_pow(double e, const uint32_t* cnt, const double* __restrict__ w, int C, double ia, double ib,
                                                            double* term, double* H) {
    const double inv = 1.0 / e;
    double T = 0.0;
    for (int c = 0; c < C; ++c) {
        const uint32_t v = cnt[c * 64];
        const double a = (w[c] * (double)(v & 0xFFFFu)) * ia, b = (w[c] * (double)(v >> 16)) * ib;
        const double t = pow(fabs(pow(a, inv) - pow(b, inv)), e);
        term[c * 64] = t;
        T += t;
    }
    *H = pow(T / 2.0, inv);
    return T;
}

// Per wavefront, in dynamic LDS: two key tiles | accumulator columns [C][64] f64 | (ATTR_POW: term columns [C][64] f64) |
// count columns [C][64] | carry row [C] | two category tiles
static size_t attribution_wave_bytes(int C, bool pow_terms) {
    return ((size_t)kSweepTile * 16 + (size_t)C * 512 * (pow_terms ? 2 : 1) + (size_t)C * 260 + (size_t)kSweepTile * 4 + 15) & ~(size_t)15;
}

// MODE: ATTR_*.  TAB: both stores have slots of at most kSqrtTab points, the square-root tables are read from LDS (ATTR_H2U alone
// reads them).  WPB: pairs (wavefronts) per workgroup.
template <int MODE, bool TAB, int WPB>
__global__ __launch_bounds__(64 * WPB) void k_attribution(AttributionArgs aa, int wave_bytes) {
    constexpr int TILE = kSweepTile;
    constexpr uint32_t kOneA = 1u, kOneB = 1u << 16, kMaskA = 0xFFFFu;
    extern __shared__ __attribute__((aligned(16))) unsigned char attr_smem[];
    __shared__ double t_sqrt[TAB ? kAttrTab : 1], t_rsqrt[TAB ? kAttrTab : 1];
    const SweepArgs& args = aa.sw;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const DevConfig* __restrict__ cfgp = args.cfg;
    const int C = cfgp->n_categories;
    const double* __restrict__ g_sqrt = args.sqrt_tab;
    const double* __restrict__ g_rsqrt = args.rsqrt_tab;
    const double* __restrict__ cat_w = cfgp->cat_w;
    if constexpr (TAB) {
        for (int k = tid; k < kAttrTab; k += 64 * WPB) { t_sqrt[k] = g_sqrt[k]; t_rsqrt[k] = g_rsqrt[k]; }
        __syncthreads();
    }
    unsigned char* const base = attr_smem + (size_t)wv * wave_bytes;
    uint64_t* const sA = reinterpret_cast<uint64_t*>(base);
    uint64_t* const sB = sA + TILE;
    double* const acc0 = reinterpret_cast<double*>(sB + TILE);
    double* const acc = acc0 + lane;                          // this lane's accumulator column: acc[c * 64]
    double* const term = acc + (size_t)C * 64;                // ATTR_POW: this lane's term column
    uint32_t* const cnt0 = reinterpret_cast<uint32_t*>(acc0 + (size_t)C * 64 * (MODE == ATTR_POW ? 2 : 1));
    uint32_t* const cnt = cnt0 + lane;                        // this lane's count column: cnt[c * 64]
    uint32_t* const carry = cnt0 + (size_t)C * 64;            // per category: counts before the current tile
    uint16_t* const cA = reinterpret_cast<uint16_t*>(carry + C);
    uint16_t* const cB = cA + TILE;
    auto sqrt_cnt = [&](int k) -> double { if constexpr (TAB) return t_sqrt[k]; else return g_sqrt[k]; };
    auto rsqrt_cnt = [&](int k) -> double { if constexpr (TAB) return t_rsqrt[k]; else return g_rsqrt[k]; };

    const int n_sets = args.env_a.cdf_keys;
    const double* __restrict__ finf_tab = cfgp->wf_finf;
    const double expo = cfgp->sd_p0;
    const int64_t pstride = (int64_t)gridDim.x * WPB;
    for (int64_t p = (int64_t)blockIdx.x * WPB + wv; p < args.n_pairs; p += pstride) {
        double* const out = aa.out + p * (int64_t)C;
        const int4 m = args.meta[p];
        const int mx = __builtin_amdgcn_readfirstlane(m.x), my = __builtin_amdgcn_readfirstlane(m.y);
        const int mz = __builtin_amdgcn_readfirstlane(m.z), mw = __builtin_amdgcn_readfirstlane(m.w);
        const int nA = mz & 0xFFFFFF, nB = mw & 0xFFFFFF;
        const int wfi = __builtin_amdgcn_readfirstlane(args.wf_index ? args.wf_index[p] : 0);
        const bool bad_wf = wfi < 0 || wfi >= n_sets;
        // anchor out of range / overflowed or empty environment (flagged where it happened), or an index outside the dictionary
        if (nA <= 0 || nB <= 0 || nA > kRadialMaxPoints || nB > kRadialMaxPoints || bad_wf) {
            if (bad_wf && lane == 0) sweep_report(args.hst, ST_BAD_WF);
            for (int c = lane; c < C; c += 64) out[c] = nan("");
            continue;
        }
        const int64_t ea = mx, eb = my;
        const int c0a = (mz >> 24) & 255, c0b = (mw >> 24) & 255;
        const uint64_t* __restrict__ kA = args.env_a.key + ea * args.env_a.stride + (int64_t)wfi * args.env_a.set_stride;
        const uint64_t* __restrict__ kB = args.env_b.key + eb * args.env_b.stride + (int64_t)wfi * args.env_b.set_stride;
        const uint8_t* __restrict__ tA = args.env_a.cat + ea * args.env_a.stride;
        const uint8_t* __restrict__ tB = args.env_b.cat + eb * args.env_b.stride;
        const double Finf = finf_tab[wfi];

        bool bad_cat = c0a >= C || c0b >= C, zero_norm = false;
        int totA = 1, totB = 1;  // points seen per side (incl. the anchor)
        // One interval of width dF in key space on this lane's counts: dF * H * t_c / T into the lane's accumulator column.
        auto add_interval = [&](double dF) {
            if constexpr (MODE == ATTR_H2U) {
                if (!(dF > 0.0)) return;  // ties, pieces outside the weight function's support: + 0.0 to sums that are never -0.0
                const double ra_ = rsqrt_cnt(totA), rb_ = rsqrt_cnt(totB);
                double T = 0.0;
                for (int c = 0; c < C; ++c) {
                    const uint32_t v = cnt[c * 64];
                    const double d = sqrt_cnt((int)(v & kMaskA)) * ra_ - sqrt_cnt((int)(v >> 16)) * rb_;
                    T = fma(d, d, T);
                }
                if (!(T > 0.0)) return;
                const double g = dF * sqrt_unit(0.5 * T) / T;
                for (int c = 0; c < C; ++c) {
                    const uint32_t v = cnt[c * 64];
                    const double d = sqrt_cnt((int)(v & kMaskA)) * ra_ - sqrt_cnt((int)(v >> 16)) * rb_;
                    acc[c * 64] += g * (d * d);
                }
            } else {
                double sa_ = 0.0, sb_ = 0.0;  // pmf.rs:67-68: fresh sums
                for (int c = 0; c < C; ++c) {
                    const uint32_t v = cnt[c * 64];
                    sa_ += cat_w[c] * (double)(v & kMaskA);
                    sb_ += cat_w[c] * (double)(v >> 16);
                }
                if (sa_ == 0.0 || sb_ == 0.0) { zero_norm = true; return; }
                const double ia = 1.0 / sa_, ib = 1.0 / sb_;
                if constexpr (MODE == ATTR_H2W) {
                    auto diff = [&](int c) -> double {
                        const uint32_t v = cnt[c * 64];
                        return sqrt((cat_w[c] * (double)(v & kMaskA)) * ia) - sqrt((cat_w[c] * (double)(v >> 16)) * ib);
                    };
                    double T = 0.0;
                    for (int c = 0; c < C; ++c) { const double d = diff(c); T = fma(d, d, T); }
                    if (!(T > 0.0)) return;
                    const double g = dF * sqrt(0.5 * T) / T;
                    for (int c = 0; c < C; ++c) { const double d = diff(c); acc[c * 64] += g * (d * d); }
                } else {
                    double H;
                    const double T = attribution_terms_pow(expo, cnt, cat_w, C, ia, ib, term, &H);
                    if (!(T > 0.0)) return;
                    const double g = dF * H / T;
                    for (int c = 0; c < C; ++c) acc[c * 64] += g * term[c * 64];
                }
            }
        };

        // empty accumulators, the two anchors (src/locohd.rs:82-84) in the carry row and in every lane's column
        wave_sync_lds();
        for (int c = lane; c < C; c += 64) carry[c] = (c == c0a ? kOneA : 0u) | (c == c0b ? kOneB : 0u);
        for (int c = 0; c < C; ++c) {
            cnt[c * 64] = (c == c0a ? kOneA : 0u) | (c == c0b ? kOneB : 0u);
            acc[c * 64] = 0.0;
        }
        wave_sync_lds();
        double F_carry = u2d(kA[0]);  // F(0): both anchors sit at distance 0

        const int mA = nA - 1, mB = nB - 1, M = mA + mB;  // non-anchor events
        int ia = 0, ib = 0;
        for (int k0 = 0; k0 < M; k0 += TILE) {
            const int T = min(TILE, M - k0);
            const int nAt = min(TILE, mA - ia), nBt = min(TILE, mB - ib);
            wave_sync_lds();  // previous tile fully consumed
            for (int t = lane; t < nAt; t += 64) { sA[t] = kA[1 + ia + t]; cA[t] = tA[1 + ia + t]; }
            for (int t = lane; t < nBt; t += 64) { sB[t] = kB[1 + ib + t]; cB[t] = tB[1 + ib + t]; }
            wave_sync_lds();
            const int epl = (T + 63) >> 6;
            const int d0 = min(lane * epl, T), d1 = min(d0 + epl, T);
            const int i1 = merge_path(sA, nAt, sB, nBt, d1);
            int i0 = __shfl_up(i1, 1);
            if (lane == 0) i0 = 0;
            const int iend = __builtin_amdgcn_readlane(i1, 63);
            const int j0 = d0 - i0, j1 = d1 - i1;
            const int last = (T - 1) / epl;  // the last lane with events (wave-uniform)
            const bool has = d0 < d1;

            // pass 1: histogram of this lane's chunk into its column, wave scan per category
            for (int c = 0; c < C; ++c) cnt[c * 64] = 0u;
            for (int i = i0; i < i1; ++i) {
                const int ct = cA[i];
                if (ct >= C) bad_cat = true; else cnt[ct * 64] += kOneA;
            }
            for (int j = j0; j < j1; ++j) {
                const int ct = cB[j];
                if (ct >= C) bad_cat = true; else cnt[ct * 64] += kOneB;
            }
            totA = 1 + ia + i0;
            totB = 1 + ib + j0;
            for (int c = 0; c < C; ++c) {
                const uint32_t own = cnt[c * 64];
                const uint32_t incl = wave_incl_scan_u32(own + (lane == 0 ? carry[c] : 0u));
                cnt[c * 64] = incl - own;
                if (lane == 63) carry[c] = incl;
            }

            // pass 2: this lane's events, one after the other; every interval is added on the counts in front of the event that ends it
            int i = i0, j = j0;
            uint64_t ka = (i < i1) ? sA[i] : kPadKey, kb = (j < j1) ? sB[j] : kPadKey;
            const double firstF = has ? u2d(ka <= kb ? ka : kb) : 0.0;
            const double nextF = shfl_f64(firstF, min(lane + 1, 63));  // the first event of the next lane's chunk
            double Fp = F_carry;
            bool open = lane == 0;  // lane 0 closes the interval the previous tile (or the anchors) left open
            for (int e = d0; e < d1; ++e) {
                const bool takeA = (ka <= kb);  // an exhausted run shows the pad key (> every real key)
                const uint64_t key = takeA ? ka : kb;
                const int ct = takeA ? cA[i] : cB[j];
                if (takeA) { ++i; ka = (i < i1) ? sA[i] : kPadKey; } else { ++j; kb = (j < j1) ? sB[j] : kPadKey; }
                const double F = u2d(key);
                if (open && !bad_cat) add_interval(F - Fp);
                open = true;
                // pmf.rs:47-63: one more point of category ct on one side
                if (ct < C) cnt[ct * 64] += takeA ? kOneA : kOneB;
                else bad_cat = true;
                totA += takeA ? 1 : 0;
                totB += takeA ? 0 : 1;
                Fp = F;
            }
            if (has && lane < last && !bad_cat) add_interval(nextF - Fp);
            F_carry = readlane_f64(Fp, last);
            ia += iend;
            ib += T - iend;
        }
        // the last interval to +inf (:165-171,204-210,212-221) on the counts of the whole pair, by lane 0
        wave_sync_lds();
        const unsigned long long anybad = __ballot(bad_cat);
        if (lane == 0 && !anybad) {
            for (int c = 0; c < C; ++c) cnt[c * 64] = carry[c];
            totA = nA;
            totB = nB;
            add_interval(Finf - F_carry);
        }
        wave_sync_lds();
        const unsigned long long anyzero = __ballot(zero_norm);
        if (lane == 0) {
            if (anybad) sweep_report(args.hst, ST_BAD_CATEGORY);
            if (anyzero) sweep_report(args.hst, ST_ZERO_NORM);
        }
        // the row: one wave reduction per category, in lane order
        for (int c = 0; c < C; ++c) {
            const double s = wave_sum_f64(acc[c * 64]);
            if (lane == 0) out[c] = (anybad || anyzero) ? nan("") : s;
        }
    }
}

// the most pairs per workgroup (4, 2 or 1) whose LDS fits
template <int MODE, bool TAB>
static void launch_attribution_t(hipStream_t s, const AttributionArgs& a) {
    const size_t wb = attribution_wave_bytes(a.n_categories, MODE == ATTR_POW);
    auto go = [&](auto wpb) {
        constexpr int WPB = decltype(wpb)::value;
        const int64_t blocks = (a.sw.n_pairs + WPB - 1) / WPB;
        k_attribution<MODE, TAB, WPB><<<(unsigned)(blocks < 8192 ? blocks : 8192), 64 * WPB, wb * WPB, s>>>(a, (int)wb);
    };
    if (wb * 4 <= (size_t)kAttrDynMax) go(std::integral_constant<int, 4>{});
    else if (wb * 2 <= (size_t)kAttrDynMax) go(std::integral_constant<int, 2>{});
    else go(std::integral_constant<int, 1>{});
}
bool launch_attribution(hipStream_t s, bool exponent2, bool unit_weights, const AttributionArgs& a) {
    if (a.sw.n_pairs <= 0) return true;
    if (a.n_categories < 1 || a.n_categories > kAttributionMaxCategories) return false;
    if (a.sw.env_a.cat16 || a.sw.env_b.cat16 || a.sw.env_a.cdf_keys < 1 || a.sw.env_a.cdf_keys != a.sw.env_b.cdf_keys) return false;
    if (attribution_wave_bytes(a.n_categories, true) > (size_t)kAttrDynMax) return false;
    const bool tab = a.sw.env_a.stride <= kSqrtTab && a.sw.env_b.stride <= kSqrtTab;
    if (!exponent2) launch_attribution_t<ATTR_POW, false>(s, a);
    else if (!unit_weights) launch_attribution_t<ATTR_H2W, false>(s, a);
    else if (tab) launch_attribution_t<ATTR_H2U, true>(s, a);
    else launch_attribution_t<ATTR_H2U, false>(s, a);
    return true;
}

template <int MODE, bool TAB>
static void raise_attribution_lds() {
    const void* list[] = {reinterpret_cast<const void*>(&k_attribution<MODE, TAB, 4>), reinterpret_cast<const void*>(&k_attribution<MODE, TAB, 2>),
                          reinterpret_cast<const void*>(&k_attribution<MODE, TAB, 1>)};
    for (const void* fn : list) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kAttrDynMax);
}
void init_attribution_kernels() {
    raise_attribution_lds<ATTR_POW, false>();
    raise_attribution_lds<ATTR_H2W, false>();
    raise_attribution_lds<ATTR_H2U, true>();
    raise_attribution_lds<ATTR_H2U, false>();
    (void)hipGetLastError();
}

}  // namespace lchd
