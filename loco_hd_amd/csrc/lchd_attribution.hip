// lchd_attribution.hip -- score attribution by category (additive, not in the reference): which primitive types carry a pair's score.
//
//   t_c(r) = |a_c^(1/e) - b_c^(1/e)|^e      T(r) = sum_c t_c(r)      H(r) = (T / 2)^(1/e)
//   out[p][c] = sum_j (F(u_{j+1}) - F(u_j)) * H_j * t_{c,j} / T_j          (a piece with T_j = 0 adds 0 to every column)
//
// over the merged breakpoints u_0 = 0 <= u_1 <= ... <= u_J of the pair's two environments (u_{J+1} = +inf), a / b the weighted,
// normalised PMFs between u_j and u_{j+1} -- exactly what the sweeps integrate, the anchors included.  Only the Hellinger distance
// is a sum of one term per category, so only it decomposes; a row sums to the pair's score.
//
// Shape: the column-tile skeleton of lchd_pair_columns.h, walked by its walk_category_columns: this file holds the terms of an interval.
// Sums: every interval adds dF * H * t_c / T for all C categories to the lane's accumulator column acc[c][lane] (LDS, in front of its
// count column); the walk reduces the columns to the row.
// Terms: always the literal per-category form.  Exponent 2: (sqrt a_c - sqrt b_c)^2, H * t_c / T = t_c / (2 H); with unit weights the
// roots come from the sqrt / rsqrt tables of the counts.  Every other exponent goes through attribution_terms_pow, out of line: the
// library's pow stays out of the exponent-2 instantiations.
#include "lchd_pair_columns.h"

namespace lchd {

constexpr int kAttrTab = kSqrtTab + 8;   // LDS square-root tables: counts 0 .. kSqrtTab (stores of at most kSqrtTab points per slot)
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

// In front of the count columns (lchd_pair_columns.h): accumulator columns [C][64] f64 | (ATTR_POW: term columns [C][64] f64)
static size_t attribution_wave_bytes(int C, bool pow_terms) { return column_wave_bytes(C, (size_t)C * 512 * (pow_terms ? 2 : 1)); }

// MODE: ATTR_*.  TAB: both stores have slots of at most kSqrtTab points, the square-root tables are read from LDS (ATTR_H2U alone
// reads them).  WPB: pairs (wavefronts) per workgroup.
template <int MODE, bool TAB, int WPB>
__global__ __launch_bounds__(64 * WPB) void k_attribution(AttributionArgs aa, int wave_bytes) {
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
    const ColumnLds l = column_carve(attr_smem + (size_t)wv * wave_bytes, C, (size_t)C * 512 * (MODE == ATTR_POW ? 2 : 1));
    double* const acc = reinterpret_cast<double*>(l.front) + lane;  // this lane's accumulator column: acc[c * 64]
    double* const term = acc + (size_t)C * 64;                      // ATTR_POW: this lane's term column
    const uint32_t* const cnt = l.cnt0 + lane;                      // this lane's count column: cnt[c * 64]
    auto sqrt_cnt = [&](int k) -> double { if constexpr (TAB) return t_sqrt[k]; else return g_sqrt[k]; };
    auto rsqrt_cnt = [&](int k) -> double { if constexpr (TAB) return t_rsqrt[k]; else return g_rsqrt[k]; };

    const double expo = cfgp->sd_p0;
    // One interval of width dF in key space on this lane's counts: dF * H * t_c / T into the lane's accumulator column.
    auto add_interval = [&](double dF, ColumnWalk& w) {
        if constexpr (MODE == ATTR_H2U) {
            if (!(dF > 0.0)) return;  // ties, pieces outside the weight function's support: + 0.0 to sums that are never -0.0
            const double ra_ = rsqrt_cnt(w.totA), rb_ = rsqrt_cnt(w.totB);
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
            if (sa_ == 0.0 || sb_ == 0.0) { w.zero_norm = true; return; }
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
    walk_category_columns<WPB>(args, aa.out, l, acc, lane, wv, add_interval, [](int, double s) { return s; });
}

template <int MODE, bool TAB>
static void launch_attribution_t(hipStream_t s, const AttributionArgs& a) {
    const size_t wb = attribution_wave_bytes(a.n_categories, MODE == ATTR_POW);
    launch_most_waves(kColumnDynMax, wb, a.sw.n_pairs, [&](auto wpb, unsigned grid) {
        constexpr int WPB = decltype(wpb)::value;
        k_attribution<MODE, TAB, WPB><<<grid, 64 * WPB, wb * WPB, s>>>(a, (int)wb);
    });
}
bool launch_attribution(hipStream_t s, bool exponent2, bool unit_weights, const AttributionArgs& a) {
    if (a.sw.n_pairs <= 0) return true;
    if (a.n_categories < 1 || a.n_categories > kAttributionMaxCategories) return false;
    if (a.sw.env_a.cat16 || a.sw.env_b.cat16 || a.sw.env_a.cdf_keys < 1 || a.sw.env_a.cdf_keys != a.sw.env_b.cdf_keys) return false;
    if (attribution_wave_bytes(a.n_categories, true) > (size_t)kColumnDynMax) return false;
    const bool tab = a.sw.env_a.stride <= kSqrtTab && a.sw.env_b.stride <= kSqrtTab;
    if (!exponent2) launch_attribution_t<ATTR_POW, false>(s, a);
    else if (!unit_weights) launch_attribution_t<ATTR_H2W, false>(s, a);
    else if (tab) launch_attribution_t<ATTR_H2U, true>(s, a);
    else launch_attribution_t<ATTR_H2U, false>(s, a);
    return true;
}

template <int MODE, bool TAB>
static void raise_attribution_lds() {
    raise_dynamic_lds({kernel_ptr(&k_attribution<MODE, TAB, 4>), kernel_ptr(&k_attribution<MODE, TAB, 2>), kernel_ptr(&k_attribution<MODE, TAB, 1>)},
                      kColumnDynMax);
}
void init_attribution_kernels() {
    raise_attribution_lds<ATTR_POW, false>();
    raise_attribution_lds<ATTR_H2W, false>();
    raise_attribution_lds<ATTR_H2U, true>();
    raise_attribution_lds<ATTR_H2U, false>();
    (void)hipGetLastError();
}

}  // namespace lchd
