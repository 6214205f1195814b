// lchd_category_gradient.hip -- category-weight gradients (additive, not in the reference): dS/dw_c of a pair's score, the derivative
// with respect to the category_weights of the configuration (src/locohd.rs:48,82: p_c = w_c n_c / sum_k w_k n_k).
//
// Between two merged breakpoints u_j <= u_{j+1} of the pair's two environments (u_0 = 0, u_{J+1} = +inf), with n^A / n^B the category
// counts of the piece (anchors included), p_c = w_c n^A_c / sum_k w_k n^A_k, q_c likewise from n^B, D(p, q) the statistical distance,
// x_c = p_c dD/dp_c and y_c = q_c dD/dq_c:
//
//   w_c dp_k/dw_c = p_c (delta_kc - p_k)         w_c dD/dw_c = x_c + y_c - p_c sum_k x_k - q_c sum_k y_k
//   out[p][c]     = dS_p/dw_c = (1 / w_c) * sum_j (F(u_{j+1}) - F(u_j)) * (w_c dD/dw_c)_j
//
//   Hellinger, exponent e (statistical_distances.rs:4-10): d_c = p_c^(1/e) - q_c^(1/e), T = sum_c |d_c|^e, D = (T / 2)^(1/e),
//     x_c = (D / (e T)) |d_c|^(e-1) sgn(d_c) p_c^(1/e)        y_c = -(D / (e T)) |d_c|^(e-1) sgn(d_c) q_c^(1/e)
//     e = 2: w_c dH/dw_c = (sqrt p_c - sqrt q_c)^2 / (4 H) - (p_c + q_c) H / 4
//   Kullback-Leibler, eps (:23-29; side A is the first argument, as in the sweeps):
//     x_c = p_c [ln((p_c + eps) / (q_c + eps)) + p_c / (p_c + eps)]        y_c = -p_c q_c / (q_c + eps)
//
// Every x_c, y_c is finite at p_c = 0 or q_c = 0: nothing here divides by a PMF entry.  Conventions: a Hellinger piece with T = 0 adds 0
// to every column (the distance has a kink there; 0 is the subgradient the attribution's convention implies); a category with d_c = 0
// has x_c = y_c = 0 for every exponent (sgn 0 = 0); a piece with dF <= 0 adds nothing.  So a category neither environment holds has an
// exactly zero column, identical environments give a row of exact zeros under Hellinger, one category gives exact zeros, and
// sum_c w_c out[p][c] = 0 up to rounding (the score is homogeneous of degree 0 in w).
//
// Shape: the column-tile skeleton of lchd_pair_columns.h, walked by its walk_category_columns: this file holds the terms of an interval.
// Sums: acc[c][lane] (LDS) takes dF * (w_c dD/dw_c); the walk reduces the columns in lane order, then the division by w_c writes the
// row: the bits of a row are a function of the stored pair alone.
// Modes: Hellinger-2 computes T and H in one pass over the categories and accumulates in a second (sqrt, the collapsed form above);
// every other exponent stages s_c p_c^(1/e), s_c q_c^(1/e) in two LDS term columns (category_gradient_terms_pow, out of line: the library's pow
// stays out of the other instantiations); Kullback-Leibler stages x_c, y_c there.
#include "lchd_pair_columns.h"

namespace lchd {

enum { CG_H2 = 0, CG_POW = 1, CG_KL = 2 };  // Hellinger-2 / any other Hellinger exponent / Kullback-Leibler

// The terms of one lane's count column for a general exponent e, with s_c = |d_c|^(e-1) sgn(d_c) (0 where d_c = 0):
// ta[c * 64] = s_c p_c^(1/e), tb[c * 64] = s_c q_c^(1/e); *Sa, *Sb their sums over c; *D = (T / 2)^(1/e); returns T.
static __device__ __noinline__ double category_gradient_terms_pow(double e, const uint32_t* cnt, const double* __restrict__ w, int C, double ia,
                                                                  double ib, double* ta, double* tb, double* Sa, double* Sb, double* D) {
    const double inv = 1.0 / e;
    double T = 0.0, sa = 0.0, sb = 0.0;
    for (int c = 0; c < C; ++c) {
        const uint32_t v = cnt[c * 64];
        const double a = pow((w[c] * (double)(v & 0xFFFFu)) * ia, inv), b = pow((w[c] * (double)(v >> 16)) * ib, inv);
        const double d = a - b;
        const double s = d != 0.0 ? copysign(pow(fabs(d), e - 1.0), d) : 0.0;
        ta[c * 64] = s * a;
        tb[c * 64] = s * b;
        T += fabs(d) * fabs(s);
        sa += s * a;
        sb += s * b;
    }
    *Sa = sa;
    *Sb = sb;
    *D = pow(T / 2.0, inv);
    return T;
}

// In front of the count columns (lchd_pair_columns.h): accumulator columns [C][64] f64 | (CG_POW, CG_KL: two term columns [C][64] f64)
static size_t category_gradient_wave_bytes(int C, bool terms) { return column_wave_bytes(C, (size_t)C * 512 * (terms ? 3 : 1)); }

// MODE: CG_*.  WPB: pairs (wavefronts) per workgroup.
template <int MODE, int WPB>
__global__ __launch_bounds__(64 * WPB) void k_category_gradient(CategoryGradientArgs ga, int wave_bytes) {
    constexpr bool TERMS = MODE != CG_H2;
    extern __shared__ __attribute__((aligned(16))) unsigned char cg_smem[];
    const SweepArgs& args = ga.sw;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const DevConfig* __restrict__ cfgp = args.cfg;
    const int C = cfgp->n_categories;
    const double* __restrict__ cat_w = cfgp->cat_w;
    const ColumnLds l = column_carve(cg_smem + (size_t)wv * wave_bytes, C, (size_t)C * 512 * (TERMS ? 3 : 1));
    double* const acc = reinterpret_cast<double*>(l.front) + lane;  // this lane's accumulator column: acc[c * 64]
    double* const ta = acc + (size_t)C * 64;                        // TERMS: this lane's two term columns
    double* const tb = ta + (size_t)C * 64;
    const uint32_t* const cnt = l.cnt0 + lane;                      // this lane's count column: cnt[c * 64]

    const double prm0 = cfgp->sd_p0;  // the Hellinger exponent / the Kullback-Leibler epsilon
    // One interval of width dF in key space on this lane's counts: dF * (w_c dD/dw_c) into the lane's accumulator column.
    auto add_interval = [&](double dF, ColumnWalk& w) {
        if (!(dF > 0.0)) return;  // ties, pieces outside the weight function's support
        if (C == 1) return;       // p = q = (1) whatever w is: exact zeros (w n * (1 / (w n)) need not round to 1)
        double sa_ = 0.0, sb_ = 0.0;  // pmf.rs:67-68: fresh sums
        for (int c = 0; c < C; ++c) {
            const uint32_t v = cnt[c * 64];
            sa_ += cat_w[c] * (double)(v & kMaskA);
            sb_ += cat_w[c] * (double)(v >> 16);
        }
        if (sa_ == 0.0 || sb_ == 0.0) { w.zero_norm = true; return; }
        const double ia = 1.0 / sa_, ib = 1.0 / sb_;
        if constexpr (MODE == CG_H2) {
            double T = 0.0;
            for (int c = 0; c < C; ++c) {
                const uint32_t v = cnt[c * 64];
                const double d = sqrt((cat_w[c] * (double)(v & kMaskA)) * ia) - sqrt((cat_w[c] * (double)(v >> 16)) * ib);
                T = fma(d, d, T);
            }
            if (!(T > 0.0)) return;
            const double H = sqrt(0.5 * T);
            const double g = dF / (4.0 * H), h = dF * (0.25 * H);
            for (int c = 0; c < C; ++c) {
                const uint32_t v = cnt[c * 64];
                const double pa = (cat_w[c] * (double)(v & kMaskA)) * ia, qb = (cat_w[c] * (double)(v >> 16)) * ib;
                const double d = sqrt(pa) - sqrt(qb);
                acc[c * 64] += g * (d * d) - h * (pa + qb);
            }
        } else if constexpr (MODE == CG_POW) {
            double Sa, Sb, D;
            const double T = category_gradient_terms_pow(prm0, cnt, cat_w, C, ia, ib, ta, tb, &Sa, &Sb, &D);
            if (!(T > 0.0)) return;
            const double k = D / (prm0 * T);
            const double X = k * Sa, Y = -(k * Sb);  // sum_c x_c, sum_c y_c
            for (int c = 0; c < C; ++c) {
                const uint32_t v = cnt[c * 64];
                const double pa = (cat_w[c] * (double)(v & kMaskA)) * ia, qb = (cat_w[c] * (double)(v >> 16)) * ib;
                acc[c * 64] += dF * ((k * ta[c * 64] - pa * X) + (-(k * tb[c * 64]) - qb * Y));
            }
        } else {
            double X = 0.0, Y = 0.0;
            for (int c = 0; c < C; ++c) {
                const uint32_t v = cnt[c * 64];
                const double pa = (cat_w[c] * (double)(v & kMaskA)) * ia, qb = (cat_w[c] * (double)(v >> 16)) * ib;
                const double x = pa * (log((pa + prm0) / (qb + prm0)) + pa / (pa + prm0));
                const double y = -(pa * qb) / (qb + prm0);
                ta[c * 64] = x;
                tb[c * 64] = y;
                X += x;
                Y += y;
            }
            for (int c = 0; c < C; ++c) {
                const uint32_t v = cnt[c * 64];
                const double pa = (cat_w[c] * (double)(v & kMaskA)) * ia, qb = (cat_w[c] * (double)(v >> 16)) * ib;
                acc[c * 64] += dF * ((ta[c * 64] - pa * X) + (tb[c * 64] - qb * Y));
            }
        }
    };
    walk_category_columns<WPB>(args, ga.out, l, acc, lane, wv, add_interval, [&](int c, double s) { return s / cat_w[c]; });
}

template <int MODE>
static void launch_category_gradient_t(hipStream_t s, const CategoryGradientArgs& a) {
    const size_t wb = category_gradient_wave_bytes(a.n_categories, MODE != CG_H2);
    launch_most_waves(kColumnDynMax, wb, a.sw.n_pairs, [&](auto wpb, unsigned grid) {
        constexpr int WPB = decltype(wpb)::value;
        k_category_gradient<MODE, WPB><<<grid, 64 * WPB, wb * WPB, s>>>(a, (int)wb);
    });
}
bool launch_category_gradient(hipStream_t s, int sd_kind, bool exponent2, const CategoryGradientArgs& a) {
    if (a.sw.n_pairs <= 0) return true;
    if (sd_kind != SD_HELLINGER && sd_kind != SD_KL) return false;
    if (a.n_categories < 1 || a.n_categories > kAttributionMaxCategories) return false;
    if (a.sw.env_a.cat16 || a.sw.env_b.cat16 || a.sw.env_a.cdf_keys < 1 || a.sw.env_a.cdf_keys != a.sw.env_b.cdf_keys) return false;
    if (category_gradient_wave_bytes(a.n_categories, true) > (size_t)kColumnDynMax) return false;
    if (sd_kind == SD_KL) launch_category_gradient_t<CG_KL>(s, a);
    else if (exponent2) launch_category_gradient_t<CG_H2>(s, a);
    else launch_category_gradient_t<CG_POW>(s, a);
    return true;
}

template <int MODE>
static void raise_category_gradient_lds() {
    raise_dynamic_lds({kernel_ptr(&k_category_gradient<MODE, 4>), kernel_ptr(&k_category_gradient<MODE, 2>), kernel_ptr(&k_category_gradient<MODE, 1>)},
                      kColumnDynMax);
}
void init_category_gradient_kernels() {
    raise_category_gradient_lds<CG_H2>();
    raise_category_gradient_lds<CG_POW>();
    raise_category_gradient_lds<CG_KL>();
    (void)hipGetLastError();
}

}  // namespace lchd
