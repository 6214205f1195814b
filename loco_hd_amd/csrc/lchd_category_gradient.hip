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
// Shape: k_attribution's (lchd_attribution.hip), line for line: one pair per wavefront, grid-stride over pairs; tiles of kSweepTile
// merged events from the F keys and category bytes of both stores; merge path split across the lanes; per-lane count columns in LDS
// (count_A | count_B << 16), set up by a wave scan of the per-lane histograms; every lane walks its events and adds every interval on
// the counts in front of the event that ends it; lane 0 owns the interval the previous tile left open and the tail to F(inf) on the
// whole pair's counts.  Sums: acc[c][lane] (LDS) takes dF * (w_c dD/dw_c); after the last tile one wave reduction per category in lane
// order, then the division by w_c, writes the row: no floating-point atomics, no cross-wave traffic, the bits of a row are a function
// of the stored pair alone.
// Modes: Hellinger-2 computes T and H in one pass over the categories and accumulates in a second (sqrt, the collapsed form above);
// every other exponent stages s_c p_c^(1/e), s_c q_c^(1/e) in two LDS term columns (category_gradient_terms_pow, out of line: the library's pow
// stays out of the other instantiations); Kullback-Leibler stages x_c, y_c there.
#include "lchd_sweep_common.h"

namespace lchd {

constexpr int kCgDynMax = 150 * 1024;  // dynamic LDS the instantiations are allowed (the attribution kernel's budget)
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

// Per wavefront, in dynamic LDS: two key tiles | accumulator columns [C][64] f64 | (CG_POW, CG_KL: two term columns [C][64] f64) |
// count columns [C][64] | carry row [C] | two category tiles
static size_t category_gradient_wave_bytes(int C, bool terms) {
    return ((size_t)kSweepTile * 16 + (size_t)C * 512 * (terms ? 3 : 1) + (size_t)C * 260 + (size_t)kSweepTile * 4 + 15) & ~(size_t)15;
}

// MODE: CG_*.  WPB: pairs (wavefronts) per workgroup.
template <int MODE, int WPB>
__global__ __launch_bounds__(64 * WPB) void k_category_gradient(CategoryGradientArgs ga, int wave_bytes) {
    constexpr int TILE = kSweepTile;
    constexpr uint32_t kOneA = 1u, kOneB = 1u << 16, kMaskA = 0xFFFFu;
    constexpr bool TERMS = MODE != CG_H2;
    extern __shared__ __attribute__((aligned(16))) unsigned char cg_smem[];
    const SweepArgs& args = ga.sw;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const DevConfig* __restrict__ cfgp = args.cfg;
    const int C = cfgp->n_categories;
    const double* __restrict__ cat_w = cfgp->cat_w;
    unsigned char* const base = cg_smem + (size_t)wv * wave_bytes;
    uint64_t* const sA = reinterpret_cast<uint64_t*>(base);
    uint64_t* const sB = sA + TILE;
    double* const acc0 = reinterpret_cast<double*>(sB + TILE);
    double* const acc = acc0 + lane;                          // this lane's accumulator column: acc[c * 64]
    double* const ta = acc + (size_t)C * 64;                  // TERMS: this lane's two term columns
    double* const tb = ta + (size_t)C * 64;
    uint32_t* const cnt0 = reinterpret_cast<uint32_t*>(acc0 + (size_t)C * 64 * (TERMS ? 3 : 1));
    uint32_t* const cnt = cnt0 + lane;                        // this lane's count column: cnt[c * 64]
    uint32_t* const carry = cnt0 + (size_t)C * 64;            // per category: counts before the current tile
    uint16_t* const cA = reinterpret_cast<uint16_t*>(carry + C);
    uint16_t* const cB = cA + TILE;

    const int n_sets = args.env_a.cdf_keys;
    const double* __restrict__ finf_tab = cfgp->wf_finf;
    const double prm0 = cfgp->sd_p0;  // the Hellinger exponent / the Kullback-Leibler epsilon
    const int64_t pstride = (int64_t)gridDim.x * WPB;
    for (int64_t p = (int64_t)blockIdx.x * WPB + wv; p < args.n_pairs; p += pstride) {
        double* const out = ga.out + p * (int64_t)C;
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
        // One interval of width dF in key space on this lane's counts: dF * (w_c dD/dw_c) into the lane's accumulator column.
        auto add_interval = [&](double dF) {
            if (!(dF > 0.0)) return;  // ties, pieces outside the weight function's support
            if (C == 1) return;       // p = q = (1) whatever w is: exact zeros (w n * (1 / (w n)) need not round to 1)
            double sa_ = 0.0, sb_ = 0.0;  // pmf.rs:67-68: fresh sums
            for (int c = 0; c < C; ++c) {
                const uint32_t v = cnt[c * 64];
                sa_ += cat_w[c] * (double)(v & kMaskA);
                sb_ += cat_w[c] * (double)(v >> 16);
            }
            if (sa_ == 0.0 || sb_ == 0.0) { zero_norm = true; return; }
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
                Fp = F;
            }
            if (has && lane < last && !bad_cat) add_interval(nextF - Fp);
            F_carry = readlane_f64(Fp, last);
            ia += iend;
            ib += T - iend;
        }
        // the last interval to +inf on the counts of the whole pair, by lane 0
        wave_sync_lds();
        const unsigned long long anybad = __ballot(bad_cat);
        if (lane == 0 && !anybad) {
            for (int c = 0; c < C; ++c) cnt[c * 64] = carry[c];
            add_interval(Finf - F_carry);
        }
        wave_sync_lds();
        const unsigned long long anyzero = __ballot(zero_norm);
        if (lane == 0) {
            if (anybad) sweep_report(args.hst, ST_BAD_CATEGORY);
            if (anyzero) sweep_report(args.hst, ST_ZERO_NORM);
        }
        // the row: one wave reduction per category, in lane order, then 1 / w_c
        for (int c = 0; c < C; ++c) {
            const double s = wave_sum_f64(acc[c * 64]);
            if (lane == 0) out[c] = (anybad || anyzero) ? nan("") : s / cat_w[c];
        }
    }
}

// the most pairs per workgroup (4, 2 or 1) whose LDS fits
template <int MODE>
static void launch_category_gradient_t(hipStream_t s, const CategoryGradientArgs& a) {
    const size_t wb = category_gradient_wave_bytes(a.n_categories, MODE != CG_H2);
    auto go = [&](auto wpb) {
        constexpr int WPB = decltype(wpb)::value;
        const int64_t blocks = (a.sw.n_pairs + WPB - 1) / WPB;
        k_category_gradient<MODE, WPB><<<(unsigned)(blocks < 8192 ? blocks : 8192), 64 * WPB, wb * WPB, s>>>(a, (int)wb);
    };
    if (wb * 4 <= (size_t)kCgDynMax) go(std::integral_constant<int, 4>{});
    else if (wb * 2 <= (size_t)kCgDynMax) go(std::integral_constant<int, 2>{});
    else go(std::integral_constant<int, 1>{});
}
bool launch_category_gradient(hipStream_t s, int sd_kind, bool exponent2, const CategoryGradientArgs& a) {
    if (a.sw.n_pairs <= 0) return true;
    if (sd_kind != SD_HELLINGER && sd_kind != SD_KL) return false;
    if (a.n_categories < 1 || a.n_categories > kAttributionMaxCategories) return false;
    if (a.sw.env_a.cat16 || a.sw.env_b.cat16 || a.sw.env_a.cdf_keys < 1 || a.sw.env_a.cdf_keys != a.sw.env_b.cdf_keys) return false;
    if (category_gradient_wave_bytes(a.n_categories, true) > (size_t)kCgDynMax) return false;
    if (sd_kind == SD_KL) launch_category_gradient_t<CG_KL>(s, a);
    else if (exponent2) launch_category_gradient_t<CG_H2>(s, a);
    else launch_category_gradient_t<CG_POW>(s, a);
    return true;
}

template <int MODE>
static void raise_category_gradient_lds() {
    const void* list[] = {reinterpret_cast<const void*>(&k_category_gradient<MODE, 4>), reinterpret_cast<const void*>(&k_category_gradient<MODE, 2>),
                          reinterpret_cast<const void*>(&k_category_gradient<MODE, 1>)};
    for (const void* fn : list) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kCgDynMax);
}
void init_category_gradient_kernels() {
    raise_category_gradient_lds<CG_H2>();
    raise_category_gradient_lds<CG_POW>();
    raise_category_gradient_lds<CG_KL>();
    (void)hipGetLastError();
}

}  // namespace lchd
