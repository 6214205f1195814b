// lchd_weight_gradient.hip -- weight-function gradients of a pair's score (additive, not in the reference): the derivative of the score
// with respect to every parameter of the pair's weight function.
//
//   S        = sum_j (F(u_{j+1}) - F(u_j)) * H_j               (merged breakpoints u_j, H_j the statistical distance on piece j)
//   dS/dth_k = sum_j (G_k(u_{j+1}) - G_k(u_j)) * H_j           (G_k = dF/dth_k: the environments do not depend on the weight function)
//            = sum_members G_k(d_m) * (H-_m - H+_m) + G_k(inf) * H_last - G_k(0) * H_first          (summation by parts)
//
// The kernel sums the interval form, with G carried like F: per event G at the event's distance (cdf_param_grad of lchd_math.h, out of
// line), and the interval the event ends adds (G - G of the event before) * H.  An interval of zero width between tied members adds an
// exact zero, so two identical environments under Hellinger give a row of exact zeros, as their score is 0.  G_k(0) is the start of the
// first interval and G_k(inf) = 0 the end of the last (F(inf) = 1 whatever the parameters; the host layer refuses a dagum whose F(inf)
// is not 1): both are lane 0's.  No threshold caveat applies: a member entering or leaving at the threshold does not move with the
// parameters.  The only one-sidedness is at a member exactly on a kink of F (a support bound of uniform / kumaraswamy), which takes
// the inside branch as the CDF does.
//
//   k_weight_gradient   k_sensitivity's walk on k_sensitivity's lists (the INDEXED lists of lchd_sensitivity.hip: distance bits as keys,
//                       A first on ties; the same pair head, the same verdict on an unusable pair) on the column-tile skeleton of
//                       lchd_pair_columns.h.  Per event: H on the counts behind the event (sens_sd: every statistical distance), H in front
//                       of it from the previous event -- a lane's first event takes it from the previous lane, lane 0 from the previous
//                       tile, carried like F --, G[0 .. np) at the event's distance into the lane's LDS column, and
//                       acc[k] += (G_k - G_k of the event before) * H-; a lane's first event takes that G from the previous lane's column,
//                       lane 0 from the carry row.
//                       The accumulators are per-lane registers (kWeightGradientMaxParams of them, the loops over k unrolled), reduced
//                       once per pair in lane order; every output element has one writer, no floating-point atomics: the bits of a row are
//                       a function of the stored pair alone.  The same walk sums dF * H, so the call returns the scores as k_sensitivity
//                       does, bit for bit.
// LDS in front of the count columns: two G columns per lane, [NP][64] f64 each (NP the call's row width) -- the one the out-of-line leaf
// writes for the current event (after the walk: G at the lane's last event, which the next lane reads), and the one of the lane's first
// event, whose interval is known only after the walk -- and one carry row, G at the last event of the previous tile.  The leaf's output
// is an array; handing it over in LDS instead of the stack is what keeps the kernel free of scratch.
#include "lchd_pair_columns.h"

namespace lchd {

constexpr int kWgParams = kWeightGradientMaxParams;
// bytes in front of the count columns for rows of np_max parameters: the two G columns [np_max][64] and the carry row [np_max]; sized by
// the call's row width, not by kWeightGradientMaxParams -- 2 064 bytes for uniform, 16 512 at 16 parameters -- so that the usual two to
// four parameters leave the LDS for as many wavefronts per CU as k_sensitivity has
constexpr size_t wg_front(int np_max) { return ((size_t)2 * np_max * 64 + np_max) * sizeof(double); }

static __device__ __forceinline__ double wgrad_cdf(int kind, const double* p, int np, double inv, double x) { return cdf_lean(kind, p, np, inv, x) + 0.0; }
// G[0 .. np) at x into LDS: a lane's column (stride 64) or the carry row (stride 1)
static __device__ __noinline__ void wgrad_leaf(int kind, const double* p, int np, double x, double* out, int stride) {
    cdf_param_grad_strided(kind, p, np, x, out, stride);
}

// WPB: pairs (wavefronts) per workgroup.
template <int WPB>
__global__ __launch_bounds__(64 * WPB) void k_weight_gradient(WeightGradientArgs wa, int wave_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wgrad_smem[];
    const SweepArgs& args = wa.sw;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const DevConfig* __restrict__ cfgp = args.cfg;
    const int C = cfgp->n_categories, NP = wa.width;
    const double* __restrict__ cat_w = cfgp->cat_w;
    const ColumnLds l = column_carve(wgrad_smem + (size_t)wv * wave_bytes, C, wg_front(NP));
    const uint64_t *const sA = l.sA, *const sB = l.sB;
    const uint16_t *const cA = l.cA, *const cB = l.cB;
    uint32_t* const cnt = l.cnt0 + lane;                                 // this lane's count column: cnt[c * 64]
    double* const g_first = reinterpret_cast<double*>(l.front) + lane;   // G at the lane's first event of the tile: g_first[k * 64]
    double* const g_cur = g_first + NP * 64;                      // G at the current event; after the walk: at the lane's last event
    double* const g_carry = reinterpret_cast<double*>(l.front) + 2 * NP * 64;  // [k]: G at the last event of the previous tile (or at 0)

    const int n_wf = cfgp->n_wf;
    const int sd_kind = cfgp->sd_kind;
    const double prm0 = cfgp->sd_p0, prm1 = cfgp->sd_p1;
    const int64_t pstride = (int64_t)gridDim.x * WPB;
    for (int64_t p = (int64_t)blockIdx.x * WPB + wv; p < args.n_pairs; p += pstride) {
        double* const out = wa.grad + p * (int64_t)NP;
        // k_sensitivity's pair head: the lengths come from the lists, the anchors' categories from their first slots
        const int4 m = args.meta[p];
        const int mx = __builtin_amdgcn_readfirstlane(m.x), my = __builtin_amdgcn_readfirstlane(m.y);
        const int mz = __builtin_amdgcn_readfirstlane(m.z), mw = __builtin_amdgcn_readfirstlane(m.w);
        const bool usable = (mz & 0xFFFFFF) > 0 && (mw & 0xFFFFFF) > 0;  // (anchor out of range, overflowed or empty environment: flagged where it happened)
        const int64_t ea = mx, eb = my;
        const int nA = usable ? __builtin_amdgcn_readfirstlane(wa.env_a.len[ea]) : 0, nB = usable ? __builtin_amdgcn_readfirstlane(wa.env_b.len[eb]) : 0;
        const int wfi = __builtin_amdgcn_readfirstlane(args.wf_index ? args.wf_index[p] : 0);
        const bool bad_wf = wfi < 0 || wfi >= n_wf;
        if (nA <= 0 || nB <= 0 || nA > kRadialMaxPoints || nB > kRadialMaxPoints || bad_wf) {
            if (bad_wf && lane == 0) sweep_report(args.hst, ST_BAD_WF);
            for (int k = lane; k < NP; k += 64) out[k] = nan("");
            if (lane == 0) wa.scores[p] = nan("");
            continue;
        }
        const uint64_t* __restrict__ kA = reinterpret_cast<const uint64_t*>(wa.env_a.dist) + ea * wa.env_a.stride;
        const uint64_t* __restrict__ kB = reinterpret_cast<const uint64_t*>(wa.env_b.dist) + eb * wa.env_b.stride;
        const uint8_t* __restrict__ tA = wa.env_a.cat + ea * wa.env_a.stride;
        const uint8_t* __restrict__ tB = wa.env_b.cat + eb * wa.env_b.stride;
        const WfEntry wf = cfgp->wf[wfi];
        const double* __restrict__ prm = cfgp->wf_params + wf.offset;
        const double winv = cfgp->wf_inv[wfi], Finf = cfgp->wf_finf[wfi];
        const int np = min(wf.n_params, min(NP, kWgParams));  // (wave-uniform; the host layer refuses more than kWeightGradientMaxParams)

        const int c0a = tA[0], c0b = tB[0];
        bool bad_cat = c0a >= C || c0b >= C, zero_norm = false;
        // H on this lane's counts
        auto distance = [&]() -> double {
            double sa_ = 0.0, sb_ = 0.0;  // pmf.rs:67-68: fresh sums
            for (int c = 0; c < C; ++c) {
                const uint32_t v = cnt[c * 64];
                sa_ += cat_w[c] * (double)(v & kMaskA);
                sb_ += cat_w[c] * (double)(v >> 16);
            }
            if (sa_ == 0.0 || sb_ == 0.0) { zero_norm = true; return 0.0; }
            return sens_sd(sd_kind, prm0, prm1, cnt, cat_w, C, 1.0 / sa_, 1.0 / sb_);
        };
        // per parameter: the lane's sum, and G at its previous event; the columns behind the pair's np parameters stay exact zeros
        double acc[kWgParams], gp[kWgParams];
#pragma unroll
        for (int k = 0; k < kWgParams; ++k) { acc[k] = 0.0; gp[k] = 0.0; }

        // the two anchors (src/locohd.rs:82-84) in the carry row and in every lane's column
        wave_sync_lds();
        column_seed_anchors(l, cnt, C, c0a, c0b, lane);
        wave_sync_lds();
        double F_carry = wgrad_cdf(wf.kind, prm, wf.n_params, winv, 0.0);  // F(0): both anchors sit at distance 0
        double H_carry = bad_cat ? 0.0 : distance();
        double score = 0.0;  // this lane's part of sum dF * H
        if (lane == 0) wgrad_leaf(wf.kind, prm, np, 0.0, g_carry, 1);  // G(0): where the first interval starts

        const int mA = nA - 1, mB = nB - 1, M = mA + mB;  // non-anchor events
        int ia = 0, ib = 0;
        for (int k0 = 0; k0 < M; k0 += kSweepTile) {
            const ColumnTile t = column_tile_stage(l, kA, kB, tA, tB, mA, mB, M, k0, ia, ib, lane);
            const int T = t.T, d0 = t.d0, d1 = t.d1, i1 = t.i1, j1 = t.j1, iend = t.iend, last = t.last;
            const bool has = t.has;
            if (column_histogram_scan(l, cnt, t, C, lane, [](uint32_t) {})) bad_cat = true;

            // pass 2: this lane's events, one after the other
            int i = t.i0, j = t.j0;
            uint64_t ka = (i < i1) ? sA[i] : kPadKey, kb = (j < j1) ? sB[j] : kPadKey;
            const double firstF = has ? wgrad_cdf(wf.kind, prm, wf.n_params, winv, u2d(ka <= kb ? ka : kb)) : 0.0;
            const double nextF = shfl_f64(firstF, min(lane + 1, 63));  // F at the first event of the next lane's chunk
            double Fp = F_carry, Hp = 0.0;
            bool open = lane == 0;  // lane 0 closes the interval the previous tile (or the anchors) left open, on H_carry
            // the lane's first event ends an interval that starts in the previous lane (lane 0: the previous tile): added after the walk
            for (int e = d0; e < d1; ++e) {
                const bool takeA = (ka <= kb);  // an exhausted run shows the pad key (> every real key); A first on ties
                const uint64_t key = takeA ? ka : kb;
                const int ct = takeA ? cA[i] : cB[j];
                if (takeA) { ++i; ka = (i < i1) ? sA[i] : kPadKey; } else { ++j; kb = (j < j1) ? sB[j] : kPadKey; }
                const double d = u2d(key);
                double F = wgrad_cdf(wf.kind, prm, wf.n_params, winv, d);
                F = F < Fp ? Fp : F;  // (F is monotone; its floating-point evaluation may invert the last bit between neighbours)
                if (open && !bad_cat) score += (F - Fp) * (e == d0 ? H_carry : Hp);
                // pmf.rs:47-63: one more point of category ct on one side
                if (ct < C) cnt[ct * 64] += takeA ? kOneA : kOneB;
                else bad_cat = true;
                const double Hn = bad_cat ? 0.0 : distance();
                const double* const g = e == d0 ? g_first : g_cur;
                wgrad_leaf(wf.kind, prm, np, d, e == d0 ? g_first : g_cur, 64);
#pragma unroll
                for (int k = 0; k < kWgParams; ++k) {
                    if (k < np) {
                        const double gk = g[k * 64];
                        if (e != d0) acc[k] += (gk - gp[k]) * Hp;
                        gp[k] = gk;
                    }
                }
                open = true;
                Hp = Hn;
                Fp = F;
            }
            if (has && lane < last && !bad_cat) score += ((nextF < Fp ? Fp : nextF) - Fp) * Hp;
            double Hprev = shfl_up_f64(Hp, 1);  // (lanes 1 .. last: lane - 1 has events)
            if (lane == 0) Hprev = H_carry;
            // G at every lane's last event into its g_cur column; then the interval each lane's first event ends
            if (has) {
#pragma unroll
                for (int k = 0; k < kWgParams; ++k)
                    if (k < np) g_cur[k * 64] = gp[k];
            }
            wave_sync_lds();
            if (has) {
#pragma unroll
                for (int k = 0; k < kWgParams; ++k)
                    if (k < np) acc[k] += (g_first[k * 64] - (lane == 0 ? g_carry[k] : g_cur[k * 64 - 1])) * Hprev;
            }
            wave_sync_lds();
            if (lane == last) {
#pragma unroll
                for (int k = 0; k < kWgParams; ++k)
                    if (k < np) g_carry[k] = gp[k];
            }
            F_carry = readlane_f64(Fp, last);
            H_carry = readlane_f64(Hp, last);
            ia += iend;
            ib += T - iend;
        }
        // the last interval to +inf (:165-171,204-210,212-221) on the counts of the whole pair
        const unsigned long long anybad = __ballot(bad_cat), anyzero = __ballot(zero_norm);
        if (lane == 0 && Finf > F_carry) score += (Finf - F_carry) * H_carry;
        wave_sync_lds();
        if (lane == 0) {  // ... which ends at G(inf) = 0
#pragma unroll
            for (int k = 0; k < kWgParams; ++k)
                if (k < np) acc[k] += (0.0 - g_carry[k]) * H_carry;
        }
        const double total = wave_sum_f64(score);
        const bool bad = anybad || anyzero;
        if (lane == 0) {
            if (anybad) sweep_report(args.hst, ST_BAD_CATEGORY);
            if (anyzero) sweep_report(args.hst, ST_ZERO_NORM);
            wa.scores[p] = bad ? nan("") : total;
        }
        // the row: one wave reduction per parameter, in lane order
#pragma unroll
        for (int k = 0; k < kWgParams; ++k) {
            if (k < NP) {
                const double s = wave_sum_f64(acc[k]);
                if (lane == 0) out[k] = bad ? nan("") : s;
            }
        }
    }
}

bool launch_weight_gradient(hipStream_t s, const WeightGradientArgs& a) {
    if (a.sw.n_pairs <= 0) return true;
    if (a.n_categories < 1 || a.n_categories > kSensitivityMaxCategories || a.width < 1 || a.width > kWeightGradientMaxParams) return false;
    const size_t wb = column_wave_bytes(a.n_categories, wg_front(a.width));
    return launch_most_waves(kColumnDynMax, wb, a.sw.n_pairs, [&](auto wpb, unsigned grid) {
        constexpr int WPB = decltype(wpb)::value;
        k_weight_gradient<WPB><<<grid, 64 * WPB, wb * WPB, s>>>(a, (int)wb);
    });
}

void init_weight_gradient_kernels() {
    raise_dynamic_lds({kernel_ptr(&k_weight_gradient<4>), kernel_ptr(&k_weight_gradient<2>), kernel_ptr(&k_weight_gradient<1>)}, kColumnDynMax);
    (void)hipGetLastError();
}

}  // namespace lchd
