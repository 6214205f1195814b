// lchd_gradient.hip -- native coordinate gradients (additive, not in the reference): the sensitivity lists of one tile of pairs reduced
// on the device into exact fixed-point accumulators (lchd_exact_sum.h), one per atom and component.
//
//   k_grad_accumulate   one wavefront per (pair, side), lanes stride over the slots of the pair's row.  The contribution of slot k >= 1,
//                       in IEEE float64 with no contraction (the TU is built with -ffp-contract=off):
//                           use    = idx[p][k] >= 0  &&  dist[p][k] > 0  &&  isfinite(g[p][k])
//                           coef   = (v_p * g[p][k]) / dist[p][k]              (v_p = 1.0 without pair weights)
//                           step_c = coef * (x[m][c] - x[a][c])               m = idx[p][k]
//                           acc[m][c] += step_c ;  acc[a][c] += -step_c
//                       a = idx[p][0] (thresholded lists: the anchor) or a = p (dense rows: the row's own atom, which slot 0 need not
//                       name); with `disp` given, step_c = coef * disp[p][k][c] and no coordinate is read.  The member's step goes to
//                       its limbs at once (lchd_xs_add: at most three 64-bit integer atomics per component, zero chunks skipped).  The
//                       anchor's -sum(step) is first summed as integer limbs in each lane's registers, then over the wavefront with
//                       shuffles of the 64-bit limbs -- integer sums: exact, whatever the order -- and the 24 totals leave through
//                       lanes 0 .. 23, one contiguous 192-byte row of at most 24 atomics per pair and side.
//                       No floating-point atomics; an out-of-range step (lchd_exact_sum.h) adds nothing and raises the flag.
//   k_grad_finish       one lane per (atom, component): the correctly rounded double of the accumulator into grad[N][3], limbs zeroed
//                       for the next call.
//   k_strain_accumulate the strain derivative W of both sides (lchd_strain_sum.h): W[i][j] += step_i * disp[p][k][j], i <= j, over the
//                       slots k_grad_accumulate uses, from lists that carry `disp`.  Every slot of a call adds to the same 48 limbs of
//                       its side, so nothing is added per slot: a grid of at most kStrainMaxBlocks workgroups, whatever the pair count;
//                       a wavefront serves ONE side (its index's parity, which the grid stride keeps) and carries that side's 6 x 8
//                       limb partial sums in each lane's registers across its whole loop over the pairs; at the end the sums go over
//                       the wavefront with shuffles of the 64-bit limbs, and lanes 0 .. 47 issue one integer atomic each (zero sums
//                       skipped).  A partial sum takes 2^31 terms like a limb: the host layer keeps a call's slots per side below that.
//   k_strain_finish     one workgroup: both sides' six sums rounded once into the symmetric double[9] tensors, limbs zeroed.
#include "lchd_device.h"
#include "lchd_exact_sum.h"
#include "lchd_strain_sum.h"

namespace lchd {

// lane-local limbs += the chunks of one value (negate: with the opposite sign); selects, no indexed register access
__device__ __forceinline__ void grad_reg_add(int64_t (&limb)[LCHD_GRAD_LIMBS], const lchd_xs_parts& r, bool negate) {
    const bool neg = (r.negative != 0) != negate;
#pragma unroll
    for (int k = 0; k < LCHD_GRAD_LIMBS; ++k) {
        const int j = k - r.first;
        const uint32_t c = j == 0 ? r.chunk[0] : (j == 1 ? r.chunk[1] : (j == 2 ? r.chunk[2] : 0u));
        limb[k] += neg ? -(int64_t)c : (int64_t)c;
    }
}

__global__ __launch_bounds__(256) void k_grad_accumulate(GradAccumArgs ga) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    const int64_t K = ga.width;
    for (int64_t w = wave0; w < 2 * ga.n_pairs; w += n_waves) {
        const int64_t p = w >> 1;
        const GradSide& S = ga.s[w & 1];
        const int32_t* __restrict__ idx = S.idx + p * K;
        const double* __restrict__ dist = S.dist + p * K;
        const double* __restrict__ g = S.g + p * K;
        const int64_t a = ga.dense ? p : (int64_t)idx[0];
        if (a < 0 || a >= S.n) continue;  // (an unusable pair: its rows are padding and NaN)
        const double v = ga.weights ? ga.weights[p] : 1.0;
        double ax = 0.0, ay = 0.0, az = 0.0;
        if (!S.disp) { ax = S.x[a]; ay = S.y[a]; az = S.z[a]; }
        int64_t mine[3][LCHD_GRAD_LIMBS] = {};
        bool bad = false;
        for (int64_t k = 1 + lane; k < K; k += 64) {
            const int64_t m = idx[k];
            const double d = dist[k], gk = g[k];
            if (m < 0 || m >= S.n || !(d > 0.0) || !isfinite(gk)) continue;
            const double coef = (v * gk) / d;
            double step[3];
            if (S.disp) {
                const double* __restrict__ dp = S.disp + 3 * (p * K + k);
                step[0] = coef * dp[0]; step[1] = coef * dp[1]; step[2] = coef * dp[2];
            } else {
                step[0] = coef * (S.x[m] - ax); step[1] = coef * (S.y[m] - ay); step[2] = coef * (S.z[m] - az);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const lchd_xs_parts r = lchd_xs_split(step[c]);
                if (!r.ok) { bad = true; continue; }
                int64_t* const limbs = S.acc + (m * 3 + c) * LCHD_GRAD_LIMBS;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int q = r.first + j;
                    if (r.chunk[j] && q < LCHD_GRAD_LIMBS) lchd_xs_limb_add(limbs + q, r.negative ? -(int64_t)r.chunk[j] : (int64_t)r.chunk[j]);
                }
                grad_reg_add(mine[c], r, true);
            }
        }
        if (__ballot(bad) && lane == 0) lchd_xs_flag_or(ga.flag, LCHD_XS_OUT_OF_RANGE);
        // the anchor's 24 limbs: every lane ends with the wave's totals, lane i adds total i
        int64_t out = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < LCHD_GRAD_LIMBS; ++k) {
                long long t = mine[c][k];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
                if (lane == c * LCHD_GRAD_LIMBS + k) out = t;
            }
        if (lane < 3 * LCHD_GRAD_LIMBS && out != 0) lchd_xs_limb_add(S.acc + a * (3 * LCHD_GRAD_LIMBS) + lane, out);
    }
}

__global__ __launch_bounds__(256) void k_grad_finish(int64_t* __restrict__ acc, int64_t n3, double* __restrict__ grad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n3) return;
    int64_t* const limbs = acc + i * LCHD_GRAD_LIMBS;
    int64_t mine[LCHD_GRAD_LIMBS];
#pragma unroll
    for (int k = 0; k < LCHD_GRAD_LIMBS; ++k) { mine[k] = limbs[k]; limbs[k] = 0; }
    grad[i] = lchd_xs_finish(mine);
}

__global__ __launch_bounds__(256) void k_strain_accumulate(GradAccumArgs ga, int64_t* __restrict__ acc_a, int64_t* __restrict__ acc_b) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    const int side = (int)(wave0 & 1);  // (n_waves is a multiple of 4: every w of this wavefront's loop has this parity)
    const GradSide& S = ga.s[side];
    const int64_t K = ga.width;
    int64_t part[LCHD_STRAIN_COMPONENTS][LCHD_GRAD_LIMBS] = {};
    bool bad = false;
    for (int64_t w = wave0; w < 2 * ga.n_pairs; w += n_waves) {
        const int64_t p = w >> 1;
        const int32_t* __restrict__ idx = S.idx + p * K;
        const double* __restrict__ dist = S.dist + p * K;
        const double* __restrict__ g = S.g + p * K;
        const double* __restrict__ disp = S.disp + 3 * (p * K);
        const int64_t a = ga.dense ? p : (int64_t)idx[0];
        if (a < 0 || a >= S.n) continue;
        const double v = ga.weights ? ga.weights[p] : 1.0;
        for (int64_t k = 1 + lane; k < K; k += 64) {
            const int64_t m = idx[k];
            const double d = dist[k], gk = g[k];
            if (m < 0 || m >= S.n || !(d > 0.0) || !isfinite(gk)) continue;
            const double dp[3] = {disp[3 * k], disp[3 * k + 1], disp[3 * k + 2]};
            if (!lchd_strain_slot(part, v, gk, d, dp)) bad = true;
        }
    }
    if (__ballot(bad) && lane == 0) lchd_xs_flag_or(ga.flag, LCHD_XS_OUT_OF_RANGE);
    // the side's 48 limbs: every lane ends with the wave's totals, lane i adds total i
    int64_t out = 0;
#pragma unroll
    for (int c = 0; c < LCHD_STRAIN_COMPONENTS; ++c)
#pragma unroll
        for (int k = 0; k < LCHD_GRAD_LIMBS; ++k) {
            long long t = part[c][k];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
            if (lane == c * LCHD_GRAD_LIMBS + k) out = t;
        }
    if (lane < LCHD_STRAIN_LIMBS && out != 0) lchd_xs_limb_add((side ? acc_b : acc_a) + lane, out);
}

// acc: [2][LCHD_STRAIN_LIMBS], side A then side B
__global__ __launch_bounds__(128) void k_strain_finish(int64_t* __restrict__ acc, double* __restrict__ strain_a, double* __restrict__ strain_b) {
    const int t = threadIdx.x, side = t / 9, e = t % 9, i = e / 3, j = e % 3;
    double v = 0.0;
    if (t < 18) {
        const int64_t* const limbs = acc + side * LCHD_STRAIN_LIMBS + lchd_strain_component(i < j ? i : j, i < j ? j : i) * LCHD_GRAD_LIMBS;
        int64_t mine[LCHD_GRAD_LIMBS];
#pragma unroll
        for (int k = 0; k < LCHD_GRAD_LIMBS; ++k) mine[k] = limbs[k];
        v = lchd_xs_finish(mine);
    }
    __syncthreads();
    if (t < 18) (side ? strain_b : strain_a)[e] = v;
    if (t < 2 * LCHD_STRAIN_LIMBS) acc[t] = 0;
}

bool launch_strain_accumulate(hipStream_t s, const GradAccumArgs& a, int64_t* acc) {
    if (a.n_pairs <= 0) return true;
    if (a.width < 1 || !a.flag || !acc) return false;
    for (int k = 0; k < 2; ++k)
        if (!a.s[k].idx || !a.s[k].dist || !a.s[k].g || !a.s[k].disp || a.s[k].n < 1 || (a.dense && a.s[k].n < a.n_pairs)) return false;
    const int64_t blocks = (2 * a.n_pairs + 3) / 4;
    k_strain_accumulate<<<(unsigned)(blocks < kStrainMaxBlocks ? blocks : kStrainMaxBlocks), 256, 0, s>>>(a, acc, acc + LCHD_STRAIN_LIMBS);
    return true;
}

bool launch_strain_finish(hipStream_t s, int64_t* acc, double* strain_a, double* strain_b) {
    if (!acc || !strain_a || !strain_b) return false;
    k_strain_finish<<<1, 128, 0, s>>>(acc, strain_a, strain_b);
    return true;
}

bool launch_grad_accumulate(hipStream_t s, const GradAccumArgs& a) {
    if (a.n_pairs <= 0) return true;
    if (a.width < 1 || !a.flag) return false;
    for (int k = 0; k < 2; ++k)
        if (!a.s[k].idx || !a.s[k].dist || !a.s[k].g || !a.s[k].acc || a.s[k].n < 1 || (a.dense && a.s[k].n < a.n_pairs) ||
            (!a.s[k].disp && (!a.s[k].x || !a.s[k].y || !a.s[k].z)))
            return false;
    const int64_t blocks = (2 * a.n_pairs + 3) / 4;
    k_grad_accumulate<<<(unsigned)(blocks < 65536 ? blocks : 65536), 256, 0, s>>>(a);
    return true;
}

bool launch_grad_finish(hipStream_t s, int64_t* acc, int64_t n_atoms, double* grad) {
    if (n_atoms <= 0) return true;
    const int64_t n3 = 3 * n_atoms, blocks = (n3 + 255) / 256;
    if (!acc || !grad || blocks > 0x7FFFFFFF) return false;
    k_grad_finish<<<(unsigned)blocks, 256, 0, s>>>(acc, n3, grad);
    return true;
}

}  // namespace lchd
