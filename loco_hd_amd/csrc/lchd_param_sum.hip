// lchd_param_sum.hip -- reduced parameter gradients (additive, not in the reference): the rows of one tile of a per-pair parameter-gradient
// call (k_category_gradient: [P][C]; k_weight_gradient: scores[P] | grad[P][NP]) multiplied by the pair weights and added into exact
// fixed-point accumulators (lchd_exact_sum.h), one per bucket and column.  The per-slot arithmetic is lchd_param_sum.h's.
//
//   k_param_accumulate<DICT>  Every pair of a call adds to the same few accumulators, so nothing is added per pair: a grid of at most
//                       kParamSumMaxBlocks workgroups (LCHD_PARAM_SUM_BLOCKS lowers the cap), whatever the pair count.  Lanes own columns:
//                       with W' the power of two >= W, a wavefront is 64 / W' row slices of W' lanes, slice s of wavefront i reads row
//                       (i * 64 / W' + s) of every stride -- consecutive rows, consecutive addresses.  The use test reads the row's
//                       first column through a shuffle from the slice's lane 0.
//                       DICT = false (one bucket, or no bucket array: everything goes to bucket 0): each lane keeps its column's eight
//                       limb partial sums in registers across its whole stride loop; at the end the partial sums of a column are added over its 64 / W' lanes with shuffles of the 64-bit
//                       limbs -- integer sums: exact, whatever the order -- and the lanes of slice 0 issue one integer atomic per
//                       non-zero limb: at most one per limb, column and wavefront.
//                       DICT = true (bucket = wf_index[p]): the bucket changes from row to row, so a lane cannot carry one column's sums;
//                       each term goes to acc[bucket][column] at once (lchd_xs_add_parts: at most three integer atomics).
//                       A dictionary WITHOUT an index scores every pair with function 0: that is the single-bucket form into row 0 of
//                       acc[n_wf][W]; the other rows stay zero.
//                       The weight form's tile scores are copied to the caller's array by the lanes of column 0.  No floating-point
//                       atomics; an out-of-range term adds nothing and the flag is ORed once per wavefront.
//   k_param_finish      one lane per accumulator: the correctly rounded double into out[buckets][W], limbs zeroed for the next call.
#include "lchd_device.h"
#include "lchd_exact_sum.h"
#include "lchd_param_sum.h"

namespace lchd {

template <bool DICT>
__global__ __launch_bounds__(256) void k_param_accumulate(ParamSumArgs a) {
    const int lane = threadIdx.x & 63;
    const int W = a.width, Wp = a.width_pow2, slices = 64 / Wp;
    const int col = lane & (Wp - 1), slice = lane / Wp;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * 4;
    int64_t part[LCHD_GRAD_LIMBS] = {};
    bool bad = false;
    // (every lane of a wavefront takes every trip of the loop: the shuffle below needs the slice's lane 0)
    for (int64_t base = wave0 * slices; base < a.n_pairs; base += n_waves * slices) {
        const int64_t p = base + slice;
        const bool in = p < a.n_pairs && col < W;
        const double x = in ? a.rows[p * a.ld + col] : 0.0;
        const double x0 = __shfl(x, slice * Wp);
        if (in && col == 0 && a.scores_out) a.scores_out[p] = a.scores_in[p];
        if (in && lchd_param_use(x0)) {
            const double v = a.weights ? a.weights[p] : 1.0;
            if (DICT) {
                const int b = a.bucket[p];
                const lchd_xs_parts r = lchd_xs_split(v * x);
                if (b < 0 || b >= a.n_buckets) {  // (the per-pair pass fails such a tile before it is added: never taken)
                } else if (!r.ok) {
                    bad = true;
                } else {
                    lchd_xs_add_parts(a.acc + ((int64_t)b * W + col) * LCHD_GRAD_LIMBS, r);
                }
            } else if (!lchd_param_slot(part, v, x)) {
                bad = true;
            }
        }
    }
    if (__ballot(bad) && lane == 0) lchd_xs_flag_or(a.flag, LCHD_XS_OUT_OF_RANGE);
    if (DICT) return;
    // the column's eight limbs over its lanes (lanes col, col + W', ...): the lanes of slice 0 end with the totals
#pragma unroll
    for (int k = 0; k < LCHD_GRAD_LIMBS; ++k) {
        long long t = part[k];
        for (int off = 32; off >= Wp; off >>= 1) t += __shfl_xor(t, off);
        if (slice == 0 && col < W && t != 0) lchd_xs_limb_add(a.acc + (int64_t)col * LCHD_GRAD_LIMBS + k, t);
    }
}

__global__ __launch_bounds__(256) void k_param_finish(int64_t* __restrict__ acc, int64_t n, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int64_t* const limbs = acc + i * LCHD_GRAD_LIMBS;
    int64_t mine[LCHD_GRAD_LIMBS];
#pragma unroll
    for (int k = 0; k < LCHD_GRAD_LIMBS; ++k) { mine[k] = limbs[k]; limbs[k] = 0; }
    out[i] = lchd_xs_finish(mine);
}

bool launch_param_accumulate(hipStream_t s, const ParamSumArgs& a, int max_blocks) {
    if (a.n_pairs <= 0) return true;
    if (a.width < 1 || a.width > kParamSumMaxWidth || a.ld < a.width || !a.rows || !a.acc || !a.flag || a.n_buckets < 1 ||
        (!a.scores_out != !a.scores_in))
        return false;
    ParamSumArgs k = a;
    k.width_pow2 = 1;
    while (k.width_pow2 < a.width) k.width_pow2 <<= 1;
    const int64_t per_block = 4 * (64 / k.width_pow2);  // rows one workgroup takes per stride
    const int64_t blocks = (a.n_pairs + per_block - 1) / per_block;
    const int cap = max_blocks > 0 && max_blocks < kParamSumMaxBlocks ? max_blocks : kParamSumMaxBlocks;
    const unsigned grid = (unsigned)(blocks < cap ? blocks : cap);
    if (a.bucket) k_param_accumulate<true><<<grid, 256, 0, s>>>(k);
    else k_param_accumulate<false><<<grid, 256, 0, s>>>(k);
    return true;
}

bool launch_param_finish(hipStream_t s, int64_t* acc, int64_t n, double* out) {
    if (n <= 0) return true;
    const int64_t blocks = (n + 255) / 256;
    if (!acc || !out || blocks > 0x7FFFFFFF) return false;
    k_param_finish<<<(unsigned)blocks, 256, 0, s>>>(acc, n, out);
    return true;
}

}  // namespace lchd
