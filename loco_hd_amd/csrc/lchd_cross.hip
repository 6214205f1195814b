// lchd_cross.hip -- cross-scoring (additive, not in the reference): every anchor of one list against every anchor of another, and per
// row the k best matches.  The scores come from the thresholded pass as it is (lchd_capi.hip runs it per row tile); this translation
// unit holds what stands in front of it and behind it:
//   k_cross_pairs    the pair records of one row tile, written where the pass reads them: pair p = i * n_b + j of the tile is
//                    (anchors_a[row0 + i], anchors_b[j]).  One thread per record, one 16-byte store each; no pair list ever exists on
//                    the host.  The anchors are copied as they are: the pass checks them like any caller's.
//   k_nearest_rows   one wavefront per row of the tile's [rows][n_b] scores.  The comparison key is (score, column) exactly: the score
//                    as its order-preserving 64-bit image (-0 counts as +0, a NaN as the largest value), the column as the tie-break,
//                    so the k results are a function of the score matrix alone.  Lane l keeps the smallest key among the columns
//                    j = l (mod 64) that are not selected yet.  One selection step is a wave-wide minimum of the 64 candidates over DPP
//                    (row_shr 1/2/4/8, the two row broadcasts, v_readlane of lane 63); the winner's lane then needs its next
//                    candidate, the smallest key above the winner among its own n_b / 64 columns, which the whole wavefront looks
//                    for together (a second wave-wide minimum).  The row is read once plus k * n_b / 64 elements; no LDS, no
//                    atomics.  Result m of the row lives in lane m until lanes 0 .. k - 1 write scores and columns: one writer per
//                    output element, nothing depends on the tile the row is in.
#include "lchd_cross_plan.h"
#include "lchd_kcommon.h"

namespace lchd {

__global__ __launch_bounds__(256) void k_cross_pairs(const int64_t* __restrict__ anchors_a, const int64_t* __restrict__ anchors_b, uint32_t n_b,
                                                     uint32_t n_pairs, int32_t wf, int64_t* __restrict__ pairs, int32_t* __restrict__ wf_out) {
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n_pairs; p += (uint64_t)gridDim.x * 256) {
        const uint32_t i = (uint32_t)p / n_b, j = (uint32_t)p - i * n_b;
        longlong2 rec;
        rec.x = anchors_a[i];
        rec.y = anchors_b[j];
        reinterpret_cast<longlong2*>(pairs)[p] = rec;
        if (wf >= 0) wf_out[p] = wf;
    }
}

void launch_cross_pairs(hipStream_t s, const int64_t* anchors_a, const int64_t* anchors_b, int64_t row0, int64_t rows, int64_t n_b, int32_t wf,
                        int64_t* pairs, int32_t* wf_out) {
    const int64_t n_pairs = rows * n_b;
    if (n_pairs <= 0 || n_pairs > kCrossMaxTilePairs) return;  // (the entry points refuse such a tile)
    const int64_t nb = (n_pairs + 255) / 256;
    k_cross_pairs<<<(unsigned)(nb < 8192 ? nb : 8192), 256, 0, s>>>(anchors_a + row0, anchors_b, (uint32_t)n_b, (uint32_t)n_pairs, wf, pairs, wf_out);
}

// ---- k best columns per row ----------------------------------------------------------------------------------------------------------
constexpr uint64_t kNoKey = ~0ull;
constexpr uint32_t kNoCol = ~0u;  // (kNoKey, kNoCol): above every key of a column

__device__ __forceinline__ uint64_t nearest_key(double v) {
    if (v != v) return kNoKey;
    return ordered_key(v + 0.0);  // (-0 + 0 == +0: the two zeros compare equal, as the doubles do)
}
__device__ __forceinline__ bool key_less(uint64_t ka, uint32_t ja, uint64_t kb, uint32_t jb) { return ka < kb || (ka == kb && ja < jb); }

// one DPP step of the minimum: lanes without a source lane (and the rows ROW_MASK leaves out) read their own key, which changes nothing
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void key_min_step(uint64_t& k, uint32_t& j) {
    const int lo = (int)(uint32_t)k, hi = (int)(uint32_t)(k >> 32), jj = (int)j;
    const uint32_t olo = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
    const uint32_t ohi = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
    const uint32_t oj = (uint32_t)__builtin_amdgcn_update_dpp(jj, jj, CTRL, ROW_MASK, 0xf, false);
    const uint64_t ok = ((uint64_t)ohi << 32) | olo;
    if (key_less(ok, oj, k, j)) { k = ok; j = oj; }
}
// the smallest (key, column) of the 64 lanes, wave-uniform
__device__ __forceinline__ void wave_min_key(uint64_t& k, uint32_t& j) {
    key_min_step<0x111, 0xf>(k, j);  // row_shr:1
    key_min_step<0x112, 0xf>(k, j);  // row_shr:2
    key_min_step<0x114, 0xf>(k, j);  // row_shr:4
    key_min_step<0x118, 0xf>(k, j);  // row_shr:8
    key_min_step<0x142, 0xa>(k, j);  // row_bcast:15 into rows 1 and 3
    key_min_step<0x143, 0xc>(k, j);  // row_bcast:31 into rows 2 and 3: lane 63 holds the minimum
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)k, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(k >> 32), 63);
    k = ((uint64_t)hi << 32) | lo;
    j = (uint32_t)__builtin_amdgcn_readlane((int)j, 63);
}

constexpr int kNearestWaves = 4;  // rows per workgroup

__global__ __launch_bounds__(64 * kNearestWaves) void k_nearest_rows(const double* __restrict__ scores, int64_t rows, uint32_t n_b, int32_t k,
                                                                     double* __restrict__ out_scores, int32_t* __restrict__ out_cols) {
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kNearestWaves + wv;
    if (row >= rows) return;  // (wave-uniform)
    const double* __restrict__ s = scores + row * (int64_t)n_b;
    uint64_t ck = kNoKey;
    uint32_t cj = kNoCol;
    for (uint32_t j = lane; j < n_b; j += 64) {
        const uint64_t key = nearest_key(s[j]);
        if (key_less(key, j, ck, cj)) { ck = key; cj = j; }
    }
    uint32_t mine = 0;
    for (int m = 0; m < k; ++m) {  // k <= n_b: every step finds a column
        uint64_t wk = ck;
        uint32_t wj = cj;
        wave_min_key(wk, wj);
        if (lane == (uint32_t)m) mine = wj;
        const uint32_t w = wj & 63;  // the lane the winner came from
        uint64_t nk = kNoKey;
        uint32_t nj = kNoCol;
        if (n_b > 64) {  // its next candidate: the smallest key above the winner among the columns w (mod 64)
            for (uint32_t j = w + 64 * lane; j < n_b; j += 64 * 64) {
                const uint64_t key = nearest_key(s[j]);
                if (key_less(wk, wj, key, j) && key_less(key, j, nk, nj)) { nk = key; nj = j; }
            }
            wave_min_key(nk, nj);
        }
        if (lane == w) { ck = nk; cj = nj; }
    }
    if (lane < (uint32_t)k) {
        out_cols[row * k + lane] = (int32_t)mine;
        out_scores[row * k + lane] = s[mine];
    }
}

void launch_nearest_rows(hipStream_t s, const double* scores, int64_t rows, int64_t n_b, int32_t k, double* out_scores, int32_t* out_cols) {
    if (rows <= 0 || k < 1 || k > kNearestMaxK || k > n_b || rows * n_b > kCrossMaxTilePairs) return;  // (the entry points refuse these)
    const int64_t nb = (rows + kNearestWaves - 1) / kNearestWaves;
    k_nearest_rows<<<(unsigned)nb, 64 * kNearestWaves, 0, s>>>(scores, rows, (uint32_t)n_b, k, out_scores, out_cols);
}

}  // namespace lchd
