// lchd_profile.hip -- the local composition profile of an environment (additive, not in the reference): the weight-function-averaged
// PMF the sweeps integrate a distance of, written out as one vector per anchor.
//
//   P_c = sum_k (F(d_{k+1}) - F(d_k)) * w_c n_c(k) / N(k),   N(k) = sum_c' w_c' n_c'(k),   d_n = +inf
//       = w_c * sum_{j : c_j = c} T_j,                         T_j = sum_{k >= j} (F(d_{k+1}) - F(d_k)) / N(k)
//
// over one sorted environment of the store the environment kernels built (EnvStore: ascending F keys of the anchor's weight function,
// categories, lengths).  The kernel evaluates no CDF: it reads the key set of the entry's weight function, the last interval ends at
// DevConfig::wf_finf.
//
// Shape: ONE wavefront per output row, four rows per workgroup, for every environment size.  The environments of a call are many and
// of one kind -- some 10^2 points behind a threshold, or as many dense rows as a row has points -- so there are always thousands of
// wavefronts to fill the part with, and a row never needs a workgroup of its own.  One code path also keeps the arithmetic of a row a
// function of the row alone, whatever slot size the call's largest environment asked for:
//   pass 1 (forward, 64 points at a time)  the running weight N in front of every chunk, kept in LDS
//   pass 2 (backward)                      per chunk N(k) by a lane scan on top of the chunk's carry, the quotients, their suffix sums
//                                          T_j by a lane scan on top of the chunk behind, then one sum per category that occurs in
//                                          the chunk, added to the category's LDS accumulator by lane 0
// Every sum has a fixed shape (DPP scans, chunks last to first, categories in order of first occurrence): no floating-point atomics,
// the same bits for the same stored environment.  Categories are taken kProfTile at a time (pass 2 is repeated per tile), so any
// category count works; up to kProfTile categories -- every typing scheme in use -- it is one pass.
#include "lchd_sweep_common.h"

namespace lchd {

constexpr int kProfWaves = 4;
constexpr int kProfTile = 512;             // most category accumulators per wavefront (4 KB of LDS)
constexpr int kProfChunks = kProfMaxPoints / 64;  // most chunk carries per wavefront (8 KB of LDS)

// inclusive prefix sum over the lanes (the shape of wave_sum_f64, without the broadcast of the total)
__device__ __forceinline__ double wave_incl_scan_f64(double v) {
    v += dpp_mov_f64_or_zero<0x111, 0xf>(v);  // row_shr:1
    v += dpp_mov_f64_or_zero<0x112, 0xf>(v);  // row_shr:2
    v += dpp_mov_f64_or_zero<0x114, 0xf>(v);  // row_shr:4
    v += dpp_mov_f64_or_zero<0x118, 0xf>(v);  // row_shr:8
    v += dpp_mov_f64_or_zero<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
    v += dpp_mov_f64_or_zero<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3
    return v;
}

// Dynamic LDS per wavefront: `chunks` carries (what the store's stride can hold) and min(C, kProfTile) accumulators -- a few hundred
// bytes for thresholded environments of a dozen categories, so the launch is not held back by the 12 KB the largest row would need.
__global__ __launch_bounds__(64 * kProfWaves) void k_profile(ProfileArgs a, int chunks, int tile) {
    extern __shared__ double prof_smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double* const carry = prof_smem + (size_t)wave * (chunks + tile);
    double* const acc = carry + chunks;
    const DevConfig& cfg = *a.cfg;
    const int C = cfg.n_categories;
    const double* __restrict__ cat_w = cfg.cat_w;
    for (int64_t p = (int64_t)blockIdx.x * kProfWaves + wave; p < a.n; p += (int64_t)gridDim.x * kProfWaves) {
        double* const out = a.out + (a.out_row ? a.out_row[p] : p) * (int64_t)C;
        int64_t e = p;
        bool ok = true;
        if (a.anchors) {  // (an index outside the structure: flagged by the prologue)
            const int64_t ia = a.anchors[p];
            ok = ia >= 0 && ia < a.n_atoms;
            if (ok) e = a.slot[ia];
        }
        const int w = a.wf_index ? a.wf_index[p] : 0;
        if (w < 0 || w >= a.env.cdf_keys) {
            if (lane == 0) sweep_report(a.hst, ST_BAD_WF);
            ok = false;
        }
        const int n = ok ? a.env.len[e] : 0;
        if (n <= 0 || n > chunks * 64) {  // an unusable environment (flagged by the kernel that built it)
            for (int i = lane; i < C; i += 64) out[i] = nan("");
            continue;
        }
        const uint64_t* __restrict__ key = a.env.key + (int64_t)w * a.env.set_stride + e * a.env.stride;
        const uint8_t* __restrict__ c8 = a.env.cat + e * a.env.stride * (a.env.cat16 ? 2 : 1);
        const uint16_t* __restrict__ c16 = reinterpret_cast<const uint16_t*>(c8);
        const bool wide = a.env.cat16 != 0;
        const double finf = cfg.wf_finf[w];
        const int n_chunks = (n + 63) >> 6;
        auto cat_at = [&](int i) -> int {
            const int c = wide ? (int)c16[i] : (int)c8[i];
            return c < C ? c : 0;  // (the environment kernels store 0 for an id outside the map and report it)
        };
        // pass 1: the weight in front of every chunk
        double run = 0.0;
        for (int ch = 0; ch < n_chunks; ++ch) {
            const int i = (ch << 6) + lane;
            const double wv = i < n ? cat_w[cat_at(i)] : 0.0;
            if (lane == 0) carry[ch] = run;
            run += wave_sum_f64(wv);
        }
        wave_sync_lds();
        for (int t0 = 0; t0 < C; t0 += tile) {
            const int tn = min(tile, C - t0);
            for (int i = lane; i < tn; i += 64) acc[i] = 0.0;
            wave_sync_lds();
            double tail = 0.0;  // T of the first point of the chunk behind
            for (int ch = n_chunks - 1; ch >= 0; --ch) {
                const int i = (ch << 6) + lane;
                const bool valid = i < n;
                const int c = valid ? cat_at(i) : 0;
                const double wv = valid ? cat_w[c] : 0.0;
                const double N = carry[ch] + wave_incl_scan_f64(wv);
                double g = 0.0;
                if (valid) {
                    const double f0 = u2d(key[i]), f1 = i + 1 < n ? u2d(key[i + 1]) : finf;
                    g = (f1 - f0) / N;
                }
                // suffix sums: the lanes mirrored, an inclusive prefix scan, mirrored back
                const double T = shfl_f64(wave_incl_scan_f64(shfl_f64(g, 63 - lane)), 63 - lane) + tail;
                tail = readlane_f64(T, 0);
                const bool mine = valid && c >= t0 && c < t0 + tn;
                unsigned long long rem = __ballot(mine);
                while (rem) {  // one sum per category of the chunk, in order of first occurrence
                    const int leader = __ffsll((long long)rem) - 1;
                    const int cl = __builtin_amdgcn_readlane(c, leader);
                    const unsigned long long m = __ballot(mine && c == cl);
                    const double s = wave_sum_f64(((m >> lane) & 1ull) ? T : 0.0);
                    if (lane == 0) acc[cl - t0] += s;
                    rem &= ~m;
                }
            }
            wave_sync_lds();
            for (int i = lane; i < tn; i += 64) out[t0 + i] = cat_w[t0 + i] * acc[i];
            wave_sync_lds();
        }
    }
}

// The anchor list of a one-sided pass as the pair list (i, i) the prologue de-duplicates.
__global__ void k_profile_pairs(const int64_t* __restrict__ anchors, int64_t n, int64_t* __restrict__ pairs) {
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = anchors[p];
        pairs[2 * p] = i;
        pairs[2 * p + 1] = i;
    }
}
// Dense rows: every row is an environment in use (what k_env_key_sets bounds its walk with).
__global__ void k_profile_rows(DeviceStatus* st, uint32_t n_rows) {
    st->n_unique[0] = n_rows;
    st->n_unique[1] = 0u;
}
// The end of a pass without a sweep: the status words go to the host-mapped mirror, the device status is reset (publish_status; no
// record pass counted anything: n_small = ~0).
__global__ void k_profile_publish(SweepArgs args) { publish_status(args, ~0ull, 0u); }

void launch_profile(hipStream_t s, const ProfileArgs& a) {
    if (a.n <= 0) return;
    const int64_t nb = (a.n + kProfWaves - 1) / kProfWaves;
    const int chunks = (int)std::min<int64_t>((a.env.stride + 63) / 64, kProfChunks), tile = std::min(a.n_categories, kProfTile);
    const size_t lds = (size_t)kProfWaves * (size_t)(chunks + tile) * sizeof(double);  // at most 48 KB
    k_profile<<<(unsigned)(nb < 16384 ? nb : 16384), 64 * kProfWaves, lds, s>>>(a, chunks, tile);
}
void launch_profile_pairs(hipStream_t s, const int64_t* anchors, int64_t n, int64_t* pairs) {
    if (n <= 0) return;
    const int64_t nb = (n + 255) / 256;
    k_profile_pairs<<<(unsigned)(nb < 4096 ? nb : 4096), 256, 0, s>>>(anchors, n, pairs);
}
void launch_profile_rows(hipStream_t s, DeviceStatus* st, int64_t n_rows) { k_profile_rows<<<1, 1, 0, s>>>(st, (uint32_t)n_rows); }
void launch_profile_publish(hipStream_t s, DeviceStatus* st, HostStatus* hst, uint32_t seq) {
    SweepArgs args{};
    args.st = st;
    args.hst = hst;
    args.seq = seq;
    k_profile_publish<<<1, 1, 0, s>>>(args);
}

}  // namespace lchd
