// lchd_radial.hip -- radial score profiles (additive, not in the reference): the integrand of a pair's LoCoHD score resolved over
// distance bins.
//
//   out[p][k] = sum_j H_j * max(0, min(F(u_{j+1}), F(e_{k+1})) - max(F(u_j), F(e_k)))
//
// over the merged breakpoints u_0 = 0 <= u_1 <= ... <= u_J of the pair's two environments (u_{J+1} = +inf), H_j the statistical distance
// of the two PMFs between u_j and u_{j+1} -- exactly what the sweeps integrate, the anchors included -- and the caller's edges
// e_0 < ... < e_K.  With e_0 = 0 and e_K = +inf a row sums to the pair's score.
//
// The kernel works in KEY space.  It reads the F keys of both environment stores as a sweep does (EnvStore::cdf_keys >= 1, the key set
// of the pair's weight function) and the pair records of k_pair_meta; the bounds E_k = F_w(e_k) come from k_radial_bounds, which calls
// the CDF routine that wrote the keys (cdf_lean, + 0.0, running maximum: k_env_key_sets), so a point at distance exactly e_k has
// key == E_k bit for bit.  No CDF is evaluated per event.
//
// Shape: the column-tile skeleton of lchd_pair_columns.h (pair record, LDS, tile split, histogram scan) around an event loop of its
// own.  Between two events H is constant: the lane hands (F_lo, F_hi, H) to radial_split (lchd_radial_bins.h) with its running bin
// index.  The intervals of a tile ascend with the lane (the skeleton's interval rule), and so do the bins they add to.
// Sums (no floating-point atomics, a fixed shape for a stored pair):
//   a bin strictly between the first and the last bin a lane adds to in a tile is that lane's alone in the tile: plain adds to acc[k]
//   the first and the last bin of a lane may be shared with its neighbours: kept in registers, and after the walk every bin that occurs
//   among them takes ONE wave reduction (lane order), added to acc[k] by lane 0
//   the tail (F(inf) - F(u_J)) * H_J is split by lane 0 after the last tile
// Hellinger-2 with unit weights keeps the running Bhattacharyya numerator (O(1) per event, the literal form below kExactH2Below:
// lchd_team_tile.h); every other distance, and category weights, evaluate sd_eval on the lane's counts per event.
#include "lchd_pair_columns.h"
#include "lchd_radial_bins.h"

namespace lchd {

constexpr int kRadTab = kSqrtTab + 8;  // LDS square-root tables: counts 0 .. kSqrtTab (stores of at most kSqrtTab points per slot)

// StatisticalDistance::run on one lane's count column (cnt[c * 64] = count_A | count_B << 16): pmf.rs:65-83 normalises the weighted
// counts by their sums (one reciprocal per side, as the sweeps do).  Out of line: the library's pow / log stay out of the event loop's code.
static __device__ __noinline__ double radial_sd(int kind, double p0, double p1, const uint32_t* cnt, const double* __restrict__ w, int C,
                                                double ia, double ib) {
    return sd_eval<0>(kind, p0, p1, [&](int c) { return (w[c] * (double)(cnt[c * 64] & 0xFFFFu)) * ia; },
                      [&](int c) { return (w[c] * (double)(cnt[c * 64] >> 16)) * ib; }, C);
}

// In front of the count columns (lchd_pair_columns.h): bounds [65] | bin accumulators [64]
constexpr size_t kRadFront = (65 + 64) * 8;

// H2U: Hellinger-2 with unit weights.  CAT16: 16-bit category ids in the store (and the 16-bit-category pair record).  TAB: both
// stores have slots of at most kSqrtTab points, the square-root tables are read from LDS.  WPB: pairs (wavefronts) per workgroup.
template <bool H2U, bool CAT16, bool TAB, int WPB>
__global__ __launch_bounds__(64 * WPB) void k_radial(RadialArgs ra, int wave_bytes) {
    using CT = typename std::conditional<CAT16, uint16_t, uint8_t>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char rad_smem[];
    __shared__ double t_sqrt[TAB ? kRadTab : 1], t_rsqrt[TAB ? kRadTab : 1];
    const SweepArgs& args = ra.sw;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const DevConfig* __restrict__ cfgp = args.cfg;
    const int C = cfgp->n_categories, K = ra.n_bins;
    const double* __restrict__ g_sqrt = args.sqrt_tab;
    const double* __restrict__ g_rsqrt = args.rsqrt_tab;
    const double* __restrict__ cat_w = cfgp->cat_w;
    if constexpr (TAB) {
        for (int k = tid; k < kRadTab; k += 64 * WPB) { t_sqrt[k] = g_sqrt[k]; t_rsqrt[k] = g_rsqrt[k]; }
        __syncthreads();
    }
    const ColumnLds l = column_carve(rad_smem + (size_t)wv * wave_bytes, C, kRadFront);
    const uint64_t *const sA = l.sA, *const sB = l.sB;
    const uint16_t *const cA = l.cA, *const cB = l.cB;
    double* const Eb = reinterpret_cast<double*>(l.front);  // [K + 1] bounds of this pair's weight function
    double* const acc = Eb + 65;                            // [K]
    uint32_t* const cnt = l.cnt0 + lane;                    // this lane's column: cnt[c * 64]
    auto sqrt_cnt = [&](int k) -> double { if constexpr (TAB) return t_sqrt[k]; else return g_sqrt[k]; };
    auto rsqrt_cnt = [&](int k) -> double { if constexpr (TAB) return t_rsqrt[k]; else return g_rsqrt[k]; };

    const int n_sets = args.env_a.cdf_keys;
    const double* __restrict__ finf_tab = cfgp->wf_finf;
    const int sd_kind = cfgp->sd_kind;
    const double prm0 = cfgp->sd_p0, prm1 = cfgp->sd_p1;
    const int64_t pstride = (int64_t)gridDim.x * WPB;
    for (int64_t p = (int64_t)blockIdx.x * WPB + wv; p < args.n_pairs; p += pstride) {
        double* const out = ra.out + p * (int64_t)K;
        const PairHead h = pair_head_load<CAT16>(args, p, n_sets, lane);
        if (!h.usable) {
            for (int k = lane; k < K; k += 64) out[k] = nan("");
            continue;
        }
        const int64_t ea = h.ea, eb = h.eb;
        const int nA = h.nA, nB = h.nB, c0a = h.c0a, c0b = h.c0b, wfi = h.wfi;
        const uint64_t* __restrict__ kA = args.env_a.key + ea * args.env_a.stride + (int64_t)wfi * args.env_a.set_stride;
        const uint64_t* __restrict__ kB = args.env_b.key + eb * args.env_b.stride + (int64_t)wfi * args.env_b.set_stride;
        const CT* __restrict__ tA = reinterpret_cast<const CT*>(args.env_a.cat) + ea * args.env_a.stride;
        const CT* __restrict__ tB = reinterpret_cast<const CT*>(args.env_b.cat) + eb * args.env_b.stride;
        const double Finf = finf_tab[wfi];

        bool bad_cat = c0a >= C || c0b >= C, zero_norm = false;
        int totA = 1, totB = 1;     // points seen per side (incl. the anchor)
        double ra_ = 1.0, rb_ = 1.0;  // H2U: 1 / sqrt(total)
        double D = 0.0;             // H2U: sum_c sqrt(a_c b_c)
        auto exact_h2 = [&]() -> double {  // statistical_distances.rs:4-10, the literal difference-of-roots form
            double acc2 = 0.0;
            for (int c = 0; c < C; ++c) {
                const uint32_t v = cnt[c * 64];
                const double d = sqrt_cnt((int)(v & kMaskA)) * ra_ - sqrt_cnt((int)(v >> 16)) * rb_;
                acc2 = fma(d, d, acc2);
            }
            return 0.5 * acc2;
        };
        auto distance = [&]() -> double {
            if constexpr (H2U) {
                double h2 = 1.0 - (ra_ * rb_) * D;
                if (h2 < kExactH2Below) h2 = exact_h2();
                return sqrt_unit(h2);
            } else {
                double sa_ = 0.0, sb_ = 0.0;  // pmf.rs:67-68: fresh sums
                for (int c = 0; c < C; ++c) {
                    const uint32_t v = cnt[c * 64];
                    sa_ += cat_w[c] * (double)(v & kMaskA);
                    sb_ += cat_w[c] * (double)(v >> 16);
                }
                if (sa_ == 0.0 || sb_ == 0.0) zero_norm = true;
                return radial_sd(sd_kind, prm0, prm1, cnt, cat_w, C, 1.0 / sa_, 1.0 / sb_);
            }
        };

        // this pair's bounds, empty accumulators, the two anchors (src/locohd.rs:82-84) in the carry row and in every lane's column
        wave_sync_lds();
        for (int k = lane; k <= K; k += 64) Eb[k] = ra.bounds[(int64_t)wfi * (K + 1) + k];
        for (int k = lane; k < K; k += 64) acc[k] = 0.0;
        column_seed_anchors(l, cnt, C, c0a, c0b, lane);
        if (H2U && c0a == c0b && !bad_cat) D = 1.0;
        wave_sync_lds();
        double F_carry = u2d(kA[0]);  // F(0): both anchors sit at distance 0
        double H_carry = bad_cat ? 0.0 : distance();

        const int mA = nA - 1, mB = nB - 1, M = mA + mB;  // non-anchor events
        int ia = 0, ib = 0;
        for (int k0 = 0; k0 < M; k0 += kSweepTile) {
            const ColumnTile t = column_tile_stage(l, kA, kB, tA, tB, mA, mB, M, k0, ia, ib, lane);
            const int T = t.T, d0 = t.d0, d1 = t.d1, i0 = t.i0, i1 = t.i1, j0 = t.j0, j1 = t.j1, iend = t.iend, last = t.last;
            const bool has = t.has;
            totA = 1 + ia + i0;
            totB = 1 + ib + j0;
            if constexpr (H2U) D = 0.0;
            const bool bad_chunk = column_histogram_scan(l, cnt, t, C, lane, [&](uint32_t excl) {
                if constexpr (H2U) D += sqrt_cnt((int)(excl & kMaskA)) * sqrt_cnt((int)(excl >> 16));
            });
            if (bad_chunk) bad_cat = true;
            if constexpr (H2U) { ra_ = rsqrt_cnt(totA); rb_ = rsqrt_cnt(totB); }

            // pass 2: this lane's events, one after the other; every interval goes through radial_split with the running bin index
            int i = i0, j = j0;
            uint64_t ka = (i < i1) ? sA[i] : kPadKey, kb = (j < j1) ? sB[j] : kPadKey;
            const double firstF = has ? u2d(ka <= kb ? ka : kb) : 0.0;
            const double nextF = shfl_f64(firstF, min(lane + 1, 63));  // the first event of the next lane's chunk
            int curb = -1, bLo = -1, bHi = -1;  // the bin being added to; the first and the last bin of this lane in this tile
            double curv = 0.0, vLo = 0.0, vHi = 0.0;
            auto emit = [&](int k, double v) {
                if (k == curb) { curv += v; return; }
                if (curb >= 0) {
                    if (bLo < 0) { bLo = curb; vLo = curv; }
                    else acc[curb] += curv;  // between this lane's first and last bin: no other lane of the tile adds to it
                }
                curb = k;
                curv = v;
            };
            double Fp = F_carry, Hp = H_carry;
            bool open = lane == 0;  // lane 0 closes the interval the previous tile (or the anchors) left open
            int bin = has ? radial_bin_of(Eb, K, open ? F_carry : firstF) : 0;
            for (int e = d0; e < d1; ++e) {
                const bool takeA = (ka <= kb);  // an exhausted run shows the pad key (> every real key)
                const uint64_t key = takeA ? ka : kb;
                const int ct = takeA ? cA[i] : cB[j];
                if (takeA) { ++i; ka = (i < i1) ? sA[i] : kPadKey; } else { ++j; kb = (j < j1) ? sB[j] : kPadKey; }
                const double F = u2d(key);
                if (open) radial_split(Fp, F, Hp, Eb, K, bin, emit);
                open = true;
                // pmf.rs:47-63: one more point of category ct on one side
                const bool okc = ct < C;
                const int cs = okc ? ct : 0;
                const uint32_t old = cnt[cs * 64];
                cnt[cs * 64] = old + (okc ? (takeA ? kOneA : kOneB) : 0u);
                totA += takeA ? 1 : 0;
                totB += takeA ? 0 : 1;
                if constexpr (H2U) {
                    const int cntA_ = (int)(old & kMaskA), cntB_ = (int)(old >> 16);
                    const int mine = takeA ? cntA_ : cntB_, other = takeA ? cntB_ : cntA_;
                    const double delta = (sqrt_cnt(mine + 1) - sqrt_cnt(mine)) * sqrt_cnt(other);
                    const double r = rsqrt_cnt(takeA ? totA : totB);
                    ra_ = takeA ? r : ra_;
                    rb_ = takeA ? rb_ : r;
                    D += okc ? delta : 0.0;
                }
                Hp = distance();
                Fp = F;
            }
            if (has && lane < last) radial_split(Fp, nextF, Hp, Eb, K, bin, emit);
            if (curb >= 0) {
                if (bLo < 0) { bLo = curb; vLo = curv; }
                else { bHi = curb; vHi = curv; }
            }
            F_carry = readlane_f64(Fp, last);
            H_carry = readlane_f64(Hp, last);
            // the first / last bins of the lanes: one wave reduction per bin that occurs among them
            wave_sync_lds();
            unsigned long long remLo = __ballot(bLo >= 0), remHi = __ballot(bHi >= 0);
            while (remLo | remHi) {
                const int k = remLo ? __builtin_amdgcn_readlane(bLo, __ffsll((long long)remLo) - 1)
                                    : __builtin_amdgcn_readlane(bHi, __ffsll((long long)remHi) - 1);
                const double s = wave_sum_f64((bLo == k ? vLo : 0.0) + (bHi == k ? vHi : 0.0));
                if (lane == 0) acc[k] += s;
                remLo &= ~__ballot(bLo == k);
                remHi &= ~__ballot(bHi == k);
            }
            ia += iend;
            ib += T - iend;
        }
        // the last interval to +inf (:165-171,204-210,212-221), split like every other
        wave_sync_lds();
        if (lane == 0) {
            int bin = radial_bin_of(Eb, K, F_carry);
            radial_split(F_carry, Finf, H_carry, Eb, K, bin, [&](int k, double v) { acc[k] += v; });
        }
        wave_sync_lds();
        const unsigned long long anybad = __ballot(bad_cat), anyzero = __ballot(zero_norm);
        if (lane == 0) {
            if (anybad) sweep_report(args.hst, ST_BAD_CATEGORY);
            if (anyzero) sweep_report(args.hst, ST_ZERO_NORM);
        }
        for (int k = lane; k < K; k += 64) out[k] = anybad ? nan("") : acc[k];
    }
}

// E[w][k] = F_w(e_k) with the arithmetic that writes the keys (k_env_key_sets: cdf_lean, + 0.0, running maximum); e_K = +inf: F_w(inf).
__global__ void k_radial_bounds(const DevConfig* __restrict__ cfgp, RadialEdges ed, double* __restrict__ bounds) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= cfgp->n_wf) return;
    const WfEntry wf = cfgp->wf[w];
    const double* __restrict__ prm = cfgp->wf_params + wf.offset;
    const double winv = cfgp->wf_inv[w], finf = cfgp->wf_finf[w];
    uint64_t run = 0;
    for (int k = 0; k < ed.n; ++k) {
        const double e = ed.e[k];
        const uint64_t f = d2u(e == (double)INFINITY ? finf : cdf_lean(wf.kind, prm, wf.n_params, winv, e) + 0.0);
        run = (k && run > f) ? run : f;
        bounds[(int64_t)w * ed.n + k] = u2d(run);
    }
}

void launch_radial_bounds(hipStream_t s, const DevConfig* cfg, int n_wf, const RadialEdges& edges, double* bounds) {
    k_radial_bounds<<<(n_wf + 63) / 64, 64, 0, s>>>(cfg, edges, bounds);
}

// (not launch_most_waves' rule: the width follows the category type and count, 4 x (9 KB + 260 bytes per category) fit below 65 categories)
template <bool H2U, bool CAT16, bool TAB, int WPB>
static void launch_radial_k(hipStream_t s, const RadialArgs& a) {
    const size_t wb = column_wave_bytes(a.n_categories, kRadFront);
    const int64_t blocks = (a.sw.n_pairs + WPB - 1) / WPB;
    k_radial<H2U, CAT16, TAB, WPB><<<(unsigned)(blocks < 8192 ? blocks : 8192), 64 * WPB, wb * WPB, s>>>(a, (int)wb);
}
template <bool H2U, bool TAB>
static void launch_radial_t(hipStream_t s, const RadialArgs& a) {
    if (a.sw.env_a.cat16) launch_radial_k<H2U, true, TAB, 1>(s, a);
    else if (a.n_categories <= 64) launch_radial_k<H2U, false, TAB, 4>(s, a);
    else launch_radial_k<H2U, false, TAB, 1>(s, a);
}
bool launch_radial(hipStream_t s, bool hellinger2_unit, const RadialArgs& a) {
    if (a.sw.n_pairs <= 0) return true;
    if (a.n_categories > kWideCategories || a.n_bins < 1 || a.n_bins > kRadialMaxBins) return false;
    if (a.sw.env_a.cat16 != a.sw.env_b.cat16 || a.sw.env_a.cdf_keys < 1 || a.sw.env_a.cdf_keys != a.sw.env_b.cdf_keys) return false;
    const bool tab = a.sw.env_a.stride <= kSqrtTab && a.sw.env_b.stride <= kSqrtTab;
    if (!hellinger2_unit) launch_radial_t<false, false>(s, a);
    else if (tab) launch_radial_t<true, true>(s, a);
    else launch_radial_t<true, false>(s, a);
    return true;
}

template <bool H2U, bool TAB>
static void raise_radial_lds() {
    raise_dynamic_lds({kernel_ptr(&k_radial<H2U, true, TAB, 1>), kernel_ptr(&k_radial<H2U, false, TAB, 4>), kernel_ptr(&k_radial<H2U, false, TAB, 1>)},
                      kColumnDynMax);
}
void init_radial_kernels() {
    raise_radial_lds<false, false>();
    raise_radial_lds<true, true>();
    raise_radial_lds<true, false>();
    (void)hipGetLastError();
}

}  // namespace lchd
