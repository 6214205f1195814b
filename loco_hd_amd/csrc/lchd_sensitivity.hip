// lchd_sensitivity.hip -- neighbour sensitivities of a pair's score (additive, not in the reference): the derivative of the score with
// respect to the distance of every member of the pair's two environments.
//
//   S = sum_j (F(u_{j+1}) - F(u_j)) * H_j                    (merged breakpoints u_j, H_j the statistical distance on piece j)
//   g = dS/dd = w(d) * (H- - H+)                             (w = F', H- / H+ the distance on the piece that ends / starts at the point)
//
// Moving a member moves one breakpoint: the piece in front of it grows by w(d) dd, the piece behind it shrinks by as much.  Members
// entering or leaving at the threshold are ignored (exact when the weight function's support ends at or inside the threshold), and at
// ties the derivative is one-sided: tied events are treated one at a time in list order.
//
// The environment stores of the scoring passes hold keys and categories only, so a sorted slot cannot be traced back to an atom.  This
// translation unit therefore builds its own lists and sweeps them:
//   k_atom_of_pos   the inverse of the prologue's atom -> cell-order position map
//   k_env_indexed   one INDEXED environment list per de-duplicated anchor: (distance f64, atom index u32, category u8) per accepted
//                   point, sorted ascending by (distance bits, atom index) with the anchor first -- one defined order among ties,
//                   whatever order the appends took.  Same cell walk, distance expression, threshold comparison and tag rule as
//                   k_env_cells (env_dist2 / env_accepts below are those lines; tag_pair_accepted and cell_coord are lchd_kcommon.h's).
//   k_rows_indexed  the same lists for DENSE rows (from_coords / from_dmxs): every column of row r a member, sorted by (distance bits,
//                   column index) with no forced anchor; a dense row has no threshold, so dS/dd is the whole derivative away from ties
//   k_sensitivity   the column-tile skeleton of lchd_pair_columns.h (LDS, tile split, histogram scan; the keys are the distance bits,
//                   A first on ties) around an event loop and a pair head of its own: the lengths come from the lists, the anchors'
//                   categories from their first slots.  Per event it evaluates H on the counts behind the event
//                   (sd_eval on the weighted, normalised counts: every statistical distance), has H in front of it from the previous
//                   event -- a lane's first event takes it from the previous lane, lane 0 from the previous tile, carried like F --
//                   and writes g to the event's slot of the pair's row of side A or B.  The same walk sums dF * H: the call returns
//                   the scores without a second pass.  No floating-point atomics: every output element has one writer, and the
//                   score is one wave reduction in lane order.
//   k_sens_resolve_images   behind the two above when a list indexes a periodic image cloud: per member slot the displacement from the
//                   anchor, the image code, and the source atom in place of the cloud index (see the kernel)
//   k_sens_min_image_disp   behind k_rows_indexed + k_sensitivity on dense rows from coordinates: per member slot the displacement from
//                   the row's atom to the member's nearest periodic image, the vector behind the minimum-image distance (see the kernel)
#include "lchd_min_image.h"
#include "lchd_pair_columns.h"

namespace lchd {

constexpr int kIdxLdsPoints = 2048;       // k_env_indexed sorts lists of at most this many (padded) points in LDS, longer ones in place

// ---- indexed environment lists -------------------------------------------------------------------------------------------------------
__global__ void k_atom_of_pos(const uint32_t* __restrict__ pos_a, int32_t n_a, uint32_t* __restrict__ inv_a, const uint32_t* __restrict__ pos_b,
                              int32_t n_b, uint32_t* __restrict__ inv_b) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_a) { const uint32_t p = pos_a[i]; if (p < (uint32_t)n_a) inv_a[p] = (uint32_t)i; }
    else if (i - n_a < n_b) { const uint32_t p = pos_b[i - n_a]; if (p < (uint32_t)n_b) inv_b[p] = (uint32_t)(i - n_a); }
}

// k_env_cells' distance (utils.rs:1-8 order; the TU is built with -ffp-contract=off) and acceptance test (:521, :524-528)
__device__ __forceinline__ double env_dist2(const CellRec& r, double ax, double ay, double az) {
    const double dx = r.x - ax, dy = r.y - ay, dz = r.z - az;
    double d2 = dx * dx;
    d2 = d2 + dy * dy;
    d2 = d2 + dz * dz;
    return d2;
}
template <bool TAGLIST>
__device__ __forceinline__ bool env_accepts(const DevConfig& cfg, double d2, double thr2, bool is_anchor, int32_t atag, int32_t tag) {
    if (!(d2 < thr2)) return false;
    if constexpr (TAGLIST) return is_anchor || tag_pair_accepted(cfg, atag, tag);
    else return is_anchor || ((atag == tag) == (cfg.tag_accept_same != 0));
}

// bitonic sort of n2 (a power of two) triples by (key, sec); pads carry (kPadKey, ~0u)
template <int NT>
__device__ __forceinline__ void bitonic_sort_indexed(uint64_t* key, uint32_t* sec, uint8_t* cat, int n2, int tid) {
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += NT) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const bool up = ((i & k) == 0);
                const uint64_t a = key[i], b = key[l];
                const uint32_t sa = sec[i], sb = sec[l];
                const bool a_gt = a > b || (a == b && sa > sb), a_lt = a < b || (a == b && sa < sb);
                if (up ? a_gt : a_lt) {
                    key[i] = b; key[l] = a;
                    sec[i] = sb; sec[l] = sa;
                    const uint8_t ca = cat[i];
                    cat[i] = cat[l];
                    cat[l] = ca;
                }
            }
            __syncthreads();
        }
    }
}

// One 256-thread workgroup per de-duplicated anchor; workgroups [0, s[0].max_envs) build side A, the rest side B.
template <bool TAGLIST>
__global__ __launch_bounds__(256) void k_env_indexed(IndexedArgs ia) {
    constexpr int NT = 256;
    __shared__ uint64_t l_key[kIdxLdsPoints];
    __shared__ uint32_t l_sec[kIdxLdsPoints];
    __shared__ uint8_t l_cat[kIdxLdsPoints];
    __shared__ int count_s;
    const int side = (int64_t)blockIdx.x >= ia.s[0].max_envs ? 1 : 0;
    const IndexedSide& S = ia.s[side];
    const int64_t e = (int64_t)blockIdx.x - (side ? ia.s[0].max_envs : 0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (e >= (int64_t)ia.st->n_unique[side] || e >= S.max_envs) return;
    const DevConfig cfg = *ia.cfg;
    const GridView g = S.g;
    const AnchorRec arec = S.uniq[e];
    const double ax = arec.x, ay = arec.y, az = arec.z, thr2 = ia.thr * ia.thr;
    const int32_t atag = (int32_t)arec.tag;
    const int cap = (int)S.env.stride, reach = ia.reach;
    uint64_t* const gk = reinterpret_cast<uint64_t*>(S.env.dist) + e * S.env.stride;
    uint32_t* const gi = S.env.idx + e * S.env.stride;
    uint8_t* const gc = S.env.cat + e * S.env.stride;
    const int cx = cell_coord(ax, g.min[0], g.inv[0], g.dim[0]);
    const int cy = cell_coord(ay, g.min[1], g.inv[1], g.dim[1]);
    const int cz = cell_coord(az, g.min[2], g.inv[2], g.dim[2]);
    const int x0 = max(cx - reach, 0), x1 = min(cx + reach, g.dim[0] - 1);
    if (tid == 0) count_s = 0;
    __syncthreads();
    for (int zz = max(cz - reach, 0); zz <= min(cz + reach, g.dim[2] - 1); ++zz)
        for (int yy = max(cy - reach, 0); yy <= min(cy + reach, g.dim[1] - 1); ++yy) {
            // the x-neighbour cells of one (y, z) row are contiguous in the cell-ordered records
            const int row = (int)((((int64_t)arec.sid * g.dim[2] + zz) * g.dim[1] + yy) * g.dim[0]);
            const int beg = (int)g.cell_start[row + x0], end = (int)g.cell_start[row + x1 + 1];
            for (int base = beg + wave * 64; base < end; base += NT) {
                const int idx = base + lane;
                bool ok = false;
                double d2 = 0.0;
                uint32_t ccat = 0;
                if (idx < end) {
                    const CellRec r = g.rec[idx];
                    d2 = env_dist2(r, ax, ay, az);
                    ccat = r.cat;
                    ok = env_accepts<TAGLIST>(cfg, d2, thr2, (uint32_t)idx == arec.apos, atag, (int32_t)r.tag);
                }
                const unsigned long long m = __ballot(ok);
                int wbase = 0;
                if (lane == 0 && m) wbase = atomicAdd(&count_s, __popcll(m));
                wbase = __shfl(wbase, 0);
                if (ok) {
                    const int pos = wbase + __popcll(m & ((1ull << lane) - 1ull));
                    if (pos < cap) {
                        gk[pos] = d2u(sqrt(d2));
                        gi[pos] = (uint32_t)idx == arec.apos ? 0u : S.atom_of[idx] + 1u;  // the anchor sorts in front of every other point at distance 0
                        gc[pos] = (uint8_t)(ccat > 255u ? 255u : ccat);
                    }
                }
            }
        }
    __syncthreads();
    const int count = count_s;
    if (count > cap || count == 0) {
        // Does not fit its slot: the scoring store of this pass flagged the same environment (the host repeats the pass with larger
        // slots); the slot receives the anchor alone, a valid one-point list.  An empty list (non-finite coordinates) stays empty.
        if (tid == 0) {
            S.env.len[e] = count ? 1 : 0;
            gk[0] = 0ull;
            gi[0] = arec.atom;
            const uint32_t acat = g.rec[arec.apos].cat;
            gc[0] = (uint8_t)(acat > 255u ? 255u : acat);
        }
        return;
    }
    const int n2 = next_pow2(count);  // <= cap: the launcher takes power-of-two strides only
    if (n2 <= kIdxLdsPoints) {
        for (int i = tid; i < n2; i += NT) {
            const bool in = i < count;
            l_key[i] = in ? gk[i] : kPadKey;
            l_sec[i] = in ? gi[i] : ~0u;
            l_cat[i] = in ? gc[i] : (uint8_t)0;
        }
        __syncthreads();
        bitonic_sort_indexed<NT>(l_key, l_sec, l_cat, n2, tid);
        for (int i = tid; i < count; i += NT) {
            gk[i] = l_key[i];
            gi[i] = l_sec[i] ? l_sec[i] - 1u : arec.atom;
            gc[i] = l_cat[i];
        }
    } else {
        for (int i = count + tid; i < n2; i += NT) { gk[i] = kPadKey; gi[i] = ~0u; gc[i] = 0; }
        __syncthreads();
        bitonic_sort_indexed<NT>(gk, gi, gc, n2, tid);
        for (int i = tid; i < count; i += NT) gi[i] = gi[i] ? gi[i] - 1u : arec.atom;
    }
    if (tid == 0) S.env.len[e] = count;
}

bool launch_env_indexed(hipStream_t s, const IndexedArgs& a) {
    const int64_t blocks = a.s[0].max_envs + a.s[1].max_envs;
    if (blocks <= 0) return true;
    for (int k = 0; k < 2; ++k) {
        const int64_t st = a.s[k].env.stride;
        if (a.s[k].max_envs > 0 && (st < 1 || st > kRadialMaxPoints + 1 || (st & (st - 1)))) return false;
    }
    if (blocks > 0x7FFFFFFF || a.reach < 1) return false;
    const int64_t n = (int64_t)a.s[0].n + (a.s[1].max_envs > 0 ? (int64_t)a.s[1].n : 0);
    k_atom_of_pos<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(a.s[0].g.pos_of, a.s[0].n, a.s[0].atom_of, a.s[1].g.pos_of,
                                                            a.s[1].max_envs > 0 ? a.s[1].n : 0, a.s[1].atom_of);
    if (a.tag_list) k_env_indexed<true><<<(unsigned)blocks, 256, 0, s>>>(a);
    else k_env_indexed<false><<<(unsigned)blocks, 256, 0, s>>>(a);
    return true;
}

// ---- indexed lists of dense rows -----------------------------------------------------------------------------------------------------
// bitonic sort of n2 (a power of two) pairs by (key, sec); pads carry (kPadKey, ~0u)
template <int NT>
__device__ __forceinline__ void bitonic_sort_pairs(uint64_t* key, uint32_t* sec, int n2, int tid) {
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += NT) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const bool up = ((i & k) == 0);
                const uint64_t a = key[i], b = key[l];
                const uint32_t sa = sec[i], sb = sec[l];
                const bool a_gt = a > b || (a == b && sa > sb), a_lt = a < b || (a == b && sa < sb);
                if (up ? a_gt : a_lt) {
                    key[i] = b; key[l] = a;
                    sec[i] = sb; sec[l] = sa;
                }
            }
            __syncthreads();
        }
    }
}

// One 256-thread workgroup per row; workgroups [0, rows) build side A, the rest side B.  Dynamic LDS (all of the kernel's: the base
// stays 16-byte aligned): keys [n2] | columns [n2] of a row sorted in LDS, nothing for a row sorted in place.
__global__ __launch_bounds__(256) void k_rows_indexed(RowsIndexedArgs ra) {
    constexpr int NT = 256;
    extern __shared__ __attribute__((aligned(16))) unsigned char rows_smem[];
    const int side = (int64_t)blockIdx.x >= ra.rows ? 1 : 0;
    const RowsIndexedSide& S = ra.s[side];
    const int64_t r = (int64_t)blockIdx.x - (side ? ra.rows : 0);
    const int tid = threadIdx.x;
    const int n = S.cols, n2 = next_pow2(n);  // n2 <= stride: the launcher takes power-of-two strides of at least cols
    const CloudView& c = S.c;
    uint64_t* const gk = reinterpret_cast<uint64_t*>(S.env.dist) + r * S.env.stride;
    uint32_t* const gi = S.env.idx + r * S.env.stride;
    uint8_t* const gc = S.env.cat + r * S.env.stride;
    const double* __restrict__ row = S.dmx ? S.dmx + r * S.ld : nullptr;
    double ax = 0.0, ay = 0.0, az = 0.0;
    if (!row) { ax = c.x[r]; ay = c.y[r]; az = c.z[r]; }
    bool bad = false, bad_c = false;
    // k_env_rows' distance: a given entry with its check (negative or NaN: reported, counted as 0; -0.0 -> +0.0), or the root of the
    // squared distance in utils.rs:1-8 order, uncontracted
    auto dist_of = [&](int i) -> double {
        if (row) {
            double v = row[i];
            if (!(v >= 0.0)) { bad = true; v = 0.0; }
            return v + 0.0;
        }
        const double dx = ax - c.x[i], dy = ay - c.y[i], dz = az - c.z[i];
        double d2 = dx * dx;
        d2 = d2 + dy * dy;
        d2 = d2 + dz * dz;
        return sqrt(d2);
    };
    const int C = ra.cfg->n_categories;
    uint64_t first;
    if (n2 <= kRowsIdxLdsPoints) {
        uint64_t* const key = reinterpret_cast<uint64_t*>(rows_smem);
        uint32_t* const sec = reinterpret_cast<uint32_t*>(rows_smem + (size_t)n2 * 8);
        for (int i = tid; i < n2; i += NT) {
            key[i] = i < n ? d2u(dist_of(i)) : kPadKey;
            sec[i] = i < n ? (uint32_t)i : ~0u;
        }
        __syncthreads();
        bitonic_sort_pairs<NT>(key, sec, n2, tid);
        for (int i = tid; i < n; i += NT) {  // (the n real pairs sort in front of every pad: a column index is below ~0u)
            const uint32_t col = sec[i];
            const uint8_t ct = c.cat[col];
            bad_c |= (int)ct >= C;
            gk[i] = key[i];
            gi[i] = col;
            gc[i] = ct;
        }
        first = key[0];
    } else {
        for (int i = tid; i < n2; i += NT) {
            gk[i] = i < n ? d2u(dist_of(i)) : kPadKey;
            gi[i] = i < n ? (uint32_t)i : ~0u;
        }
        __syncthreads();
        bitonic_sort_pairs<NT>(gk, gi, n2, tid);
        for (int i = tid; i < n; i += NT) {
            const uint8_t ct = c.cat[gi[i]];
            bad_c |= (int)ct >= C;
            gc[i] = ct;
        }
        first = gk[0];
    }
    if (tid == 0) {
        S.env.len[r] = n;
        if (first != 0ull) atomicOr(&ra.st->flags, ST_FIRST_NOT_ZERO);  // src/locohd.rs:74-77, on the distance
    }
    const unsigned long long any_bad = __ballot(bad), any_bad_c = __ballot(bad_c);
    if ((tid & 63) == 0) {
        if (any_bad) atomicOr(&ra.st->flags, ST_BAD_DISTANCE);
        if (any_bad_c) atomicOr(&ra.st->flags, ST_BAD_CATEGORY);
    }
}

bool launch_rows_indexed(hipStream_t s, const RowsIndexedArgs& a) {
    const int64_t blocks = 2 * a.rows;
    if (a.rows <= 0) return true;
    size_t lds = 0;
    for (int k = 0; k < 2; ++k) {
        const int64_t st = a.s[k].env.stride;
        const int cols = a.s[k].cols;
        if (st < 1 || st > kRadialMaxPoints + 1 || (st & (st - 1)) || cols < 1 || cols > st || cols > kRadialMaxPoints) return false;
        if (a.s[k].c.n < cols || (!a.s[k].dmx && a.s[k].c.n < a.rows)) return false;  // (a category per column, coordinates per row)
        const size_t n2 = (size_t)next_pow2_host(cols);
        if (n2 <= (size_t)kRowsIdxLdsPoints) lds = std::max(lds, n2 * 12);
    }
    if (blocks > 0x7FFFFFFF) return false;
    k_rows_indexed<<<(unsigned)blocks, 256, lds, s>>>(a);
    return true;
}

// ---- the sweep -----------------------------------------------------------------------------------------------------------------------
static __device__ __noinline__ double sens_pdf(int kind, const double* p, int np, double x) { return pdf_eval(kind, p, np, x); }

// WPB: pairs (wavefronts) per workgroup.
template <int WPB>
__global__ __launch_bounds__(64 * WPB) void k_sensitivity(SensitivityArgs sa, int wave_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sens_smem[];
    const SweepArgs& args = sa.sw;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const DevConfig* __restrict__ cfgp = args.cfg;
    const int C = cfgp->n_categories, K = sa.width;
    const double* __restrict__ cat_w = cfgp->cat_w;
    const ColumnLds l = column_carve(sens_smem + (size_t)wv * wave_bytes, C, 0);  // (nothing in front of the count columns)
    const uint64_t *const sA = l.sA, *const sB = l.sB;
    const uint16_t *const cA = l.cA, *const cB = l.cB;
    uint32_t* const cnt = l.cnt0 + lane;  // this lane's count column: cnt[c * 64]

    const int n_wf = cfgp->n_wf;
    const int sd_kind = cfgp->sd_kind;
    const double prm0 = cfgp->sd_p0, prm1 = cfgp->sd_p1;
    const int64_t pstride = (int64_t)gridDim.x * WPB;
    for (int64_t p = (int64_t)blockIdx.x * WPB + wv; p < args.n_pairs; p += pstride) {
        const int64_t row = p * (int64_t)K;
        double *const gA = sa.out.g_a + row, *const gB = sa.out.g_b + row;
        const int4 m = args.meta[p];
        const int mx = __builtin_amdgcn_readfirstlane(m.x), my = __builtin_amdgcn_readfirstlane(m.y);
        const int mz = __builtin_amdgcn_readfirstlane(m.z), mw = __builtin_amdgcn_readfirstlane(m.w);
        const bool usable = (mz & 0xFFFFFF) > 0 && (mw & 0xFFFFFF) > 0;  // (anchor out of range, overflowed or empty environment: flagged where it happened)
        const int64_t ea = mx, eb = my;
        const int nA = usable ? __builtin_amdgcn_readfirstlane(sa.env_a.len[ea]) : 0, nB = usable ? __builtin_amdgcn_readfirstlane(sa.env_b.len[eb]) : 0;
        const int wfi = __builtin_amdgcn_readfirstlane(args.wf_index ? args.wf_index[p] : 0);
        const bool bad_wf = wfi < 0 || wfi >= n_wf;
        // ... or an index outside the dictionary, or a list longer than the caller's rows (the host reports the width it takes)
        if (nA <= 0 || nB <= 0 || nA > kRadialMaxPoints || nB > kRadialMaxPoints || nA > K || nB > K || bad_wf) {
            if (bad_wf && lane == 0) sweep_report(args.hst, ST_BAD_WF);
            for (int t = lane; t < K; t += 64) {
                gA[t] = nan(""); gB[t] = nan("");
                sa.out.dist_a[row + t] = 0.0; sa.out.dist_b[row + t] = 0.0;
                sa.out.idx_a[row + t] = -1; sa.out.idx_b[row + t] = -1;
            }
            if (lane == 0) { sa.out.scores[p] = nan(""); sa.out.count_a[p] = 0; sa.out.count_b[p] = 0; }
            continue;
        }
        const uint64_t* __restrict__ kA = reinterpret_cast<const uint64_t*>(sa.env_a.dist) + ea * sa.env_a.stride;
        const uint64_t* __restrict__ kB = reinterpret_cast<const uint64_t*>(sa.env_b.dist) + eb * sa.env_b.stride;
        const uint8_t* __restrict__ tA = sa.env_a.cat + ea * sa.env_a.stride;
        const uint8_t* __restrict__ tB = sa.env_b.cat + eb * sa.env_b.stride;
        const uint32_t* __restrict__ xA = sa.env_a.idx + ea * sa.env_a.stride;
        const uint32_t* __restrict__ xB = sa.env_b.idx + eb * sa.env_b.stride;
        const WfEntry wf = cfgp->wf[wfi];
        const double* __restrict__ prm = cfgp->wf_params + wf.offset;
        const double winv = cfgp->wf_inv[wfi], Finf = cfgp->wf_finf[wfi];
        // the lists themselves, the padding, and the slots no event writes: the anchor's (0) and those behind the list
        for (int t = lane; t < K; t += 64) {
            sa.out.idx_a[row + t] = t < nA ? (int32_t)xA[t] : -1;
            sa.out.idx_b[row + t] = t < nB ? (int32_t)xB[t] : -1;
            sa.out.dist_a[row + t] = t < nA ? u2d(kA[t]) : 0.0;
            sa.out.dist_b[row + t] = t < nB ? u2d(kB[t]) : 0.0;
            if (t == 0 || t >= nA) gA[t] = 0.0;
            if (t == 0 || t >= nB) gB[t] = 0.0;
        }
        if (lane == 0) { sa.out.count_a[p] = nA; sa.out.count_b[p] = nB; }

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

        // the two anchors (src/locohd.rs:82-84) in the carry row and in every lane's column
        wave_sync_lds();
        column_seed_anchors(l, cnt, C, c0a, c0b, lane);
        wave_sync_lds();
        double F_carry = cdf_lean(wf.kind, prm, wf.n_params, winv, 0.0) + 0.0;  // F(0): both anchors sit at distance 0
        double H_carry = bad_cat ? 0.0 : distance();
        double score = 0.0;  // this lane's part of sum dF * H

        const int mA = nA - 1, mB = nB - 1, M = mA + mB;  // non-anchor events
        int ia = 0, ib = 0;
        for (int k0 = 0; k0 < M; k0 += kSweepTile) {
            const ColumnTile t = column_tile_stage(l, kA, kB, tA, tB, mA, mB, M, k0, ia, ib, lane);
            const int T = t.T, d0 = t.d0, d1 = t.d1, i0 = t.i0, i1 = t.i1, j0 = t.j0, j1 = t.j1, iend = t.iend, last = t.last;
            const bool has = t.has;
            if (column_histogram_scan(l, cnt, t, C, lane, [](uint32_t) {})) bad_cat = true;

            // pass 2: this lane's events, one after the other
            int i = i0, j = j0;
            uint64_t ka = (i < i1) ? sA[i] : kPadKey, kb = (j < j1) ? sB[j] : kPadKey;
            const double firstF = has ? cdf_lean(wf.kind, prm, wf.n_params, winv, u2d(ka <= kb ? ka : kb)) + 0.0 : 0.0;
            const double nextF = shfl_f64(firstF, min(lane + 1, 63));  // F at the first event of the next lane's chunk
            double Fp = F_carry, Hp = 0.0;
            bool open = lane == 0;  // lane 0 closes the interval the previous tile (or the anchors) left open, on H_carry
            // the lane's first event: H in front of it is the previous lane's (lane 0: the previous tile's) last value -- written after the walk
            double* first_out = nullptr;
            double first_w = 0.0, first_H = 0.0;
            for (int e = d0; e < d1; ++e) {
                const bool takeA = (ka <= kb);  // an exhausted run shows the pad key (> every real key); A first on ties
                const uint64_t key = takeA ? ka : kb;
                const int ct = takeA ? cA[i] : cB[j];
                double* const slot = takeA ? gA + (1 + ia + i) : gB + (1 + ib + j);
                if (takeA) { ++i; ka = (i < i1) ? sA[i] : kPadKey; } else { ++j; kb = (j < j1) ? sB[j] : kPadKey; }
                const double d = u2d(key);
                double F = cdf_lean(wf.kind, prm, wf.n_params, winv, d) + 0.0;
                F = F < Fp ? Fp : F;  // (F is monotone; its floating-point evaluation may invert the last bit between neighbours)
                if (open && !bad_cat) score += (F - Fp) * (e == d0 ? H_carry : Hp);
                // pmf.rs:47-63: one more point of category ct on one side
                if (ct < C) cnt[ct * 64] += takeA ? kOneA : kOneB;
                else bad_cat = true;
                const double Hn = bad_cat ? 0.0 : distance();
                const double w = sens_pdf(wf.kind, prm, wf.n_params, d);
                if (e == d0) { first_out = slot; first_w = w; first_H = Hn; }
                else *slot = w * (Hp - Hn);
                open = true;
                Hp = Hn;
                Fp = F;
            }
            if (has && lane < last && !bad_cat) score += ((nextF < Fp ? Fp : nextF) - Fp) * Hp;
            double Hprev = shfl_up_f64(Hp, 1);  // (lanes 1 .. last: lane - 1 has events)
            if (lane == 0) Hprev = H_carry;
            if (first_out) *first_out = first_w * (Hprev - first_H);
            F_carry = readlane_f64(Fp, last);
            H_carry = readlane_f64(Hp, last);
            ia += iend;
            ib += T - iend;
        }
        // the last interval to +inf (:165-171,204-210,212-221) on the counts of the whole pair
        const unsigned long long anybad = __ballot(bad_cat), anyzero = __ballot(zero_norm);
        if (lane == 0 && Finf > F_carry) score += (Finf - F_carry) * H_carry;
        const double total = wave_sum_f64(score);
        if (lane == 0) {
            if (anybad) sweep_report(args.hst, ST_BAD_CATEGORY);
            if (anyzero) sweep_report(args.hst, ST_ZERO_NORM);
            sa.out.scores[p] = (anybad || anyzero) ? nan("") : total;
        }
        if (anybad || anyzero) {  // the rows of an unusable pair are NaN, as its score is (the event stores above have landed first)
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
            for (int t = lane; t < K; t += 64) { gA[t] = nan(""); gB[t] = nan(""); }
        }
    }
}

bool launch_sensitivity(hipStream_t s, const SensitivityArgs& a) {
    if (a.sw.n_pairs <= 0) return true;
    if (a.n_categories < 1 || a.n_categories > kSensitivityMaxCategories || a.width < 1) return false;
    const size_t wb = column_wave_bytes(a.n_categories, 0);
    return launch_most_waves(kColumnDynMax, wb, a.sw.n_pairs, [&](auto wpb, unsigned grid) {
        constexpr int WPB = decltype(wpb)::value;
        k_sensitivity<WPB><<<grid, 64 * WPB, wb * WPB, s>>>(a, (int)wb);
    });
}

// ---- lists that index image clouds ---------------------------------------------------------------------------------------------------
// Behind k_env_indexed + k_sensitivity on an image cloud a slot names a position of that cloud: a wrapped original or a ghost.  This
// kernel turns the [P][K] slots of both sides (blockIdx.y) into what a caller can use, in place:
//   disp   x_img[member] - x_img[anchor] per axis: the three subtractions env_dist2 made (same operands, uncontracted), so
//          dist = sqrt(disp . disp) in its order; 0 in slot 0 and in the padding
//   image  the member's image code (0: a home atom, the padding, a side that is no image cloud)
//   idx    the member's source atom (unchanged for a side that is no image cloud; the padding stays -1)
// The list order stays the one k_env_indexed gave: ascending by (distance bits, image-cloud index).  The wrapped originals come first in
// an image cloud and the ghosts follow in (source atom, image code) order, so among exact ties: home atoms before ghosts, then the
// source index, then the image code.
// Lane-to-slot mapping: idx is rewritten in place, so the lane that reads a slot must be the one that writes it -- a lane owns whole
// slots.  Four consecutive slots of the flat [P * K] range per lane make every stream a full 16-byte access where the arrays are
// 16-byte aligned (VEC): one 16-byte load and store of idx, six 16-byte stores of its 96 contiguous bytes of disp, one 4-byte store of
// image; consecutive lanes continue where the last ended, so a wavefront covers 1 KiB of idx and 6 KiB of disp without a gap.  The
// coordinate reads are gathers by nature (member and anchor positions).  Every output element has one writer; no atomics.
template <bool VEC>
__global__ __launch_bounds__(256) void k_sens_resolve_images(SensResolveArgs ra) {
    const int side = blockIdx.y;
    const SensResolveSide& S = ra.s[side];
    const int64_t K = ra.width, slots = ra.n_pairs * K;
    const int64_t s0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (s0 >= slots) return;
    const int m = (int)(slots - s0 < 4 ? slots - s0 : 4);
    const bool wide = VEC && m == 4;
    int32_t id[4] = {-1, -1, -1, -1};
    if (wide) {
        const int4 v = *reinterpret_cast<const int4*>(S.idx + s0);
        id[0] = v.x; id[1] = v.y; id[2] = v.z; id[3] = v.w;
    } else {
        for (int q = 0; q < m; ++q) id[q] = S.idx[s0 + q];
    }
    int8_t im[4] = {0, 0, 0, 0};
    double d[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int64_t p = s0 / K, k = s0 - p * K;
    bool fresh = true, anchored = false;
    double ax = 0.0, ay = 0.0, az = 0.0;
    for (int q = 0; q < m; ++q, ++k) {
        if (k == K) { k = 0; ++p; fresh = true; }
        if (fresh) {  // (an anchor below the source's size sits at its own index in the image cloud: the wrapped original)
            const int64_t an = ra.anchors[2 * p + side];
            anchored = an >= 0 && an < S.n;
            if (anchored) { ax = S.x[an]; ay = S.y[an]; az = S.z[an]; }
            fresh = false;
        }
        const int64_t mem = id[q];
        if (mem < 0 || mem >= S.n || !anchored) continue;  // padding (or a pair the pass has flagged): idx stays, image 0, disp 0
        if (k != 0) { d[3 * q] = S.x[mem] - ax; d[3 * q + 1] = S.y[mem] - ay; d[3 * q + 2] = S.z[mem] - az; }
        if (S.origin) { im[q] = S.code[mem]; id[q] = S.origin[mem]; }
    }
    if (wide) {
        if (S.origin) *reinterpret_cast<int4*>(S.idx + s0) = make_int4(id[0], id[1], id[2], id[3]);
        *reinterpret_cast<uint32_t*>(S.image + s0) = (uint32_t)(uint8_t)im[0] | (uint32_t)(uint8_t)im[1] << 8 | (uint32_t)(uint8_t)im[2] << 16 |
                                                    (uint32_t)(uint8_t)im[3] << 24;
        double2* const out = reinterpret_cast<double2*>(S.disp + 3 * s0);
        for (int j = 0; j < 6; ++j) out[j] = make_double2(d[2 * j], d[2 * j + 1]);
    } else {
        for (int q = 0; q < m; ++q) {
            if (S.origin) S.idx[s0 + q] = id[q];
            S.image[s0 + q] = im[q];
            for (int j = 0; j < 3; ++j) S.disp[3 * (s0 + q) + j] = d[3 * q + j];
        }
    }
}

bool launch_sens_resolve(hipStream_t s, const SensResolveArgs& a) {
    if (a.n_pairs <= 0) return true;
    if (a.width < 1) return false;
    const int64_t quads = (a.n_pairs * (int64_t)a.width + 3) / 4, blocks = (quads + 255) / 256;
    if (blocks > 0x7FFFFFFF) return false;
    uintptr_t low = 0;  // 16-byte accesses where every array of both sides allows them
    for (int k = 0; k < 2; ++k)
        low |= reinterpret_cast<uintptr_t>(a.s[k].idx) | reinterpret_cast<uintptr_t>(a.s[k].disp) | (reinterpret_cast<uintptr_t>(a.s[k].image) & 3) << 2;
    const dim3 grid((unsigned)blocks, 2);
    if ((low & 15) == 0) k_sens_resolve_images<true><<<grid, 256, 0, s>>>(a);
    else k_sens_resolve_images<false><<<grid, 256, 0, s>>>(a);
    return true;
}

// ---- displacements of dense minimum-image rows ---------------------------------------------------------------------------------------
// Behind k_rows_indexed + k_sensitivity on dense rows from coordinates: a minimum-image row stores |w| alone, and the direction of a
// member is no longer x[member] - x[r] once an image was chosen.  For every slot [row r][k] of one side (one launch per side) this
// kernel writes disp[r][k][3] = -w with d = x[r] - x[member] per axis and
//   an open side      w = d
//   a diagonal cell   w_k = d_k - L_k rint(d_k / L_k)
//   any other cell    the first of the 27 candidates v + ((i a + j b) + k c) (i outermost, k innermost) with the smallest
//                     (wx wx + wy wy) + wz wz, an update on strict < only
// -- the arithmetic of the row producer (lchd_min_image.h) and, on an open side, of k_rows_indexed, so sqrt((dx dx + dy dy) + dz dz) of
// disp is dist[r][k] bit for bit (a negation is exact).  Slot 0 is computed like every other slot; the padding (idx < 0) gets 0.
// Lane-to-slot mapping and access widths are k_sens_resolve_images': four consecutive slots of the flat [rows * K] range per lane, one
// 16-byte idx load and six 16-byte disp stores where the arrays are 16-byte aligned (VEC), the scalar form otherwise (a block carved
// from a host call's output is not always aligned).  The coordinate reads are gathers; the cell is wave-uniform (a kernel argument,
// by value).  Every output element has one writer; no atomics.
// KIND (SensDispSide::kind) is a template parameter: the open and the per-axis form do not carry the registers of the 27-candidate
// search (its lattice shifts are loop-invariant f64 values, which live in VGPRs).
template <int KIND, bool VEC>
__global__ __launch_bounds__(256) void k_sens_min_image_disp(SensDispSide S, int64_t rows, int32_t width) {
    const int64_t K = width, slots = rows * K;
    const int64_t s0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (s0 >= slots) return;
    const int m = (int)(slots - s0 < 4 ? slots - s0 : 4);
    const bool wide = VEC && m == 4;
    int32_t id[4] = {-1, -1, -1, -1};
    if (wide) {
        const int4 v = *reinterpret_cast<const int4*>(S.idx + s0);
        id[0] = v.x; id[1] = v.y; id[2] = v.z; id[3] = v.w;
    } else {
        for (int q = 0; q < m; ++q) id[q] = S.idx[s0 + q];
    }
    double R[9], I[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) { R[q] = S.cell.v[q]; I[q] = S.cell.v[9 + q]; }  // (KIND 0 reads none of them, KIND 1 the diagonal of R)
    double d[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int64_t r = s0 / K, k = s0 - r * K;
    bool fresh = true;
    double ax = 0.0, ay = 0.0, az = 0.0;
    // one copy of the 27-candidate search in the code, not four: the loop stays rolled, and the slot's registers are picked by compares
#pragma unroll 1
    for (int q = 0; q < m; ++q, ++k) {
        if (k == K) { k = 0; ++r; fresh = true; }
        if (fresh) {
            if (r < S.n) { ax = S.x[r]; ay = S.y[r]; az = S.z[r]; }
            fresh = false;
        }
        const int64_t mem = q == 0 ? id[0] : (q == 1 ? id[1] : (q == 2 ? id[2] : id[3]));
        if (mem < 0 || mem >= S.n || r >= S.n) continue;  // padding (or a row the pass has flagged): disp 0
        const double dx = ax - S.x[mem], dy = ay - S.y[mem], dz = az - S.z[mem];
        double w[3] = {dx, dy, dz};
        if constexpr (KIND == 1) min_image_box_vec(dx, dy, dz, R[0], R[4], R[8], w);
        else if constexpr (KIND == 2) min_image_cell_vec(dx, dy, dz, R, I, w);
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t == q) { d[3 * t] = -w[0]; d[3 * t + 1] = -w[1]; d[3 * t + 2] = -w[2]; }
    }
    if (wide) {
        double2* const out = reinterpret_cast<double2*>(S.disp + 3 * s0);
        for (int j = 0; j < 6; ++j) out[j] = make_double2(d[2 * j], d[2 * j + 1]);
    } else {
        for (int q = 0; q < m; ++q)
            for (int j = 0; j < 3; ++j) S.disp[3 * (s0 + q) + j] = d[3 * q + j];
    }
}

bool launch_sens_min_image_disp(hipStream_t s, const SensDispArgs& a) {
    if (a.rows <= 0) return true;
    if (a.width < 1) return false;
    const int64_t quads = (a.rows * (int64_t)a.width + 3) / 4, blocks = (quads + 255) / 256;
    if (blocks > 0x7FFFFFFF) return false;
    for (int k = 0; k < 2; ++k)
        if (a.s[k].kind < 0 || a.s[k].kind > 2 || a.s[k].n < a.rows) return false;
    const unsigned grid = (unsigned)blocks;
    for (int k = 0; k < 2; ++k) {  // one launch per side: the instantiation of the side's kind, 16-byte accesses where its arrays allow them
        const SensDispSide& S = a.s[k];
        const bool vec = ((reinterpret_cast<uintptr_t>(S.idx) | reinterpret_cast<uintptr_t>(S.disp)) & 15) == 0;
        auto go = [&](auto kind) {
            constexpr int KIND = decltype(kind)::value;
            if (vec) k_sens_min_image_disp<KIND, true><<<grid, 256, 0, s>>>(S, a.rows, a.width);
            else k_sens_min_image_disp<KIND, false><<<grid, 256, 0, s>>>(S, a.rows, a.width);
        };
        if (S.kind == 0) go(std::integral_constant<int, 0>{});
        else if (S.kind == 1) go(std::integral_constant<int, 1>{});
        else go(std::integral_constant<int, 2>{});
    }
    return true;
}

void init_sensitivity_kernels() {
    raise_dynamic_lds({kernel_ptr(&k_sensitivity<4>), kernel_ptr(&k_sensitivity<2>), kernel_ptr(&k_sensitivity<1>)}, kColumnDynMax);
    raise_dynamic_lds({kernel_ptr(&k_rows_indexed)}, kRowsIdxLdsPoints * 12);
    (void)hipGetLastError();
}

}  // namespace lchd
