// lchd_ensemble.hip -- the small kernels of the dense ensemble call (lchd_ensemble_from_coords / _from_dmxs in lchd_capi.hip):
// M structures of one topology scored all-vs-all, pair (i, j) row r = from_coords(seq, seq, X[i], X[j])[r]
// (python_codes/ensembles/compare_ensembles.py:277-296 of the reference: one from_dmxs call per pair i < j).
//
// A structure's n dense rows are the same in every one of its M - 1 comparisons, so they are sorted ONCE into an environment
// store that holds the rows of a block of resident structures (slot s * n + r = row r of the structure in slot s), and every
// structure pair becomes n sweep records (slot(i) * n + r, slot(j) * n + r) over that one store.  The kernels here:
//   k_ens_dist     distance rows of a block of structures from their coordinates (utils.rs:1-8 order, uncontracted), the input
//                  of the existing row sorts (lchd_env_rows.hip, given-row form)
//   k_min_image_rows  the same rows in a periodic cell: every atom at the distance of its nearest periodic image (minimum image),
//                  in a diagonal cell (orthorhombic box) per axis, in any other cell among the 27 shifts of the wrapped displacement
//   k_ens_excl     the caller's excluded (row, column) entries set to +inf (the script's homo-residue ban, :261-263)
//   k_ens_iota     identity slot map (SweepArgs::slot_a / slot_b: a record's "anchor" IS its environment slot)
//   k_ens_records  structure-pair list -> sweep records and per-record weight-function indices, on the device
//   k_ens_scatter  the scores of a pass into their (pair, row) places of the caller's output
#include "lchd_device.h"
#include "lchd_min_image.h"

namespace lchd {

__global__ __launch_bounds__(256) void k_ens_dist(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z,
                                                  int64_t atom0, int32_t n, int64_t n_rows, double* __restrict__ dmx) {
    for (int64_t g = blockIdx.x; g < n_rows; g += gridDim.x) {
        const int64_t k = g / n, r = g - k * n;
        const int64_t base = atom0 + k * n;
        const double ax = x[base + r], ay = y[base + r], az = z[base + r];
        double* __restrict__ row = dmx + g * n;
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const double dx = ax - x[base + i], dy = ay - y[base + i], dz = az - z[base + i];
            double d2 = dx * dx;  // utils.rs:1-8 order (the build has -ffp-contract=off): the bits k_env_rows2 computes from coordinates
            d2 = d2 + dy * dy;
            d2 = d2 + dz * dz;
            row[i] = sqrt(d2);
        }
    }
}

// ---- minimum-image rows (lchd_from_coords_periodic / lchd_ensemble_from_coords_periodic; the arithmetic is part of the contract in
// include/loco_hd_hip.h: plain f64, IEEE division, rint = round to nearest even, every sum left to right, nothing fused) -----------
// min_image_box / min_image_cell: lchd_min_image.h, shared with the displacement kernel of the dense sensitivity call.

// One workgroup per row, as k_ens_dist.  The cell is wave-uniform: `one` (kernel argument) or, with per-structure cells, record
// struct0 + k of `recs`, loaded once per row through an index made of blockIdx only.  CELL = false: every cell is diagonal.
// vec2: n and atom0 are even and every array is 16-byte aligned, so a lane takes two neighbours (16-byte loads and stores).
template <bool CELL>
__global__ __launch_bounds__(256) void k_min_image_rows(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z,
                                                        int64_t atom0, int32_t n, int64_t n_rows, MinImageCell one,
                                                        const double* __restrict__ recs, int64_t struct0, int32_t vec2,
                                                        double* __restrict__ dmx) {
    for (int64_t g = blockIdx.x; g < n_rows; g += gridDim.x) {
        const int64_t k = g / n, r = g - k * n;
        const int64_t base = atom0 + k * n;
        double R[9], I[9], diag;
        if (recs) {
            const double* __restrict__ p = recs + (struct0 + k) * kMinImageRecord;
#pragma unroll
            for (int q = 0; q < 9; ++q) { R[q] = p[q]; I[q] = p[9 + q]; }
            diag = p[18];
        } else {
#pragma unroll
            for (int q = 0; q < 9; ++q) { R[q] = one.v[q]; I[q] = one.v[9 + q]; }
            diag = one.v[18];
        }
        const bool box = !CELL || diag != 0.0;
        const double ax = x[base + r], ay = y[base + r], az = z[base + r];
        auto dist = [&](double px, double py, double pz) -> double {
            const double dx = ax - px, dy = ay - py, dz = az - pz;
            if (box) return min_image_box(dx, dy, dz, R[0], R[4], R[8]);
            if constexpr (CELL) return min_image_cell(dx, dy, dz, R, I);
            return 0.0;
        };
        double* __restrict__ row = dmx + g * n;
        if (vec2) {
            for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * (int)blockDim.x) {
                const double2 px = *reinterpret_cast<const double2*>(x + base + i);
                const double2 py = *reinterpret_cast<const double2*>(y + base + i);
                const double2 pz = *reinterpret_cast<const double2*>(z + base + i);
                *reinterpret_cast<double2*>(row + i) = make_double2(dist(px.x, py.x, pz.x), dist(px.y, py.y, pz.y));
            }
        } else {
            for (int i = threadIdx.x; i < n; i += blockDim.x) row[i] = dist(x[base + i], y[base + i], z[base + i]);
        }
    }
}

__global__ __launch_bounds__(256) void k_ens_excl(const int32_t* __restrict__ excl_start, const int32_t* __restrict__ excl_idx, int32_t n,
                                                  int64_t n_rows, double* __restrict__ dmx) {
    for (int64_t g = blockIdx.x; g < n_rows; g += gridDim.x) {
        const int r = (int)(g % n);
        const int e0 = excl_start[r], e1 = excl_start[r + 1];
        for (int e = e0 + (int)threadIdx.x; e < e1; e += blockDim.x) dmx[g * n + excl_idx[e]] = __builtin_inf();
    }
}

__global__ void k_ens_iota(uint32_t* __restrict__ slot, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) slot[i] = (uint32_t)i;
}

// plan[k] = {slot of structure i, slot of structure j, output pair index, 0} for the k-th structure pair of a pass
__global__ void k_ens_records(const int4* __restrict__ plan, int64_t n_plan, int32_t n, const int32_t* __restrict__ wf, int64_t* __restrict__ anchors,
                              int32_t* __restrict__ wf_rec) {
    const int64_t total = n_plan * n;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = q / n, r = q - k * n;
        const int4 p = plan[k];
        anchors[2 * q] = (int64_t)p.x * n + r;
        anchors[2 * q + 1] = (int64_t)p.y * n + r;
        if (wf_rec) wf_rec[q] = wf[r];
    }
}

__global__ void k_ens_scatter(const double* __restrict__ scores, const int4* __restrict__ plan, int64_t n_plan, int32_t n, double* __restrict__ out) {
    const int64_t total = n_plan * n;
    for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = q / n, r = q - k * n;
        out[(int64_t)plan[k].z * n + r] = scores[q];
    }
}

static unsigned grid_for(int64_t items, int per_block, unsigned most) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b > most ? most : b));
}

void launch_ens_dist(hipStream_t s, const CloudView& c, int64_t atom0, int32_t n, int64_t n_rows, const int32_t* excl_start,
                     const int32_t* excl_idx, double* dmx) {
    if (n_rows <= 0) return;
    const unsigned grid = grid_for(n_rows, 1, 1u << 20);
    k_ens_dist<<<grid, 256, 0, s>>>(c.x, c.y, c.z, atom0, n, n_rows, dmx);
    if (excl_start) k_ens_excl<<<grid, 256, 0, s>>>(excl_start, excl_idx, n, n_rows, dmx);
}
void launch_min_image_rows(hipStream_t s, const CloudView& c, int64_t atom0, int32_t n, int64_t n_rows, const MinImageCell& one,
                           const double* d_recs, bool all_diagonal, const int32_t* excl_start, const int32_t* excl_idx, double* dmx) {
    if (n_rows <= 0) return;
    const unsigned grid = grid_for(n_rows, 1, 1u << 20);
    auto aligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    const int32_t vec2 = (n % 2 == 0 && atom0 % 2 == 0 && aligned(c.x) && aligned(c.y) && aligned(c.z) && aligned(dmx)) ? 1 : 0;
    const int64_t struct0 = atom0 / n;
    if (all_diagonal) k_min_image_rows<false><<<grid, 256, 0, s>>>(c.x, c.y, c.z, atom0, n, n_rows, one, d_recs, struct0, vec2, dmx);
    else k_min_image_rows<true><<<grid, 256, 0, s>>>(c.x, c.y, c.z, atom0, n, n_rows, one, d_recs, struct0, vec2, dmx);
    if (excl_start) k_ens_excl<<<grid, 256, 0, s>>>(excl_start, excl_idx, n, n_rows, dmx);
}
void launch_ens_iota(hipStream_t s, uint32_t* slot, int64_t n) {
    if (n > 0) k_ens_iota<<<grid_for(n, 256, 4096), 256, 0, s>>>(slot, n);
}
void launch_ens_records(hipStream_t s, const int4* plan, int64_t n_plan, int32_t n, const int32_t* wf, int64_t* anchors, int32_t* wf_rec) {
    if (n_plan > 0) k_ens_records<<<grid_for(n_plan * n, 256, 8192), 256, 0, s>>>(plan, n_plan, n, wf, anchors, wf_rec);
}
void launch_ens_scatter(hipStream_t s, const double* scores, const int4* plan, int64_t n_plan, int32_t n, double* out) {
    if (n_plan > 0) k_ens_scatter<<<grid_for(n_plan * n, 256, 8192), 256, 0, s>>>(scores, plan, n_plan, n, out);
}

}  // namespace lchd
