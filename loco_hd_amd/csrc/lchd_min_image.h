// lchd_min_image.h -- device only: the minimum-image arithmetic of the dense periodic calls, shared by the row producer
// (k_min_image_rows, lchd_ensemble.hip) and the displacement kernel of the dense sensitivity call (k_sens_min_image_disp,
// lchd_sensitivity.hip).  The arithmetic is part of the contract in include/loco_hd_hip.h ("minimum-image dense rows"): plain f64, IEEE
// division, rint = round to nearest even, every sum left to right, nothing fused (the build has -ffp-contract=off).
// Every function comes in two forms: the distance (what a row stores) and the chosen vector w (what a gradient needs), with
// sqrt((wx wx + wy wy) + wz wz) of the chosen vector equal to the distance bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace lchd {

// A diagonal cell: per axis d - L rint(d / L).
__device__ __forceinline__ void min_image_box_vec(double dx, double dy, double dz, double lx, double ly, double lz, double (&w)[3]) {
    w[0] = dx - lx * rint(dx / lx);
    w[1] = dy - ly * rint(dy / ly);
    w[2] = dz - lz * rint(dz / lz);
}
__device__ __forceinline__ double min_image_box(double dx, double dy, double dz, double lx, double ly, double lz) {
    double w[3];
    min_image_box_vec(dx, dy, dz, lx, ly, lz, w);
    return sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
}
// Any other cell, R = the Minkowski-reduced vectors (rows), I = their inverse: fractional coordinates wrapped to [-1/2, 1/2], back to
// Cartesian, then the 27 neighbours v + (i a + j b) + k c (i outermost, k innermost; for a reduced cell no other lattice translate is
// nearer, lchd_cell_reduce.h).  f(wx, wy, wz, d2) sees every candidate in that order.
template <class F>
__device__ __forceinline__ void min_image_cell_candidates(double dx, double dy, double dz, const double (&R)[9], const double (&I)[9], F&& f) {
    double f0 = (dx * I[0] + dy * I[3]) + dz * I[6];
    double f1 = (dx * I[1] + dy * I[4]) + dz * I[7];
    double f2 = (dx * I[2] + dy * I[5]) + dz * I[8];
    f0 = f0 - rint(f0);
    f1 = f1 - rint(f1);
    f2 = f2 - rint(f2);
    const double vx = (f0 * R[0] + f1 * R[3]) + f2 * R[6];
    const double vy = (f0 * R[1] + f1 * R[4]) + f2 * R[7];
    const double vz = (f0 * R[2] + f1 * R[5]) + f2 * R[8];
#pragma unroll
    for (int i = -1; i <= 1; ++i)
#pragma unroll
        for (int j = -1; j <= 1; ++j)
#pragma unroll
            for (int k = -1; k <= 1; ++k) {
                const double wx = vx + (((double)i * R[0] + (double)j * R[3]) + (double)k * R[6]);
                const double wy = vy + (((double)i * R[1] + (double)j * R[4]) + (double)k * R[7]);
                const double wz = vz + (((double)i * R[2] + (double)j * R[5]) + (double)k * R[8]);
                f(wx, wy, wz, (wx * wx + wy * wy) + wz * wz);
            }
}
// the distance to the shortest of them
__device__ __forceinline__ double min_image_cell(double dx, double dy, double dz, const double (&R)[9], const double (&I)[9]) {
    double best = __builtin_inf();
    min_image_cell_candidates(dx, dy, dz, R, I, [&](double, double, double, double d2) { best = fmin(best, d2); });
    return sqrt(best);
}
// the shortest of them: the first candidate with the smallest d2 (an update on strict < only); w stays 0 if no candidate compares
__device__ __forceinline__ void min_image_cell_vec(double dx, double dy, double dz, const double (&R)[9], const double (&I)[9], double (&w)[3]) {
    double best = __builtin_inf();
    w[0] = w[1] = w[2] = 0.0;
    min_image_cell_candidates(dx, dy, dz, R, I, [&](double wx, double wy, double wz, double d2) {
        if (d2 < best) { best = d2; w[0] = wx; w[1] = wy; w[2] = wz; }
    });
}

}  // namespace lchd
