// lchd_cell_reduce.h -- host only, no device: the cell of the dense minimum-image calls (lchd_cell_reduce, include/loco_hd_hip.h).
//
// The row producers of lchd_ensemble.hip find the nearest periodic image of a displacement among the 27 shifts {-1, 0, 1}^3 of its
// wrapped form.  That is all there is only for a Minkowski-reduced basis (every vector is no longer than itself plus any {-1, 0, 1}
// combination of the other two), so a cell is reduced here first.  The lattice does not change: the reduced vectors are an integer
// combination T . cell with det T = +-1, found in integers and evaluated ONCE from the caller's cell, so the rounding of a reduced
// vector is that of one three-term sum whatever the number of steps.  Every sum runs left to right, nothing is fused
// (-ffp-contract=off, Makefile): a caller can compute the very same numbers.
#pragma once
#include <cmath>
#include <cstdint>

namespace lchd {

constexpr int kMinImageRecord = 19;  // doubles per cell of the row producers: reduced cell (9, row 0 = a), its inverse (9), 1.0 if diagonal else 0.0

inline double cell_norm2(const double* v) { return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]; }
// row r of T . cell: out[d] = (T[0] a[d] + T[1] b[d]) + T[2] c[d]
inline void cell_combine_row(const int64_t* t, const double* cell, double* out) {
    for (int d = 0; d < 3; ++d) out[d] = ((double)t[0] * cell[d] + (double)t[1] * cell[3 + d]) + (double)t[2] * cell[6 + d];
}
inline bool cell_is_diagonal(const double* cell) {
    return cell[1] == 0.0 && cell[2] == 0.0 && cell[3] == 0.0 && cell[5] == 0.0 && cell[6] == 0.0 && cell[7] == 0.0;
}
// inverse[3 d + k] = (cross product of the other two vectors, cyclic)[d] / det: the arithmetic of lchd_cell_validate.  False for a cell
// that rule calls singular.
inline bool cell_inverse(const double* cell, double* inverse) {
    const double *a = cell, *b = cell + 3, *c = cell + 6;
    auto cross = [](const double* u, const double* v, double* o) {
        o[0] = u[1] * v[2] - u[2] * v[1]; o[1] = u[2] * v[0] - u[0] * v[2]; o[2] = u[0] * v[1] - u[1] * v[0];
    };
    auto norm = [](const double* u) { return std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]); };
    double x[3][3];
    cross(b, c, x[0]); cross(c, a, x[1]); cross(a, b, x[2]);
    const double det = a[0] * x[0][0] + a[1] * x[0][1] + a[2] * x[0][2];
    if (!(std::fabs(det) > 0.0) || !std::isfinite(det) || std::fabs(det) < 1e-12 * (norm(a) * norm(b) * norm(c))) return false;
    for (int d = 0; d < 3; ++d)
        for (int k = 0; k < 3; ++k) inverse[3 * d + k] = x[k][d] / det;
    return true;
}

// 0: done; 1: a non-finite entry; 2: singular.  A diagonal cell comes back as it is, with the inverse diag(1 / L).
// Reduction: as long as some vector v_k gets strictly shorter (in the norm cell_norm2 computes) by adding i v_p + j v_q of the other
// two -- i, j from {-1, 0, 1} and the rounded projection coefficients -rint(v_k . v_p / v_p . v_p), -rint(v_k . v_q / v_q . v_q), the
// shortest candidate wins, the first one among equals (i outer, ascending in the order -1, 0, 1, projection) -- replace it; k = 0, 1, 2
// in turn, starting over after every replacement.  Every candidate is evaluated from its integer row and the caller's cell, so a
// replacement strictly lowers a function of T: the loop ends.
inline int cell_reduce(const double* cell, double* reduced, double* inverse) {
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(cell[k])) return 1;
    if (!cell_inverse(cell, inverse)) return 2;
    if (cell_is_diagonal(cell)) {
        for (int k = 0; k < 9; ++k) { reduced[k] = cell[k]; inverse[k] = 0.0; }
        for (int k = 0; k < 3; ++k) inverse[4 * k] = 1.0 / cell[4 * k];
        return 0;
    }
    int64_t T[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int k = 0; k < 9; ++k) reduced[k] = cell[k];
    for (int step = 0; step < 4096; ++step) {
        bool changed = false;
        for (int k = 0; k < 3 && !changed; ++k) {
            const int p = (k + 1) % 3, q = (k + 2) % 3;
            const double *vk = reduced + 3 * k, *vp = reduced + 3 * p, *vq = reduced + 3 * q;
            const double mp = -std::rint(((vk[0] * vp[0] + vk[1] * vp[1]) + vk[2] * vp[2]) / cell_norm2(vp));
            const double mq = -std::rint(((vk[0] * vq[0] + vk[1] * vq[1]) + vk[2] * vq[2]) / cell_norm2(vq));
            if (!(std::fabs(mp) < 9.0e15) || !(std::fabs(mq) < 9.0e15)) return 2;
            const int64_t ci[4] = {-1, 0, 1, (int64_t)mp}, cj[4] = {-1, 0, 1, (int64_t)mq};
            double best = cell_norm2(vk);
            int64_t best_row[3] = {T[k][0], T[k][1], T[k][2]};
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) {
                    int64_t row[3];
                    for (int d = 0; d < 3; ++d) row[d] = T[k][d] + ci[i] * T[p][d] + cj[j] * T[q][d];
                    double w[3];
                    cell_combine_row(row, cell, w);
                    const double n2 = cell_norm2(w);
                    if (n2 < best) { best = n2; best_row[0] = row[0]; best_row[1] = row[1]; best_row[2] = row[2]; changed = true; }
                }
            if (changed) {
                for (int d = 0; d < 3; ++d) T[k][d] = best_row[d];
                cell_combine_row(T[k], cell, reduced + 3 * k);
            }
        }
        if (!changed) break;
    }
    return cell_inverse(reduced, inverse) ? 0 : 2;
}

}  // namespace lchd
