// lchd_radial_bins.h -- the interval-splitting arithmetic of the radial score profiles (lchd_radial.hip), written once for host and
// device.  No HIP header, compilable alone (tests/test_radial_host.py builds it with the host compiler).
//
// A radial profile resolves a pair's LoCoHD integrand over distance bins.  Everything happens in KEY space: the breakpoints are the F
// values the environment store holds, the bin bounds are E_0 <= E_1 <= ... <= E_K with E_k = F(e_k) from the same CDF routine.  Between
// two consecutive breakpoints f_lo <= f_hi the statistical distance H is constant, and the interval adds
//   H * max(0, min(f_hi, E_{k+1}) - max(f_lo, E_k))     to bin k.
// The intervals of a sweep come in ascending order, so a caller keeps ONE running bin index and the walk below only ever moves it up: an
// interval costs one step per bound it crosses, not a loop over the K bins.
#pragma once

#if defined(__HIPCC__)
#define LCHD_RB_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define LCHD_RB_HD inline
#endif

namespace lchd {

constexpr int kRadialMaxBins = 64;  // bins of one call (lchd_radial_validate: at most kRadialMaxBins + 1 edges)

// The bin an interval that starts at key f begins in: the largest k in [0, K - 1] with E[k] <= f, 0 for a key below E[0].
LCHD_RB_HD int radial_bin_of(const double* E, int K, double f) {
    int lo = 0, hi = K - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (E[mid] <= f) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The additions of one interval [f_lo, f_hi] of constant distance H: emit(k, v) for every bin k the interval overlaps, k ascending.
// E: K + 1 non-decreasing bounds.  bin: the running index, in [0, K - 1] and not above radial_bin_of(E, K, f_lo); left at the bin the
// interval ends in.  What lies below E[0] or above E[K] is dropped; an interval that ends exactly on a bound stays in the bin below it
// (the bound's own bin would receive a zero); a bin of zero width (E[k] == E[k + 1]) receives zeros only.
template <class Emit>
LCHD_RB_HD void radial_split(double f_lo, double f_hi, double H, const double* E, int K, int& bin, Emit&& emit) {
    double lo = f_lo > E[0] ? f_lo : E[0];
    const double hi = f_hi < E[K] ? f_hi : E[K];
    if (!(hi > lo)) return;
    while (bin + 1 < K && lo >= E[bin + 1]) ++bin;  // bins that end at or below the interval's start
    while (bin + 1 < K && hi > E[bin + 1]) {
        emit(bin, H * (E[bin + 1] - lo));
        lo = E[bin + 1];
        ++bin;
    }
    emit(bin, H * (hi - lo));
}

}  // namespace lchd
