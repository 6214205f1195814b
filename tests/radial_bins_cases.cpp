// Stand-alone driver of loco_hd_amd/csrc/lchd_radial_bins.h for tests/test_radial_host.py: the header is compiled with the host compiler
// alone.  stdin: K, the K + 1 bounds, N, then N intervals "f_lo f_hi H" in ascending order.  The intervals are walked with ONE running bin
// index, as a lane of the kernel does; stdout: the K bin sums (hex floats), then the bin index after every interval.
#include <cstdio>
#include <vector>

#include "lchd_radial_bins.h"

int main() {
    int K = 0, N = 0;
    if (scanf("%d", &K) != 1 || K < 1 || K > lchd::kRadialMaxBins) return 2;
    std::vector<double> E(K + 1), acc(K, 0.0);
    for (double& e : E)
        if (scanf("%lf", &e) != 1) return 2;
    if (scanf("%d", &N) != 1) return 2;
    std::vector<int> bins;
    int bin = -1;
    for (int i = 0; i < N; ++i) {
        double lo, hi, h;
        if (scanf("%lf %lf %lf", &lo, &hi, &h) != 3) return 2;
        if (bin < 0) bin = lchd::radial_bin_of(E.data(), K, lo);
        int last = -1;
        bool ascending = true;
        lchd::radial_split(lo, hi, h, E.data(), K, bin, [&](int k, double v) {
            if (k < 0 || k >= K || k < last) ascending = false; else acc[k] += v;
            last = k;
        });
        if (!ascending) return 3;
        bins.push_back(bin);
    }
    for (double v : acc) printf("%a ", v);
    printf("\n");
    for (int b : bins) printf("%d ", b);
    printf("\n");
    return 0;
}
