// lchd_math.h -- the numeric leaves of the LoCoHD path, written once for host and device.
//
//   CDFs                    /root/reference/src/locohd/weight_function/cdfs.rs:5-63
//   statistical distances   /root/reference/src/locohd/pmf/statistical_distances.rs:4-78
//
// Everything is f64, like the reference.  Device code gets these through the kernels' translation
// unit (ocml exp/pow/log/sqrt), host code (lchd_wf_cdf, lchd_sd_run) through libm.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LCHD_HD __host__ __device__ __forceinline__
#else
#define LCHD_HD inline
#endif

// Loop over categories: with NMAX > 0 the loop is fully unrolled to NMAX iterations and guarded by c < n
// (register-resident state on the device); with NMAX == 0 it is a plain runtime loop (host).
// (unroll count 1 = "do not unroll": a bare `unroll` on the runtime loop draws -Wpass-failed from every instantiation with NMAX == 0)
#define LCHD_PRAGMA_(x) _Pragma(#x)
#define LCHD_FOR_C(NMAX, n, c) \
    LCHD_PRAGMA_(clang loop unroll_count((NMAX) > 0 ? (NMAX) : 1)) for (int c = 0; c < ((NMAX) > 0 ? (NMAX) : (n)); ++c) if ((NMAX) == 0 || c < (n))

namespace lchd {

enum { WF_HYPER_EXP = 0, WF_DAGUM = 1, WF_UNIFORM = 2, WF_KUMARASWAMY = 3 };
enum { SD_HELLINGER = 0, SD_KS = 1, SD_KL = 2, SD_RENYI = 3 };

// cdfs.rs:5-21: 1 - sum_i a_i exp(-b_i x) / sum_i a_i, params = (a_1..a_n, b_1..b_n)
LCHD_HD double cdf_hyper_exp(const double* p, int np, double x) {
    double norm = 0.0, sum = 0.0;
    const int n = np / 2;
    for (int i = 0; i < n; ++i) {
        sum += p[i] * exp(-p[n + i] * x);
        norm += p[i];
    }
    return 1.0 - sum / norm;
}
// cdfs.rs:27-29: (1 + (x/B)^-A)^-P, params = (A, B, P)
LCHD_HD double cdf_dagum(const double* p, double x) { return pow(1.0 + pow(x / p[1], -p[0]), -p[2]); }
// cdfs.rs:39-45
LCHD_HD double cdf_uniform(const double* p, double x) {
    if (x < p[0]) return 0.0;
    if (x > p[1]) return 1.0;
    return (x - p[0]) / (p[1] - p[0]);
}
// cdfs.rs:56-63
LCHD_HD double cdf_kumaraswamy(const double* p, double x) {
    if (x < p[0]) return 0.0;
    if (x > p[1]) return 1.0;
    const double z = (x - p[0]) / (p[1] - p[0]);
    return 1.0 - pow(1.0 - pow(z, p[2]), p[3]);
}
LCHD_HD double cdf_eval(int kind, const double* p, int np, double x) {
    switch (kind) {
        case WF_HYPER_EXP: return cdf_hyper_exp(p, np, x);
        case WF_DAGUM: return cdf_dagum(p, x);
        case WF_UNIFORM: return cdf_uniform(p, x);
        default: return cdf_kumaraswamy(p, x);
    }
}

// The densities w = F' (additive, not in the reference): the analytic derivative of each CDF as written above; 0 for x < 0.
// d/dx [1 - sum_i a_i exp(-b_i x) / sum_i a_i]
LCHD_HD double pdf_hyper_exp(const double* p, int np, double x) {
    if (x < 0.0) return 0.0;
    double norm = 0.0, sum = 0.0;
    const int n = np / 2;
    for (int i = 0; i < n; ++i) {
        sum += p[i] * p[n + i] * exp(-p[n + i] * x);
        norm += p[i];
    }
    return sum / norm;
}
// d/dx (1 + (x/B)^-A)^-P = (A P / x) t (1 + t)^(-P - 1), t = (x/B)^-A; 0 at x = 0 (the limit for A P > 1)
LCHD_HD double pdf_dagum(const double* p, double x) {
    if (!(x > 0.0)) return 0.0;
    const double t = pow(x / p[1], -p[0]);
    return p[0] * p[2] / x * t * pow(1.0 + t, -p[2] - 1.0);
}
// 1 / (b - a) on [a, b), 0 elsewhere
LCHD_HD double pdf_uniform(const double* p, double x) { return (x < 0.0 || x < p[0] || !(x < p[1])) ? 0.0 : 1.0 / (p[1] - p[0]); }
// d/dx [1 - (1 - z^a)^b] = a b z^(a-1) (1 - z^a)^(b-1) / (x_max - x_min) on [x_min, x_max], 0 elsewhere
LCHD_HD double pdf_kumaraswamy(const double* p, double x) {
    if (x < 0.0 || x < p[0] || x > p[1]) return 0.0;
    const double z = (x - p[0]) / (p[1] - p[0]);
    return p[2] * p[3] * pow(z, p[2] - 1.0) * pow(1.0 - pow(z, p[2]), p[3] - 1.0) / (p[1] - p[0]);
}
LCHD_HD double pdf_eval(int kind, const double* p, int np, double x) {
    switch (kind) {
        case WF_HYPER_EXP: return pdf_hyper_exp(p, np, x);
        case WF_DAGUM: return pdf_dagum(p, x);
        case WF_UNIFORM: return pdf_uniform(p, x);
        default: return pdf_kumaraswamy(p, x);
    }
}

// The parameter derivatives G_k = dF/dtheta_k (additive, not in the reference): the analytic derivative of each CDF as written above with
// respect to each of its parameters, in the order a WeightFunction takes them.  out[k * stride], k < np.  Conventions:
//   x = +inf (and x < 0) gives 0 in every family: F(inf) = 1 whatever the parameters (a dagum with F(inf) != 1 is refused by the callers)
//   x = 0 gives the formula's value; a dagum at x = 0 gives 0
//   a product of the form 0 * ln 0 is 0
//   where the limit is infinite -- kumaraswamy's dF/dx_min, dF/dx_max with alpha < 1 at z = 0 and with beta < 1 at z = 1, a set of
//   distances of measure zero -- the value is 0; every other non-finite intermediate (a dagum with B = 0) gives 0 as well, so the output
//   is finite for every parameter set lchd_wf_validate accepts
//   a point exactly on a support bound of uniform / kumaraswamy takes the inside branch, as the CDF does: one-sided there
LCHD_HD void cdf_param_grad_strided(int kind, const double* p, int np, double x, double* out, int stride) {
    for (int k = 0; k < np; ++k) out[k * stride] = 0.0;
    if (!(x >= 0.0) || x == (double)INFINITY) return;
    switch (kind) {
        case WF_HYPER_EXP: {  // N = sum a_i: dF/da_k = ((1 - F) - e^(-b_k x)) / N, dF/db_k = a_k x e^(-b_k x) / N
            const int n = np / 2;
            double norm = 0.0, sum = 0.0;
            for (int i = 0; i < n; ++i) {
                const double e = exp(-p[n + i] * x);
                out[(n + i) * stride] = e;  // (kept in the slot it ends in)
                sum += p[i] * e;
                norm += p[i];
            }
            const double tail = sum / norm;  // 1 - F
            for (int i = 0; i < n; ++i) {
                const double e = out[(n + i) * stride];
                out[i * stride] = (tail - e) / norm;
                out[(n + i) * stride] = p[i] * x * e / norm;
            }
            break;
        }
        case WF_DAGUM: {  // t = (x/B)^-A: dF/dP = -F ln(1 + t), dF/dt = -P (1 + t)^(-P-1), dt/dA = -t ln(x/B), dt/dB = A t / B
            if (x == 0.0) return;
            const double r = x / p[1], t = pow(r, -p[0]);
            if (!(t > 0.0) || t == (double)INFINITY) return;  // (F is 1 or 0 there and flat in every parameter)
            const double dFdt = -p[2] * pow(1.0 + t, -p[2] - 1.0);
            out[0] = dFdt * (-t * log(r));
            out[stride] = dFdt * (p[0] * t / p[1]);
            out[2 * stride] = -pow(1.0 + t, -p[2]) * log1p(t);
            break;
        }
        case WF_UNIFORM: {  // on a <= x <= b: (x - b) / (b - a)^2, -(x - a) / (b - a)^2
            if (x < p[0] || x > p[1]) return;
            const double L = p[1] - p[0];
            out[0] = (x - p[1]) / (L * L);
            out[stride] = -(x - p[0]) / (L * L);
            break;
        }
        default: {  // kumaraswamy, z = (x - x_min) / L: dF/dz = a b z^(a-1) (1 - z^a)^(b-1), dz/dx_min = -(1 - z) / L, dz/dx_max = -z / L,
                    // dF/da = b (1 - z^a)^(b-1) z^a ln z, dF/db = -(1 - z^a)^b ln(1 - z^a)
            if (x < p[0] || x > p[1]) return;
            const double L = p[1] - p[0], z = (x - p[0]) / L, a = p[2], b = p[3];
            const double za = pow(z, a), u = 1.0 - za;
            const double dFdz = a * b * pow(z, a - 1.0) * pow(u, b - 1.0);
            out[0] = dFdz * (-(1.0 - z) / L);
            out[stride] = dFdz * (-z / L);
            const double zlnz = (z > 0.0 && z < 1.0) ? za * log(z) : 0.0;
            out[2 * stride] = zlnz != 0.0 ? b * pow(u, b - 1.0) * zlnz : 0.0;
            out[3 * stride] = (u > 0.0 && u < 1.0) ? -pow(u, b) * log1p(-za) : 0.0;
            break;
        }
    }
    for (int k = 0; k < np; ++k)
        if (!(fabs(out[k * stride]) < (double)INFINITY)) out[k * stride] = 0.0;
}
LCHD_HD void cdf_param_grad(int kind, const double* p, int np, double x, double* out) { cdf_param_grad_strided(kind, p, np, x, out, 1); }

// statistical_distances.rs:4-10.  P1/P2 are callables c -> probability so that kernels can feed
// register-resident state without materialising the normalised vectors (pmf.rs:78-81 does).
template <int NMAX, class P1, class P2>
LCHD_HD double sd_hellinger(P1 p1, P2 p2, int n, double e) {
    const double inv = 1.0 / e;
    double dist = 0.0;
    LCHD_FOR_C(NMAX, n, c) dist += pow(fabs(pow(p1(c), inv) - pow(p2(c), inv)), e);
    return pow(dist / 2.0, inv);
}
// exponent 2 (the default, src/locohd.rs:365-370): pow(x, .5) == sqrt(x) and pow(|d|, 2) == d*d
template <int NMAX, class P1, class P2>
LCHD_HD double sd_hellinger2(P1 p1, P2 p2, int n) {
    double dist = 0.0;
    LCHD_FOR_C(NMAX, n, c) {
        const double d = sqrt(p1(c)) - sqrt(p2(c));
        dist += d * d;
    }
    return sqrt(dist / 2.0);
}
// :12-21
template <int NMAX, class P1, class P2>
LCHD_HD double sd_ks(P1 p1, P2 p2, int n) {
    double best = 0.0;
    LCHD_FOR_C(NMAX, n, c) {
        const double d = fabs(p1(c) - p2(c));
        best = (c == 0 || d >= best) ? d : best;
    }
    return best;
}
// :23-29
template <int NMAX, class P1, class P2>
LCHD_HD double sd_kl(P1 p1, P2 p2, int n, double eps) {
    double dist = 0.0;
    LCHD_FOR_C(NMAX, n, c) {
        const double x = p1(c);
        dist += x * log((x + eps) / (p2(c) + eps));
    }
    return dist;
}
// :31-78
template <int NMAX, class P1, class P2>
LCHD_HD double sd_renyi(P1 p1, P2 p2, int n, double alpha, double eps) {
    if (alpha == 1.0) return sd_kl<NMAX>(p1, p2, n, eps);
    if (alpha == INFINITY) {
        double best = 0.0;
        LCHD_FOR_C(NMAX, n, c) {
            const double r = (p1(c) + eps) / (p2(c) + eps);
            best = (c == 0 || r >= best) ? r : best;
        }
        return log(best);
    }
    if (alpha == 0.0) {
        double s = 0.0;
        LCHD_FOR_C(NMAX, n, c) s += (p1(c) > 0.0) ? p2(c) : 0.0;
        return -log(s);
    }
    double s = 0.0;
    LCHD_FOR_C(NMAX, n, c) {
        const double x = p1(c);
        s += x * pow((x + eps) / (p2(c) + eps), alpha - 1.0);
    }
    return log(s) / (alpha - 1.0);
}
// StatisticalDistance::run dispatch, :123-142
template <int NMAX, class P1, class P2>
LCHD_HD double sd_eval(int kind, double prm0, double prm1, P1 p1, P2 p2, int n) {
    switch (kind) {
        case SD_HELLINGER: return (prm0 == 2.0) ? sd_hellinger2<NMAX>(p1, p2, n) : sd_hellinger<NMAX>(p1, p2, n, prm0);
        case SD_KS: return sd_ks<NMAX>(p1, p2, n);
        case SD_KL: return sd_kl<NMAX>(p1, p2, n, prm0);
        default: return sd_renyi<NMAX>(p1, p2, n, prm0, prm1);
    }
}

}  // namespace lchd
