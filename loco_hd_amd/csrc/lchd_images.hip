// lchd_images.hip -- periodic boundaries for from_primitives: the periodic images of a structure, materialised as an ordinary cloud.
//
// The reference searches an open system (KdTree::within_radius over the structure's own atoms, src/locohd.rs:504-528 of the reference).
// With an orthorhombic box (Lx, Ly, Lz) the environment of an anchor holds every periodic image of every atom of its structure that
// lies closer than the threshold.  Nothing of that search changes here: the images are resolved BEFORE it, into a cloud that holds the
// wrapped originals at their indices 0 .. n - 1 followed by the ghost atoms, and the cell lists, environment and sweep kernels run on
// that cloud as on any other (the cell build keys cells by the per-atom structure id, so ghosts need not follow their structure).
//
//   wrap      w = x - floor(x / L) * L, and 0 where that rounds to L                       (per axis, box of the atom's structure)
//   images    w + L exists iff w < reach, w - L exists iff w >= L - reach; both are that single f64 addition
//   ghosts    every combination of per-axis choices {original, +L, -L} except "all original": at most 26 per atom
//   order     the ghosts of atom i occupy n + offset[i] ... in ascending image code cx + 3 cy + 9 cz (c: 0 original, 1 +L, 2 -L)
//
// reach <= min(L) (lchd_box_validate), so one layer of images is all there is, and threshold <= reach is checked by the pass.
// Three steps, one launch each (the scan of more than kImgScanSpan atoms: two): k_img_count, the exclusive scan, k_img_emit.
//
// A triclinic cell (lattice vectors a, b, c = the rows of a 3 x 3 matrix, any non-singular one) takes the same three steps with
// k_img_count_cell / k_img_emit_cell; the scan does not know the difference.  Per cell the host prepares the matrix, its inverse and
// the perpendicular widths w_k = |det| / |cross of the other two vectors| (kImgCellRecord doubles, lchd_cell_validate's arithmetic).
//
//   wrap      f = x . inverse, p = x - (floor(f0) a + floor(f1) b + floor(f2) c); g = p . inverse are the fractional coordinates
//   images    along axis k: p + a_k exists iff g_k w_k < reach, p - a_k iff (1 - g_k) w_k <= reach -- the slab within `reach` of the
//             cell's faces, a superset of what any point of the cell can see; the search measures real distances and stays exact
//   ghosts    p[d] + t[d] with t[d] = (i a[d] + j b[d]) + k c[d], i, j, k in {0, 1, -1} as doubles: plain f64 products and sums in
//             that order, never contracted (-ffp-contract=off of the Makefile: the kernels below hold no fused multiply-add), so that a host
//             can rebuild them bit for bit
//   order     as above: ascending image code c0 + 3 c1 + 9 c2 (c: 0 original, 1 plus, 2 minus)
//
// reach <= min(w) (lchd_cell_validate): a shift of 2 along axis k is at least w_k away from every point of the cell.
#include "lchd_kcommon.h"

namespace lchd {

__device__ __forceinline__ double img_wrap(double x, double L) {
    const double w = x - floor(x / L) * L;
    return w == L ? 0.0 : w;
}
// per-axis choices of one wrapped coordinate: bit 0 the image w + L exists, bit 1 the image w - L
__device__ __forceinline__ int img_choices(double w, double L, double reach) { return (w < reach ? 1 : 0) | (w >= L - reach ? 2 : 0); }
__device__ __forceinline__ int img_ways(int ch) { return 1 + (ch & 1) + (ch >> 1); }
__device__ __forceinline__ const double* img_box(const ImageArgs& a, int64_t i) {
    return a.boxes + 3 * (size_t)((a.n_boxes > 1 && a.src.sid) ? a.src.sid[i] : 0);
}

// The lanes' bounding boxes and non-finite flags into the seven ordered-key words: one atomic per word and wavefront.
__device__ __forceinline__ void img_reduce_bbox(const ImageArgs& a, double (&mn)[3], double (&mx)[3], bool bad) {
    for (int m = 32; m > 0; m >>= 1)
        for (int k = 0; k < 3; ++k) { mn[k] = fmin(mn[k], shfl_xor_f64(mn[k], m)); mx[k] = fmax(mx[k], shfl_xor_f64(mx[k], m)); }
    const unsigned long long anybad = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && (int64_t)blockIdx.x * kImgScanSpan + (threadIdx.x & ~63) < a.src.n) {
        for (int k = 0; k < 3; ++k) { atomicMin(&a.bbox[k], ordered_key(mn[k])); atomicMax(&a.bbox[3 + k], ordered_key(mx[k])); }
        if (anybad) atomicOr(&a.bbox[6], 1ull);
    }
}

// One lane per atom: the wrapped original into slot i (coordinates and labels), its ghost count into count[i], the bounding box of the
// atom and its ghosts into the seven ordered-key words (k_frames_unpack's reduction: one atomic per word and wavefront).
__global__ __launch_bounds__(kImgScanSpan) void k_img_count(ImageArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kImgScanSpan + threadIdx.x;
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool bad = false;
    if (i < a.src.n) {
        const double* L = img_box(a, i);
        const double v[3] = {a.src.x[i], a.src.y[i], a.src.z[i]};
        double w[3];
        int ways = 1;
        for (int k = 0; k < 3; ++k) {
            w[k] = img_wrap(v[k], L[k]);
            bad = bad || !(fabs(w[k]) < INFINITY);
            const int ch = img_choices(w[k], L[k], a.reach);
            ways *= img_ways(ch);
            mn[k] = (ch & 2) ? w[k] - L[k] : w[k];
            mx[k] = (ch & 1) ? w[k] + L[k] : w[k];
        }
        a.x[i] = w[0]; a.y[i] = w[1]; a.z[i] = w[2];
        a.cat[i] = a.src.cat[i];
        if (a.cat_hi) { a.cat_hi[i] = a.src.cat_hi[i]; a.cat_narrow[i] = a.src_narrow[i]; }
        a.tag[i] = a.src.tag[i];
        if (a.sid) a.sid[i] = a.src.sid[i];
        a.count[i] = (uint32_t)(ways - 1);
    }
    img_reduce_bbox(a, mn, mx, bad);
}

// Exclusive scan of one block span: DPP scan per wavefront, the wavefronts' totals through LDS.  Returns the lane's exclusive prefix
// inside the span; *span_total (all lanes) = the span's sum.
__device__ __forceinline__ uint32_t img_span_scan(uint32_t v, uint32_t* span_total) {
    constexpr int kWaves = kImgScanSpan / 64;
    __shared__ uint32_t wave_sum[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan_u32(v);
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int w = 0; w < kWaves; ++w) { before += w < wave ? wave_sum[w] : 0u; all += wave_sum[w]; }
    __syncthreads();  // (the caller may scan again: wave_sum is free from here on)
    *span_total = all;
    return before + incl - v;
}
// offset[i] = ghosts of the atoms of i's span before i; span_sum[b] = ghosts of span b (one workgroup per span).  With a single span
// (n <= kImgScanSpan) this is the whole scan: the total goes straight to *total.
__global__ __launch_bounds__(kImgScanSpan) void k_img_scan_spans(const uint32_t* __restrict__ count, int64_t n, uint32_t* __restrict__ offset,
                                                                 unsigned long long* __restrict__ span_sum, unsigned long long* total) {
    const int64_t i = (int64_t)blockIdx.x * kImgScanSpan + threadIdx.x;
    uint32_t all;
    const uint32_t ex = img_span_scan(i < n ? count[i] : 0u, &all);
    if (i < n) offset[i] = ex;
    if (threadIdx.x == 0) {
        if (span_sum) span_sum[blockIdx.x] = all;
        if (total) *total = all;
    }
}
// span_sum[b] -> ghosts of all spans before b (in place), by one workgroup that carries the running sum from chunk to chunk
__global__ __launch_bounds__(kImgScanSpan) void k_img_scan_sums(unsigned long long* span_sum, int64_t n_spans, unsigned long long* total) {
    unsigned long long carry = 0;
    for (int64_t base = 0; base < n_spans; base += kImgScanSpan) {
        const int64_t b = base + threadIdx.x;
        const uint32_t v = b < n_spans ? (uint32_t)span_sum[b] : 0u;  // (a span holds at most 26 * kImgScanSpan ghosts)
        uint32_t all;
        const uint32_t ex = img_span_scan(v, &all);
        if (b < n_spans) span_sum[b] = carry + ex;
        carry += all;
    }
    if (threadIdx.x == 0) *total = carry;
}

// One lane per atom: its ghosts at n + offset in ascending image code, x fastest; every ghost carries its atom's labels.
// Reads the wrapped coordinates k_img_count left in slot i, so the choices are the ones that were counted.
__global__ __launch_bounds__(kImgScanSpan) void k_img_emit(ImageArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kImgScanSpan + threadIdx.x;
    if (i >= a.src.n) return;
    const double* L = img_box(a, i);
    const double w[3] = {a.x[i], a.y[i], a.z[i]};
    double im[3][3];
    int ch[3];
    for (int k = 0; k < 3; ++k) {
        ch[k] = img_choices(w[k], L[k], a.reach) << 1 | 1;  // bit c: choice c of this axis exists (0 original, 1 +L, 2 -L)
        im[k][0] = w[k]; im[k][1] = w[k] + L[k]; im[k][2] = w[k] - L[k];
    }
    int64_t o = (int64_t)a.src.n + (int64_t)((a.span_sum ? a.span_sum[i / kImgScanSpan] : 0ull) + a.offset[i]);
    const uint8_t cat = a.cat[i];
    const int32_t tag = a.tag[i];
    for (int cz = 0; cz < 3; ++cz)
        for (int cy = 0; cy < 3; ++cy)
            for (int cx = 0; cx < 3; ++cx) {
                if (!((ch[0] >> cx) & (ch[1] >> cy) & (ch[2] >> cz) & 1) || (cx | cy | cz) == 0) continue;
                if (o >= a.capacity) return;  // (never: the host sized the arrays from the scan's total)
                a.x[o] = im[0][cx]; a.y[o] = im[1][cy]; a.z[o] = im[2][cz];
                a.cat[o] = cat;
                if (a.cat_hi) { a.cat_hi[o] = a.cat_hi[i]; a.cat_narrow[o] = a.cat_narrow[i]; }
                a.tag[o] = tag;
                if (a.sid) a.sid[o] = a.sid[i];
                ++o;
            }
}

// ---- triclinic cells ----------------------------------------------------------------------------------------------------------
// The record of the atom's cell: R[0..8] the cell (row 0 = a), R[9..17] its inverse, R[18..20] the perpendicular widths.
__device__ __forceinline__ const double* img_cell(const ImageArgs& a, int64_t i) {
    return a.cells + kImgCellRecord * (size_t)((a.n_boxes > 1 && a.src.sid) ? a.src.sid[i] : 0);
}
// row vector times the inverse: the fractional coordinates of a point
__device__ __forceinline__ void img_frac(const double* R, const double (&v)[3], double (&f)[3]) {
    for (int k = 0; k < 3; ++k) f[k] = (v[0] * R[9 + k] + v[1] * R[12 + k]) + v[2] * R[15 + k];
}
// per-axis choices of a fractional coordinate: bit 0 the image + a_k exists, bit 1 the image - a_k
__device__ __forceinline__ int img_choices_cell(double g, double w, double reach) {
    return (g * w < reach ? 1 : 0) | ((1.0 - g) * w <= reach ? 2 : 0);
}
// component d of the shift i a + j b + k c, the coefficients as doubles: THE expression of the contract
__device__ __forceinline__ double img_shift(const double* R, int d, double i, double j, double k) {
    return (i * R[d] + j * R[3 + d]) + k * R[6 + d];
}
__device__ __forceinline__ double img_coef(int choice) { return choice == 0 ? 0.0 : (choice == 1 ? 1.0 : -1.0); }

// k_img_count for a triclinic cell.  The bounding box is taken over the very sums k_img_emit_cell will write (a ghost's coordinate
// mixes all three lattice vectors, so there is no per-axis shortcut that rounds the same way).
__global__ __launch_bounds__(kImgScanSpan) void k_img_count_cell(ImageArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kImgScanSpan + threadIdx.x;
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool bad = false;
    if (i < a.src.n) {
        const double* R = img_cell(a, i);
        const double v[3] = {a.src.x[i], a.src.y[i], a.src.z[i]};
        double f[3], p[3], g[3];
        img_frac(R, v, f);
        for (int k = 0; k < 3; ++k) f[k] = floor(f[k]);
        for (int d = 0; d < 3; ++d) {
            p[d] = v[d] - img_shift(R, d, f[0], f[1], f[2]);
            bad = bad || !(fabs(p[d]) < INFINITY);
        }
        img_frac(R, p, g);
        int ch[3];
        for (int k = 0; k < 3; ++k) ch[k] = img_choices_cell(g[k], R[18 + k], a.reach) << 1 | 1;  // bit c: choice c of this axis exists
        int ways = 0;
        for (int c2 = 0; c2 < 3; ++c2)
            for (int c1 = 0; c1 < 3; ++c1)
                for (int c0 = 0; c0 < 3; ++c0) {
                    if (!((ch[0] >> c0) & (ch[1] >> c1) & (ch[2] >> c2) & 1)) continue;
                    ++ways;
                    for (int d = 0; d < 3; ++d) {
                        const double q = (c0 | c1 | c2) ? p[d] + img_shift(R, d, img_coef(c0), img_coef(c1), img_coef(c2)) : p[d];
                        mn[d] = fmin(mn[d], q); mx[d] = fmax(mx[d], q);
                    }
                }
        if (bad) ways = 1;  // (a NaN compares false everywhere; keep the count well defined, the build is refused anyway)
        a.x[i] = p[0]; a.y[i] = p[1]; a.z[i] = p[2];
        a.cat[i] = a.src.cat[i];
        if (a.cat_hi) { a.cat_hi[i] = a.src.cat_hi[i]; a.cat_narrow[i] = a.src_narrow[i]; }
        a.tag[i] = a.src.tag[i];
        if (a.sid) a.sid[i] = a.src.sid[i];
        a.count[i] = (uint32_t)(ways - 1);
    }
    img_reduce_bbox(a, mn, mx, bad);
}

// k_img_emit for a triclinic cell: the fractional coordinates are recomputed from the wrapped coordinates k_img_count_cell left in
// slot i by the same expression, so the choices are the ones that were counted.
__global__ __launch_bounds__(kImgScanSpan) void k_img_emit_cell(ImageArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kImgScanSpan + threadIdx.x;
    if (i >= a.src.n) return;
    const double* R = img_cell(a, i);
    const double p[3] = {a.x[i], a.y[i], a.z[i]};
    double g[3];
    img_frac(R, p, g);
    int ch[3];
    for (int k = 0; k < 3; ++k) ch[k] = img_choices_cell(g[k], R[18 + k], a.reach) << 1 | 1;
    int64_t o = (int64_t)a.src.n + (int64_t)((a.span_sum ? a.span_sum[i / kImgScanSpan] : 0ull) + a.offset[i]);
    const int64_t end = o + a.count[i];  // (what was counted, whatever a non-finite coordinate does to the comparisons)
    const uint8_t cat = a.cat[i];
    const int32_t tag = a.tag[i];
    for (int c2 = 0; c2 < 3; ++c2)
        for (int c1 = 0; c1 < 3; ++c1)
            for (int c0 = 0; c0 < 3; ++c0) {
                if (!((ch[0] >> c0) & (ch[1] >> c1) & (ch[2] >> c2) & 1) || (c0 | c1 | c2) == 0) continue;
                if (o >= end || o >= a.capacity) return;  // (never: the host sized the arrays from the scan's total)
                a.x[o] = p[0] + img_shift(R, 0, img_coef(c0), img_coef(c1), img_coef(c2));
                a.y[o] = p[1] + img_shift(R, 1, img_coef(c0), img_coef(c1), img_coef(c2));
                a.z[o] = p[2] + img_shift(R, 2, img_coef(c0), img_coef(c1), img_coef(c2));
                a.cat[o] = cat;
                if (a.cat_hi) { a.cat_hi[o] = a.cat_hi[i]; a.cat_narrow[o] = a.cat_narrow[i]; }
                a.tag[o] = tag;
                if (a.sid) a.sid[o] = a.sid[i];
                ++o;
            }
}

// ---- the way back ---------------------------------------------------------------------------------------------------------------
// One lane per source atom: origin / code of its own slot and of its ghosts.  Nothing of the build is kept but count / offset / span_sum
// and the wrapped coordinates in slot i, so the per-axis choices are derived again from those by the rule that counted and emitted them
// (img_choices on the box edges, img_choices_cell on the fractional coordinates), and the codes are walked in the emit kernels' order:
// ghost number `rank` of atom i sits at n + span_sum[i / span] + offset[i] + rank.  CELL picks the rule; the rest is one body.
template <bool CELL>
__global__ __launch_bounds__(kImgScanSpan) void k_img_origin(ImageArgs a, int32_t* __restrict__ origin, int8_t* __restrict__ code) {
    const int64_t i = (int64_t)blockIdx.x * kImgScanSpan + threadIdx.x;
    if (i >= a.src.n || i >= a.capacity) return;
    const double p[3] = {a.x[i], a.y[i], a.z[i]};
    int ch[3];  // bit c: choice c of this axis exists (0 original, 1 plus, 2 minus)
    if constexpr (CELL) {
        const double* R = img_cell(a, i);
        double g[3];
        img_frac(R, p, g);
        for (int k = 0; k < 3; ++k) ch[k] = img_choices_cell(g[k], R[18 + k], a.reach) << 1 | 1;
    } else {
        const double* L = img_box(a, i);
        for (int k = 0; k < 3; ++k) ch[k] = img_choices(p[k], L[k], a.reach) << 1 | 1;
    }
    origin[i] = (int32_t)i;
    code[i] = 0;
    int64_t o = (int64_t)a.src.n + (int64_t)((a.span_sum ? a.span_sum[i / kImgScanSpan] : 0ull) + a.offset[i]);
    const int64_t end = min(o + (int64_t)a.count[i], a.capacity);  // (what was counted and emitted: never more slots than those)
    for (int c2 = 0; c2 < 3; ++c2)
        for (int c1 = 0; c1 < 3; ++c1)
            for (int c0 = 0; c0 < 3; ++c0) {
                if (!((ch[0] >> c0) & (ch[1] >> c1) & (ch[2] >> c2) & 1) || (c0 | c1 | c2) == 0) continue;
                if (o >= end) return;
                origin[o] = (int32_t)i;
                code[o] = (int8_t)(c0 + 3 * c1 + 9 * c2);
                ++o;
            }
}

static unsigned img_blocks(int64_t n) { return (unsigned)((n + kImgScanSpan - 1) / kImgScanSpan); }
void launch_img_count(hipStream_t s, const ImageArgs& a) {
    static const unsigned long long init[7] = {~0ull, ~0ull, ~0ull, 0ull, 0ull, 0ull, 0ull};
    (void)hipMemcpyAsync(a.bbox, init, sizeof init, hipMemcpyHostToDevice, s);
    if (a.cells) k_img_count_cell<<<img_blocks(a.src.n), kImgScanSpan, 0, s>>>(a);
    else k_img_count<<<img_blocks(a.src.n), kImgScanSpan, 0, s>>>(a);
}
void launch_img_scan(hipStream_t s, const ImageArgs& a) {
    const unsigned spans = img_blocks(a.src.n);
    if (!a.span_sum) {
        k_img_scan_spans<<<1, kImgScanSpan, 0, s>>>(a.count, a.src.n, a.offset, nullptr, a.bbox + 7);
    } else {
        k_img_scan_spans<<<spans, kImgScanSpan, 0, s>>>(a.count, a.src.n, a.offset, a.span_sum, nullptr);
        k_img_scan_sums<<<1, kImgScanSpan, 0, s>>>(a.span_sum, spans, a.bbox + 7);
    }
}
void launch_img_emit(hipStream_t s, const ImageArgs& a) {
    if (a.cells) k_img_emit_cell<<<img_blocks(a.src.n), kImgScanSpan, 0, s>>>(a);
    else k_img_emit<<<img_blocks(a.src.n), kImgScanSpan, 0, s>>>(a);
}
void launch_img_origin(hipStream_t s, const ImageArgs& a, int32_t* origin, int8_t* code) {
    if (a.src.n <= 0) return;
    if (a.cells) k_img_origin<true><<<img_blocks(a.src.n), kImgScanSpan, 0, s>>>(a, origin, code);
    else k_img_origin<false><<<img_blocks(a.src.n), kImgScanSpan, 0, s>>>(a, origin, code);
}

}  // namespace lchd
