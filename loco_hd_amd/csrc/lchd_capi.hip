// lchd_capi.hip -- host side of the C ABI declared in include/loco_hd_hip.h.
//
// Owns: validation (the reference's PyValueError sites), packing of caller buffers into SoA device
// arrays, the device workspace, kernel sequencing on one HIP stream, the status read-back and its
// translation into the reference's error classes.  No scoring arithmetic happens on the host: every
// from_* entry point launches the gfx950 kernels of lchd_*.hip and fails with LCHD_EDEVICE when
// no GPU is usable.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/loco_hd_hip.h"
#include "lchd_cross_plan.h"
#include "lchd_device.h"
#include "lchd_math.h"
#include "lchd_radial_bins.h"
#include "lchd_strain_sum.h"

using namespace lchd;

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[1024] = "";
static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
extern "C" const char* lchd_last_error(void) { return g_err; }
extern "C" const char* lchd_version(void) { return "loco_hd_hip 0.1 (gfx950)"; }

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(LCHD_EDEVICE, "HIP error %d (%s) at %s:%d: %s", (int)e_,      \
                                          hipGetErrorName(e_), __FILE__, __LINE__, #expr);              \
    } while (0)

// ------------------------------------------------------------------------------------------------
// host-side leaves
// ------------------------------------------------------------------------------------------------
static const char* wf_name(int kind) {
    static const char* names[4] = {"hyper_exp", "dagum", "uniform", "kumaraswamy"};
    return (kind >= 0 && kind < 4) ? names[kind] : "?";
}

extern "C" int lchd_wf_validate(int32_t kind, const double* p, int32_t np) {  // weight_function.rs:22-93
    const char* nm = wf_name(kind);
    auto exactly = [&](int n) { return np == n ? 0 : fail(LCHD_EVALUE, "For function \"%s\" there must be exactly %d parameters!", nm, n); };
    switch (kind) {
        case LCHD_WF_HYPER_EXP:
            if (np % 2 != 0) return fail(LCHD_EVALUE, "For function \"%s\" there must be an even number of parameters!", nm);
            for (int i = 0; i < np; ++i)
                if (p[i] <= 0.0) return fail(LCHD_EVALUE, "For function \"%s\" all parameters must be positive!", nm);
            return LCHD_OK;
        case LCHD_WF_DAGUM:
            if (int rc = exactly(3)) return rc;
            if (p[0] < 0.0 || p[1] < 0.0 || p[2] < 0.0) return fail(LCHD_EVALUE, "For function \"%s\" all parameters must be positive!", nm);
            return LCHD_OK;
        case LCHD_WF_UNIFORM:
            if (int rc = exactly(2)) return rc;
            if (p[0] < 0.0) return fail(LCHD_EVALUE, "For function \"%s\" the first parameter must be non-negative!", nm);
            if (p[1] <= 0.0) return fail(LCHD_EVALUE, "For function \"%s\" the second parameter must be positive!", nm);
            if (p[0] >= p[1]) return fail(LCHD_EVALUE, "For function \"%s\" the first parameter must be smaller than the second!", nm);
            return LCHD_OK;
        case LCHD_WF_KUMARASWAMY:
            if (int rc = exactly(4)) return rc;
            if (p[0] < 0.0) return fail(LCHD_EVALUE, "For function \"%s\" the first parameter must be non-negative!", nm);
            if (p[1] <= 0.0 || p[2] <= 0.0 || p[3] <= 0.0)
                return fail(LCHD_EVALUE, "For function \"%s\" after the first parameter all parameters must be positive!", nm);
            if (p[0] >= p[1]) return fail(LCHD_EVALUE, "For function \"%s\" the first parameter must be smaller than the second!", nm);
            return LCHD_OK;
        default: return fail(LCHD_EVALUE, "No function implemented with this name!");
    }
}

extern "C" int lchd_wf_cdf(int32_t kind, const double* p, int32_t np, const double* x, int64_t n, double* out) {
    for (int64_t i = 0; i < n; ++i) {  // weight_function.rs:95-116
        if (x[i] < 0.0) return fail(LCHD_EVALUE, "Invalid input value: %g. All values must be non-negative!", x[i]);
        out[i] = cdf_eval(kind, p, np, x[i]);
    }
    return LCHD_OK;
}

// the density F' of the same function (additive: lchd_math.h); a negative x is no error here, the density there is 0
extern "C" int lchd_wf_pdf(int32_t kind, const double* p, int32_t np, const double* x, int64_t n, double* out) {
    if (n > 0 && (!p || !x || !out)) return fail(LCHD_EVALUE, "null pointer");
    for (int64_t i = 0; i < n; ++i) out[i] = pdf_eval(kind, p, np, x[i]);
    return LCHD_OK;
}

// the parameter derivatives dF/dtheta_k of the same function (additive: lchd_math.h, cdf_param_grad); out: [n][n_params]
extern "C" int lchd_wf_cdf_grad(int32_t kind, const double* p, int32_t np, const double* x, int64_t n, double* out) {
    if (int rc = lchd_wf_validate(kind, p, np)) return rc;
    if (n > 0 && (!x || !out)) return fail(LCHD_EVALUE, "null pointer");
    for (int64_t i = 0; i < n; ++i) {
        if (x[i] < 0.0) return fail(LCHD_EVALUE, "Invalid input value: %g. All values must be non-negative!", x[i]);
        cdf_param_grad(kind, p, np, x[i], out + i * (int64_t)np);
    }
    return LCHD_OK;
}

extern "C" int lchd_sd_validate(int32_t kind, int32_t np) {  // statistical_distances.rs:96-121
    static const int want[4] = {1, 0, 1, 2};
    static const char* names[4] = {"Hellinger", "Kolmogorov-Smirnov", "Kullback-Leibler", "Renyi"};
    if (kind < 0 || kind > 3) return fail(LCHD_EVALUE, "Invalid statistical distance name!");
    if (np != want[kind]) return fail(LCHD_EVALUE, "Invalid number of parameters for %s: %d", names[kind], np);
    return LCHD_OK;
}

extern "C" int lchd_sd_run(int32_t kind, const double* prm, const double* p1, const double* p2, int32_t n, double* out) {
    if (kind < 0 || kind > 3) return fail(LCHD_EVALUE, "Invalid statistical distance name!");
    if (n <= 0 && kind == LCHD_SD_KOLMOGOROV_SMIRNOV) return fail(LCHD_EPANIC, "called `Option::unwrap()` on a `None` value");
    const double a = (kind == LCHD_SD_KOLMOGOROV_SMIRNOV) ? 0.0 : prm[0], b = (kind == LCHD_SD_RENYI) ? prm[1] : 0.0;
    // Hellinger with a runtime exponent: the reference calls powf even for e == 2 (statistical_distances.rs:5-9)
    if (kind == LCHD_SD_HELLINGER)
        *out = sd_hellinger<0>([&](int c) { return p1[c]; }, [&](int c) { return p2[c]; }, n, a);
    else
        *out = sd_eval<0>(kind, a, b, [&](int c) { return p1[c]; }, [&](int c) { return p2[c]; }, n);
    return LCHD_OK;
}

extern "C" int lchd_config_validate(int64_t n_given, int64_t n_map, const double* w, int64_t nw) {  // src/locohd.rs:305-346
    if (n_given == 0) return fail(LCHD_EVALUE, "The number of possible categories (primitive types) cannot be zero!");
    if (nw != n_map)
        return fail(LCHD_EVALUE, "LoCoHD parameters 'categories' and 'category_weights' must have the same lengths! "
                                 "Instead, they have lengths of %lld vs. %lld!", (long long)n_map, (long long)nw);
    long long bad = 0;
    for (int64_t i = 0; i < nw; ++i) bad += (w[i] <= 0.0);
    if (bad) return fail(LCHD_EVALUE, "LoCoHD parameter 'category_weights' must only contain positive values! "
                                      "Instead, it contains %lld non-positive values!", bad);
    return LCHD_OK;
}

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
struct lchd_cloud {
    double *x = nullptr, *y = nullptr, *z = nullptr;
    uint8_t* cat = nullptr;
    uint8_t* cat_hi = nullptr;  // high byte of the category ids (allocated when an id beyond 254 occurs: more than 255 categories)
    uint8_t* cat_narrow = nullptr;  // with cat_hi: the one-byte view for configurations of at most 255 categories (ids beyond 254 -> 255,
                                    // "not in the category map": the narrow kernels would otherwise score id 256 as category 0)
    int32_t* tag = nullptr;
    int32_t* sid = nullptr;  // batch of structures: structure id per atom (nullptr = one structure)
    int32_t n_struct = 1;
    int32_t struct_size = 0;  // > 0: structure k is atoms [k * struct_size, (k + 1) * struct_size)
    int64_t n = 0;
    // trajectory-frames buffer (lchd_frames_create): capacity, staging and cross-stream hand-off
    int64_t n_tmpl = 0;        // atoms per frame
    int32_t cap_frames = 0;    // frames the arrays can hold
    double* d_raw = nullptr;   // device staging of the caller's [frames][atoms][3] block
    double* h_pinned = nullptr;
    // frames given as float32 SOURCE atoms (lchd_frames_set_sources): CSR map primitive atom -> source atoms
    int32_t *d_src_start = nullptr, *d_src_idx = nullptr, *d_tiles = nullptr;
    int32_t n_tiles = 0;
    int64_t n_src = 0;
    float *d_raw32 = nullptr, *h_pinned32 = nullptr;
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;  // timing of the most recent load (only when the context's timing is on)
    bool t_valid = false;
    unsigned long long* d_bbox = nullptr;  // [7]: order-preserving keys of min xyz, max xyz, non-finite flag
    unsigned long long* d_bbox_part = nullptr;  // per-workgroup partials of the centroid kernel
    hipEvent_t ev_ready = nullptr, ev_used = nullptr;
    bool bbox_pending = false, used_valid = false;
    double bbmin[3] = {0, 0, 0}, bbmax[3] = {0, 0, 0};
    // image cloud (lchd_cloud_create_images): the periodic images of another cloud; d_bbox holds 8 words (the ghost total last)
    double reach = INFINITY;   // the largest threshold a pass may search this cloud with (+inf: every cloud that is not an image cloud)
    bool images = false;
    int64_t img_cap = 0;       // atoms the arrays hold (they only grow)
    uint32_t *d_img_count = nullptr, *d_img_offset = nullptr;  // [img_scan_cap] ghosts per source atom / their exclusive scan per span
    unsigned long long* d_img_spans = nullptr;                 // [img_scan_cap / kImgScanSpan + 1]
    int64_t img_scan_cap = 0;
    double* d_boxes = nullptr; // [boxes_cap][3]
    int32_t boxes_cap = 0;
    bool img_cell = false;     // built from triclinic cells (lchd_cloud_create_images_cell), not boxes: the family is fixed at creation
    double* d_cells = nullptr; // [cells_cap][kImgCellRecord]
    int32_t cells_cap = 0;
    std::vector<double> h_cells;  // what the last build copied to d_cells (the copy is asynchronous)
    // the way back from a slot to its source atom (images_origin): built by the first call that asks after a build, stale after every build
    int64_t n_home = 0;        // source atoms of the last build (slots 0 .. n_home - 1 hold the wrapped originals)
    int32_t img_boxes = 0;     // boxes / cells the last build was given
    int32_t* d_img_origin = nullptr;  // [origin_cap] source atom of every slot
    int8_t* d_img_code = nullptr;     // [origin_cap] image code of every slot (0: an original)
    int64_t origin_cap = 0;    // follows img_cap
    bool origin_valid = false;
    // wide: the configuration has more than 255 categories (two-byte ids where the structure carries them)
    CloudView view(bool wide) const {
        const bool two = wide && cat_hi;
        return CloudView{x, y, z, (!wide && cat_narrow) ? cat_narrow : cat, two ? cat_hi : nullptr, tag, (int32_t)n, sid, n_struct, sid ? struct_size : 0};
    }
};

enum { PH_CELLS = 0, PH_ANCHORS = 1, PH_ENV = 2, PH_SWEEP = 3, PH_N = 4 };

// What lchd_ctx_last_grid reports about one side of a pass: the planned grid and which cell-list build launch_prologue picked.
struct GridRecord {
    int32_t dim[3] = {0, 0, 0};
    int64_t n_cells = 0;
    int32_t build = 0;
};
// What lchd_ctx_last_anchors reports about one side of a pass: which de-duplication launch_prologue picked and what the pass's kernels
// counted (the host status mirror's n_unique / n_dup_b).
struct AnchorRecord {
    int32_t mode = 0;
    int64_t n_unique = 0;
    int64_t n_repeated = -1;  // mode 4 only
};
// What lchd_ctx_last_sweep reports: the plan launch_sweep followed, what k_pair_meta published about the pass's pairs, the rule in force.
struct SweepRecord {
    lchd_sweep_plan plan{};
    int64_t stats[4] = {-1, -1, -1, -1};  // n_duo, n_c8, largest environment, pairs left to the companion
    int32_t rule = -1;
    int32_t repeated = 0;
};

// Calls on one context are serialised (include/loco_hd_hip.h, "Threads"): every entry point that takes a context holds it for its
// whole duration (CtxLock below).  The owner may re-enter (lchd_from_primitives_dev is lchd_from_primitives_dev_async +
// lchd_ctx_finish).  Between lchd_from_primitives_dev_async and lchd_ctx_finish the context stays with the thread that enqueued the
// pass: that thread may go on calling (and gets today's errors, e.g. LCHD_EVALUE for a second async call), a call from any other
// thread waits until the pass has been finished -- lchd_ctx_finish itself excepted, which any thread may make.
struct CtxMutex {
    std::mutex m;
    std::condition_variable cv;
    std::thread::id owner{};        // the thread inside an entry point (depth > 0)
    int depth = 0;
    bool async_open = false;        // an asynchronous pass is pending ...
    std::thread::id async_owner{};  // ... enqueued by this thread
};

struct lchd_ctx {
    CtxMutex mu;
    int device = 0;
    hipStream_t stream = nullptr;
    Tuning tune{};  // LCHD_* test / tuning hooks, read once in lchd_ctx_create
    Tuning tune_env{};  // ... as read from the environment (lchd_ctx_set_deterministic(0) returns to them)
    bool deterministic = false;
    // configuration
    bool cfg_set = false;
    bool hellinger2 = false, unit_weights = false, wf_pow = false;  // which sweep kernel variant applies
    bool finf_differ = false;  // the weight functions of a dictionary do not share F(+inf) (degenerate parameters): no key sets
    int wf_np_max = 0;         // the most parameters of any weight function of the configuration: the row width of a weight-function gradient
    bool wf_finf_off = false;  // a weight function's F(+inf) is not 1 (a degenerate dagum): no weight-function gradient
    int sd_fast = 0;  // Kullback-Leibler (1) / Renyi (2) with parameters the O(1)-per-event sweep handles (lchd_sweep_inc.hip)
    DevConfig h_cfg{};
    DevConfig* d_cfg = nullptr;
    char* d_blob = nullptr;
    size_t blob_cap = 0;
    // workspace arena
    char* ws = nullptr;
    size_t ws_cap = 0;
    DeviceStatus* d_status = nullptr;  // clean (all zero) between passes: k_pair_meta's last workgroup resets it
    HostStatus* h_status = nullptr;    // pinned, device-visible: the kernels publish into it with plain stores (no D2H copy)
    bool status_dirty = false;         // a pass was abandoned half-way: memset d_status before the next one
    uint32_t seq = 0;                  // pass counter (HostStatus::snapshot_seq)
    unsigned long long* d_points = nullptr;
    double* d_tabs = nullptr;  // sqrt(k) | 1/sqrt(k), 65536 entries each
    unsigned char* d_wide_scratch = nullptr;  // more than kWideCategories categories: per-workgroup state of k_sweep_wide<.., HUGE> (lchd_ctx_set_config)
    size_t wide_scratch_cap = 0;
    int wide_scratch_waves = 0;
    double* d_powtab = nullptr;  // k^(1/e) | k^(-1/e) for the configured Hellinger exponent (allocated when one is first configured)
    double powtab_e = 0.0;       // the exponent the table holds
    DoneState* d_done = nullptr;     // 'last workgroup' counters / accumulators of k_pair_meta (zero between kernels)
    uint32_t* d_left = nullptr;      // two counter slots of the leftover list (SweepArgs::left_count / left_zero), 128 B apart
    int left_slot = 0;               // the slot the next record pass appends to (zero by then: the previous one zeroed it)
    // host-pointer calls: one grow-only device block + pinned staging block per context (no allocation in the steady state)
    char *d_io = nullptr, *h_io = nullptr;
    size_t io_cap = 0;
    std::vector<char> cfg_blob_host;  // last configuration blob uploaded (identical configurations are not uploaded again)
    PassHints hints{};  // what the thresholded passes of this context looked like so far (lchd_pass_plan.h): plan_pass and launch_sweep read it
    lchd_dense_record last_dense{};  // what the most recent dense call ran (lchd_ctx_last_dense): plan of the attempt that stood, attempts, canon, bitonic rows
    bool last_dense_valid = false;   // ... and whether it ran to its end
    int64_t n_per_pair_passes = 0;  // passes whose side B was not de-duplicated (PassPlan::per_pair)
    // second pass over the pairs of overflowed environments (lchd_ctx_finish): grow-only device blocks outside the arena
    char *d_ovf_bits = nullptr, *d_ovf_lists = nullptr;
    size_t ovf_bits_cap = 0, ovf_lists_cap = 0;
    char* d_radial_bounds = nullptr;  // radial profiles: [n_wf][edges] bin bounds in key space (grow-only, outside the arena: the store builders lay the arena out)
    size_t radial_bounds_cap = 0;
    char* d_indexed = nullptr;        // sensitivity calls: the indexed environment lists of both sides (grow-only, outside the arena likewise)
    size_t indexed_cap = 0;
    int64_t sens_needed = 0;          // lchd_sensitivity_needed_width: the longest list among the pairs of the last sensitivity call
    char* d_cross = nullptr;          // cross-scoring calls: the pair records, wf indices and score scratch of one row tile (grow-only likewise)
    size_t cross_cap = 0;
    char* d_grad = nullptr;           // native gradient calls: the sensitivity lists of one tile of pairs (grow-only likewise)
    size_t grad_cap = 0;
    char* d_grad_acc = nullptr;       // ... and the exact accumulators of both sides with the status word in front: all zero between calls
    size_t grad_acc_cap = 0;
    bool grad_acc_dirty = false;      // a gradient call was abandoned between its first tile and k_grad_finish: memset before the next one
    int32_t grad_width = 0;           // the row width the last thresholded gradient call ended with (the next one starts there)
    int64_t n_subset_passes = 0;    // second passes run so far
    size_t last_store_bytes = 0;    // environment-store bytes (keys + categories, both sides) of the passes of the last from_primitives call
    int64_t n_passes = 0;           // from_primitives passes enqueued so far (a call is one pass unless a capacity / launch-set retry repeats it)
    // timing
    bool timing = false;
    hipEvent_t ev[PH_N + 1] = {};
    float ms[PH_N] = {-1, -1, -1, -1};
    // a from_primitives call that has been enqueued but not finished (lchd_from_primitives_dev_async)
    struct PassRequest {  // what the caller (or rescore_overflow_pairs) asked for
        lchd_cloud *a = nullptr, *b = nullptr;
        const int64_t* anchors = nullptr;
        const int32_t* wf = nullptr;
        int64_t n_pairs = 0;
        double thr = 0.0;
        double* out = nullptr;
        int cap = 0;
        bool subset = false;    // the pass IS a second pass over the pairs of overflowed environments
        bool repeated = false;  // the pass repeats one whose companion sweep had been left out
    };
    struct PassLaunched {  // what prims_enqueue put on the stream for it
        SweepArgs sw{};
        const uint32_t *ovf_a = nullptr, *ovf_b = nullptr;  // overflow lists of the enqueued pass (null: its kernels keep none)
        int64_t n_slots_a = 0, n_slots_b = 0;               // environment slots per side
        GridRecord grid[2];                                 // grids and cell-list builds of the enqueued pass
        int dedup[2] = {0, 0};                              // ... and its de-duplication modes (launch_prologue's dedup_out)
        lchd_sweep_plan plan{};                             // what launch_sweep launched for it
        SweepLaunched sweep{};                              // ... and reported back
    };
    struct {
        bool active = false;
        PassRequest req;
        PassPlan plan;  // plan_pass's decisions for the enqueued pass
        PassLaunched run;
    } pend;
    // multi-GPU sharding helpers (lchd_shard_*): device state, host-mapped counts, the plan they belong to
    ShardState* d_shard = nullptr;
    hipStream_t shard_stream = nullptr;  // the plan kernel runs (and is waited for) here: the wait does not include the scoring passes
    hipEvent_t shard_ev = nullptr;       // ... and the selection on the context's stream is ordered behind it
    hipEvent_t shard_sel_ev = nullptr;   // the last selection (reads the plan's bin table): the next plan is ordered behind it
    bool shard_sel_pending = false;
    int64_t* h_counts = nullptr;
    uint32_t* d_bad = nullptr;
    int shard_world = 0;
    int64_t shard_pairs = 0, shard_atoms = 0, shard_atoms_b = 0;
    // most recent sweep (for lchd_ctx_last_env_points)
    SweepArgs last{};
    bool last_valid = false;
    GridRecord last_grid[2];  // ... and its grids and cell-list builds (for lchd_ctx_last_grid)
    AnchorRecord last_anchors[2];  // ... and its anchor de-duplication (for lchd_ctx_last_anchors)
    SweepRecord last_sweep;   // ... and its sweep kernels (for lchd_ctx_last_sweep)
    bool last_sweep_valid = false;  // (host data only: it outlives the I/O block of a host-pointer call, which last_valid does not)
};

struct Arena {
    char* base;
    size_t off = 0, cap;
    bool dry;
    Arena(char* b, size_t c, bool d) : base(b), cap(c), dry(d) {}
    template <class T>
    T* take(size_t n) {
        off = (off + 255) & ~size_t(255);
        T* p = dry ? nullptr : reinterpret_cast<T*>(base + off);
        off += n * sizeof(T);
        return p;
    }
};

// HIP's current device is per-thread state that torch, another context or another library may change between two calls:
// every entry point that takes a context makes the context's device current for its duration and restores the caller's.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int device) {  // device < 0: nothing to do
        if (device < 0) return;
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) switched = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceGuard() {
        if (switched && prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define CTX_GUARD(c) DeviceGuard device_guard_((c)->device)

struct CtxLock {
    lchd_ctx* c;
    CtxLock(lchd_ctx* ctx, bool finishing) : c(ctx) {  // ctx == nullptr: nothing to lock (the entry point fails on it)
        if (!c) return;
        CtxMutex& mu = c->mu;
        const std::thread::id me = std::this_thread::get_id();
        std::unique_lock<std::mutex> lk(mu.m);
        if (mu.depth > 0 && mu.owner == me) {
            ++mu.depth;
            return;
        }
        mu.cv.wait(lk, [&] { return mu.depth == 0 && (!mu.async_open || mu.async_owner == me || finishing); });
        mu.owner = me;
        mu.depth = 1;
    }
    ~CtxLock() {
        if (!c) return;
        CtxMutex& mu = c->mu;
        std::lock_guard<std::mutex> lk(mu.m);
        if (--mu.depth > 0) return;
        mu.async_open = c->pend.active;  // (written by the owner only: stable here)
        mu.async_owner = mu.owner;
        mu.owner = std::thread::id();
        mu.cv.notify_all();
    }
    CtxLock(const CtxLock&) = delete;
    CtxLock& operator=(const CtxLock&) = delete;
};
#define CTX_LOCK(c) CtxLock ctx_lock_((c), false)
#define CTX_LOCK_FINISH(c) CtxLock ctx_lock_((c), true)

static int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}
static Tuning tuning_from_env() {  // the ONLY place that reads LCHD_* hooks (tests and tuning runs; unset in production)
    Tuning t;
    t.no_struct_cells = getenv("LCHD_NO_STRUCT_CELLS") != nullptr;
    t.no_share = getenv("LCHD_NO_SHARED_ENVS") != nullptr;
    t.no_cdf_keys = getenv("LCHD_NO_CDF_KEYS") != nullptr;
    t.no_key_sets = getenv("LCHD_NO_KEY_SETS") != nullptr;
    t.no_duo = getenv("LCHD_NO_DUO") != nullptr;
    t.force_wide = env_int("LCHD_FORCE_WIDE", 0) != 0;
    t.force_generic = env_int("LCHD_FORCE_GENERIC", 0) != 0;
    t.force_bigenv = env_int("LCHD_FORCE_BIGENV", 0) != 0;
    t.no_inline_meta = getenv("LCHD_NO_INLINE_META") != nullptr;
    t.no_count8 = getenv("LCHD_NO_COUNT8") != nullptr;
    t.no_c8_team = getenv("LCHD_NO_C8_TEAM") != nullptr;
    t.old_rows = getenv("LCHD_OLD_ROWS") != nullptr;
    t.no_dense_fused = getenv("LCHD_NO_DENSE_FUSED") != nullptr;
    t.no_env_group = getenv("LCHD_NO_ENV_GROUP") != nullptr;
    t.no_overflow_subset = getenv("LCHD_NO_OVERFLOW_SUBSET") != nullptr;
    t.env_apw = env_int("LCHD_ENV_APW", 0);
    t.no_sd_inc = getenv("LCHD_NO_SD_INC") != nullptr;
    t.force_cmax = env_int("LCHD_FORCE_CMAX", 0);
    t.per_pair = env_int("LCHD_PER_PAIR", 0);
    t.pre_rows = env_int("LCHD_PRE_ROWS", 0);
    t.team_batch = env_int("LCHD_TEAM_BATCH", 0);
    t.team_grid = env_int("LCHD_TEAM_GRID", 0);
    t.ensemble_block = env_int("LCHD_ENSEMBLE_BLOCK", 0);
    t.param_sum_blocks = env_int("LCHD_PARAM_SUM_BLOCKS", 0);
    return t;
}

static int ensure_ws(lchd_ctx* ctx, size_t need) {
    if (need <= ctx->ws_cap) return LCHD_OK;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->ws) HIP_TRY(hipFree(ctx->ws));
    ctx->ws = nullptr;
    ctx->ws_cap = 0;
    ctx->last_valid = ctx->last_sweep_valid = false;
    size_t got = need + need / 8 + (1 << 20);
    hipError_t e = hipMalloc(&ctx->ws, got);
    if (e != hipSuccess) {  // without the growth margin
        (void)hipGetLastError();
        got = need;
        e = hipMalloc(&ctx->ws, got);
    }
    if (e != hipSuccess) {
        ctx->ws = nullptr;
        (void)hipGetLastError();
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        return fail(LCHD_EUNSUPPORTED, "this call needs a device workspace of %zu bytes (environment store included) but only %zu of %zu "
                                       "bytes are free on the device", need, free_b, total_b);
    }
    ctx->ws_cap = got;
    return LCHD_OK;
}

extern "C" int lchd_ctx_create(int32_t device, lchd_ctx** out) {
    if (!out) return fail(LCHD_EVALUE, "null output pointer");
    *out = nullptr;
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0)
        return fail(LCHD_EDEVICE, "no usable HIP device (hipGetDeviceCount -> %d, %d devices): the LoCoHD scoring path has no "
                                  "CPU fallback", (int)e, n_dev);
    if (device >= n_dev) return fail(LCHD_EDEVICE, "device %d requested, %d HIP devices visible", device, n_dev);
    int cur = 0;
    HIP_TRY(hipGetDevice(&cur));
    lchd_ctx* c = new lchd_ctx();
    c->device = device >= 0 ? device : cur;
    c->tune = c->tune_env = tuning_from_env();
    CTX_GUARD(c);  // the caller's current device is restored on every path out of here
    auto bail = [&](hipError_t err, const char* what) {
        lchd_ctx_destroy(c);
        return fail(LCHD_EDEVICE, "HIP error %d (%s) in lchd_ctx_create: %s", (int)err, hipGetErrorName(err), what);
    };
    if ((e = hipMalloc(&c->d_cfg, sizeof(DevConfig))) != hipSuccess) return bail(e, "hipMalloc(config)");
    if ((e = hipMalloc(&c->d_status, sizeof(DeviceStatus))) != hipSuccess) return bail(e, "hipMalloc(status)");
    if ((e = hipMemset(c->d_status, 0, sizeof(DeviceStatus))) != hipSuccess) return bail(e, "hipMemset(status)");
    if ((e = hipMalloc(&c->d_points, sizeof(unsigned long long))) != hipSuccess) return bail(e, "hipMalloc(points)");
    if ((e = hipHostMalloc(&c->h_status, sizeof(HostStatus))) != hipSuccess) return bail(e, "hipHostMalloc(status)");
    memset(c->h_status, 0, sizeof(HostStatus));
    if ((e = hipMalloc(&c->d_tabs, sizeof(double) * 2 * 65536)) != hipSuccess) return bail(e, "hipMalloc(tables)");
    // (+ one cache line behind it: k_dense_fused's row counter, zero between launches -- k_dense_publish resets it)
    if ((e = hipMalloc(&c->d_done, sizeof(DoneState) + 128)) != hipSuccess) return bail(e, "hipMalloc(done)");
    if ((e = hipMemset(c->d_done, 0, sizeof(DoneState) + 128)) != hipSuccess) return bail(e, "hipMemset(done)");
    if ((e = hipMalloc(&c->d_left, 256)) != hipSuccess) return bail(e, "hipMalloc(leftover counters)");
    if ((e = hipMemset(c->d_left, 0, 256)) != hipSuccess) return bail(e, "hipMemset(leftover counters)");
    init_device_kernels();  // per device, not per process
    init_dense_fused_kernels();
    launch_fill_sqrt_tables(c->stream, c->d_tabs, c->d_tabs + 65536);
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return bail(e, "table fill");
    for (auto& ev : c->ev)
        if ((e = hipEventCreate(&ev)) != hipSuccess) return bail(e, "hipEventCreate");
    *out = c;
    return LCHD_OK;
}

extern "C" void lchd_ctx_destroy(lchd_ctx* c) {
    if (!c) return;
    CTX_GUARD(c);
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(c->ws);
    (void)hipFree(c->d_blob);
    (void)hipFree(c->d_cfg);
    (void)hipFree(c->d_status);
    (void)hipFree(c->d_points);
    (void)hipFree(c->d_tabs);
    (void)hipFree(c->d_powtab);
    (void)hipFree(c->d_wide_scratch);
    (void)hipFree(c->d_done);
    (void)hipFree(c->d_left);
    (void)hipFree(c->d_io);
    (void)hipFree(c->d_ovf_bits);
    (void)hipFree(c->d_ovf_lists);
    (void)hipFree(c->d_radial_bounds);
    (void)hipFree(c->d_indexed);
    (void)hipFree(c->d_cross);
    (void)hipFree(c->d_grad);
    (void)hipFree(c->d_grad_acc);
    (void)hipFree(c->d_shard);
    (void)hipFree(c->d_bad);
    if (c->shard_stream) (void)hipStreamDestroy(c->shard_stream);
    if (c->shard_ev) (void)hipEventDestroy(c->shard_ev);
    if (c->shard_sel_ev) (void)hipEventDestroy(c->shard_sel_ev);
    if (c->h_counts) (void)hipHostFree(c->h_counts);
    if (c->h_io) (void)hipHostFree(c->h_io);
    if (c->h_status) (void)hipHostFree(c->h_status);
    for (auto& ev : c->ev)
        if (ev) (void)hipEventDestroy(ev);
    delete c;
}

extern "C" int lchd_ctx_set_stream(lchd_ctx* c, void* s) {
    CTX_LOCK(c);
    if (!c) return fail(LCHD_EVALUE, "null context");
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    CTX_GUARD(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->stream = reinterpret_cast<hipStream_t>(s);
    return LCHD_OK;
}

extern "C" int lchd_ctx_enable_timing(lchd_ctx* c, int32_t on) {
    CTX_LOCK(c);
    if (!c) return fail(LCHD_EVALUE, "null context");
    c->timing = on != 0;
    return LCHD_OK;
}
extern "C" double lchd_ctx_last_ms(lchd_ctx* c, const char* phase) {
    CTX_LOCK(c);
    static const char* names[PH_N] = {"cells", "anchors", "env", "sweep"};
    if (!c || !phase) return -1.0;
    for (int i = 0; i < PH_N; ++i)
        if (!strcmp(phase, names[i])) return c->ms[i];
    return -1.0;
}
extern "C" int64_t lchd_ctx_last_env_points(lchd_ctx* c) {
    CTX_LOCK(c);
    if (!c || !c->last_valid || c->pend.active) return -1;
    CTX_GUARD(c);
    launch_env_points(c->stream, c->last, c->d_points);
    unsigned long long v = 0;
    if (hipMemcpyAsync(&v, c->d_points, sizeof v, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return -1;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    return (int64_t)v;
}

extern "C" int lchd_ctx_last_grid(lchd_ctx* c, int32_t side, int32_t dims_out[3], int64_t* n_cells_out, int32_t* build_out) {
    CTX_LOCK(c);
    if (!c || !c->last_valid || c->pend.active || side < 0 || side > 1) return -1;
    const GridRecord& g = c->last_grid[side];
    for (int k = 0; k < 3; ++k)
        if (dims_out) dims_out[k] = g.dim[k];
    if (n_cells_out) *n_cells_out = g.n_cells;
    if (build_out) *build_out = g.build;
    return 0;
}

extern "C" int lchd_ctx_last_anchors(lchd_ctx* c, int32_t side, int64_t* n_unique_out, int32_t* mode_out, int64_t* n_repeated_out) {
    CTX_LOCK(c);
    if (!c || !c->last_valid || c->pend.active || side < 0 || side > 1) return -1;
    const AnchorRecord& r = c->last_anchors[side];
    if (n_unique_out) *n_unique_out = r.n_unique;
    if (mode_out) *mode_out = r.mode;
    if (n_repeated_out) *n_repeated_out = r.n_repeated;
    return 0;
}

extern "C" int lchd_ctx_last_sweep(lchd_ctx* c, lchd_sweep_plan* plan_out, int64_t stats_out[4], int32_t* rule_out, int32_t* repeated_out) {
    CTX_LOCK(c);
    if (!c || !c->last_sweep_valid || c->pend.active) return -1;
    const SweepRecord& r = c->last_sweep;
    if (plan_out) *plan_out = r.plan;
    for (int k = 0; k < 4; ++k)
        if (stats_out) stats_out[k] = r.stats[k];
    if (rule_out) *rule_out = r.rule;
    if (repeated_out) *repeated_out = r.repeated;
    return 0;
}

// One sweep family for every pair: the one-pair-per-wavefront k_sweep that reads its square-root tables from global memory (tiles
// and per-lane chunks are functions of the pair alone), behind the row-sort kernels for dense rows.  No team sweeps, no
// one-launch small-call sweep, no launch-set hints from earlier passes, no fused dense kernel, no O(1) Kullback-Leibler / Renyi
// form: a pair's score then depends on the pair and the configuration only -- not on the other pairs of the call, on what the
// context scored before, or on whether the pair was reached through a second pass.  (Environments of more than 65 535 points
// still take the 64-bit-count sweep, whatever the mode.)
extern "C" int lchd_ctx_set_deterministic(lchd_ctx* c, int32_t on) {
    CTX_LOCK(c);
    if (!c) return fail(LCHD_EVALUE, "null context");
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    c->deterministic = on != 0;
    c->tune = c->tune_env;
    if (c->deterministic) {
        Tuning& t = c->tune;
        t.no_duo = t.no_count8 = t.no_c8_team = t.no_inline_meta = t.force_bigenv = t.no_dense_fused = t.no_sd_inc = t.no_sweep_hint = true;
    }
    c->hints.sweep_hint = 0;
    return LCHD_OK;
}
extern "C" int32_t lchd_ctx_get_deterministic(lchd_ctx* c) { CTX_LOCK(c); return (c && c->deterministic) ? 1 : 0; }

extern "C" int lchd_ctx_last_dense(lchd_ctx* c, lchd_dense_record* record_out) {
    CTX_LOCK(c);
    if (!c || !record_out || !c->last_dense_valid) return -1;
    *record_out = c->last_dense;
    return 0;
}
extern "C" int32_t lchd_ctx_last_dense_fused(lchd_ctx* c) {
    CTX_LOCK(c);
    return (c && c->last_dense_valid && c->last_dense.plan.path == LCHD_DENSE_FUSED) ? 1 : 0;
}
extern "C" int64_t lchd_ctx_pass_count(lchd_ctx* c) { CTX_LOCK(c); return c ? c->n_passes : -1; }

extern "C" int lchd_ctx_set_config(lchd_ctx* c, const lchd_config* cfg) {
    CTX_LOCK(c);
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context/config");
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    CTX_GUARD(c);
    const int C = cfg->n_categories;
    if (C <= 0) return fail(LCHD_EVALUE, "The number of possible categories (primitive types) cannot be zero!");
    if (C > kHugeCategories)
        return fail(LCHD_EUNSUPPORTED, "at most %d categories are supported (category ids travel as 16 bits on the device; got %d)", kHugeCategories, C);
    if (C > kWideCategories) {
        // beyond what the sweep's per-lane count columns fit in LDS: a global-memory scratch block per workgroup (k_sweep_wide<.., HUGE>),
        // up to 1 GB of them (256 workgroups at most, 8 at least)
        const size_t per = wide_scratch_bytes_per_wave(C);
        const int waves = (int)std::max<size_t>(8, std::min<size_t>(256, ((size_t)1 << 30) / per));
        if (c->wide_scratch_cap < per * (size_t)waves) {
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (c->d_wide_scratch) (void)hipFree(c->d_wide_scratch);
            c->d_wide_scratch = nullptr;
            c->wide_scratch_cap = 0;
            if (hipMalloc(&c->d_wide_scratch, per * (size_t)waves) != hipSuccess) {
                (void)hipGetLastError();
                return fail(LCHD_EUNSUPPORTED, "%d categories need %zu bytes of sweep scratch on the device", C, per * (size_t)waves);
            }
            c->wide_scratch_cap = per * (size_t)waves;
        }
        c->wide_scratch_waves = waves;
    }
    if (int rc = lchd_config_validate(C, C, cfg->category_weights, C)) return rc;
    if (cfg->n_weight_functions <= 0) return fail(LCHD_EVALUE, "at least one weight function is required");
    if (int rc = lchd_sd_validate(cfg->sd_kind, cfg->sd_n_params)) return rc;
    size_t n_params = 0;
    for (int i = 0; i < cfg->n_weight_functions; ++i) {
        const lchd_weight_function& w = cfg->weight_functions[i];
        if (int rc = lchd_wf_validate(w.kind, w.params, w.n_params)) return rc;
        n_params += (size_t)w.n_params;
    }
    // blob: [cat_w][wf entries][wf params][F(+inf) per wf][reciprocal of the CDF's constant divisor per wf][tag pairs]
    const size_t o_w = 0, o_e = o_w + sizeof(double) * C, o_p = o_e + sizeof(WfEntry) * cfg->n_weight_functions;
    const size_t o_f = o_p + sizeof(double) * n_params, o_i = o_f + sizeof(double) * cfg->n_weight_functions;
    const size_t o_t = o_i + sizeof(double) * cfg->n_weight_functions;
    const size_t total = o_t + sizeof(uint64_t) * (size_t)cfg->n_tag_pairs;
    std::vector<char> blob(total + 8);
    c->finf_differ = false;
    memcpy(blob.data() + o_w, cfg->category_weights, sizeof(double) * C);
    WfEntry* ent = reinterpret_cast<WfEntry*>(blob.data() + o_e);
    double* prm = reinterpret_cast<double*>(blob.data() + o_p);
    double* finf = reinterpret_cast<double*>(blob.data() + o_f);
    double* winv = reinterpret_cast<double*>(blob.data() + o_i);
    int off = 0;
    for (int i = 0; i < cfg->n_weight_functions; ++i) {
        const lchd_weight_function& w = cfg->weight_functions[i];
        ent[i] = WfEntry{w.kind, w.n_params, off, 0};
        memcpy(prm + off, w.params, sizeof(double) * w.n_params);
        finf[i] = cdf_eval(w.kind, w.params, w.n_params, (double)INFINITY);
        if (i > 0 && !(finf[i] == finf[0])) c->finf_differ = true;  // (set to false above)
        // hyper_exp divides by sum_i a_i, uniform / kumaraswamy by (x_max - x_min) (cdfs.rs:15-20,44,61): constants of the
        // weight function, so the kernels multiply by the reciprocal (<= 1 ulp from the quotient) instead of dividing per point
        winv[i] = 1.0;
        if (w.kind == LCHD_WF_HYPER_EXP) {
            double norm = 0.0;
            for (int k = 0; k < w.n_params / 2; ++k) norm += w.params[k];
            winv[i] = 1.0 / norm;
        } else if (w.kind == LCHD_WF_UNIFORM || w.kind == LCHD_WF_KUMARASWAMY) {
            winv[i] = 1.0 / (w.params[1] - w.params[0]);
        }
        off += w.n_params;
    }
    uint64_t* tp = reinterpret_cast<uint64_t*>(blob.data() + o_t);
    for (int64_t i = 0; i < cfg->n_tag_pairs; ++i)
        tp[i] = ((uint64_t)(uint32_t)cfg->tag_pairs[2 * i] << 32) | (uint32_t)cfg->tag_pairs[2 * i + 1];
    std::sort(tp, tp + cfg->n_tag_pairs);
    // the words of DevConfig that are not in the blob, appended so that ONE comparison decides whether anything changed
    const int32_t extra[10] = {C, cfg->n_weight_functions, cfg->sd_kind, cfg->sd_n_params, cfg->tag_mode, cfg->tag_accept_same,
                               cfg->tag_accepted_pairs, cfg->tag_ordered, (int32_t)cfg->n_tag_pairs, 0};
    std::vector<char> sig(blob.begin(), blob.begin() + total);
    sig.insert(sig.end(), reinterpret_cast<const char*>(extra), reinterpret_cast<const char*>(extra) + sizeof extra);
    sig.insert(sig.end(), reinterpret_cast<const char*>(cfg->sd_params), reinterpret_cast<const char*>(cfg->sd_params) + sizeof cfg->sd_params);
    if (c->cfg_set && sig == c->cfg_blob_host) return LCHD_OK;  // same configuration as the last call: already on the device
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (total + 8 > c->blob_cap) {
        if (c->d_blob) HIP_TRY(hipFree(c->d_blob));
        c->d_blob = nullptr;
        HIP_TRY(hipMalloc(&c->d_blob, total + 4096));
        c->blob_cap = total + 4096;
    }
    HIP_TRY(hipMemcpy(c->d_blob, blob.data(), total, hipMemcpyHostToDevice));
    c->cfg_set = false;
    c->hints.sweep_hint = 0;  // another configuration: what the last pass looked like says nothing about the next
    c->hints.b_use_once = false;
    c->cfg_blob_host.swap(sig);
    DevConfig h{};
    h.n_categories = C;
    h.n_wf = cfg->n_weight_functions;
    h.sd_kind = cfg->sd_kind;
    h.tag_mode = cfg->tag_mode;
    h.tag_accept_same = cfg->tag_accept_same;
    h.tag_accepted_pairs = cfg->tag_accepted_pairs;
    h.tag_ordered = cfg->tag_ordered;
    h.n_tag_pairs = (int32_t)cfg->n_tag_pairs;
    h.sd_p0 = cfg->sd_n_params > 0 ? cfg->sd_params[0] : 0.0;
    h.sd_p1 = cfg->sd_n_params > 1 ? cfg->sd_params[1] : 0.0;
    h.cat_w = reinterpret_cast<const double*>(c->d_blob + o_w);
    h.wf = reinterpret_cast<const WfEntry*>(c->d_blob + o_e);
    h.wf_params = reinterpret_cast<const double*>(c->d_blob + o_p);
    h.wf_finf = reinterpret_cast<const double*>(c->d_blob + o_f);
    h.wf_inv = reinterpret_cast<const double*>(c->d_blob + o_i);
    h.tag_pairs = reinterpret_cast<const uint64_t*>(c->d_blob + o_t);
    h.pow_tab = nullptr;
    if (cfg->sd_kind == LCHD_SD_HELLINGER && cfg->sd_params[0] != 2.0) {  // power tables of the general-exponent Hellinger distance
        if (!c->d_powtab) HIP_TRY(hipMalloc(&c->d_powtab, sizeof(double) * 2 * 65536));
        if (c->powtab_e != cfg->sd_params[0]) {
            launch_fill_pow_tables(c->stream, c->d_powtab, cfg->sd_params[0]);
            HIP_TRY(hipGetLastError());
            c->powtab_e = cfg->sd_params[0];
        }
        h.pow_tab = c->d_powtab;
    }
    HIP_TRY(hipMemcpy(c->d_cfg, &h, sizeof h, hipMemcpyHostToDevice));
    c->h_cfg = h;
    c->hellinger2 = (cfg->sd_kind == LCHD_SD_HELLINGER && cfg->sd_params[0] == 2.0);
    c->unit_weights = std::all_of(cfg->category_weights, cfg->category_weights + C, [](double v) { return v == 1.0; });
    // k_sweep_inc drops terms of second order in eps * (largest count): eps <= 1e-9 keeps them below 3e-13.  Renyi: a moderate order
    // (the tables hold k^alpha for k <= 512) and a finite eps^(1 - alpha); alpha = 1 is the Kullback-Leibler form (:36-38).
    c->sd_fast = 0;
    if (c->unit_weights) {
        if (cfg->sd_kind == LCHD_SD_KULLBACK_LEIBLER && cfg->sd_params[0] > 0.0 && cfg->sd_params[0] <= 1e-9) c->sd_fast = 1;
        if (cfg->sd_kind == LCHD_SD_RENYI && cfg->sd_params[1] > 0.0 && cfg->sd_params[1] <= 1e-9) {
            const double al = cfg->sd_params[0];
            if (al == 1.0) c->sd_fast = 1;
            else if (al >= 0.01 && al <= 20.0 && std::isfinite(std::pow(cfg->sd_params[1], 1.0 - al)) && std::pow(cfg->sd_params[1], 1.0 - al) < 1e250 &&
                     cfg->sd_params[1] * 512.0 * std::max(1.0, std::fabs(al - 1.0)) <= 1e-6)
                c->sd_fast = 2;
        }
        // Kolmogorov-Smirnov on unit weights: max_c |a_c N_b - b_c N_a| / (N_a N_b) on integer counts (the KSM team sweep)
        if (cfg->sd_kind == LCHD_SD_KOLMOGOROV_SMIRNOV) c->sd_fast = 3;
    }
    c->wf_np_max = 0;
    c->wf_finf_off = false;
    for (int i = 0; i < cfg->n_weight_functions; ++i) {
        c->wf_np_max = std::max(c->wf_np_max, (int)cfg->weight_functions[i].n_params);
        c->wf_finf_off = c->wf_finf_off || !(finf[i] == 1.0);
    }
    c->wf_pow = false;
    for (int i = 0; i < cfg->n_weight_functions; ++i)
        c->wf_pow = c->wf_pow || cfg->weight_functions[i].kind == LCHD_WF_DAGUM || cfg->weight_functions[i].kind == LCHD_WF_KUMARASWAMY ||
                    (cfg->weight_functions[i].kind == LCHD_WF_HYPER_EXP && cfg->weight_functions[i].n_params > 8);  // not register-resident
    c->cfg_set = true;
    return LCHD_OK;
}

// ------------------------------------------------------------------------------------------------
// clouds
// ------------------------------------------------------------------------------------------------
static int upload_coords(lchd_ctx* c, lchd_cloud* cl, const double* xyz) {
    const int64_t n = cl->n;
    std::vector<double> soa((size_t)3 * n);
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            const double v = xyz[3 * i + k];
            if (!std::isfinite(v)) return fail(LCHD_EVALUE, "non-finite coordinate at atom %lld", (long long)i);
            soa[(size_t)k * n + i] = v;
            mn[k] = std::min(mn[k], v);
            mx[k] = std::max(mx[k], v);
        }
    for (int k = 0; k < 3; ++k) { cl->bbmin[k] = n ? mn[k] : 0.0; cl->bbmax[k] = n ? mx[k] : 0.0; }
    if (n) {
        HIP_TRY(hipMemcpyAsync(cl->x, soa.data(), sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(cl->y, soa.data() + n, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(cl->z, soa.data() + 2 * n, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return LCHD_OK;
}

// Category ids travel as one byte (255 = not in the category map) -- or, as soon as an id beyond 254 occurs (more than 255
// categories), as two: low byte | high byte, 0xFFFF = not in the map.
static bool cats_need_hi(const int32_t* cat, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (cat[i] >= 255 && cat[i] < 65535) return true;
    return false;
}
static void cats_encode(const int32_t* cat, int64_t n, uint8_t* lo, uint8_t* hi /* or nullptr */) {
    for (int64_t i = 0; i < n; ++i) {
        if (hi) {
            const uint32_t v = (cat[i] >= 0 && cat[i] < 65535) ? (uint32_t)cat[i] : 0xFFFFu;
            lo[i] = (uint8_t)(v & 255u);
            hi[i] = (uint8_t)(v >> 8);
        } else {
            lo[i] = (cat[i] >= 0 && cat[i] < 255) ? (uint8_t)cat[i] : (uint8_t)255;
        }
    }
}

extern "C" int lchd_cloud_create(lchd_ctx* c, const double* xyz, const int32_t* cat, const int32_t* tag, int64_t n, lchd_cloud** out) {
    CTX_LOCK(c);
    if (!c || !out) return fail(LCHD_EVALUE, "null context");
    *out = nullptr;
    if (n < 0 || n > (int64_t)1 << 30) return fail(LCHD_EUNSUPPORTED, "cloud size %lld out of range", (long long)n);
    if (n > 0 && !cat) return fail(LCHD_EVALUE, "null category array");
    CTX_GUARD(c);
    lchd_cloud* cl = new lchd_cloud();
    cl->n = n;
    const size_t m = (size_t)std::max<int64_t>(n, 1);
    auto bail = [&](hipError_t e, const char* what) {  // nothing allocated so far outlives a failed call
        lchd_cloud_destroy(c, cl);
        return fail(LCHD_EDEVICE, "HIP error %d (%s) in lchd_cloud_create: %s", (int)e, hipGetErrorName(e), what);
    };
    hipError_t e;
    if ((e = hipMalloc(&cl->x, sizeof(double) * m)) != hipSuccess) return bail(e, "hipMalloc(x)");
    if ((e = hipMalloc(&cl->y, sizeof(double) * m)) != hipSuccess) return bail(e, "hipMalloc(y)");
    if ((e = hipMalloc(&cl->z, sizeof(double) * m)) != hipSuccess) return bail(e, "hipMalloc(z)");
    if ((e = hipMalloc(&cl->cat, m)) != hipSuccess) return bail(e, "hipMalloc(cat)");
    if ((e = hipMalloc(&cl->tag, sizeof(int32_t) * m)) != hipSuccess) return bail(e, "hipMalloc(tag)");
    if (xyz) {
        if (int rc = upload_coords(c, cl, xyz)) { lchd_cloud_destroy(c, cl); return rc; }
    } else {
        if ((e = hipMemsetAsync(cl->x, 0, sizeof(double) * m, c->stream)) != hipSuccess) return bail(e, "hipMemset(x)");
        if ((e = hipMemsetAsync(cl->y, 0, sizeof(double) * m, c->stream)) != hipSuccess) return bail(e, "hipMemset(y)");
        if ((e = hipMemsetAsync(cl->z, 0, sizeof(double) * m, c->stream)) != hipSuccess) return bail(e, "hipMemset(z)");
    }
    if (n) {
        const bool wide = cats_need_hi(cat, n);
        std::vector<uint8_t> c8((size_t)n), c8h(wide ? (size_t)n : 0);
        cats_encode(cat, n, c8.data(), wide ? c8h.data() : nullptr);
        if ((e = hipMemcpy(cl->cat, c8.data(), (size_t)n, hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "hipMemcpy(cat)");
        if (wide) {
            if ((e = hipMalloc(&cl->cat_hi, (size_t)n)) != hipSuccess) return bail(e, "hipMalloc(cat_hi)");
            if ((e = hipMemcpy(cl->cat_hi, c8h.data(), (size_t)n, hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "hipMemcpy(cat_hi)");
            cats_encode(cat, n, c8.data(), nullptr);  // the one-byte view: ids beyond 254 are outside every map of at most 255 categories
            if ((e = hipMalloc(&cl->cat_narrow, (size_t)n)) != hipSuccess) return bail(e, "hipMalloc(cat_narrow)");
            if ((e = hipMemcpy(cl->cat_narrow, c8.data(), (size_t)n, hipMemcpyHostToDevice)) != hipSuccess) return bail(e, "hipMemcpy(cat_narrow)");
        }
        if (tag) e = hipMemcpy(cl->tag, tag, sizeof(int32_t) * n, hipMemcpyHostToDevice);
        else e = hipMemset(cl->tag, 0, sizeof(int32_t) * n);
        if (e != hipSuccess) return bail(e, "tags");
    }
    // (the copies and fills above went through the null stream; the context may launch on a non-blocking stream that is not
    // ordered behind it: creating a structure is rare, so simply wait for the device)
    if ((e = hipDeviceSynchronize()) != hipSuccess) return bail(e, "hipDeviceSynchronize");
    *out = cl;
    return LCHD_OK;
}

extern "C" int lchd_cloud_create_batch(lchd_ctx* c, const double* xyz, const int32_t* cat, const int32_t* tag, const int32_t* sid,
                                       int64_t n, int32_t n_struct, lchd_cloud** out) {
    CTX_LOCK(c);
    if (!c || !out) return fail(LCHD_EVALUE, "null context");
    if (n_struct < 1 || !sid) return fail(LCHD_EVALUE, "a batch needs n_struct >= 1 and a structure id per atom");
    for (int64_t i = 0; i < n; ++i)
        if (sid[i] < 0 || sid[i] >= n_struct) return fail(LCHD_EVALUE, "structure id %d of atom %lld is outside [0, %d)", sid[i], (long long)i, n_struct);
    CTX_GUARD(c);
    lchd_cloud* cl = nullptr;
    if (int rc = lchd_cloud_create(c, xyz, cat, tag, n, &cl)) return rc;
    cl->n_struct = n_struct;
    if (n && n % n_struct == 0 && n / n_struct <= INT32_MAX) {  // regular batch: equal-sized structures stored one after the other?
        const int64_t k = n / n_struct;
        bool regular = true;
        for (int64_t i = 0; i < n && regular; ++i) regular = sid[i] == (int32_t)(i / k);
        cl->struct_size = regular ? (int32_t)k : 0;
    }
    if (n) {
        hipError_t e = hipMalloc(&cl->sid, sizeof(int32_t) * n);
        if (e == hipSuccess) e = hipMemcpy(cl->sid, sid, sizeof(int32_t) * n, hipMemcpyHostToDevice);
        if (e != hipSuccess) { lchd_cloud_destroy(c, cl); return fail(LCHD_EDEVICE, "HIP error %d while uploading structure ids", (int)e); }
    }
    *out = cl;
    return LCHD_OK;
}

extern "C" int64_t lchd_cloud_size(const lchd_cloud* cl) { return cl ? cl->n : -1; }
extern "C" int32_t lchd_cloud_structures(const lchd_cloud* cl) { return cl ? cl->n_struct : -1; }

extern "C" int lchd_cloud_set_coords(lchd_ctx* c, lchd_cloud* cl, const double* xyz) {
    CTX_LOCK(c);
    if (!c || !cl || !xyz) return fail(LCHD_EVALUE, "null argument");
    if (c->pend.active && (c->pend.req.a == cl || c->pend.req.b == cl))
        return fail(LCHD_EVALUE, "this structure is in use by an unfinished asynchronous call");
    if (cl->images) return fail(LCHD_EVALUE, "an image cloud takes its coordinates from its source (lchd_cloud_update_images)");
    CTX_GUARD(c);
    return upload_coords(c, cl, xyz);
}

extern "C" void lchd_cloud_destroy(lchd_ctx* c, lchd_cloud* cl) {
    CTX_LOCK(c);
    if (!cl) return;
    DeviceGuard device_guard_(c ? c->device : -1);
    if (c) (void)hipStreamSynchronize(c->stream);
    (void)hipFree(cl->x);
    (void)hipFree(cl->y);
    (void)hipFree(cl->z);
    (void)hipFree(cl->cat);
    (void)hipFree(cl->cat_hi);
    (void)hipFree(cl->cat_narrow);
    (void)hipFree(cl->tag);
    (void)hipFree(cl->sid);
    (void)hipFree(cl->d_raw);
    (void)hipFree(cl->d_bbox);
    (void)hipFree(cl->d_bbox_part);
    (void)hipFree(cl->d_src_start);
    (void)hipFree(cl->d_src_idx);
    (void)hipFree(cl->d_tiles);
    (void)hipFree(cl->d_raw32);
    (void)hipFree(cl->d_img_count);
    (void)hipFree(cl->d_img_offset);
    (void)hipFree(cl->d_img_spans);
    (void)hipFree(cl->d_img_origin);
    (void)hipFree(cl->d_img_code);
    (void)hipFree(cl->d_boxes);
    (void)hipFree(cl->d_cells);
    if (cl->h_pinned32) (void)hipHostFree(cl->h_pinned32);
    if (cl->h_pinned) (void)hipHostFree(cl->h_pinned);
    if (cl->ev_ready) (void)hipEventDestroy(cl->ev_ready);
    if (cl->ev_used) (void)hipEventDestroy(cl->ev_used);
    if (cl->ev_t0) (void)hipEventDestroy(cl->ev_t0);
    if (cl->ev_t1) (void)hipEventDestroy(cl->ev_t1);
    delete cl;
}

// ------------------------------------------------------------------------------------------------
// status -> reference error classes
// ------------------------------------------------------------------------------------------------
enum Driver { DRV_ANCHORS, DRV_DMXS, DRV_PRIMS };

static int status_to_rc(uint32_t f, Driver drv) {
    if (f == 0) return LCHD_OK;
    if (f & ST_BAD_ANCHOR) return fail(LCHD_EPANIC, "index out of bounds: an anchor index is outside its structure (src/locohd.rs:521)");
    if (f & ST_EMPTY_ENV) return fail(LCHD_EPANIC, "index out of bounds: an environment is empty (src/locohd.rs:74)");
    if (f & ST_BAD_WF) return fail(LCHD_EVALUE, "weight-function index out of range");
    if (drv == DRV_ANCHORS) {
        if (f & ST_FIRST_NOT_ZERO) return fail(LCHD_EVALUE, "The dists list must start with a distance of 0!");
        if (f & ST_BAD_CATEGORY) return fail(LCHD_EVALUE, "Category not found!");
        if (f & ST_ZERO_NORM) return fail(LCHD_EVALUE, "Zero norm error for PMF");
    }
    if (f & (ST_FIRST_NOT_ZERO | ST_BAD_CATEGORY | ST_ZERO_NORM | ST_BAD_DISTANCE))
        return fail(LCHD_EVALUE, drv == DRV_PRIMS ? "The from_anchors function returned an error during the LoCoHD calculations!"
                                                  : "The stat_dist_integral function returned an error during the LoCoHD calculations!");
    return fail(LCHD_EDEVICE, "unexpected device status 0x%x", f);
}

// Status protocol of a pass.  begin_pass: the device status is clean unless a pass was abandoned half-way; the host-mapped
// mirror's error words and sequence number are reset by the CPU (no pass is in flight).  After the stream has been waited
// for, pass_flags() = what the kernels up to the record pass reported (snapshot by k_pair_meta) | what the sweeps reported.
static int begin_pass(lchd_ctx* c) {
    if (c->status_dirty) {
        HIP_TRY(hipMemsetAsync(c->d_status, 0, sizeof(DeviceStatus), c->stream));
        HIP_TRY(hipMemsetAsync(c->d_done, 0, sizeof(DoneState), c->stream));
        HIP_TRY(hipMemsetAsync(c->d_left, 0, 256, c->stream));
        c->status_dirty = false;
    }
    HostStatus* h = c->h_status;
    for (uint32_t& w : h->sweep_flags) w = 0u;
    h->flags = 0u;
    h->max_env = 0u;
    h->snapshot_seq = 0u;
    c->seq = c->seq == 0xFFFFFFFFu ? 1u : c->seq + 1u;
    return LCHD_OK;
}
static int pass_flags(lchd_ctx* c, uint32_t* flags) {
    const HostStatus* h = c->h_status;
    if (h->snapshot_seq != c->seq) {  // the record pass never ran to its end
        c->status_dirty = true;
        return fail(LCHD_EDEVICE, "the device did not complete the pass (status snapshot %u, expected %u)", h->snapshot_seq, c->seq);
    }
    uint32_t f = h->flags;
    for (int k = 0; k < 8; ++k)
        if (h->sweep_flags[k]) f |= 1u << k;
    *flags = f;
    return LCHD_OK;
}
static int wait_pass(lchd_ctx* c, uint32_t* flags) {
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        c->status_dirty = true;
        return fail(LCHD_EDEVICE, "HIP error %d (%s) while waiting for the pass", (int)e, hipGetErrorName(e));
    }
    return pass_flags(c, flags);
}

static void mark(lchd_ctx* c, int i) {
    if (c->timing) (void)hipEventRecord(c->ev[i], c->stream);
}
static void collect_times(lchd_ctx* c, int first, int last) {
    for (int i = 0; i < PH_N; ++i) c->ms[i] = -1.f;
    if (!c->timing) return;
    for (int i = first; i < last; ++i) {
        float t = -1.f;
        if (hipEventElapsedTime(&t, c->ev[i], c->ev[i + 1]) == hipSuccess) c->ms[i] = t;
    }
}

// ------------------------------------------------------------------------------------------------
// from_primitives on device-resident clouds
// ------------------------------------------------------------------------------------------------
struct GridPlan {
    double min[3], inv[3];
    int dim[3];
    int n_cells;
};

// The grid of one side of a thresholded pass: a pure function of the bounding box, the structure count, the threshold and the
// neighbourhood reach of the environment kernel (no context, no device).
extern "C" int lchd_plan_grid(const double bbmin[3], const double bbmax[3], int32_t n_struct, double thr, int32_t reach,
                              int32_t dims_out[3], double cell_out[3], int64_t* n_cells_out) {
    if (!bbmin || !bbmax || !dims_out || !cell_out || !n_cells_out) return fail(LCHD_EVALUE, "null argument");
    if (n_struct < 1 || reach < 1 || !(thr > 0.0)) return fail(LCHD_EVALUE, "lchd_plan_grid: n_struct >= 1, reach >= 1 and thr > 0 are required");
    // cells are at least (1 + 1e-9) * thr / reach wide so that |dx| < thr can never leave the (2 reach + 1)^3 neighbourhood of
    // the anchor's cell through rounding (reach 1: k_env_cells / k_env_collect; reach 2: k_env_group)
    const double cell0 = thr / reach * (1.0 + 1e-9);
    int dim[3];
    long long total = 1;
    for (int k = 0; k < 3; ++k) {
        const double ext = bbmax[k] - bbmin[k];
        double nd = std::floor(ext / cell0);
        if (!(nd >= 1.0)) nd = 1.0;
        if (nd > 1024.0) nd = 1024.0;
        dim[k] = (int)nd;
        total *= dim[k];
    }
    total *= n_struct;
    while (total > (1ll << 23)) {  // bound the cell arrays (8M cells): coarsen the largest axis
        int k = (dim[0] >= dim[1] && dim[0] >= dim[2]) ? 0 : (dim[1] >= dim[2] ? 1 : 2);
        if (dim[k] == 1) break;
        total /= dim[k];
        dim[k] = (dim[k] + 1) / 2;
        total *= dim[k];
    }
    for (int k = 0; k < 3; ++k) {
        const double ext = bbmax[k] - bbmin[k];
        dims_out[k] = dim[k];
        cell_out[k] = ext > 0.0 ? ext / dim[k] : 1.0;
    }
    *n_cells_out = (int64_t)n_struct * dim[0] * dim[1] * dim[2];
    return LCHD_OK;
}

// Which kernel sorts the dense rows of a call: plan_dense (lchd_dense_plan.h), the decision dense_pass and ensemble_core follow.
extern "C" int lchd_plan_dense(const lchd_dense_query* query, lchd_dense_plan* plan_out) {
    if (!query || !plan_out) return fail(LCHD_EVALUE, "null argument");
    if (!dense_query_ok(*query)) return fail(LCHD_EVALUE, "lchd_plan_dense: n_categories >= 1, attempt 0 or 1 and known hook bits are required");
    *plan_out = plan_dense(*query);
    return LCHD_OK;
}
// Which sweep kernels a pass launches: plan_sweep (lchd_kernels.hip), the decision launch_sweep follows.
extern "C" int lchd_plan_sweep(const lchd_sweep_query* query, lchd_sweep_plan* plan_out) {
    if (!query || !plan_out) return fail(LCHD_EVALUE, "null argument");
    if (query->n_pairs < 1 || query->n_categories < 1) return fail(LCHD_EVALUE, "lchd_plan_sweep: n_pairs >= 1 and n_categories >= 1 are required");
    if (!plan_sweep(*query, *plan_out)) return fail(LCHD_EDEVICE, "lchd_plan_sweep: internal error: the launch set %u would not give every pair exactly one kernel", plan_out->families);
    return LCHD_OK;
}

static GridPlan plan_grid(const lchd_cloud* cl, double thr, int reach) {
    GridPlan g{};
    int32_t dim[3];
    double cell[3];
    int64_t n_cells = 0;
    (void)lchd_plan_grid(cl->bbmin, cl->bbmax, cl->n_struct, thr, reach, dim, cell, &n_cells);
    for (int k = 0; k < 3; ++k) {
        g.min[k] = cl->bbmin[k];
        g.dim[k] = dim[k];
        g.inv[k] = 1.0 / (cell[k] * (1.0 + 1e-12));
    }
    g.n_cells = (int)n_cells;
    return g;
}

struct SideBufs {
    uint32_t *cell_of, *cell_count, *cell_start, *pos_of, *slot, *scan_tmp, *bits, *wpre, *chunk_base;
    uint8_t* flag8;
    AnchorRec* uniq;
    CellRec* rec;
    EnvStore env;
    double* raw_key;   // environments of more than 16384 points: unsorted scratch rows (k_env_collect)
    uint8_t* raw_cat;
    uint32_t* ovf_list;  // slots of the environments that overflowed (EnvSide::ovf_list)
};

// Workspace layout of one pass.  Everything that must be zero when the prologue starts -- the general cell list's counters
// and the anchor flags of both sides -- is carved as ONE contiguous region (flags_a, flags_b last), so at most one memset
// precedes the kernels.  Who zeroes it (launch_prologue):
//   fused            nobody: the flags are an LDS bit set and the general counters are not used.  One exception: a side B without
//                    de-duplication keeps its repeat bit set in flags_b (k_pair_anchor_recs), and side B's workgroup of
//                    k_prologue_fused clears those (n_b + 31) / 32 words
//   per structure    (both sides) the spare workgroups of k_cells_struct2 zero flags_a .. the end of the region
//   anything else    one memset over the whole region
struct PassBufs {
    SideBufs a, b;
    int4* pair_meta;
    uint32_t* left_list;  // pairs the team kernel's rule leaves over (SweepArgs::left_list)
    char* zero_base;
    size_t zero_bytes;
};
static void carve_pass(Arena& ar, const PassQuery& q, const PassPlan& plan, int cells_a, int cells_b, PassBufs& pb) {
    const int cap = q.cap;
    const bool cat16 = plan.cat16;
    const size_t ma = (size_t)std::max<int64_t>(q.n_a, 1), mb = (size_t)std::max<int64_t>(q.n_b, 1);
    ar.off = (ar.off + 255) & ~size_t(255);
    const size_t z0 = ar.off;
    pb.a.cell_count = ar.take<uint32_t>((size_t)cells_a + 1);
    pb.b.cell_count = ar.take<uint32_t>((size_t)cells_b + 1);
    pb.a.flag8 = reinterpret_cast<uint8_t*>(ar.take<uint4>((ma + 31) / 32 * 2 + 2));  // one byte per atom, padded to whole 32-byte words
    pb.b.flag8 = reinterpret_cast<uint8_t*>(ar.take<uint4>((mb + 31) / 32 * 2 + 2));
    pb.zero_base = ar.dry ? nullptr : ar.base + z0;
    pb.zero_bytes = ar.off - z0;
    for (int side = 0; side < 2; ++side) {
        SideBufs& b = side ? pb.b : pb.a;
        const size_t m = side ? mb : ma;
        const int n_cells = side ? cells_b : cells_a;
        const size_t ne = (size_t)std::max<int64_t>(side ? plan.max_env_b : plan.max_env_a, 1);
        b.cell_of = ar.take<uint32_t>(m);
        b.slot = ar.take<uint32_t>(m + 1);
        b.bits = ar.take<uint32_t>((m + 31) / 32 + 1);
        b.wpre = ar.take<uint32_t>((m + 31) / 32 + 2);
        b.chunk_base = ar.take<uint32_t>((m >> 18) + 2);
        b.cell_start = ar.take<uint32_t>((size_t)n_cells + 1);
        b.rec = ar.take<CellRec>(m + kEnvGroupRecPad);  // (k_env_group reads up to 7 records past a cell row's end)
        b.pos_of = ar.take<uint32_t>(m);
        b.uniq = ar.take<AnchorRec>(ne);
        b.scan_tmp = ar.take<uint32_t>(std::max<size_t>(m, (size_t)n_cells) / 4096 + 4);
        b.env.key = ar.take<uint64_t>(ne * (size_t)cap * (size_t)std::max(plan.key_sets, 1));
        b.env.set_stride = (int64_t)(ne * (size_t)cap);
        b.env.cat = ar.take<uint8_t>(ne * (size_t)cap * (cat16 ? 2 : 1));
        b.env.len = ar.take<int32_t>(ne);
        b.env.cat0 = (cap == kEnvGroupCap && !cat16) ? ar.take<uint8_t>(ne) : nullptr;  // (written by k_env_group only: build_prims_store drops it otherwise)
        const int pw = plan.pre_words;  // prefix-count rows (k_env_group, configurations of at most 16 categories)
        b.env.pre = pw > 0 ? ar.take<uint64_t>(ne * (size_t)(cap / kPreStep) * (size_t)pw) : nullptr;  // (one row per kPreStep points)
        b.env.pre_words = pw;
        b.env.stride = cap;
        b.env.cdf_keys = 0;
        b.env.cat16 = cat16 ? 1 : 0;
        b.raw_key = cap > 16384 ? ar.take<double>(ne * (size_t)cap) : nullptr;
        b.raw_cat = cap > 16384 ? ar.take<uint8_t>(ne * (size_t)cap) : nullptr;
        b.ovf_list = cap <= 16384 ? ar.take<uint32_t>(ne) : nullptr;
    }
    pb.pair_meta = ar.take<int4>((size_t)q.n_pairs);
    pb.left_list = ar.take<uint32_t>((size_t)q.n_pairs);
}

// A frames buffer computes its bounding box on the device while it is being filled; fetch it before planning a grid.
static int resolve_bbox(lchd_ctx* c, lchd_cloud* cl) {
    if (!cl->bbox_pending) return LCHD_OK;
    HIP_TRY(hipEventSynchronize(cl->ev_ready));
    unsigned long long k[7];
    HIP_TRY(hipMemcpy(k, cl->d_bbox, sizeof k, hipMemcpyDeviceToHost));
    cl->bbox_pending = false;
    if (k[6]) return fail(LCHD_EVALUE, "non-finite coordinate in a trajectory frame");
    auto dec = [](unsigned long long u) { u = (u >> 63) ? (u ^ 0x8000000000000000ull) : ~u; double d; memcpy(&d, &u, 8); return d; };
    for (int q = 0; q < 3; ++q) { cl->bbmin[q] = dec(k[q]); cl->bbmax[q] = dec(k[3 + q]); }
    return LCHD_OK;
}

static void fill_sweep_args(lchd_ctx* c, SweepArgs& sw) {
    sw.cfg = c->d_cfg;
    sw.st = c->d_status;
    sw.hst = c->h_status;
    sw.seq = c->seq;
    sw.sd_fast = c->tune.no_sd_inc ? 0 : c->sd_fast;
    sw.sqrt_tab = c->d_tabs;
    sw.rsqrt_tab = c->d_tabs + 65536;
    sw.done = c->d_done;
    sw.wide_scratch = c->d_wide_scratch;
    sw.wide_scratch_per_wave = (int64_t)wide_scratch_bytes_per_wave(c->h_cfg.n_categories);
    sw.wide_scratch_waves = c->wide_scratch_waves;
}

// What plan_pass is asked about the pending request: its sizes, the configuration and the context's hooks and hints.
static PassQuery pass_query(const lchd_ctx* c) {
    const auto& R = c->pend.req;
    PassQuery q;
    q.n_a = R.a->n; q.n_b = R.b->n; q.n_pairs = R.n_pairs;
    q.same_object = R.a == R.b;
    q.has_wf_index = R.wf != nullptr;
    q.cap = R.cap; q.subset = R.subset;
    q.n_categories = c->h_cfg.n_categories; q.n_wf = c->h_cfg.n_wf;
    q.hellinger2 = c->hellinger2; q.sd_fast = c->sd_fast; q.unit_weights = c->unit_weights; q.finf_differ = c->finf_differ;
    q.deterministic = c->deterministic; q.tag_mode = c->h_cfg.tag_mode;
    q.tune = c->tune; q.hints = c->hints;
    return q;
}

// The grid of one side as the kernels read it, and the side as the prologue takes it.
static GridView grid_view(const GridPlan& g, const SideBufs& s) {
    GridView v{};
    for (int k = 0; k < 3; ++k) { v.min[k] = g.min[k]; v.inv[k] = g.inv[k]; v.cell[k] = 1.0 / g.inv[k]; v.dim[k] = g.dim[k]; }
    v.n_cells = g.n_cells;
    v.cell_start = s.cell_start;
    v.rec = s.rec;
    v.pos_of = s.pos_of;
    return v;
}
static PrepSide prep_side(const CloudView& cv, const GridView& gv, const SideBufs& sbuf) {
    PrepSide ps{};
    ps.c = cv; ps.g = gv;
    ps.cell_start = sbuf.cell_start; ps.rec = sbuf.rec; ps.pos_of = sbuf.pos_of;
    ps.cell_of = sbuf.cell_of; ps.cell_count = sbuf.cell_count; ps.scan_tmp = sbuf.scan_tmp;
    ps.flag8 = sbuf.flag8; ps.bits = sbuf.bits; ps.wpre = sbuf.wpre; ps.chunk_base = sbuf.chunk_base; ps.slot = sbuf.slot; ps.uniq = sbuf.uniq;
    return ps;
}

// The environment store of one thresholded pass, and what its consumer (a sweep: prims_enqueue; a profile kernel: consumer_prims_pass)
// reads next to it.
struct PrimsStore {
    bool begun = false;     // begin_pass has succeeded and the prologue is on the stream: the pass counts, and the members below describe it
    GridPlan grid[2];
    PassBufs pb{};          // (pb.a.env / pb.b.env: the stores as the environment kernels wrote them, set 0 first)
    EnvStore env[2];        // the stores as a consumer reads them: the F sets of a dictionary, else pb's
    int builds[2] = {0, 0}, dedup[2] = {0, 0};  // launch_prologue's builds_out / dedup_out
    size_t store_bytes = 0; // keys + categories of both sides
};

// The front half of a thresholded pass, shared by the scoring pass and the composition pass: grids -> workspace -> prologue ->
// environment kernel -> tie canonicalisation (deterministic mode) -> key sets of a dictionary; timing marks 0 to 3; no host
// synchronisation (the workspace only grows between passes).  `plan` is the caller's, amended as it sees fit.
// pairs: DEVICE [n_pairs][2], or null: the list is (anchors[p], anchors[p]), written into the workspace behind the pass's buffers.
static int build_prims_store(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int64_t* pairs, const int64_t* anchors, int64_t n_pairs,
                             double thr, const PassQuery& q, const PassPlan& plan, PrimsStore& st) {
    const bool same = plan.same, per_pair = plan.per_pair;
    const int64_t max_env_a = plan.max_env_a, max_env_b = plan.max_env_b;
    const int cap = q.cap;
    st.grid[0] = plan_grid(a, thr, plan.reach);
    st.grid[1] = plan_grid(b, thr, plan.reach);
    const GridPlan &ga = st.grid[0], &gb = st.grid[1];
    PassBufs& pb = st.pb;
    int64_t* own_pairs = nullptr;
    for (int dry = 1; dry >= 0; --dry) {
        Arena ar(dry ? nullptr : c->ws, dry ? 0 : c->ws_cap, dry != 0);
        carve_pass(ar, q, plan, ga.n_cells, gb.n_cells, pb);
        if (!pairs) own_pairs = ar.take<int64_t>(2 * (size_t)n_pairs);
        if (dry) if (int rc = ensure_ws(c, ar.off + 4096)) return rc;
    }
    SideBufs &sa = pb.a, &sb = pb.b;
    sa.env.cdf_keys = sb.env.cdf_keys = plan.dict_sets ? 0 : plan.key_sets;  // (what the environment kernels write into set 0)
    if (!plan.group) sa.env.cat0 = sb.env.cat0 = nullptr;
    const GridView gva = grid_view(ga, sa), gvb = grid_view(gb, sb);
    const CloudView cva = a->view(plan.cat16), cvb = b->view(plan.cat16);
    hipStream_t s = c->stream;
    // frames buffers are filled on another stream: order this pass behind their upload
    if (a->ev_ready && a->cap_frames) HIP_TRY(hipStreamWaitEvent(s, a->ev_ready, 0));
    if (b != a && b->ev_ready && b->cap_frames) HIP_TRY(hipStreamWaitEvent(s, b->ev_ready, 0));
    if (int rc = begin_pass(c)) return rc;
    c->status_dirty = true;  // until the whole pass has been enqueued
    st.begun = true;
    mark(c, 0);
    if (!pairs) {
        launch_profile_pairs(s, anchors, n_pairs, own_pairs);
        pairs = own_pairs;
    }
    {
        PrepSide psa = prep_side(cva, gva, sa), psb = prep_side(cvb, gvb, sb);
        psb.no_anchors = per_pair ? 1 : 0;  // (side B without de-duplication: no flags, no slots -- one environment per pair)
        (void)launch_prologue(s, c->tune, pairs, n_pairs, psa, psb, pb.zero_base, pb.zero_bytes, c->d_status, same, st.builds, st.dedup);
        if (per_pair) launch_pair_anchor_recs(s, pairs, n_pairs, psb, c->d_status);
    }
    mark(c, 1);
    mark(c, 2);  // (cell lists and anchor de-duplication are one phase now; "anchors" reads 0)
    const EnvSide esa{cva, gva, sa.uniq, sa.env, max_env_a, sa.raw_key, sa.raw_cat, sa.ovf_list},
                  esb{cvb, gvb, sb.uniq, sb.env, max_env_b, sb.raw_key, sb.raw_cat, sb.ovf_list};
    st.store_bytes = (size_t)(std::max<int64_t>(max_env_a, 1) + std::max<int64_t>(max_env_b, 1)) * (size_t)cap * ((plan.cat16 ? 2 : 1) + 8 * (size_t)std::max(plan.key_sets, 1));
    if (plan.group) {
        if (!launch_env_group(s, c->d_cfg, plan.tag_list, plan.group_small, esa, esb, thr, plan.apw, c->d_status))
            return fail(LCHD_EDEVICE, "the grouped environment kernel rejected its launch configuration");
    } else if (!launch_env_cells(s, cap, c->d_cfg, plan.tag_list, esa, esb, thr, c->d_status))
        return fail(LCHD_EUNSUPPORTED, plan.cat16 ? "with more than 255 categories an environment may hold at most 8192 points (capacity %d asked for)"
                                                  : "no environment kernel variant with capacity %d", cap);
    if (c->deterministic)  // one order among equal keys, whatever order the cell lists' and the buckets' atomics produced (utils.rs:25-39: a stable sort)
        launch_env_canon(s, sa.env, same ? sa.env : sb.env, max_env_a, same ? 0 : max_env_b, c->d_status);
    st.env[0] = sa.env;
    st.env[1] = sb.env;
    if (plan.dict_sets) {
        const int n_wf = c->h_cfg.n_wf;
        launch_env_key_sets(s, c->d_cfg, sa.env, sb.env, n_wf, max_env_a + max_env_b, c->d_status);
        for (EnvStore& e : st.env) {  // a consumer's view of the store: the F sets
            e.key += e.set_stride;
            e.cdf_keys = n_wf;
        }
    }
    mark(c, 3);
    return LCHD_OK;
}

// Everything of one from_primitives pass: plan -> environment store -> sweep.
static int prims_enqueue(lchd_ctx* c) {
    const auto& R = c->pend.req;
    auto& L = c->pend.run;
    ++c->n_passes;
    lchd_cloud *a = R.a, *b = R.b;
    const int64_t n_pairs = R.n_pairs;
    const PassQuery q = pass_query(c);
    const PassPlan plan = c->pend.plan = plan_pass(q);
    const bool same = plan.same, per_pair = plan.per_pair;
    PrimsStore st;
    const int rc = build_prims_store(c, a, b, R.anchors, nullptr, n_pairs, R.thr, q, plan, st);
    if (st.begun) {
        for (int side = 0; side < 2; ++side) {
            const GridPlan& g = st.grid[side];
            L.grid[side] = GridRecord{{g.dim[0], g.dim[1], g.dim[2]}, g.n_cells, st.builds[side]};
            L.dedup[side] = st.dedup[side];
        }
        L.ovf_a = st.pb.a.ovf_list;
        L.ovf_b = st.pb.b.ovf_list;
        L.n_slots_a = plan.max_env_a;
        L.n_slots_b = plan.max_env_b;
        c->last_store_bytes += st.store_bytes;
    }
    if (rc) return rc;
    const PassBufs& pb = st.pb;
    hipStream_t s = c->stream;
    SweepArgs sw{};
    fill_sweep_args(c, sw);
    sw.env_a = st.env[0];
    sw.env_b = st.env[same ? 0 : 1];
    sw.anchors = R.anchors;
    sw.slot_a = pb.a.slot;
    sw.slot_b = same ? pb.a.slot : (per_pair ? nullptr : pb.b.slot);  // (nullptr: side B's slot of pair p is p)
    sw.n_slot_a = a->n;
    sw.n_slot_b = b->n;
    sw.wf_index = R.wf;
    sw.n_pairs = n_pairs;
    sw.out = R.out;
    sw.meta = pb.pair_meta;
    if (!c->deterministic) {  // (deterministic mode: no team kernels, no companion)
        sw.left_list = pb.left_list;
        sw.left_count = c->d_left + 32 * c->left_slot;
        sw.left_zero = c->d_left + 32 * (c->left_slot ^ 1);
        sw.left_expected = R.subset ? n_pairs : c->hints.last_left;
    }
    L.sweep = launch_sweep(s, c->tune, c->h_cfg.n_categories, c->hellinger2, c->unit_weights, c->wf_pow, c->hints.sweep_hint, sw, &L.plan);
    if (!L.sweep.ok) return fail(LCHD_EDEVICE, "internal error: the sweep launch set %u would not give every pair exactly one kernel", L.plan.families);
    if (L.sweep.left_counters_used) c->left_slot ^= 1;  // (the record pass ran and zeroed the other slot)
    mark(c, 4);
    if (a->ev_used) { HIP_TRY(hipEventRecord(a->ev_used, s)); a->used_valid = true; }
    if (b->ev_used) { HIP_TRY(hipEventRecord(b->ev_used, s)); b->used_valid = true; }
    HIP_TRY(hipGetLastError());
    c->status_dirty = false;  // the record pass of this sequence leaves the device status clean
    L.sw = sw;
    return LCHD_OK;
}

extern "C" int lchd_from_primitives_dev_async(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int64_t* d_anchors,
                                              const int32_t* d_wf_index, int64_t n_pairs, double thr, double* d_out) {
    CTX_LOCK(c);
    if (!c || !a || !b) return fail(LCHD_EVALUE, "null argument");
    if (!c->cfg_set) return fail(LCHD_EVALUE, "lchd_ctx_set_config has not been called");
    if (c->pend.active) return fail(LCHD_EVALUE, "a previous asynchronous call has not been finished (lchd_ctx_finish)");
    c->last_valid = c->last_sweep_valid = false;
    if (n_pairs <= 0) return LCHD_OK;
    if (!d_anchors || !d_out) return fail(LCHD_EVALUE, "null anchor / score pointer");
    if (n_pairs > (int64_t)0x7FFFFFFF) return fail(LCHD_EUNSUPPORTED, "more than 2^31 - 1 anchor pairs in one call (%lld): split the list", (long long)n_pairs);
    if (!(thr > 0.0))  // within_radius returns nothing => dists[0] panics (src/locohd.rs:74)
        return fail(LCHD_EPANIC, "index out of bounds: threshold_distance = %g leaves every environment empty", thr);
    if (a->n == 0 || b->n == 0) return fail(LCHD_EPANIC, "index out of bounds: anchor pairs given for an empty structure");
    if (thr > a->reach || thr > b->reach)  // (an image cloud holds the images within its reach of the box, no others)
        return fail(LCHD_EVALUE, "threshold_distance = %g is beyond the reach %g the periodic images were built with", thr, std::min(a->reach, b->reach));
    if (!std::isfinite(thr)) thr = 1.7e308;
    CTX_GUARD(c);
    if (int rc = resolve_bbox(c, a)) return rc;
    if (int rc = resolve_bbox(c, b)) return rc;
    auto& R = c->pend.req;
    R.a = a; R.b = b; R.anchors = d_anchors; R.wf = d_wf_index; R.n_pairs = n_pairs; R.thr = thr; R.out = d_out;
    R.cap = c->hints.cap_hint;
    R.subset = false;
    R.repeated = false;
    c->last_store_bytes = 0;
    if (int rc = prims_enqueue(c)) return rc;
    c->pend.active = true;
    return LCHD_OK;
}

static int grow_block(char*& blk, size_t& cap, size_t need) {
    if (need <= cap) return LCHD_OK;
    if (blk) (void)hipFree(blk);
    blk = nullptr;
    cap = 0;
    const size_t got = need + need / 4 + 4096;
    if (hipMalloc(&blk, got) != hipSuccess) {
        (void)hipGetLastError();
        return fail(LCHD_EUNSUPPORTED, "no device memory for %zu bytes of the second pass over overflowed environments", got);
    }
    cap = got;
    return LCHD_OK;
}

static int finish_passes(lchd_ctx* c, uint32_t* flags_out);

// The pass that just finished flagged environments that did not fit their slots, and they are few: instead of repeating the
// WHOLE pass with larger slots (fixed stride: every environment of the call would pay for the largest one -- one 6 000-point
// cluster in a sparse 2 10^5-point cloud turns a 1.8 GB store into 15 GB), only the pairs that touch such an environment are
// scored again: selected on the device in list order, run as a pass of their own (its own unique anchors, slots of the size the
// overflow asked for, the regular retry loop), their scores scattered over the first pass's.  The first pass gave those
// environments the anchor alone (a valid one-point environment), so every other score and status word of it stands.
// *handled = false: not applicable (too many overflowed environments, nothing recorded), the caller repeats the whole pass.
static int rescore_overflow_pairs(lchd_ctx* c, uint32_t f1, int64_t biggest, bool* handled, uint32_t* flags_out) {
    *handled = false;
    auto& P = c->pend;
    const auto& L = P.run;
    const HostStatus* h = c->h_status;
    const uint32_t na = h->n_overflow[0], nb = h->n_overflow[1];
    const uint64_t n_uniq = (uint64_t)h->n_unique[0] + h->n_unique[1];
    if (P.req.subset || P.plan.per_pair || c->tune.no_overflow_subset || !L.ovf_a || na + nb == 0 || (f1 & ST_EMPTY_ENV)) return LCHD_OK;  // (per_pair: the selection kernels read side B's slot map)
    if ((uint64_t)(na + nb) * 8 > n_uniq) return LCHD_OK;  // not a minority: larger slots for everything
    hipStream_t s = c->stream;
    const SweepArgs sw = L.sw;  // the finished pass's arrays (the arena stays as it is until the second pass is enqueued)
    const bool same = P.plan.same;
    // bit sets over the slots + the selection's scratch
    const size_t wa = (size_t)(L.n_slots_a + 31) / 32 + 1, wb = same ? 0 : (size_t)(L.n_slots_b + 31) / 32 + 1;
    const size_t o_cnt = (wa + wb) * 4, o_tot = o_cnt + (size_t)kOverflowWaves * 8, bits_bytes = o_tot + 8;
    if (int rc = grow_block(c->d_ovf_bits, c->ovf_bits_cap, bits_bytes)) return rc;
    uint32_t* bits_a = reinterpret_cast<uint32_t*>(c->d_ovf_bits);
    uint32_t* bits_b = same ? bits_a : bits_a + wa;
    HIP_TRY(hipMemsetAsync(c->d_ovf_bits, 0, bits_bytes, s));
    launch_mark_overflow(s, L.ovf_a, na, L.ovf_b, nb, bits_a, bits_b);
    OverflowSelect sel{};
    sel.anchors = sw.anchors; sel.n_pairs = sw.n_pairs; sel.slot_a = sw.slot_a; sel.slot_b = sw.slot_b;
    sel.bits_a = bits_a; sel.bits_b = bits_b; sel.wf = sw.wf_index;
    sel.wave_count = reinterpret_cast<unsigned long long*>(c->d_ovf_bits + o_cnt);
    unsigned long long* d_total = reinterpret_cast<unsigned long long*>(c->d_ovf_bits + o_tot);
    launch_count_overflow(s, sel, d_total);
    unsigned long long n_sub = 0;
    HIP_TRY(hipMemcpyAsync(&n_sub, d_total, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (n_sub == 0 || n_sub * 2 > (unsigned long long)sw.n_pairs) return LCHD_OK;  // (most pairs touch one: the whole pass again)
    const size_t o_anc = (size_t)n_sub * 8, o_out = o_anc + (size_t)n_sub * 16, o_wf = o_out + (size_t)n_sub * 8,
                 list_bytes = o_wf + (sw.wf_index ? (size_t)n_sub * 4 : 0);
    if (int rc = grow_block(c->d_ovf_lists, c->ovf_lists_cap, list_bytes)) return rc;
    sel.sel_index = reinterpret_cast<int64_t*>(c->d_ovf_lists);
    sel.sel_anchors = reinterpret_cast<int64_t*>(c->d_ovf_lists + o_anc);
    sel.sel_wf = sw.wf_index ? reinterpret_cast<int32_t*>(c->d_ovf_lists + o_wf) : nullptr;
    double* sub_out = reinterpret_cast<double*>(c->d_ovf_lists + o_out);
    launch_write_overflow(s, sel);
    HIP_TRY(hipGetLastError());
    // the second pass: the context's hints describe the caller's workload, not this selection -- saved and restored around it
    const auto saved = P;
    const PassHints saved_hints = c->hints;
    auto& R = P.req;
    R.anchors = sel.sel_anchors; R.wf = sel.sel_wf; R.n_pairs = (int64_t)n_sub; R.out = sub_out;
    // (an anchor whose candidate table overflowed reported its candidates, an upper bound: a few large slots cost little here)
    R.cap = next_pow2_host(std::max<int64_t>(std::max<int64_t>(biggest, h->max_bound), saved.req.cap + 1));
    R.subset = true;
    c->hints.sweep_hint = 0;
    c->hints.last_biggest = biggest;
    ++c->n_subset_passes;
    uint32_t f2 = 0;
    int rc = prims_enqueue(c);
    if (!rc) rc = finish_passes(c, &f2);
    P = saved;
    c->hints = saved_hints;
    if (rc) return rc;
    launch_scatter_scores(s, sub_out, sel.sel_index, (int64_t)n_sub, saved.req.out);
    HIP_TRY(hipStreamSynchronize(s));
    c->last_valid = false;  // (c->last would describe the first pass, whose arena the second one has reused)
    c->last_sweep_valid = false;  // (... and the sweep record the second pass's selection)
    *flags_out = (f1 & ~ST_ENV_OVERFLOW) | f2;
    *handled = true;
    return LCHD_OK;
}

// The record of a finished pass: the counts are the words k_pair_meta published into the host-mapped mirror, the rule in force is
// rule_in_force (lchd_sweep_common.h) evaluated here from the same counts.
static SweepRecord sweep_record(const lchd_sweep_plan& plan, const HostStatus& h, int64_t n_pairs, bool repeated) {
    SweepRecord r;
    r.plan = plan;
    r.repeated = repeated ? 1 : 0;
    if (h.n_small == ~0ull) return r;  // (no record pass: the inline sweep counts nothing)
    const unsigned long long P = (unsigned long long)n_pairs, n_duo = h.n_duo, n_c8 = h.n_c8;
    if (plan.families & (LCHD_SWEEP_TEAM240 | LCHD_SWEEP_TEAM480 | LCHD_SWEEP_C8)) {
        const unsigned long long n_small = plan.small_rule ? n_c8 : n_duo;
        if (plan.forced || 2 * n_small >= P) r.rule = plan.small_rule;
        else if (plan.second_rule && 2 * n_c8 >= P) r.rule = plan.second_rule;
    }
    r.stats[0] = (int64_t)n_duo;
    r.stats[1] = (int64_t)n_c8;
    r.stats[2] = (int64_t)h.max_env;
    r.stats[3] = r.rule < 0 ? -1 : n_pairs - (int64_t)std::min(r.rule == 0 ? n_duo : n_c8, P);
    return r;
}

// What the lchd_ctx_last_* read-backs report about the pass that stood.
static void record_last_pass(lchd_ctx* c, const HostStatus& h) {
    const auto& P = c->pend;
    c->last = P.run.sw;
    c->last_grid[0] = P.run.grid[0];
    c->last_grid[1] = P.run.grid[1];
    for (int side = 0; side < 2; ++side)
        c->last_anchors[side] = AnchorRecord{P.run.dedup[side], (int64_t)h.n_unique[side], P.run.dedup[side] == 4 ? (int64_t)h.n_dup_b : (int64_t)-1};
    c->last_sweep = sweep_record(P.run.plan, h, P.req.n_pairs, P.req.repeated);
    c->last_sweep_valid = true;
    c->last_valid = true;
}

// Waits for the enqueued pass and repeats it while the device asks for it (larger slots, the full launch set); *flags_out = the
// status words of the pass that stood.  Every decision is pass_verdict's and every hint hints_after_pass's / hints_for_repeat's
// (lchd_pass_plan.h); this loop waits, asks, and enqueues.
static int finish_passes(lchd_ctx* c, uint32_t* flags_out) {
    auto& P = c->pend;
    auto& R = P.req;
    for (int attempt = 0; attempt < 6; ++attempt) {
        uint32_t f = 0;
        if (int rc = wait_pass(c, &f)) return rc;
        collect_times(c, 0, 4);
        // what the pairs of THIS pass looked like (a second pass over overflowed environments overwrites the mirror with its selection's numbers)
        const HostStatus h = *c->h_status;
        const PassOutcome o = pass_verdict(f, h, P.plan, P.run.sweep, c->h_cfg.n_categories, R.n_pairs, R.cap, R.subset);
        switch (o.verdict) {
            case PassVerdict::BAD_ANCHOR:
                *flags_out = f;
                return LCHD_OK;
            case PassVerdict::UNSUPPORTED:
                return fail(LCHD_EUNSUPPORTED, "an environment holds %lld points; beyond 65535 per environment this build handles at most %d "
                                               "categories and 2^23 points (the 64-bit-count sweep)", (long long)o.biggest, kMaxCategories);
            case PassVerdict::STANDS:
                if (P.plan.per_pair) ++c->n_per_pair_passes;
                record_last_pass(c, h);
                c->hints = hints_after_pass(c->hints, h, P.plan, P.run.sweep, R.n_pairs, R.b ? R.b->n : 0, R.subset);
                *flags_out = f;
                return LCHD_OK;
            case PassVerdict::OVERFLOW: {
                bool handled = false;
                if (int rc = rescore_overflow_pairs(c, f, o.biggest, &handled, flags_out)) return rc;
                if (handled) {  // the next call of this configuration starts from the first pass's launch set
                    if (h.n_small != ~0ull) c->hints.sweep_hint = sweep_hint_from_counts(h.n_duo, h.n_c8, R.n_pairs, false);
                    return LCHD_OK;
                }
                R.cap = o.grown_cap;
                break;
            }
            case PassVerdict::REPEAT_FULL_SET: R.repeated = true; break;
            case PassVerdict::REPEAT_REGULAR: break;
        }
        c->hints = hints_for_repeat(c->hints, o, R.subset);
        if (int rc = prims_enqueue(c)) return rc;
    }
    return fail(LCHD_EDEVICE, "environment capacity retry did not converge");
}

extern "C" int lchd_ctx_finish(lchd_ctx* c) {
    CTX_LOCK_FINISH(c);
    if (!c) return fail(LCHD_EVALUE, "null context");
    if (!c->pend.active) return LCHD_OK;
    c->pend.active = false;
    CTX_GUARD(c);
    uint32_t f = 0;
    if (int rc = finish_passes(c, &f)) return rc;
    return status_to_rc(f, DRV_PRIMS);
}

extern "C" int64_t lchd_ctx_subset_pass_count(lchd_ctx* c) { CTX_LOCK(c); return c ? c->n_subset_passes : -1; }
extern "C" int64_t lchd_ctx_per_pair_pass_count(lchd_ctx* c) { CTX_LOCK(c); return c ? c->n_per_pair_passes : -1; }
extern "C" int64_t lchd_ctx_last_store_bytes(lchd_ctx* c) { CTX_LOCK(c); return c ? (int64_t)c->last_store_bytes : -1; }

extern "C" int lchd_from_primitives_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int64_t* d_anchors,
                                        const int32_t* d_wf_index, int64_t n_pairs, double thr, double* d_out) {
    CTX_LOCK(c);
    if (int rc = lchd_from_primitives_dev_async(c, a, b, d_anchors, d_wf_index, n_pairs, thr, d_out)) return rc;
    return lchd_ctx_finish(c);
}

// ------------------------------------------------------------------------------------------------
// trajectory frames: a batch cloud whose structures are frames of one template structure
// ------------------------------------------------------------------------------------------------
extern "C" int lchd_frames_create(lchd_ctx* c, const lchd_cloud* tmpl, int32_t capacity_frames, lchd_cloud** out) {
    CTX_LOCK(c);
    if (!c || !tmpl || !out || capacity_frames < 1) return fail(LCHD_EVALUE, "bad argument");
    CTX_GUARD(c);
    if (tmpl->sid || tmpl->images) return fail(LCHD_EVALUE, "the template of a frames buffer must be a single structure");
    const int64_t nt = tmpl->n, total = nt * capacity_frames;
    if (nt < 1 || total > ((int64_t)1 << 30)) return fail(LCHD_EUNSUPPORTED, "frames buffer of %lld atoms is out of range", (long long)total);
    lchd_cloud* cl = new lchd_cloud();
    cl->n_tmpl = nt;
    cl->struct_size = (int32_t)nt;
    cl->cap_frames = capacity_frames;
    cl->n = 0;
    cl->n_struct = 1;
    auto bail = [&](hipError_t e, const char* what) {
        lchd_cloud_destroy(c, cl);
        return fail(LCHD_EDEVICE, "HIP error %d in %s", (int)e, what);
    };
    hipError_t e;
    if ((e = hipMalloc(&cl->x, sizeof(double) * total)) != hipSuccess) return bail(e, "hipMalloc(x)");
    if ((e = hipMalloc(&cl->y, sizeof(double) * total)) != hipSuccess) return bail(e, "hipMalloc(y)");
    if ((e = hipMalloc(&cl->z, sizeof(double) * total)) != hipSuccess) return bail(e, "hipMalloc(z)");
    if ((e = hipMalloc(&cl->cat, total)) != hipSuccess) return bail(e, "hipMalloc(cat)");
    if ((e = hipMalloc(&cl->tag, sizeof(int32_t) * total)) != hipSuccess) return bail(e, "hipMalloc(tag)");
    if ((e = hipMalloc(&cl->sid, sizeof(int32_t) * total)) != hipSuccess) return bail(e, "hipMalloc(sid)");
    if ((e = hipMalloc(&cl->d_raw, sizeof(double) * 3 * total)) != hipSuccess) return bail(e, "hipMalloc(raw)");
    if ((e = hipMalloc(&cl->d_bbox, sizeof(unsigned long long) * 7)) != hipSuccess) return bail(e, "hipMalloc(bbox)");
    if ((e = hipHostMalloc(&cl->h_pinned, sizeof(double) * 3 * total)) != hipSuccess) return bail(e, "hipHostMalloc");
    if ((e = hipEventCreateWithFlags(&cl->ev_ready, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
    if ((e = hipEventCreateWithFlags(&cl->ev_used, hipEventDisableTiming)) != hipSuccess) return bail(e, "hipEventCreate");
    launch_frames_labels(c->stream, tmpl->cat, tmpl->tag, nt, capacity_frames, cl->cat, cl->tag, cl->sid);
    if (tmpl->cat_hi) {  // more than 255 categories: the high bytes and the one-byte view travel with every frame as well
        if ((e = hipMalloc(&cl->cat_hi, total)) != hipSuccess) return bail(e, "hipMalloc(cat_hi)");
        if ((e = hipMalloc(&cl->cat_narrow, total)) != hipSuccess) return bail(e, "hipMalloc(cat_narrow)");
        launch_frames_labels(c->stream, tmpl->cat_hi, tmpl->tag, nt, capacity_frames, cl->cat_hi, cl->tag, cl->sid);
        launch_frames_labels(c->stream, tmpl->cat_narrow, tmpl->tag, nt, capacity_frames, cl->cat_narrow, cl->tag, cl->sid);
    }
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return bail(e, "frames label fill");
    *out = cl;
    return LCHD_OK;
}

extern "C" int lchd_frames_load(lchd_ctx* c, lchd_cloud* fr, const double* xyz, int32_t n_frames, void* hip_stream) {
    CTX_LOCK(c);
    if (!c || !fr || !xyz || !fr->cap_frames) return fail(LCHD_EVALUE, "not a frames buffer");
    if (n_frames < 1 || n_frames > fr->cap_frames) return fail(LCHD_EVALUE, "%d frames do not fit a buffer of %d", n_frames, fr->cap_frames);
    if (c->pend.active && (c->pend.req.a == fr || c->pend.req.b == fr))
        return fail(LCHD_EVALUE, "this frames buffer is in use by an unfinished asynchronous call");
    CTX_GUARD(c);
    hipStream_t s = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->stream;
    const int64_t total = fr->n_tmpl * n_frames;
    // the pinned staging block is free again once the previous upload from it has completed
    if (fr->ev_ready && fr->bbox_pending) HIP_TRY(hipEventSynchronize(fr->ev_ready));
    memcpy(fr->h_pinned, xyz, sizeof(double) * 3 * (size_t)total);
    if (fr->used_valid) HIP_TRY(hipStreamWaitEvent(s, fr->ev_used, 0));  // do not overwrite frames a running pass still reads
    HIP_TRY(hipMemcpyAsync(fr->d_raw, fr->h_pinned, sizeof(double) * 3 * (size_t)total, hipMemcpyHostToDevice, s));
    launch_frames_unpack(s, fr->d_raw, total, fr->x, fr->y, fr->z, fr->d_bbox);
    HIP_TRY(hipEventRecord(fr->ev_ready, s));
    HIP_TRY(hipGetLastError());
    fr->n = total;
    fr->n_struct = n_frames;
    fr->bbox_pending = true;
    return LCHD_OK;
}

extern "C" int lchd_frames_set_sources(lchd_ctx* c, lchd_cloud* fr, const int32_t* src_start, const int32_t* src_idx,
                                       int64_t n_src_atoms) {
    CTX_LOCK(c);
    if (!c || !fr || !fr->cap_frames || !src_start || !src_idx) return fail(LCHD_EVALUE, "not a frames buffer / null map");
    if (c->pend.active && (c->pend.req.a == fr || c->pend.req.b == fr))
        return fail(LCHD_EVALUE, "this frames buffer is in use by an unfinished asynchronous call");
    CTX_GUARD(c);
    const int64_t np = fr->n_tmpl;
    if (n_src_atoms < 1 || n_src_atoms * (int64_t)fr->cap_frames > ((int64_t)1 << 31))
        return fail(LCHD_EUNSUPPORTED, "%lld source atoms x %d frames is out of range", (long long)n_src_atoms, fr->cap_frames);
    if (src_start[0] != 0) return fail(LCHD_EVALUE, "src_start[0] must be 0");
    for (int64_t p = 0; p < np; ++p)  // np.mean of an empty list is NaN in the reference (atom_converter_utils.py:126): refuse it here
        if (src_start[p + 1] <= src_start[p]) return fail(LCHD_EVALUE, "primitive atom %lld has no source atoms", (long long)p);
    const int64_t nnz = src_start[np];
    for (int64_t k = 0; k < nnz; ++k)
        if (src_idx[k] < 0 || src_idx[k] >= n_src_atoms)
            return fail(LCHD_EVALUE, "source atom index %d at position %lld is outside [0, %lld)", src_idx[k], (long long)k, (long long)n_src_atoms);
    // Tiles: consecutive primitive atoms whose members span at most `span` consecutive source atoms (staged through LDS);
    // spans are balanced so that the tiles of a frame carry similar byte counts.  A primitive atom that alone spans more
    // becomes a tile of its own that gathers from global memory.
    std::vector<int32_t> tiles;
    {
        const int cap = centroid_tile_span();
        int64_t glo = n_src_atoms, ghi = 0;
        for (int64_t k = 0; k < nnz; ++k) { glo = std::min<int64_t>(glo, src_idx[k]); ghi = std::max<int64_t>(ghi, src_idx[k] + 1); }
        const int64_t pieces = std::max<int64_t>(1, (ghi - glo + cap - 1) / cap);
        const int span = (int)std::min<int64_t>(cap, (ghi - glo + pieces - 1) / pieces + 64);
        int64_t p0 = 0;
        int lo = 0, hi = 0;
        auto close = [&](int64_t p1) { if (p1 > p0) { tiles.push_back((int32_t)p0); tiles.push_back((int32_t)p1); tiles.push_back(lo); tiles.push_back(hi); } };
        for (int64_t p = 0; p < np; ++p) {
            int plo = src_idx[src_start[p]], phi = plo + 1;
            for (int k = src_start[p]; k < src_start[p + 1]; ++k) { plo = std::min(plo, src_idx[k]); phi = std::max(phi, src_idx[k] + 1); }
            if (phi - plo > span) {  // cannot be staged: its own global-gather tile
                close(p);
                tiles.push_back((int32_t)p); tiles.push_back((int32_t)p + 1); tiles.push_back(-1); tiles.push_back(-1);
                p0 = p + 1;
                continue;
            }
            if (p == p0) { lo = plo; hi = phi; continue; }
            const int nlo = std::min(lo, plo), nhi = std::max(hi, phi);
            if (nhi - nlo > span) { close(p); p0 = p; lo = plo; hi = phi; }
            else { lo = nlo; hi = nhi; }
        }
        close(np);
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (fr->ev_ready && fr->bbox_pending) HIP_TRY(hipEventSynchronize(fr->ev_ready));
    (void)hipFree(fr->d_src_start); fr->d_src_start = nullptr;
    (void)hipFree(fr->d_src_idx); fr->d_src_idx = nullptr;
    (void)hipFree(fr->d_tiles); fr->d_tiles = nullptr;
    (void)hipFree(fr->d_raw32); fr->d_raw32 = nullptr;
    if (fr->h_pinned32) { (void)hipHostFree(fr->h_pinned32); fr->h_pinned32 = nullptr; }
    fr->n_src = 0;
    const size_t raw_elems = (size_t)3 * (size_t)n_src_atoms * (size_t)fr->cap_frames;
    {   // all or nothing: a failure leaves the buffer without sources (n_src == 0) and without half-made allocations
        hipError_t e = hipMalloc(&fr->d_src_start, sizeof(int32_t) * (size_t)(np + 1));
        if (e == hipSuccess) e = hipMalloc(&fr->d_src_idx, sizeof(int32_t) * (size_t)nnz);
        if (e == hipSuccess) e = hipMalloc(&fr->d_raw32, sizeof(float) * raw_elems);
        if (e == hipSuccess) e = hipHostMalloc(&fr->h_pinned32, sizeof(float) * raw_elems);
        if (e == hipSuccess) e = hipMemcpy(fr->d_src_start, src_start, sizeof(int32_t) * (size_t)(np + 1), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(fr->d_src_idx, src_idx, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice);
        if (e == hipSuccess && !fr->d_bbox_part) e = hipMalloc(&fr->d_bbox_part, sizeof(unsigned long long) * 7 * (size_t)bbox_parts_capacity());
        if (e == hipSuccess) e = hipMalloc(&fr->d_tiles, sizeof(int32_t) * tiles.size());
        if (e == hipSuccess) e = hipMemcpy(fr->d_tiles, tiles.data(), sizeof(int32_t) * tiles.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(fr->d_src_start); fr->d_src_start = nullptr;
            (void)hipFree(fr->d_src_idx); fr->d_src_idx = nullptr;
            (void)hipFree(fr->d_tiles); fr->d_tiles = nullptr;
            (void)hipFree(fr->d_raw32); fr->d_raw32 = nullptr;
            if (fr->h_pinned32) { (void)hipHostFree(fr->h_pinned32); fr->h_pinned32 = nullptr; }
            return fail(LCHD_EDEVICE, "HIP error %d (%s) in lchd_frames_set_sources", (int)e, hipGetErrorName(e));
        }
    }
    fr->n_tiles = (int32_t)(tiles.size() / 4);
    fr->n_src = n_src_atoms;
    return LCHD_OK;
}

// host_src: copy through the pinned block first; otherwise `atom_xyz` is already a DEVICE pointer
static int frames_load_atoms(lchd_ctx* c, lchd_cloud* fr, const float* atom_xyz, int32_t n_frames, void* hip_stream, bool host_src) {
    if (!c || !fr || !atom_xyz || !fr->cap_frames) return fail(LCHD_EVALUE, "not a frames buffer");
    if (!fr->n_src) return fail(LCHD_EVALUE, "lchd_frames_set_sources has not been called on this frames buffer");
    if (n_frames < 1 || n_frames > fr->cap_frames) return fail(LCHD_EVALUE, "%d frames do not fit a buffer of %d", n_frames, fr->cap_frames);
    if (c->pend.active && (c->pend.req.a == fr || c->pend.req.b == fr))
        return fail(LCHD_EVALUE, "this frames buffer is in use by an unfinished asynchronous call");
    CTX_GUARD(c);
    hipStream_t s = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c->stream;
    const size_t elems = (size_t)3 * (size_t)fr->n_src * (size_t)n_frames;
    const float* d_src = atom_xyz;
    if (host_src) {
        if (fr->ev_ready && fr->bbox_pending) HIP_TRY(hipEventSynchronize(fr->ev_ready));  // pinned block free again
        memcpy(fr->h_pinned32, atom_xyz, sizeof(float) * elems);
    }
    if (fr->used_valid) HIP_TRY(hipStreamWaitEvent(s, fr->ev_used, 0));
    if (host_src) {
        HIP_TRY(hipMemcpyAsync(fr->d_raw32, fr->h_pinned32, sizeof(float) * elems, hipMemcpyHostToDevice, s));
        d_src = fr->d_raw32;
    }
    fr->t_valid = false;
    if (c->timing) {
        if (!fr->ev_t0) { HIP_TRY(hipEventCreate(&fr->ev_t0)); HIP_TRY(hipEventCreate(&fr->ev_t1)); }
        HIP_TRY(hipEventRecord(fr->ev_t0, s));
    }
    launch_frames_centroids(s, d_src, fr->n_src, fr->d_src_start, fr->d_src_idx, fr->d_tiles, fr->n_tiles, fr->n_tmpl, n_frames, fr->x,
                            fr->y, fr->z, fr->d_bbox, fr->d_bbox_part);
    if (c->timing) { HIP_TRY(hipEventRecord(fr->ev_t1, s)); fr->t_valid = true; }
    HIP_TRY(hipEventRecord(fr->ev_ready, s));
    HIP_TRY(hipGetLastError());
    fr->n = fr->n_tmpl * n_frames;
    fr->n_struct = n_frames;
    fr->bbox_pending = true;
    return LCHD_OK;
}

extern "C" int lchd_frames_load_atoms(lchd_ctx* c, lchd_cloud* fr, const float* atom_xyz, int32_t n_frames, void* hip_stream) {
    CTX_LOCK(c);
    return frames_load_atoms(c, fr, atom_xyz, n_frames, hip_stream, true);
}
extern "C" int lchd_frames_load_atoms_dev(lchd_ctx* c, lchd_cloud* fr, const float* d_atom_xyz, int32_t n_frames, void* hip_stream) {
    CTX_LOCK(c);
    return frames_load_atoms(c, fr, d_atom_xyz, n_frames, hip_stream, false);
}
extern "C" double lchd_frames_last_convert_ms(lchd_ctx* c, lchd_cloud* fr) {
    CTX_LOCK(c);
    if (!c || !fr || !fr->t_valid) return -1.0;
    CTX_GUARD(c);
    float t = -1.f;
    if (hipEventSynchronize(fr->ev_t1) != hipSuccess || hipEventElapsedTime(&t, fr->ev_t0, fr->ev_t1) != hipSuccess) return -1.0;
    return t;
}

/* Read back the primitive-atom coordinates of a frames buffer (or any cloud) as [n][3] f64: lets a caller check the device
 * centroids against its own np.mean, and feeds generate_primitive_pdb for a frame. */
extern "C" int lchd_cloud_get_coords(lchd_ctx* c, lchd_cloud* cl, double* xyz_out, int64_t n) {
    CTX_LOCK(c);
    if (!c || !cl || !xyz_out) return fail(LCHD_EVALUE, "null argument");
    if (n != cl->n) return fail(LCHD_EVALUE, "the cloud holds %lld atoms, not %lld", (long long)cl->n, (long long)n);
    CTX_GUARD(c);
    if (cl->ev_ready && cl->bbox_pending) HIP_TRY(hipEventSynchronize(cl->ev_ready));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<double> soa((size_t)3 * (size_t)n);
    if (n) {
        HIP_TRY(hipMemcpy(soa.data(), cl->x, sizeof(double) * n, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(soa.data() + n, cl->y, sizeof(double) * n, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(soa.data() + 2 * n, cl->z, sizeof(double) * n, hipMemcpyDeviceToHost));
    }
    for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) xyz_out[3 * i + k] = soa[(size_t)k * n + i];
    return LCHD_OK;
}

// ------------------------------------------------------------------------------------------------
// periodic boundaries: the periodic images of a cloud as a cloud (kernels: lchd_images.hip)
// ------------------------------------------------------------------------------------------------
extern "C" int32_t lchd_images_scan_span(void) { return kImgScanSpan; }

extern "C" int lchd_box_validate(const double* boxes, int32_t n_boxes, double reach) {
    if (!boxes || n_boxes < 1) return fail(LCHD_EVALUE, "a periodic box is three edge lengths (Lx, Ly, Lz); none given");
    if (!std::isfinite(reach) || !(reach > 0.0)) return fail(LCHD_EVALUE, "the reach of the periodic images must be finite and > 0, got %g", reach);
    for (int32_t b = 0; b < n_boxes; ++b)
        for (int k = 0; k < 3; ++k) {
            const double L = boxes[3 * (size_t)b + k];
            if (!std::isfinite(L) || !(L > 0.0)) return fail(LCHD_EVALUE, "box %d: edge %d is %g; every edge must be finite and > 0", b, k, L);
            if (reach > L)
                return fail(LCHD_EVALUE, "box %d: the reach %g exceeds the edge %g; one layer of periodic images covers a threshold up to the smallest edge", b, reach, L);
        }
    return LCHD_OK;
}

// A triclinic cell on the host: rec = cell (9), inverse (9), perpendicular widths (3).  The arithmetic is part of the contract of
// lchd_cell_validate (include/loco_hd_hip.h): plain f64, left to right, nothing contracted (-ffp-contract=off, Makefile).
static void cross3(const double* u, const double* v, double* o) {
    o[0] = u[1] * v[2] - u[2] * v[1]; o[1] = u[2] * v[0] - u[0] * v[2]; o[2] = u[0] * v[1] - u[1] * v[0];
}
static double norm3(const double* u) { return std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]); }
static int cell_record(const double* cell, int32_t index, double reach, double* rec /* [kImgCellRecord] or null */) {
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(cell[k])) return fail(LCHD_EVALUE, "cell %d: entry %d is %g; every entry of a cell must be finite", index, k, cell[k]);
    const double *a = cell, *b = cell + 3, *c = cell + 6;
    double x[3][3];  // x[k] = the cross product of the other two vectors, cyclic: a . x[0] = b . x[1] = c . x[2] = det
    cross3(b, c, x[0]); cross3(c, a, x[1]); cross3(a, b, x[2]);
    const double det = a[0] * x[0][0] + a[1] * x[0][1] + a[2] * x[0][2];
    if (!(std::fabs(det) > 0.0) || !std::isfinite(det) || std::fabs(det) < 1e-12 * (norm3(a) * norm3(b) * norm3(c)))
        return fail(LCHD_EVALUE, "cell %d is singular (determinant %g): its three vectors must span a volume", index, det);
    for (int k = 0; k < 3; ++k) {
        const double w = std::fabs(det) / norm3(x[k]);
        if (!std::isfinite(w) || !(w > 0.0)) return fail(LCHD_EVALUE, "cell %d is singular (width %d is %g)", index, k, w);
        if (reach > w)
            return fail(LCHD_EVALUE, "cell %d: the reach %g exceeds the perpendicular width %g of axis %d; one layer of periodic images covers a threshold up to the smallest width",
                        index, reach, w, k);
        if (rec) rec[18 + k] = w;
    }
    if (rec)
        for (int d = 0; d < 3; ++d)
            for (int k = 0; k < 3; ++k) { rec[3 * d + k] = cell[3 * d + k]; rec[9 + 3 * d + k] = x[k][d] / det; }  // column k of the inverse = x[k] / det
    return LCHD_OK;
}

// Every cell against the reach; with `recs` ([n_cells][kImgCellRecord]) their device records are filled on the way.
static int cell_records(const double* cells, int32_t n_cells, double reach, double* recs) {
    if (!cells || n_cells < 1) return fail(LCHD_EVALUE, "a periodic cell is three lattice vectors (a 3 x 3 matrix); none given");
    if (!std::isfinite(reach) || !(reach > 0.0)) return fail(LCHD_EVALUE, "the reach of the periodic images must be finite and > 0, got %g", reach);
    for (int32_t b = 0; b < n_cells; ++b)
        if (int rc = cell_record(cells + 9 * (size_t)b, b, reach, recs ? recs + (size_t)kImgCellRecord * b : nullptr)) return rc;
    return LCHD_OK;
}
extern "C" int lchd_cell_validate(const double* cells, int32_t n_cells, double reach) { return cell_records(cells, n_cells, reach, nullptr); }

// The cell of the dense minimum-image calls (lchd_cell_reduce.h): validated with the messages of lchd_cell_validate (no reach: a dense
// row has no threshold), Minkowski-reduced, with the inverse of the reduced cell.
static int min_image_cell(const double* cell, int32_t index, double* reduced, double* inverse) {
    if (int rc = cell_record(cell, index, 0.0, nullptr)) return rc;
    if (cell_reduce(cell, reduced, inverse) != 0)
        return fail(LCHD_EVALUE, "cell %d is singular: its three vectors must span a volume", index);
    return LCHD_OK;
}
static int min_image_record(const double* cell, int32_t index, MinImageCell& rec) {
    if (int rc = min_image_cell(cell, index, rec.v, rec.v + 9)) return rc;
    rec.v[18] = cell_is_diagonal(rec.v) ? 1.0 : 0.0;
    return LCHD_OK;
}
extern "C" int lchd_cell_reduce(const double* cell, double* reduced, double* inverse) {
    if (!cell || !reduced || !inverse) return fail(LCHD_EVALUE, "null argument");
    return min_image_cell(cell, 0, reduced, inverse);
}

template <class T>
static int grow_array(T*& p, size_t n) {
    (void)hipFree(p);
    p = nullptr;
    HIP_TRY(hipMalloc(&p, sizeof(T) * std::max<size_t>(n, 1)));
    return LCHD_OK;
}
static int images_reserve(lchd_cloud* img, const lchd_cloud* src, int64_t cap) {  // (the stream is idle: nothing reads the arrays)
    if (cap <= img->img_cap && (!src->cat_hi || img->cat_hi) && (!src->sid || img->sid)) return LCHD_OK;
    cap = std::max(cap, img->img_cap);
    img->img_cap = 0;
    if (int rc = grow_array(img->x, (size_t)cap)) return rc;
    if (int rc = grow_array(img->y, (size_t)cap)) return rc;
    if (int rc = grow_array(img->z, (size_t)cap)) return rc;
    if (int rc = grow_array(img->cat, (size_t)cap)) return rc;
    if (int rc = grow_array(img->tag, (size_t)cap)) return rc;
    if (src->cat_hi) {
        if (int rc = grow_array(img->cat_hi, (size_t)cap)) return rc;
        if (int rc = grow_array(img->cat_narrow, (size_t)cap)) return rc;
    }
    if (src->sid)
        if (int rc = grow_array(img->sid, (size_t)cap)) return rc;
    img->img_cap = cap;
    return LCHD_OK;
}

// count -> scan -> (read the total back, size the arrays) -> emit, on the context's stream behind the source's pending upload
// (boxes: [n_boxes][3] edges, or for a cell cloud [n_boxes][9] cells)
static int images_build(lchd_ctx* c, lchd_cloud* img, lchd_cloud* src, const double* boxes, int32_t n_boxes) {
    const bool cell = img->img_cell;
    if (n_boxes != 1 && n_boxes != src->n_struct)
        return fail(LCHD_EVALUE, "%d %s given for %d structures: pass one %s, or one per structure", n_boxes, cell ? "cells" : "boxes",
                    src->n_struct, cell ? "cell" : "box");
    if (cell) {  // validated and turned into records in one go (the last build's copy out of h_cells was waited for in that build)
        img->h_cells.resize((size_t)kImgCellRecord * std::max(n_boxes, 1));
        if (int rc = cell_records(boxes, n_boxes, img->reach, img->h_cells.data())) return rc;
    } else if (int rc = lchd_box_validate(boxes, n_boxes, img->reach)) {
        return rc;
    }
    if (src->images) return fail(LCHD_EVALUE, "the source of an image cloud must not be an image cloud");
    if (c->pend.active && (c->pend.req.a == img || c->pend.req.b == img))
        return fail(LCHD_EVALUE, "this image cloud is in use by an unfinished asynchronous call");
    const int64_t n = src->n;
    if (n > ((int64_t)1 << 27)) return fail(LCHD_EUNSUPPORTED, "periodic images of %lld atoms: at most 2^27", (long long)n);
    hipStream_t s = c->stream;
    img->origin_valid = false;  // (the ghosts move with the coordinates: the map is built again by the first call that needs it)
    img->n_home = 0;
    img->n = 0;  // (until the build has succeeded)
    img->n_struct = src->n_struct;
    img->struct_size = 0;
    HIP_TRY(hipStreamSynchronize(s));  // the last pass over the image cloud has read its arrays; they may move now
    if (n > img->img_scan_cap) {
        const int64_t cap = n + n / 4;
        img->img_scan_cap = 0;
        if (int rc = grow_array(img->d_img_count, (size_t)cap)) return rc;
        if (int rc = grow_array(img->d_img_offset, (size_t)cap)) return rc;
        if (int rc = grow_array(img->d_img_spans, (size_t)(cap / kImgScanSpan + 1))) return rc;
        img->img_scan_cap = cap;
    }
    if (!cell && n_boxes > img->boxes_cap) {
        img->boxes_cap = 0;
        if (int rc = grow_array(img->d_boxes, (size_t)3 * n_boxes)) return rc;
        img->boxes_cap = n_boxes;
    }
    if (cell && n_boxes > img->cells_cap) {
        img->cells_cap = 0;
        if (int rc = grow_array(img->d_cells, (size_t)kImgCellRecord * n_boxes)) return rc;
        img->cells_cap = n_boxes;
    }
    if (!img->d_bbox) HIP_TRY(hipMalloc(&img->d_bbox, sizeof(unsigned long long) * 8));
    if (int rc = images_reserve(img, src, 2 * n + 64)) return rc;
    if (n == 0) { for (int k = 0; k < 3; ++k) img->bbmin[k] = img->bbmax[k] = 0.0; return LCHD_OK; }
    if (cell) {
        HIP_TRY(hipMemcpyAsync(img->d_cells, img->h_cells.data(), sizeof(double) * img->h_cells.size(), hipMemcpyHostToDevice, s));
    } else {
        HIP_TRY(hipMemcpyAsync(img->d_boxes, boxes, sizeof(double) * 3 * (size_t)n_boxes, hipMemcpyHostToDevice, s));
    }
    if (src->ev_ready && src->cap_frames) HIP_TRY(hipStreamWaitEvent(s, src->ev_ready, 0));  // (a frames buffer is filled on another stream)
    ImageArgs ia{};
    ia.src = CloudView{src->x, src->y, src->z, src->cat, src->cat_hi, src->tag, (int32_t)n, src->sid, src->n_struct, 0};
    ia.src_narrow = src->cat_narrow;
    ia.boxes = cell ? nullptr : img->d_boxes;
    ia.cells = cell ? img->d_cells : nullptr;
    ia.n_boxes = n_boxes;
    ia.reach = img->reach;
    ia.count = img->d_img_count;
    ia.offset = img->d_img_offset;
    ia.span_sum = n > kImgScanSpan ? img->d_img_spans : nullptr;
    ia.bbox = img->d_bbox;
    auto point_at_arrays = [&] {
        ia.x = img->x; ia.y = img->y; ia.z = img->z;
        ia.cat = img->cat;
        ia.cat_hi = src->cat_hi ? img->cat_hi : nullptr;
        ia.cat_narrow = src->cat_hi ? img->cat_narrow : nullptr;
        ia.tag = img->tag;
        ia.sid = src->sid ? img->sid : nullptr;
        ia.capacity = img->img_cap;
    };
    point_at_arrays();
    launch_img_count(s, ia);
    launch_img_scan(s, ia);
    unsigned long long k[8];
    HIP_TRY(hipMemcpyAsync(k, img->d_bbox, sizeof k, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (k[6]) return fail(LCHD_EVALUE, src->cap_frames ? "non-finite coordinate in a trajectory frame" : "non-finite coordinate in the source of the periodic images");
    const int64_t total = n + (int64_t)k[7];
    if (total > ((int64_t)1 << 30)) return fail(LCHD_EUNSUPPORTED, "%lld atoms and periodic images exceed a cloud", (long long)total);
    if (total > img->img_cap) {  // grow (with a margin: the rim population of a trajectory drifts) and wrap into the new arrays
        if (int rc = images_reserve(img, src, total + total / 4)) return rc;
        point_at_arrays();
        launch_img_count(s, ia);
    }
    launch_img_emit(s, ia);
    if (src->ev_used) { HIP_TRY(hipEventRecord(src->ev_used, s)); src->used_valid = true; }  // (a later load into the source waits for the emit)
    HIP_TRY(hipGetLastError());
    auto dec = [](unsigned long long u) { u = (u >> 63) ? (u ^ 0x8000000000000000ull) : ~u; double d; memcpy(&d, &u, 8); return d; };
    for (int q = 0; q < 3; ++q) { img->bbmin[q] = dec(k[q]); img->bbmax[q] = dec(k[3 + q]); }
    if (!src->cat_hi && img->cat_hi) {  // (the arrays outlive a source with wide ids: this source has none)
        (void)hipFree(img->cat_hi); (void)hipFree(img->cat_narrow);
        img->cat_hi = img->cat_narrow = nullptr;
    }
    if (!src->sid && img->sid) { (void)hipFree(img->sid); img->sid = nullptr; }
    img->n = total;
    img->n_home = n;
    img->img_boxes = n_boxes;
    return LCHD_OK;
}

// origin / code of every slot of a built image cloud, on the context's stream (behind the build, in front of whatever reads them).
// Nothing is launched while the map of the last build stands; the arrays follow the cloud's capacity, so they move only when it grows.
static int images_origin(lchd_ctx* c, lchd_cloud* img) {
    if (img->origin_valid || img->n == 0) return LCHD_OK;
    if (img->origin_cap < img->img_cap) {
        HIP_TRY(hipStreamSynchronize(c->stream));  // (a call that read the old arrays has finished)
        img->origin_cap = 0;
        if (int rc = grow_array(img->d_img_origin, (size_t)img->img_cap)) return rc;
        if (int rc = grow_array(img->d_img_code, (size_t)img->img_cap)) return rc;
        img->origin_cap = img->img_cap;
    }
    ImageArgs ia{};
    ia.src = CloudView{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, (int32_t)img->n_home, img->sid, img->n_struct, 0};
    ia.boxes = img->img_cell ? nullptr : img->d_boxes;
    ia.cells = img->img_cell ? img->d_cells : nullptr;
    ia.n_boxes = img->img_boxes;
    ia.reach = img->reach;
    ia.x = img->x; ia.y = img->y; ia.z = img->z;
    ia.capacity = std::min(img->n, img->origin_cap);
    ia.count = img->d_img_count;
    ia.offset = img->d_img_offset;
    ia.span_sum = img->n_home > kImgScanSpan ? img->d_img_spans : nullptr;
    launch_img_origin(c->stream, ia, img->d_img_origin, img->d_img_code);
    HIP_TRY(hipGetLastError());
    img->origin_valid = true;
    return LCHD_OK;
}

/* origin / code of every slot of an image cloud as HOST arrays (lchd_cloud_get_coords' rules). */
extern "C" int lchd_cloud_image_origin(lchd_ctx* c, lchd_cloud* img, int32_t* origin_out, int8_t* code_out, int64_t n) {
    CTX_LOCK(c);
    if (!c || !img || !origin_out || !code_out) return fail(LCHD_EVALUE, "null argument");
    if (!img->images) return fail(LCHD_EVALUE, "not an image cloud (lchd_cloud_create_images)");
    if (n != img->n) return fail(LCHD_EVALUE, "the cloud holds %lld atoms, not %lld", (long long)img->n, (long long)n);
    CTX_GUARD(c);
    if (int rc = images_origin(c, img)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n) {
        HIP_TRY(hipMemcpy(origin_out, img->d_img_origin, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(code_out, img->d_img_code, (size_t)n, hipMemcpyDeviceToHost));
    }
    return LCHD_OK;
}
extern "C" int64_t lchd_cloud_home_size(const lchd_cloud* cl) { return cl ? (cl->images ? cl->n_home : cl->n) : -1; }

static int images_create(lchd_ctx* c, lchd_cloud* src, const double* boxes, int32_t n_boxes, double reach, bool cell, lchd_cloud** out) {
    CTX_LOCK(c);
    if (!c || !src || !out) return fail(LCHD_EVALUE, "null argument");
    *out = nullptr;
    CTX_GUARD(c);
    lchd_cloud* img = new lchd_cloud();
    img->images = true;
    img->img_cell = cell;
    img->reach = reach;
    if (int rc = images_build(c, img, src, boxes, n_boxes)) {
        lchd_cloud_destroy(c, img);
        return rc;
    }
    *out = img;
    return LCHD_OK;
}

extern "C" int lchd_cloud_create_images(lchd_ctx* c, lchd_cloud* src, const double* boxes, int32_t n_boxes, double reach, lchd_cloud** out) {
    return images_create(c, src, boxes, n_boxes, reach, false, out);
}
extern "C" int lchd_cloud_create_images_cell(lchd_ctx* c, lchd_cloud* src, const double* cells, int32_t n_cells, double reach, lchd_cloud** out) {
    return images_create(c, src, cells, n_cells, reach, true, out);
}

static int images_update(lchd_ctx* c, lchd_cloud* img, lchd_cloud* src, const double* boxes, int32_t n_boxes, bool cell) {
    CTX_LOCK(c);
    if (!c || !img || !src) return fail(LCHD_EVALUE, "null argument");
    if (!img->images) return fail(LCHD_EVALUE, "not an image cloud (lchd_cloud_create_images)");
    if (img->img_cell != cell)
        return fail(LCHD_EVALUE, cell ? "this image cloud was built from boxes: update it with lchd_cloud_update_images"
                                      : "this image cloud was built from cells: update it with lchd_cloud_update_images_cell");
    CTX_GUARD(c);
    return images_build(c, img, src, boxes, n_boxes);
}
extern "C" int lchd_cloud_update_images(lchd_ctx* c, lchd_cloud* img, lchd_cloud* src, const double* boxes, int32_t n_boxes) {
    return images_update(c, img, src, boxes, n_boxes, false);
}
extern "C" int lchd_cloud_update_images_cell(lchd_ctx* c, lchd_cloud* img, lchd_cloud* src, const double* cells, int32_t n_cells) {
    return images_update(c, img, src, cells, n_cells, true);
}

// ------------------------------------------------------------------------------------------------
// host-pointer drivers
// ------------------------------------------------------------------------------------------------
static int check_wf_index(const lchd_config* cfg, const int32_t* wf_index, int64_t n) {
    if (!wf_index) return LCHD_OK;
    for (int64_t i = 0; i < n; ++i)
        if (wf_index[i] < 0 || wf_index[i] >= cfg->n_weight_functions)
            return fail(LCHD_EVALUE, "weight-function index %d out of range at position %lld", wf_index[i], (long long)i);
    return LCHD_OK;
}

// One structure of a host-pointer call inside the context's I/O block: SoA coordinates, tags, categories.  Fills the pinned
// staging copy (AoS -> SoA, finiteness check, bounding box) and points a stack-allocated lchd_cloud at the device copy.
static int stage_cloud(const double* xyz, const int32_t* cat, const int32_t* tag, int64_t n, char* h_base, char* d_base, size_t& off,
                       lchd_cloud& cl, bool allow_wide) {
    auto take = [&](size_t bytes) { off = (off + 255) & ~size_t(255); const size_t o = off; off += bytes; return o; };
    const size_t m = (size_t)std::max<int64_t>(n, 1);
    const size_t ox = take(8 * m), oy = take(8 * m), oz = take(8 * m), ot = take(4 * m), oc = take(m), och = take(m);
    cl.x = reinterpret_cast<double*>(d_base + ox);
    cl.y = reinterpret_cast<double*>(d_base + oy);
    cl.z = reinterpret_cast<double*>(d_base + oz);
    cl.tag = reinterpret_cast<int32_t*>(d_base + ot);
    cl.cat = reinterpret_cast<uint8_t*>(d_base + oc);
    cl.cat_hi = nullptr;
    cl.n = n;
    if (!h_base) return LCHD_OK;  // sizing pass
    // (two-byte ids only under a configuration with more than 255 categories: otherwise an id beyond 254 is simply not in the map)
    const bool wide = allow_wide && cats_need_hi(cat, n);
    if (wide) cl.cat_hi = reinterpret_cast<uint8_t*>(d_base + och);
    double *hx = reinterpret_cast<double*>(h_base + ox), *hy = reinterpret_cast<double*>(h_base + oy), *hz = reinterpret_cast<double*>(h_base + oz);
    int32_t* ht = reinterpret_cast<int32_t*>(h_base + ot);
    uint8_t* hc = reinterpret_cast<uint8_t*>(h_base + oc);
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = 0; i < n; ++i) {
        const double v[3] = {xyz ? xyz[3 * i] : 0.0, xyz ? xyz[3 * i + 1] : 0.0, xyz ? xyz[3 * i + 2] : 0.0};  // (no coordinates: given distance rows)
        if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || !std::isfinite(v[2])) return fail(LCHD_EVALUE, "non-finite coordinate at atom %lld", (long long)i);
        hx[i] = v[0]; hy[i] = v[1]; hz[i] = v[2];
        for (int k = 0; k < 3; ++k) { mn[k] = std::min(mn[k], v[k]); mx[k] = std::max(mx[k], v[k]); }
        ht[i] = tag ? tag[i] : 0;
    }
    cats_encode(cat, n, hc, wide ? reinterpret_cast<uint8_t*>(h_base + och) : nullptr);
    for (int k = 0; k < 3; ++k) { cl.bbmin[k] = n ? mn[k] : 0.0; cl.bbmax[k] = n ? mx[k] : 0.0; }
    return LCHD_OK;
}

// Scores of a host-pointer call with at most this many pairs are stored by the sweep kernels straight into the pinned,
// device-visible staging block (8 bytes per pair over the host link): no device-to-host copy operation behind the pass.
constexpr int64_t kDirectOutPairs = 1 << 16;

static int grow_io(lchd_ctx* c, size_t total) {
    if (total <= c->io_cap) return LCHD_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    (void)hipFree(c->d_io); c->d_io = nullptr;
    if (c->h_io) { (void)hipHostFree(c->h_io); c->h_io = nullptr; }
    c->io_cap = 0;
    const size_t want = total + total / 4 + (1 << 16);
    HIP_TRY(hipMalloc(&c->d_io, want));
    hipError_t e = hipHostMalloc(&c->h_io, want);
    if (e != hipSuccess) {
        (void)hipFree(c->d_io); c->d_io = nullptr; c->h_io = nullptr;
        return fail(LCHD_EDEVICE, "HIP error %d (%s) in hipHostMalloc of the staging block", (int)e, hipGetErrorName(e));
    }
    c->io_cap = want;
    return LCHD_OK;
}

// One host-pointer from_primitives call on one context, split so that a device group can have every device's pass in flight
// at the same time.  `subset` (or nullptr = all pairs) lists the positions in anchors / wf_index / out this context scores.
// Large host-pointer calls (a million pairs: 16 MB of anchors in, 8 MB of scores out) spend more time copying between the caller's
// pageable arrays and the pinned staging block than the GPU spends scoring them.  Above kPipePairs the pair list therefore travels
// in chunks -- chunk k + 1 is copied into the staging block (by up to four threads: one core moves ~10 GB/s, the host link ~50) while
// the DMA engine sends chunk k -- and the scores come back the same way.
constexpr int64_t kPipePairs = (int64_t)1 << 18;
static void parallel_copy(void* dst, const void* src, size_t bytes) {
    const int nt = bytes >= ((size_t)6 << 20) ? 4 : (bytes >= ((size_t)2 << 20) ? 2 : 1);
    if (nt == 1) { memcpy(dst, src, bytes); return; }
    const size_t part = ((bytes / nt) + 4095) & ~(size_t)4095;
    std::thread th[3];
    int started = 0;
    for (int k = 1; k < nt; ++k) {
        const size_t o = (size_t)k * part;
        if (o >= bytes) break;
        const size_t len = std::min(part, bytes - o);
        try {
            th[started] = std::thread([=] { memcpy(static_cast<char*>(dst) + o, static_cast<const char*>(src) + o, len); });
            ++started;
        } catch (...) {  // no thread to be had: this part on the calling thread
            memcpy(static_cast<char*>(dst) + o, static_cast<const char*>(src) + o, len);
        }
    }
    memcpy(dst, src, std::min(part, bytes));
    for (int k = 0; k < started; ++k) th[k].join();
}

struct HostCall {
    lchd_cloud a, b;  // point into the context's device I/O block; referenced by the pending pass until it is finished
    size_t o_out = 0;
    bool direct = false;
    int64_t n = 0;
    bool enqueued = false;
};
static int host_call_enqueue(lchd_ctx* c, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a, const int32_t* tag_a, int64_t n_a,
                             const double* xyz_b, const int32_t* cat_b, const int32_t* tag_b, int64_t n_b, const int64_t* anchors,
                             const int32_t* wf_index, const int64_t* subset, int64_t n, double thr, HostCall& hc) {
    hc.n = n;
    hc.enqueued = false;
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    CTX_GUARD(c);
    if (int rc = lchd_ctx_set_config(c, cfg)) return rc;
    if (n == 0) return LCHD_OK;
    // Everything a call sends to the device travels as ONE block through pinned staging and ONE asynchronous copy; the block
    // and its staging twin belong to the context and only ever grow (the reference clones its arguments per call as well,
    // primitive_atom.rs:5, but a device allocation costs far more than a Vec).
    size_t o_anchors = 0, o_wf = 0, in_bytes = 0, total = 0;
    for (int pass = 0; pass < 2; ++pass) {
        size_t off = 0;
        char* hb = pass ? c->h_io : nullptr;
        if (int rc = stage_cloud(xyz_a, cat_a, tag_a, n_a, hb, c->d_io, off, hc.a, cfg->n_categories > kMaxCategories)) return rc;
        if (int rc = stage_cloud(xyz_b, cat_b, tag_b, n_b, hb, c->d_io, off, hc.b, cfg->n_categories > kMaxCategories)) return rc;
        auto take = [&](size_t bytes) { off = (off + 255) & ~size_t(255); const size_t o = off; off += bytes; return o; };
        o_anchors = take(sizeof(int64_t) * 2 * (size_t)n);
        o_wf = take(wf_index ? sizeof(int32_t) * (size_t)n : 0);
        in_bytes = off;
        hc.o_out = take(sizeof(double) * (size_t)n);
        total = off;
        if (pass == 0)
            if (int rc = grow_io(c, total)) return rc;
    }
    int64_t* ha = reinterpret_cast<int64_t*>(c->h_io + o_anchors);
    int32_t* hw = reinterpret_cast<int32_t*>(c->h_io + o_wf);
    bool piped = false;
    if (!subset && n >= kPipePairs) {
        // the structures (and whatever lies in front of the pair list) first, then the list chunk by chunk: the copy of chunk k + 1
        // into the staging block overlaps the DMA of chunk k
        HIP_TRY(hipMemcpyAsync(c->d_io, c->h_io, o_anchors, hipMemcpyHostToDevice, c->stream));
        const int64_t chunk = std::max<int64_t>(kPipePairs, (n + 3) / 4);
        for (int64_t p0 = 0; p0 < n; p0 += chunk) {
            const size_t o = o_anchors + sizeof(int64_t) * 2 * (size_t)p0, len = sizeof(int64_t) * 2 * (size_t)std::min<int64_t>(chunk, n - p0);
            parallel_copy(c->h_io + o, reinterpret_cast<const char*>(anchors) + (o - o_anchors), len);
            HIP_TRY(hipMemcpyAsync(c->d_io + o, c->h_io + o, len, hipMemcpyHostToDevice, c->stream));
        }
        if (wf_index) {
            parallel_copy(hw, wf_index, sizeof(int32_t) * (size_t)n);
            HIP_TRY(hipMemcpyAsync(c->d_io + o_wf, c->h_io + o_wf, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
        }
        piped = true;
    } else if (!subset) {
        memcpy(ha, anchors, sizeof(int64_t) * 2 * (size_t)n);
        if (wf_index) memcpy(hw, wf_index, sizeof(int32_t) * (size_t)n);
    } else {
        for (int64_t k = 0; k < n; ++k) {
            ha[2 * k] = anchors[2 * subset[k]];
            ha[2 * k + 1] = anchors[2 * subset[k] + 1];
            if (wf_index) hw[k] = wf_index[subset[k]];
        }
    }
    if (!piped) HIP_TRY(hipMemcpyAsync(c->d_io, c->h_io, in_bytes, hipMemcpyHostToDevice, c->stream));
    const int64_t* d_anchors = reinterpret_cast<const int64_t*>(c->d_io + o_anchors);
    const int32_t* d_wf = wf_index ? reinterpret_cast<const int32_t*>(c->d_io + o_wf) : nullptr;
    hc.direct = n <= kDirectOutPairs;
    double* d_out = reinterpret_cast<double*>((hc.direct ? c->h_io : c->d_io) + hc.o_out);
    if (int rc = lchd_from_primitives_dev_async(c, &hc.a, &hc.b, d_anchors, d_wf, n, thr, d_out)) return rc;
    hc.enqueued = true;
    return LCHD_OK;
}
static int host_call_finish(lchd_ctx* c, HostCall& hc, const int64_t* subset, double* out) {
    if (!hc.enqueued) return LCHD_OK;
    hc.enqueued = false;
    CTX_GUARD(c);
    int rc = lchd_ctx_finish(c);
    if (!rc && !hc.direct && !subset && hc.n >= kPipePairs) {
        // the scores come back in chunks: chunk k is copied out to the caller's array while the DMA engine fetches chunk k + 1
        const int64_t chunk = std::max<int64_t>(kPipePairs, (hc.n + 3) / 4);
        hipError_t e = hipSuccess;
        int n_ev = 0;
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int64_t p0 = 0; p0 < hc.n && e == hipSuccess; p0 += chunk, ++n_ev) {
            const size_t o = hc.o_out + sizeof(double) * (size_t)p0, len = sizeof(double) * (size_t)std::min<int64_t>(chunk, hc.n - p0);
            e = hipMemcpyAsync(c->h_io + o, c->d_io + o, len, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[n_ev], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventRecord(ev[n_ev], c->stream);
        }
        int k = 0;
        for (int64_t p0 = 0; p0 < hc.n && e == hipSuccess; p0 += chunk, ++k) {
            e = hipEventSynchronize(ev[k]);
            if (e == hipSuccess)
                parallel_copy(out + p0, c->h_io + hc.o_out + sizeof(double) * (size_t)p0, sizeof(double) * (size_t)std::min<int64_t>(chunk, hc.n - p0));
        }
        for (int q = 0; q < 4; ++q)
            if (ev[q]) (void)hipEventDestroy(ev[q]);
        if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); rc = fail(LCHD_EDEVICE, "HIP error %d in D2H scores", (int)e); }
        c->last_valid = false;
        c->pend.req.a = c->pend.req.b = nullptr;
        return rc;
    }
    if (!rc && !hc.direct) {
        hipError_t e = hipMemcpyAsync(c->h_io + hc.o_out, c->d_io + hc.o_out, sizeof(double) * (size_t)hc.n, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = fail(LCHD_EDEVICE, "HIP error %d in D2H scores", (int)e);
    }
    if (!rc) {
        const double* h = reinterpret_cast<const double*>(c->h_io + hc.o_out);
        if (!subset) memcpy(out, h, sizeof(double) * (size_t)hc.n);
        else for (int64_t k = 0; k < hc.n; ++k) out[subset[k]] = h[k];
    }
    c->last_valid = false;  // the anchors of this call live in the I/O block, which the next call overwrites
    c->pend.req.a = c->pend.req.b = nullptr;  // the clouds of the call are gone
    return rc;
}

extern "C" int lchd_from_primitives(lchd_ctx* c, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a,
                                    const int32_t* tag_a, int64_t n_a, const double* xyz_b, const int32_t* cat_b,
                                    const int32_t* tag_b, int64_t n_b, const int64_t* anchors, const int32_t* wf_index,
                                    int64_t n_pairs, double thr, double* out) {
    CTX_LOCK(c);
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    if (int rc = check_wf_index(cfg, wf_index, n_pairs)) return rc;
    if (n_a < 0 || n_b < 0 || n_a > ((int64_t)1 << 30) || n_b > ((int64_t)1 << 30)) return fail(LCHD_EUNSUPPORTED, "structure size out of range");
    HostCall hc;
    if (int rc = host_call_enqueue(c, cfg, xyz_a, cat_a, tag_a, n_a, xyz_b, cat_b, tag_b, n_b, anchors, wf_index, nullptr, n_pairs, thr, hc)) return rc;
    return host_call_finish(c, hc, nullptr, out);
}

// What a host-array entry point that runs as a device call holds for its duration: temporary clouds and one device block.  Destroyed
// on exit (the clouds in the order given); a failed call keeps its own error message, whatever the clean-up's calls report.
struct HostTemps {
    lchd_ctx* c;
    lchd_cloud* clouds[4] = {nullptr, nullptr, nullptr, nullptr};
    char* d_blk = nullptr;
    int rc = LCHD_OK;  // the call's result, set by the owner before it returns
    explicit HostTemps(lchd_ctx* ctx) : c(ctx) {}
    ~HostTemps() {
        const std::string msg = g_err;
        for (lchd_cloud* cl : clouds) lchd_cloud_destroy(c, cl);
        (void)hipFree(d_blk);
        if (rc) snprintf(g_err, sizeof g_err, "%s", msg.c_str());
    }
    HostTemps(const HostTemps&) = delete;
    HostTemps& operator=(const HostTemps&) = delete;
};

// from_primitives in a periodic box: both structures go to the device as clouds of their own, a side with a box is replaced by its
// image cloud (reach = the threshold) and the pass runs as for any two clouds.  lchd_from_primitives above is untouched.
// (a side has at most one of box / cell; the public calls below pass one family each)
static int from_primitives_periodic(lchd_ctx* c, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a, const int32_t* tag_a,
                                    int64_t n_a, const double* xyz_b, const int32_t* cat_b, const int32_t* tag_b, int64_t n_b,
                                    const int64_t* anchors, const int32_t* wf_index, int64_t n_pairs, double thr, const double* box_a,
                                    const double* box_b, const double* cell_a, const double* cell_b, double* out) {
    CTX_LOCK(c);
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    if (int rc = check_wf_index(cfg, wf_index, n_pairs)) return rc;
    if (n_a < 0 || n_b < 0 || n_a > ((int64_t)1 << 27) || n_b > ((int64_t)1 << 27)) return fail(LCHD_EUNSUPPORTED, "structure size out of range");
    if (box_a) if (int rc = lchd_box_validate(box_a, 1, thr)) return rc;
    if (box_b) if (int rc = lchd_box_validate(box_b, 1, thr)) return rc;
    if (cell_a) if (int rc = lchd_cell_validate(cell_a, 1, thr)) return rc;
    if (cell_b) if (int rc = lchd_cell_validate(cell_b, 1, thr)) return rc;
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    if (n_pairs > 0 && (!anchors || !out)) return fail(LCHD_EVALUE, "null anchor / score pointer");
    for (int64_t p = 0; p < n_pairs; ++p)  // (an index beyond the structure would name a ghost atom of the image cloud)
        if (anchors[2 * p] < 0 || anchors[2 * p] >= n_a || anchors[2 * p + 1] < 0 || anchors[2 * p + 1] >= n_b)
            return fail(LCHD_EPANIC, "index out of bounds: an anchor index is outside its structure (src/locohd.rs:521)");
    CTX_GUARD(c);
    if (int rc = lchd_ctx_set_config(c, cfg)) return rc;
    if (n_pairs <= 0) return LCHD_OK;
    HostTemps t(c);
    lchd_cloud *&ia = t.clouds[0], *&ib = t.clouds[1], *&ca = t.clouds[2], *&cb = t.clouds[3];
    char*& d_blk = t.d_blk;
    const size_t o_wf = sizeof(int64_t) * 2 * (size_t)n_pairs, o_out = (o_wf + sizeof(int32_t) * (size_t)n_pairs + 255) & ~size_t(255);
    auto run = [&]() -> int {
        if (int rc = lchd_cloud_create(c, xyz_a, cat_a, tag_a, n_a, &ca)) return rc;
        if (int rc = lchd_cloud_create(c, xyz_b, cat_b, tag_b, n_b, &cb)) return rc;
        if (box_a) if (int rc = lchd_cloud_create_images(c, ca, box_a, 1, thr, &ia)) return rc;
        if (box_b) if (int rc = lchd_cloud_create_images(c, cb, box_b, 1, thr, &ib)) return rc;
        if (cell_a) if (int rc = lchd_cloud_create_images_cell(c, ca, cell_a, 1, thr, &ia)) return rc;
        if (cell_b) if (int rc = lchd_cloud_create_images_cell(c, cb, cell_b, 1, thr, &ib)) return rc;
        HIP_TRY(hipMalloc(&d_blk, o_out + sizeof(double) * (size_t)n_pairs));
        HIP_TRY(hipMemcpy(d_blk, anchors, o_wf, hipMemcpyHostToDevice));
        if (wf_index) HIP_TRY(hipMemcpy(d_blk + o_wf, wf_index, sizeof(int32_t) * (size_t)n_pairs, hipMemcpyHostToDevice));
        if (int rc = lchd_from_primitives_dev(c, ia ? ia : ca, ib ? ib : cb, reinterpret_cast<const int64_t*>(d_blk),
                                              wf_index ? reinterpret_cast<const int32_t*>(d_blk + o_wf) : nullptr, n_pairs, thr,
                                              reinterpret_cast<double*>(d_blk + o_out)))
            return rc;
        HIP_TRY(hipMemcpy(out, d_blk + o_out, sizeof(double) * (size_t)n_pairs, hipMemcpyDeviceToHost));
        return LCHD_OK;
    };
    t.rc = run();
    c->last_valid = false;  // the anchors and the clouds of this call go away (`t` destroys them on return)
    c->pend.req.a = c->pend.req.b = nullptr;
    return t.rc;
}
extern "C" int lchd_from_primitives_periodic(lchd_ctx* c, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a,
                                             const int32_t* tag_a, int64_t n_a, const double* xyz_b, const int32_t* cat_b,
                                             const int32_t* tag_b, int64_t n_b, const int64_t* anchors, const int32_t* wf_index,
                                             int64_t n_pairs, double thr, const double* box_a, const double* box_b, double* out) {
    return from_primitives_periodic(c, cfg, xyz_a, cat_a, tag_a, n_a, xyz_b, cat_b, tag_b, n_b, anchors, wf_index, n_pairs, thr, box_a, box_b,
                                    nullptr, nullptr, out);
}
// The same with triclinic cells (HOST [9], row 0 = a; NULL: an open side).
extern "C" int lchd_from_primitives_periodic_cell(lchd_ctx* c, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a,
                                                  const int32_t* tag_a, int64_t n_a, const double* xyz_b, const int32_t* cat_b,
                                                  const int32_t* tag_b, int64_t n_b, const int64_t* anchors, const int32_t* wf_index,
                                                  int64_t n_pairs, double thr, const double* cell_a, const double* cell_b, double* out) {
    return from_primitives_periodic(c, cfg, xyz_a, cat_a, tag_a, n_a, xyz_b, cat_b, tag_b, n_b, anchors, wf_index, n_pairs, thr, nullptr, nullptr,
                                    cell_a, cell_b, out);
}

// ------------------------------------------------------------------------------------------------
// Sharding of an anchor-pair list by side-A anchor: the rule of lchd_kernels.hip (k_shard_plan), on the host
// ------------------------------------------------------------------------------------------------
// key side 0: bins of the side-A anchor; 1: of the side-B anchor (side A's partition is unbalanced: a rank would hold more than
// 1.25 P / world + 1 pairs -- one reference anchor against thousands, python_codes/kras_scan.py:46-52); 2: contiguous slices
static int shard_rule_host(const int64_t* anchors, int64_t n_pairs, int64_t n_atoms_a, int64_t n_atoms_b, int world, std::vector<uint16_t>& rank_of_bin) {
    auto bin_of = [](int64_t a, int64_t n) { a = a < 0 ? 0 : (a >= n ? n - 1 : a); return (int)((a * kShardBins) / n); };
    std::vector<uint64_t> ha(kShardBins, 0), hb(kShardBins, 0);
    for (int64_t p = 0; p < n_pairs; ++p) {
        ++ha[bin_of(anchors[2 * p], n_atoms_a)];
        if (n_atoms_b > 0) ++hb[bin_of(anchors[2 * p + 1], n_atoms_b)];
    }
    auto plan_side = [&](const std::vector<uint64_t>& hist) {  // fills rank_of_bin; true: balanced
        std::vector<uint64_t> cnt((size_t)world, 0);
        rank_of_bin.assign(kShardBins, 0);
        uint64_t pre = 0;
        for (int b = 0; b < kShardBins; ++b) {
            const uint64_t r = std::min<uint64_t>(n_pairs > 0 ? (pre * (uint64_t)world) / (uint64_t)n_pairs : 0, (uint64_t)world - 1);
            rank_of_bin[b] = (uint16_t)r;
            cnt[r] += hist[b];
            pre += hist[b];
        }
        return *std::max_element(cnt.begin(), cnt.end()) * 4ull * (uint64_t)world <= 5ull * (uint64_t)n_pairs + 4ull * (uint64_t)world;
    };
    if (plan_side(ha)) return 0;
    if (n_atoms_b > 0 && plan_side(hb)) return 1;
    return 2;
}

static int shard_plan_enqueue(lchd_ctx* c, const int64_t* d_anchors, const int64_t* h_src, int64_t n_pairs, int64_t n_atoms_a, int64_t n_atoms_b,
                              int32_t world);
static int shard_plan_wait(lchd_ctx* c, int64_t n_pairs, int64_t n_atoms_a, int64_t n_atoms_b, int32_t world, int64_t* counts_out);

struct lchd_group {
    mutable std::mutex mu;  // lchd_group_from_primitives / lchd_group_last_counts are serialised per group
    std::vector<lchd_ctx*> ctx;
    std::vector<int64_t> last_counts;
    // the caller's pair list and the scores in the caller's order: pinned, visible to every device of the group (grow-only)
    int64_t* h_list = nullptr;
    double* h_out = nullptr;
    char* h_stage = nullptr;  // both structures, staged ONCE per call (SoA, categories, tags): every device copies from here
    size_t list_cap = 0, out_cap = 0, stage_cap = 0;
};

extern "C" int lchd_group_create(const int32_t* devices, int32_t n_devices, lchd_group** out) {
    if (!devices || !out || n_devices < 1 || n_devices > kShardMaxWorld) return fail(LCHD_EVALUE, "a device group needs 1..%d devices", kShardMaxWorld);
    *out = nullptr;
    lchd_group* g = new lchd_group();
    for (int k = 0; k < n_devices; ++k) {
        lchd_ctx* c = nullptr;
        if (int rc = lchd_ctx_create(devices[k], &c)) { lchd_group_destroy(g); return rc; }
        g->ctx.push_back(c);
    }
    g->last_counts.assign((size_t)n_devices, 0);
    *out = g;
    return LCHD_OK;
}
extern "C" void lchd_group_destroy(lchd_group* g) {
    if (!g) return;
    for (lchd_ctx* c : g->ctx) lchd_ctx_destroy(c);
    if (g->h_list) (void)hipHostFree(g->h_list);
    if (g->h_out) (void)hipHostFree(g->h_out);
    if (g->h_stage) (void)hipHostFree(g->h_stage);
    delete g;
}

// Device-side partition of a group call (no per-pair work on the calling thread): the pair list goes ONCE into a pinned block that
// every device copies from; every device plans the partition itself (k_shard_plan: the same pure function of the list on all of
// them), selects its share (k_shard_select), scores it, and writes its scores straight to their positions in ONE pinned, host-mapped
// score block (k_scatter_scores); the caller gets one bulk copy of that block.  The calling thread touches the list twice (copy in,
// copy out) whatever the number of devices; the host-side partition it replaces walked the list once per step of: histogram, W index
// lists, gather into W staging blocks, scatter of the scores -- ~5 ns per pair that did not shrink with W.
struct GroupDev {
    lchd_cloud a, b;
    size_t o_list = 0, o_sel = 0, o_idx = 0, o_sc = 0;
    int64_t n_mine = 0;
    bool planned = false, enqueued = false;
};
static int group_call_device_partition(lchd_group* g, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a, const int32_t* tag_a,
                                       int64_t n_a, const double* xyz_b, const int32_t* cat_b, const int32_t* tag_b, int64_t n_b,
                                       const int64_t* anchors, int64_t n_pairs, double thr, double* out) {
    const int world = (int)g->ctx.size();
    const size_t list_bytes = sizeof(int64_t) * 2 * (size_t)n_pairs, out_bytes = sizeof(double) * (size_t)n_pairs;
    if (g->list_cap < list_bytes) {
        if (g->h_list) (void)hipHostFree(g->h_list);
        g->h_list = nullptr; g->list_cap = 0;
        HIP_TRY(hipHostMalloc(&g->h_list, list_bytes + list_bytes / 8, hipHostMallocPortable | hipHostMallocMapped));
        g->list_cap = list_bytes + list_bytes / 8;
    }
    if (g->out_cap < out_bytes) {
        if (g->h_out) (void)hipHostFree(g->h_out);
        g->h_out = nullptr; g->out_cap = 0;
        HIP_TRY(hipHostMalloc(&g->h_out, out_bytes + out_bytes / 8, hipHostMallocPortable | hipHostMallocMapped));
        g->out_cap = out_bytes + out_bytes / 8;
    }
    memcpy(g->h_list, anchors, list_bytes);  // (the caller's memory is pageable: one copy, every device reads the pinned block)
    std::vector<GroupDev> dev((size_t)world);
    int first_rc = LCHD_OK;
    char first_msg[sizeof g_err] = "";
    auto note = [&](int rc) {
        if (rc && !first_rc) { first_rc = rc; memcpy(first_msg, g_err, sizeof g_err); }
        return rc;
    };
    const int64_t slot = n_pairs / world + n_pairs / (2 * world) + 4096;  // most pairs of a share under the balance rule (1.25 P / W + 1), with headroom
    // 1. both structures are staged ONCE (AoS -> SoA, finiteness, bounding box: host work that must not grow with the number of
    //    devices) into the group's pinned block; every device copies them and the pair list from there and plans the partition
    lchd_cloud sa, sb;  // device pointers relative to a null base: offsets
    size_t in_bytes = 0;
    {
        size_t off = 0;
        if (int rc = stage_cloud(xyz_a, cat_a, tag_a, n_a, nullptr, nullptr, off, sa, cfg->n_categories > kMaxCategories)) return rc;
        if (int rc = stage_cloud(xyz_b, cat_b, tag_b, n_b, nullptr, nullptr, off, sb, cfg->n_categories > kMaxCategories)) return rc;
        in_bytes = off;
        if (g->stage_cap < in_bytes) {
            if (g->h_stage) (void)hipHostFree(g->h_stage);
            g->h_stage = nullptr; g->stage_cap = 0;
            HIP_TRY(hipHostMalloc(&g->h_stage, in_bytes + in_bytes / 8, hipHostMallocPortable));
            g->stage_cap = in_bytes + in_bytes / 8;
        }
        off = 0;
        if (int rc = stage_cloud(xyz_a, cat_a, tag_a, n_a, g->h_stage, nullptr, off, sa, cfg->n_categories > kMaxCategories)) return rc;
        if (int rc = stage_cloud(xyz_b, cat_b, tag_b, n_b, g->h_stage, nullptr, off, sb, cfg->n_categories > kMaxCategories)) return rc;
    }
    auto rebase = [](const lchd_cloud& src, char* d_base) {  // the staged structure as device `d_base` sees it
        lchd_cloud cl = src;
        auto mv = [&](auto*& p) { p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(d_base + reinterpret_cast<uintptr_t>(p)); };
        mv(cl.x); mv(cl.y); mv(cl.z); mv(cl.tag); mv(cl.cat);  // (offsets from a null base; x sits at offset 0)
        if (cl.cat_hi) mv(cl.cat_hi);                            // (absent unless the configuration has more than 255 categories)
        return cl;
    };
    for (int r = 0; r < world; ++r) {
        lchd_ctx* c = g->ctx[(size_t)r];
        GroupDev& D = dev[(size_t)r];
        if (c->pend.active) { note(fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)")); continue; }
        CTX_GUARD(c);
        if (note(lchd_ctx_set_config(c, cfg))) continue;
        size_t off = in_bytes;
        auto take = [&](size_t bytes) { off = (off + 255) & ~size_t(255); const size_t o = off; off += bytes; return o; };
        D.o_list = take(list_bytes);
        D.o_sel = take(sizeof(int64_t) * 2 * (size_t)slot);
        D.o_idx = take(sizeof(int64_t) * (size_t)slot);
        D.o_sc = take(sizeof(double) * (size_t)slot);
        if (note(grow_io(c, off))) continue;
        D.a = rebase(sa, c->d_io);
        D.b = rebase(sb, c->d_io);
        if (hipMemcpyAsync(c->d_io, g->h_stage, in_bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) { note(fail(LCHD_EDEVICE, "H2D copy of the structures failed")); continue; }
        if (note(shard_plan_enqueue(c, reinterpret_cast<const int64_t*>(c->d_io + D.o_list), g->h_list, n_pairs, n_a, n_b, world))) continue;
        D.planned = true;
    }
    // 2. every device: its share's size, the selection, the pass
    for (int r = 0; r < world; ++r) {
        lchd_ctx* c = g->ctx[(size_t)r];
        GroupDev& D = dev[(size_t)r];
        if (!D.planned) continue;
        CTX_GUARD(c);
        int64_t counts[kShardMaxWorld];
        if (note(shard_plan_wait(c, n_pairs, n_a, n_b, world, counts))) continue;
        D.n_mine = counts[r];
        g->last_counts[(size_t)r] = D.n_mine;
        if (D.n_mine > slot) { note(fail(LCHD_EDEVICE, "a share of %lld pairs exceeds the slot of %lld", (long long)D.n_mine, (long long)slot)); continue; }
        if (D.n_mine == 0) continue;
        int64_t* d_sel = reinterpret_cast<int64_t*>(c->d_io + D.o_sel);
        int64_t* d_idx = reinterpret_cast<int64_t*>(c->d_io + D.o_idx);
        if (note(lchd_shard_select_dev(c, reinterpret_cast<const int64_t*>(c->d_io + D.o_list), n_pairs, n_a, n_b, r, d_sel, d_idx))) continue;
        if (note(lchd_from_primitives_dev_async(c, &D.a, &D.b, d_sel, nullptr, D.n_mine, thr, reinterpret_cast<double*>(c->d_io + D.o_sc)))) continue;
        D.enqueued = true;
    }
    // 3. finish (capacity retries happen here), then the scores to their positions in the pinned block
    for (int r = 0; r < world; ++r) {
        lchd_ctx* c = g->ctx[(size_t)r];
        GroupDev& D = dev[(size_t)r];
        if (!D.enqueued) continue;
        CTX_GUARD(c);
        if (note(lchd_ctx_finish(c))) { D.enqueued = false; continue; }
        launch_scatter_scores(c->stream, reinterpret_cast<const double*>(c->d_io + D.o_sc), reinterpret_cast<const int64_t*>(c->d_io + D.o_idx),
                              D.n_mine, g->h_out);
    }
    for (int r = 0; r < world; ++r) {
        lchd_ctx* c = g->ctx[(size_t)r];
        GroupDev& D = dev[(size_t)r];
        c->last_valid = false;
        c->pend.req.a = c->pend.req.b = nullptr;  // the structures of the call live in the I/O block, which the next call overwrites
        if (!D.enqueued) continue;
        CTX_GUARD(c);
        if (hipStreamSynchronize(c->stream) != hipSuccess) note(fail(LCHD_EDEVICE, "HIP error while waiting for device %d of the group", r));
    }
    if (first_rc) { memcpy(g_err, first_msg, sizeof g_err); return first_rc; }
    memcpy(out, g->h_out, out_bytes);
    return LCHD_OK;
}
extern "C" int32_t lchd_group_size(const lchd_group* g) { return g ? (int32_t)g->ctx.size() : 0; }
extern "C" int lchd_group_last_counts(const lchd_group* g, int64_t* counts_out) {
    if (!g || !counts_out) return fail(LCHD_EVALUE, "null argument");
    std::lock_guard<std::mutex> lk(g->mu);
    for (size_t k = 0; k < g->ctx.size(); ++k) counts_out[k] = g->last_counts[k];
    return LCHD_OK;
}

extern "C" int lchd_group_from_primitives(lchd_group* g, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a,
                                          const int32_t* tag_a, int64_t n_a, const double* xyz_b, const int32_t* cat_b,
                                          const int32_t* tag_b, int64_t n_b, const int64_t* anchors, const int32_t* wf_index,
                                          int64_t n_pairs, double thr, double* out) {
    if (!g || !cfg || g->ctx.empty()) return fail(LCHD_EVALUE, "null group / configuration");
    std::lock_guard<std::mutex> lk(g->mu);
    if (int rc = check_wf_index(cfg, wf_index, n_pairs)) return rc;
    if (n_a < 0 || n_b < 0 || n_a > ((int64_t)1 << 30) || n_b > ((int64_t)1 << 30)) return fail(LCHD_EUNSUPPORTED, "structure size out of range");
    const int world = (int)g->ctx.size();
    std::fill(g->last_counts.begin(), g->last_counts.end(), 0);
    if (n_pairs <= 0) {
        for (lchd_ctx* c : g->ctx)
            if (int rc = lchd_ctx_set_config(c, cfg)) return rc;  // the reference validates its arguments even for an empty list
        return LCHD_OK;
    }
    // several devices, one weight function: the partition runs on the devices (above)
    if (world > 1 && n_a > 0 && !wf_index)
        return group_call_device_partition(g, cfg, xyz_a, cat_a, tag_a, n_a, xyz_b, cat_b, tag_b, n_b, anchors, n_pairs, thr, out);
    // the pair list, binned by anchor (the rule of k_shard_plan): device r gets the positions subset[r]
    std::vector<std::vector<int64_t>> subset((size_t)world);
    if (world == 1 || n_a <= 0) {
        subset[0].resize((size_t)n_pairs);
        for (int64_t p = 0; p < n_pairs; ++p) subset[0][(size_t)p] = p;
    } else {
        std::vector<uint16_t> rob;
        const int mode = shard_rule_host(anchors, n_pairs, n_a, n_b, world, rob);
        for (int r = 0; r < world; ++r) subset[(size_t)r].reserve((size_t)(n_pairs / world + n_pairs / (4 * world) + 16));
        for (int64_t p = 0; p < n_pairs; ++p) {
            if (mode == 2) { subset[(size_t)((p * world) / n_pairs)].push_back(p); continue; }
            const int64_t n = mode == 1 ? n_b : n_a;
            int64_t a = anchors[2 * p + (mode == 1 ? 1 : 0)];
            a = a < 0 ? 0 : (a >= n ? n - 1 : a);
            subset[rob[(size_t)((a * kShardBins) / n)]].push_back(p);
        }
    }
    // enqueue every device's pass (asynchronous), then collect: the devices work concurrently
    std::vector<HostCall> calls((size_t)world);
    int first_rc = LCHD_OK;
    char first_msg[sizeof g_err] = "";
    auto note = [&](int rc) {
        if (rc && !first_rc) { first_rc = rc; memcpy(first_msg, g_err, sizeof g_err); }
    };
    for (int r = 0; r < world; ++r) {
        g->last_counts[(size_t)r] = (int64_t)subset[(size_t)r].size();
        note(host_call_enqueue(g->ctx[(size_t)r], cfg, xyz_a, cat_a, tag_a, n_a, xyz_b, cat_b, tag_b, n_b, anchors, wf_index,
                               subset[(size_t)r].data(), (int64_t)subset[(size_t)r].size(), thr, calls[(size_t)r]));
    }
    for (int r = 0; r < world; ++r) note(host_call_finish(g->ctx[(size_t)r], calls[(size_t)r], subset[(size_t)r].data(), out));
    if (first_rc) memcpy(g_err, first_msg, sizeof g_err);
    return first_rc;
}

// ---- one process per GPU: the same partition on the device ------------------------------------------------------------
static int ensure_shard_state(lchd_ctx* c) {
    if (c->d_shard) return LCHD_OK;
    // The plan kernel runs on a NON-BLOCKING side stream, which is not ordered behind work of the null stream: the state is
    // zeroed ON that stream (a plain hipMemset may still be pending when the first plan starts and would then wipe the
    // plan's bin table under the selection kernel), and the call waits for it.
    hipError_t e = hipStreamCreateWithFlags(&c->shard_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->shard_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->shard_sel_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc(&c->d_shard, sizeof(ShardState));
    if (e == hipSuccess) e = hipMemsetAsync(c->d_shard, 0, sizeof(ShardState), c->shard_stream);
    if (e == hipSuccess) e = hipHostMalloc(&c->h_counts, sizeof(int64_t) * (kShardMaxWorld + 1));
    if (e == hipSuccess) e = hipMalloc(&c->d_bad, sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemsetAsync(c->d_bad, 0, sizeof(uint32_t), c->shard_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->shard_stream);
    if (e != hipSuccess) {
        if (c->shard_stream) { (void)hipStreamDestroy(c->shard_stream); c->shard_stream = nullptr; }
        if (c->shard_ev) { (void)hipEventDestroy(c->shard_ev); c->shard_ev = nullptr; }
        if (c->shard_sel_ev) { (void)hipEventDestroy(c->shard_sel_ev); c->shard_sel_ev = nullptr; }
        (void)hipFree(c->d_shard); c->d_shard = nullptr;
        if (c->h_counts) { (void)hipHostFree(c->h_counts); c->h_counts = nullptr; }
        (void)hipFree(c->d_bad); c->d_bad = nullptr;
        return fail(LCHD_EDEVICE, "HIP error %d (%s) while allocating the sharding state", (int)e, hipGetErrorName(e));
    }
    return LCHD_OK;
}
// The plan in two halves: enqueue (asynchronous, on the context's side stream) and wait (the per-rank counts come back through
// pinned memory).  A caller that drives several devices enqueues all plans before it waits for the first.
// h_src: when not null the pair list is first copied from this (pinned) host block to d_anchors, on the same side stream.
static int shard_plan_enqueue(lchd_ctx* c, const int64_t* d_anchors, const int64_t* h_src, int64_t n_pairs, int64_t n_atoms_a, int64_t n_atoms_b,
                              int32_t world) {
    c->shard_world = 0;
    if (int rc = ensure_shard_state(c)) return rc;
    // On the context's side stream: the pair list is an INPUT (the caller has it ready), so the plan neither waits for the
    // scoring passes queued on the context's stream nor makes the host wait for them.
    if (c->shard_sel_pending) { HIP_TRY(hipStreamWaitEvent(c->shard_stream, c->shard_sel_ev, 0)); c->shard_sel_pending = false; }
    if (h_src) HIP_TRY(hipMemcpyAsync(const_cast<int64_t*>(d_anchors), h_src, sizeof(int64_t) * 2 * (size_t)n_pairs, hipMemcpyHostToDevice, c->shard_stream));
    launch_shard_plan(c->shard_stream, d_anchors, n_pairs, n_atoms_a, n_atoms_b, world, c->d_shard, c->h_counts);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->shard_ev, c->shard_stream));
    return LCHD_OK;
}
static int shard_plan_wait(lchd_ctx* c, int64_t n_pairs, int64_t n_atoms_a, int64_t n_atoms_b, int32_t world, int64_t* counts_out) {
    HIP_TRY(hipStreamSynchronize(c->shard_stream));
    int64_t total = 0;
    for (int r = 0; r < world; ++r) { counts_out[r] = c->h_counts[r]; total += counts_out[r]; }
    if (total != n_pairs) return fail(LCHD_EDEVICE, "the shard plan accounts for %lld of %lld pairs", (long long)total, (long long)n_pairs);
    c->shard_world = world; c->shard_pairs = n_pairs; c->shard_atoms = n_atoms_a; c->shard_atoms_b = n_atoms_b;
    return LCHD_OK;
}
extern "C" int lchd_shard_plan_dev(lchd_ctx* c, const int64_t* d_anchors, int64_t n_pairs, int64_t n_atoms_a, int64_t n_atoms_b, int32_t world,
                                   int64_t* counts_out) {
    CTX_LOCK(c);
    if (!c || !counts_out) return fail(LCHD_EVALUE, "null argument");
    if (world < 1 || world > kShardMaxWorld) return fail(LCHD_EVALUE, "world size %d outside [1, %d]", world, kShardMaxWorld);
    if (n_pairs < 0 || n_atoms_a < 1) return fail(LCHD_EVALUE, "bad pair / atom count");
    for (int r = 0; r < world; ++r) counts_out[r] = 0;
    c->shard_world = 0;
    if (n_pairs == 0) { c->shard_world = world; c->shard_pairs = 0; c->shard_atoms = n_atoms_a; c->shard_atoms_b = n_atoms_b; return LCHD_OK; }
    if (!d_anchors) return fail(LCHD_EVALUE, "null anchor pointer");
    CTX_GUARD(c);
    if (int rc = shard_plan_enqueue(c, d_anchors, nullptr, n_pairs, n_atoms_a, n_atoms_b, world)) return rc;
    return shard_plan_wait(c, n_pairs, n_atoms_a, n_atoms_b, world, counts_out);
}
extern "C" int lchd_shard_select_dev(lchd_ctx* c, const int64_t* d_anchors, int64_t n_pairs, int64_t n_atoms_a, int64_t n_atoms_b, int32_t rank,
                                     int64_t* d_sel_anchors, int64_t* d_sel_index) {
    CTX_LOCK(c);
    if (!c) return fail(LCHD_EVALUE, "null context");
    if (c->shard_world < 1 || n_pairs != c->shard_pairs || n_atoms_a != c->shard_atoms || n_atoms_b != c->shard_atoms_b)
        return fail(LCHD_EVALUE, "lchd_shard_plan_dev has not been called for this pair list");
    if (rank < 0 || rank >= c->shard_world) return fail(LCHD_EVALUE, "rank %d outside the planned world of %d", rank, c->shard_world);
    if (n_pairs == 0 || c->h_counts[rank] == 0) return LCHD_OK;  // nothing for this rank: the outputs may be null
    if (!d_anchors || !d_sel_anchors || !d_sel_index) return fail(LCHD_EVALUE, "null pointer");
    CTX_GUARD(c);
    HIP_TRY(hipStreamWaitEvent(c->stream, c->shard_ev, 0));
    launch_shard_select(c->stream, d_anchors, n_pairs, n_atoms_a, n_atoms_b, rank, c->shard_world, c->d_shard, d_sel_anchors, d_sel_index);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->shard_sel_ev, c->stream));
    c->shard_sel_pending = true;
    return LCHD_OK;
}
extern "C" int lchd_unshard_scores_dev(lchd_ctx* c, const double* d_gathered, const int64_t* counts, int32_t world, int64_t stride,
                                       double* d_out, int64_t n_pairs) {
    CTX_LOCK(c);
    if (!c || !counts) return fail(LCHD_EVALUE, "null argument");
    if (world < 1 || world > kShardMaxWorld) return fail(LCHD_EVALUE, "world size %d outside [1, %d]", world, kShardMaxWorld);
    ShardCounts sc{};
    int64_t total = 0;
    for (int r = 0; r < world; ++r) {
        if (counts[r] < 0 || counts[r] > stride) return fail(LCHD_EVALUE, "rank %d holds %lld scores in a slot of %lld", r, (long long)counts[r], (long long)stride);
        sc.n[r] = counts[r];
        total += counts[r];
    }
    if (total != n_pairs) return fail(LCHD_EVALUE, "the ranks hold %lld scores for %lld pairs", (long long)total, (long long)n_pairs);
    if (n_pairs == 0) return LCHD_OK;
    if (!d_gathered || !d_out) return fail(LCHD_EVALUE, "null pointer");
    CTX_GUARD(c);
    if (int rc = ensure_shard_state(c)) return rc;
    launch_unshard_scores(c->stream, d_gathered, sc, world, stride, d_out, n_pairs, c->d_bad);
    HIP_TRY(hipGetLastError());
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, c->d_bad, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (bad) {
        (void)hipMemsetAsync(c->d_bad, 0, sizeof(uint32_t), c->stream);
        return fail(LCHD_EVALUE, "a gathered pair position lies outside [0, %lld)", (long long)n_pairs);
    }
    return LCHD_OK;
}

// Shared tail of from_anchors / from_dmxs / from_coords: environments are already sorted in `ea`/`eb`
// (one per row), pair p = (row p, row p).
static int sweep_rows(lchd_ctx* c, const EnvStore& ea, const EnvStore& eb, const int32_t* d_wf, int64_t rows, double* d_out,
                      int4* d_meta, Driver drv, uint32_t* flags_out = nullptr) {
    SweepArgs sw{};
    fill_sweep_args(c, sw);
    sw.env_a = ea;
    sw.env_b = eb;
    sw.wf_index = d_wf;
    sw.n_pairs = rows;
    sw.out = d_out;
    sw.meta = d_meta;
    if (!launch_sweep(c->stream, c->tune, c->h_cfg.n_categories, c->hellinger2, c->unit_weights, c->wf_pow, 0, sw).ok)
        return fail(LCHD_EDEVICE, "internal error: the sweep launch set would not give every pair exactly one kernel");
    mark(c, 4);
    HIP_TRY(hipGetLastError());
    c->status_dirty = false;  // the record pass of this sequence resets the device status
    uint32_t f = 0;
    if (int rc = wait_pass(c, &f)) return rc;
    collect_times(c, 2, 4);
    if (flags_out) *flags_out = f;
    if (f & ST_ROW_RETRY) return LCHD_OK;  // the caller repeats the pass with the other row kernel
    return status_to_rc(f, drv);
}

// Squared diagonal of a cloud's bounding box, with a little headroom: the bound the row kernels take on a squared distance.
static double diag2(const lchd_cloud& cl) {
    double s2 = 0.0;
    for (int k = 0; k < 3; ++k) { const double e = cl.bbmax[k] - cl.bbmin[k]; s2 += e * e; }
    return s2 * (1.0 + 1e-9) + 1e-300;
}
// The store of one side's dense rows: `rows` slots of `cap` points, `sets` key sets (cdf_keys is the caller's).
static EnvStore carve_row_store(Arena& ar, int64_t rows, int64_t cap, size_t sets, bool cat16) {
    EnvStore e{};
    e.key = ar.take<uint64_t>((size_t)rows * cap * sets);
    e.cat = ar.take<uint8_t>((size_t)rows * cap * (cat16 ? 2 : 1));
    e.len = ar.take<int32_t>((size_t)rows);
    e.stride = cap;
    e.set_stride = rows * cap;
    e.cat16 = cat16 ? 1 : 0;
    return e;
}
// Where one side's dense rows come from: the side's cloud as the row kernels read it, its row length, and exactly ONE way to the rows.
// Every dense host pass (dense_pass, consumer_dense, ensemble_core) describes its sides with this and materialises them with the pair
// take_rows / produce_rows below; a periodic cell travels here and nowhere else.
struct RowSource {
    enum Kind {
        COORDS,       // open coordinates: the row kernels read them, or (as_rows) k_ens_dist writes the rows out
        CELL,         // coordinates in a periodic cell: minimum-image rows
        DEVICE_ROWS,  // m: DEVICE [..][cols], passed through
        HOST_ROWS     // m: HOST [..][cols], copied into the workspace
    } kind;
    CloudView view;         // categories; the coordinates of COORDS / CELL
    int64_t cols;
    double bound;           // coordinates read by a row kernel: >= the largest squared distance (diag2), or 0.0
    bool as_rows;           // COORDS in a pass that runs in its given-row form (the other side has a cell; every ensemble)
    const double* m;
    MinImageCell cell;      // CELL: the cell of every structure, or ...
    const double* d_cells;  // ... ensembles with a cell per structure: DEVICE [M][kMinImageRecord]
    bool all_diagonal;      // CELL: every cell is diagonal
    const int32_t* d_len;   // ragged given rows: DEVICE [rows] points of each row, or null
    const int32_t *excl_start, *excl_idx;  // ensembles: DEVICE CSR of excluded columns per row, or null
};
// A single structure's coordinates (or, with `m` set afterwards, its categories alone), optionally in a reduced periodic cell.
static RowSource cloud_source(const lchd_cloud& cl, bool cat16, int64_t cols, const MinImageCell* cell = nullptr) {
    RowSource s{};
    s.kind = cell ? RowSource::CELL : RowSource::COORDS;
    s.view = cl.view(cat16);
    s.cols = cols;
    s.bound = diag2(cl);
    if (cell) { s.cell = *cell; s.all_diagonal = cell->v[18] != 0.0; }
    return s;
}
static bool reads_rows(const RowSource& s) { return s.kind != RowSource::COORDS || s.as_rows; }  // (else: the row kernels read the coordinates)
// What a source needs from the arena for `rows` rows: nothing for rows on the device and coordinates read in place.
static double* take_rows(Arena& ar, const RowSource& s, int64_t rows) {
    return reads_rows(s) && s.kind != RowSource::DEVICE_ROWS ? ar.take<double>((size_t)rows * s.cols) : nullptr;
}
// Enqueues the copy or the producer of rows [row0, row0 + rows) into w (take_rows); d_m: what the row kernels read, null for "the
// coordinates".  row0 is also the first atom (a regular batch: row k * cols + r is atom r of structure k).  Open rows have k_ens_dist's
// arithmetic.  The only caller of the two row producers.
static int produce_rows(lchd_ctx* c, const RowSource& s, int64_t row0, int64_t rows, double* w, const double*& d_m) {
    d_m = w;
    switch (s.kind) {
    case RowSource::DEVICE_ROWS: d_m = s.m + row0 * s.cols; break;
    case RowSource::HOST_ROWS:
        HIP_TRY(hipMemcpyAsync(w, s.m + row0 * s.cols, sizeof(double) * (size_t)rows * s.cols, hipMemcpyHostToDevice, c->stream));
        break;
    case RowSource::CELL:
        launch_min_image_rows(c->stream, s.view, row0, (int32_t)s.cols, rows, s.cell, s.d_cells, s.all_diagonal, s.excl_start, s.excl_idx, w);
        break;
    case RowSource::COORDS:
        if (s.as_rows) launch_ens_dist(c->stream, s.view, row0, (int32_t)s.cols, rows, s.excl_start, s.excl_idx, w);
        break;
    }
    return LCHD_OK;
}
// The row sort of a store-building pass: row r of every side into slot r of its store -- the plan's one k_env_rows2 launch for both
// sides, or one k_env_rows launch per side (plan.rows) -- then, in deterministic mode, one order among equal keys (a row's sort places
// ties by LDS-atomic order).  false: the plan names no instantiation of its kernel; *canon: whether k_env_canon ran.
static bool sort_rows(lchd_ctx* c, const lchd_dense_plan& plan, int sides, const RowSource* src, const double* const* d_m, const EnvStore* e,
                      int64_t rows, int32_t* canon) {
    hipStream_t s = c->stream;
    if (plan.path == LCHD_DENSE_ROWS2) {
        const RowSide a{src[0].view, d_m[0], src[0].cols, src[0].cols, src[0].bound, e[0], src[0].d_len};
        const RowSide b{src[1].view, d_m[1], src[1].cols, src[1].cols, src[1].bound, e[1], src[1].d_len};
        if (!launch_env_rows2(s, plan, c->d_cfg, a, b, rows, c->d_status)) return false;
    } else {
        for (int k = 0; k < sides; ++k)
            if (!launch_env_rows(s, plan.rows[k], c->d_cfg, src[k].view, d_m[k], src[k].cols, rows, src[k].cols, src[k].bound, e[k], c->d_status,
                                 RowExtras{nullptr, src[k].d_len, nullptr}))
                return false;
    }
    *canon = c->deterministic ? 1 : 0;
    if (c->deterministic) launch_env_canon(s, e[0], e[sides - 1], rows, rows * (sides - 1), nullptr);  // (one side: no rows of a second store)
    return true;
}

static lchd_dense_query dense_query(const lchd_ctx* c, int64_t cols_a, int64_t cols_b, bool given_rows, bool ragged, int attempt, bool single_attempt) {
    lchd_dense_query q{};
    q.cols_a = cols_a;
    q.cols_b = cols_b;
    q.n_categories = c->h_cfg.n_categories;
    q.hellinger2 = c->hellinger2 ? 1 : 0;
    q.unit_weights = c->unit_weights ? 1 : 0;
    q.cat16 = c->h_cfg.n_categories > kMaxCategories ? 1 : 0;  // 16-bit ids in the environment store, k_env_rows<.., uint16_t> + k_sweep_wide<.., CAT16>
    q.given_rows = given_rows ? 1 : 0;
    q.ragged = ragged ? 1 : 0;
    q.hooks = (c->tune.old_rows ? (uint32_t)LCHD_DENSE_HOOK_OLD_ROWS : 0u) | (c->tune.no_dense_fused ? (uint32_t)LCHD_DENSE_HOOK_NO_FUSED : 0u);
    q.attempt = attempt;
    q.single_attempt = single_attempt ? 1 : 0;
    return q;
}
// One dense pass (from_coords / from_dmxs semantics: pair r = row r of A against row r of B, the environment is the whole structure):
// row sort of both structures, sweep.
struct DensePass {
    RowSource src[2];
    int64_t rows;
    const int32_t* d_wf;  // DEVICE weight-function indices or null
    double* d_out;        // device or host-mapped scores
};
// `attempt`: 0, or 1 for the repeat of a call; `retry` reports that a row defeated this attempt's kernel (the fused kernel, the
// segmented in-LDS sort): repeat with attempt 1.  The attempt's plan, canon flag and bitonic rows go into c->last_dense.
static int dense_pass(lchd_ctx* c, const DensePass& P, int attempt, bool& retry) {
    retry = false;
    const RowSource *src = P.src, &a = P.src[0], &b = P.src[1];
    const int64_t rows = P.rows;
    c->last_dense_valid = false;
    const lchd_dense_query query = dense_query(c, a.cols, b.cols, reads_rows(a), a.d_len || b.d_len, attempt, false);
    const lchd_dense_plan plan = plan_dense(query);
    if (plan.unsupported) return fail(LCHD_EUNSUPPORTED, "no dense environment kernel for this row length");
    const bool cat16 = query.cat16 != 0;
    c->last_dense.plan = plan;
    c->last_dense.attempts = attempt + 1;
    c->last_dense.canon = 0;
    c->last_dense.n_bitonic = 0;
    // The common configuration (plan_dense: Hellinger-2, unit category weights, <= 16 categories, rows of 1025 .. kDenseFusedMaxRow points): sort and
    // sweep in ONE kernel per row pair, nothing but the score is written (lchd_dense_fused.hip).  No environment store.
    const bool fused = plan.path == LCHD_DENSE_FUSED;
    uint64_t* scr_key = nullptr;
    uint8_t* scr_val = nullptr;
    int32_t scr_grid = 0;
    const size_t scr_n = fused ? dense_fused_scratch(rows, plan.scr_segs, &scr_grid) : 0;
    EnvStore e[2] = {};
    int4* d_meta = nullptr;
    double* w[2] = {nullptr, nullptr};
    for (int dry = 1; dry >= 0; --dry) {
        Arena ar(dry ? nullptr : c->ws, dry ? 0 : c->ws_cap, dry != 0);
        if (fused) {
            scr_key = ar.take<uint64_t>(scr_n);  // the distance pass's (key, value) pairs, one region per workgroup
            scr_val = ar.take<uint8_t>(scr_n);
        } else {
            for (int k = 0; k < 2; ++k) e[k] = carve_row_store(ar, rows, next_pow2_host(src[k].cols), 1, cat16);  // (scoring: one key set)
            d_meta = ar.take<int4>((size_t)rows);
        }
        for (int k = 0; k < 2; ++k) w[k] = take_rows(ar, src[k], rows);
        if (dry) if (int rc2 = ensure_ws(c, ar.off + 4096)) return rc2;
    }
    // a periodic call: events 0 and 1 bracket the row producers of both sides ("cells" of lchd_ctx_last_ms, min_image_time)
    const bool produced = a.kind == RowSource::CELL || b.kind == RowSource::CELL;
    const double* d_m[2] = {nullptr, nullptr};
    if (produced) mark(c, 0);
    for (int k = 0; k < 2; ++k)
        if (int rc2 = produce_rows(c, src[k], 0, rows, w[k], d_m[k])) return rc2;
    if (produced) mark(c, 1);
    if (fused) {
        DenseArgs da{};
        da.cfg = c->d_cfg;
        for (int k = 0; k < 2; ++k) da.s[k] = DenseSide{src[k].view, d_m[k], src[k].cols, (int32_t)src[k].cols, src[k].d_len};
        da.n_rows = rows;
        da.image_bound = std::max(a.bound, b.bound);
        da.wf_index = P.d_wf;
        da.out = P.d_out;
        da.st = c->d_status;
        da.sqrt_tab = c->d_tabs;
        da.scr_key = scr_key;
        da.scr_val = scr_val;
        da.scr_grid = scr_grid;
        da.scr_segs = plan.scr_segs;
        da.ticket = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(c->d_done) + sizeof(DoneState));
        mark(c, 2);
        if (!launch_dense_fused(c->stream, plan, da, c->h_status, c->seq))
            return fail(LCHD_EDEVICE, "internal error: the dense plan names no instantiation of the fused kernel");
        mark(c, 3);
        mark(c, 4);
        HIP_TRY(hipGetLastError());
        c->status_dirty = false;  // the kernel's companion launch hands the status over and resets it
        uint32_t f = 0;
        if (int rc2 = wait_pass(c, &f)) return rc2;
        collect_times(c, 2, 4);
        if (f & ST_ROW_RETRY) { retry = true; return LCHD_OK; }  // a row the fused kernel gives up on: the caller repeats with the two-kernel path
        if (int rc2 = status_to_rc(f, DRV_DMXS)) return rc2;
        c->last_dense_valid = true;
        return LCHD_OK;
    }
    e[0].cdf_keys = e[1].cdf_keys = (c->h_cfg.n_wf == 1 && !c->tune.no_cdf_keys) ? 1 : 0;  // (scoring honours LCHD_NO_CDF_KEYS)
    mark(c, 2);
    if (!sort_rows(c, plan, 2, src, d_m, e, rows, &c->last_dense.canon))  // (plan_dense's choice: k_env_rows2 or k_env_rows)
        return fail(LCHD_EDEVICE, "internal error: the dense plan names no instantiation of the row kernels");
    mark(c, 3);
    uint32_t f = 0;
    if (int rc2 = sweep_rows(c, e[0], e[1], P.d_wf, rows, P.d_out, d_meta, DRV_DMXS, &f)) return rc2;
    c->last_dense.n_bitonic = c->h_status->n_bitonic;
    if (f & ST_ROW_RETRY) retry = true;
    else c->last_dense_valid = true;
    return LCHD_OK;
}

// The attempts of a dense scoring call: the pass, once more when a row defeated the first attempt's kernel (a long row the fused kernel
// or the segmented in-LDS sort gives up on).  in_bytes: a host call's staged inputs, copied from c->h_io at the head of every attempt.
static int dense_attempts(lchd_ctx* c, const DensePass& P, size_t in_bytes) {
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (int rc = begin_pass(c)) return rc;
        c->status_dirty = true;  // until the record pass has been enqueued (sweep_rows)
        if (in_bytes) HIP_TRY(hipMemcpyAsync(c->d_io, c->h_io, in_bytes, hipMemcpyHostToDevice, c->stream));
        bool retry = false;
        if (int rc = dense_pass(c, P, attempt, retry)) return rc;
        if (!retry) break;
    }
    return LCHD_OK;
}
// The refusal of row lengths plan_dense has no kernel for (lchd_dense_plan::unsupported), naming one length or both.
static int fail_dense_rows(int64_t cols_a, int64_t cols_b = -1) {
    char got[48];
    if (cols_b < 0) snprintf(got, sizeof got, "%lld", (long long)cols_a);
    else snprintf(got, sizeof got, "%lld / %lld", (long long)cols_a, (long long)cols_b);
    return fail(LCHD_EUNSUPPORTED, "dense rows of more than 65535 points are supported with at most %d categories and 2^23 points (got %s)",
                kMaxCategories, got);
}

// One side of a dense host call: coordinates (xyz; optionally in a reduced periodic cell) or given rows (dmx [rows][cols]; ragged
// with row_len).
struct DenseHostSide {
    const int32_t* seq;
    int64_t len_seq;
    const double *xyz, *dmx;
    int64_t cols;
    const int32_t* row_len;
    const MinImageCell* cell;
};
static int dense_driver(lchd_ctx* c, const lchd_config* cfg, const DenseHostSide (&sd)[2], int64_t rows, const int32_t* wf_index, double* out) {
    const int64_t cols_a = sd[0].cols, cols_b = sd[1].cols;
    const int32_t *row_len_a = sd[0].row_len, *row_len_b = sd[1].row_len;
    const bool periodic = sd[0].cell || sd[1].cell;  // both structures' rows are materialised and the pass runs in its given-row form
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    CTX_GUARD(c);
    if (int rc = lchd_ctx_set_config(c, cfg)) return rc;
    if (int rc = check_wf_index(cfg, wf_index, rows)) return rc;
    c->last_valid = c->last_sweep_valid = false;
    if (rows == 0) return LCHD_OK;
    // utils.rs:25-39: the sort mask has row-length entries and indexes seq => a row longer than seq panics
    if (cols_a > sd[0].len_seq || cols_b > sd[1].len_seq) return fail(LCHD_EPANIC, "index out of bounds: a distance row is longer than its seq");
    if (cols_a == 0 || cols_b == 0) return fail(LCHD_EPANIC, "index out of bounds: empty distance row (src/locohd.rs:74)");
    if (plan_dense(dense_query(c, cols_a, cols_b, sd[0].dmx || periodic, row_len_a || row_len_b, 0, false)).unsupported)
        return fail_dense_rows(cols_a, cols_b);
    // The two structures (SoA coordinates + categories), the weight-function indices and -- for calls of up to kDirectOutPairs
    // rows -- the scores travel through the context's pinned staging block (one asynchronous copy in, none out); nothing is
    // allocated per call.
    for (int side = 0; side < 2 && (row_len_a || row_len_b); ++side) {  // ragged rows (utils.rs:25-39: a row is sorted with a prefix of seq)
        const int32_t* rl = side ? row_len_b : row_len_a;
        const int64_t cols = side ? cols_b : cols_a;
        if (!rl) return fail(LCHD_EVALUE, "row lengths must be given for both matrices or for neither");
        for (int64_t r = 0; r < rows; ++r) {
            if (rl[r] < 1) return fail(LCHD_EPANIC, "index out of bounds: empty distance row (src/locohd.rs:74)");
            if (rl[r] > cols) return fail(LCHD_EVALUE, "row %lld is longer (%d) than the padded matrix (%lld columns)", (long long)r, rl[r], (long long)cols);
        }
    }
    lchd_cloud a, b;
    const bool cat16 = cfg->n_categories > kMaxCategories;
    size_t o_wf = 0, o_out = 0, in_bytes = 0, o_la = 0, o_lb = 0;
    for (int pass = 0; pass < 2; ++pass) {
        size_t off = 0;
        char* hb = pass ? c->h_io : nullptr;
        if (int rc = stage_cloud(sd[0].xyz, sd[0].seq, nullptr, cols_a, hb, c->d_io, off, a, cat16)) return rc;
        if (int rc = stage_cloud(sd[1].xyz, sd[1].seq, nullptr, cols_b, hb, c->d_io, off, b, cat16)) return rc;
        auto take = [&](size_t bytes) { off = (off + 255) & ~size_t(255); const size_t o = off; off += bytes; return o; };
        o_wf = take(wf_index ? sizeof(int32_t) * (size_t)rows : 0);
        o_la = take(row_len_a ? sizeof(int32_t) * (size_t)rows : 0);
        o_lb = take(row_len_b ? sizeof(int32_t) * (size_t)rows : 0);
        in_bytes = off;
        o_out = take(sizeof(double) * (size_t)rows);
        if (pass == 0)
            if (int rc = grow_io(c, off)) return rc;
    }
    if (wf_index) memcpy(c->h_io + o_wf, wf_index, sizeof(int32_t) * (size_t)rows);
    if (row_len_a) memcpy(c->h_io + o_la, row_len_a, sizeof(int32_t) * (size_t)rows);
    if (row_len_b) memcpy(c->h_io + o_lb, row_len_b, sizeof(int32_t) * (size_t)rows);
    const bool direct = rows <= kDirectOutPairs;
    const lchd_cloud* cl[2] = {&a, &b};
    const size_t o_len[2] = {o_la, o_lb};
    DensePass P{};
    for (int k = 0; k < 2; ++k) {
        RowSource& s = P.src[k] = cloud_source(*cl[k], cat16, sd[k].cols, sd[k].cell);
        s.as_rows = periodic;
        if (sd[k].dmx) { s.kind = RowSource::HOST_ROWS; s.m = sd[k].dmx; }  // (straight from the caller's buffers into the workspace)
        if (sd[k].row_len) s.d_len = reinterpret_cast<const int32_t*>(c->d_io + o_len[k]);
    }
    P.rows = rows;
    P.d_wf = wf_index ? reinterpret_cast<const int32_t*>(c->d_io + o_wf) : nullptr;
    P.d_out = reinterpret_cast<double*>((direct ? c->h_io : c->d_io) + o_out);
    double* const d_out = P.d_out;
    if (int rc = dense_attempts(c, P, in_bytes)) return rc;
    if (!direct) {
        HIP_TRY(hipMemcpyAsync(c->h_io + o_out, d_out, sizeof(double) * rows, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    memcpy(out, c->h_io + o_out, sizeof(double) * (size_t)rows);
    return LCHD_OK;
}

/* from_coords with both structures already on the device (what bench.py --workload c2b measures): pair r = (atom r of a,
 * atom r of b), the environments are the whole structures.  d_wf_index / d_out are device pointers ([n] int32 or NULL,
 * [n] double).  Uses the configuration of lchd_ctx_set_config; d_out is complete on return.  cell[k]: the reduced periodic cell of
 * side k, or null (lchd_from_coords_periodic_dev). */
static int coords_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int32_t* d_wf_index, const MinImageCell* const* cell, double* d_out) {
    if (!c->cfg_set) return fail(LCHD_EVALUE, "lchd_ctx_set_config has not been called");
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    if (a->sid || b->sid) return fail(LCHD_EVALUE, "from_coords takes single structures, not batches");
    if (a->n != b->n)  // src/locohd.rs:420-428 via :472-475
        return fail(LCHD_EVALUE, "Expected matrices with the same length, got lengths %lld and %lld!", (long long)a->n, (long long)b->n);
    c->last_valid = c->last_sweep_valid = false;
    if (a->n == 0) return LCHD_OK;
    if (!d_out) return fail(LCHD_EVALUE, "null score pointer");
    const bool periodic = cell[0] || cell[1];  // both structures' rows are materialised and the pass runs in its given-row form
    if (plan_dense(dense_query(c, a->n, b->n, periodic, false, 0, false)).unsupported) return fail_dense_rows(a->n);
    CTX_GUARD(c);
    const bool cat16 = c->h_cfg.n_categories > kMaxCategories;
    DensePass P{{cloud_source(*a, cat16, a->n, cell[0]), cloud_source(*b, cat16, b->n, cell[1])}, a->n, d_wf_index, d_out};
    P.src[0].as_rows = P.src[1].as_rows = periodic;
    return dense_attempts(c, P, 0);
}
static const MinImageCell* const kNoCells[2] = {nullptr, nullptr};
extern "C" int lchd_from_coords_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int32_t* d_wf_index, double* d_out) {
    CTX_LOCK(c);
    if (!c || !a || !b) return fail(LCHD_EVALUE, "null argument");
    return coords_dev(c, a, b, d_wf_index, kNoCells, d_out);
}

// from_coords from host arrays; cell[k]: the reduced periodic cell of side k, or null (lchd_from_coords_periodic)
static int coords_host(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b, int64_t len_seq_b,
                       const double* xyz_a, int64_t n_a, const double* xyz_b, int64_t n_b, const int32_t* wf_index,
                       const MinImageCell* const* cell, double* out) {
    if (n_a != n_b)  // src/locohd.rs:420-428 via :472-475
        return fail(LCHD_EVALUE, "Expected matrices with the same length, got lengths %lld and %lld!", (long long)n_a, (long long)n_b);
    const DenseHostSide sd[2] = {{seq_a, len_seq_a, xyz_a, nullptr, n_a, nullptr, cell[0]}, {seq_b, len_seq_b, xyz_b, nullptr, n_b, nullptr, cell[1]}};
    return dense_driver(c, cfg, sd, n_a, wf_index, out);
}
extern "C" int lchd_from_coords(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b,
                                int64_t len_seq_b, const double* xyz_a, int64_t n_a, const double* xyz_b, int64_t n_b,
                                const int32_t* wf_index, double* out) {
    CTX_LOCK(c);
    if (!c) return fail(LCHD_EVALUE, "null context");
    return coords_host(c, cfg, seq_a, len_seq_a, seq_b, len_seq_b, xyz_a, n_a, xyz_b, n_b, wf_index, kNoCells, out);
}

extern "C" int lchd_from_dmxs(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b,
                              int64_t len_seq_b, const double* dmx_a, int64_t rows_a, int64_t cols_a, const double* dmx_b,
                              int64_t rows_b, int64_t cols_b, const int32_t* wf_index, double* out) {
    CTX_LOCK(c);
    if (!c) return fail(LCHD_EVALUE, "null context");
    if (rows_a != rows_b)  // src/locohd.rs:420-428
        return fail(LCHD_EVALUE, "Expected matrices with the same length, got lengths %lld and %lld!", (long long)rows_a, (long long)rows_b);
    const DenseHostSide sd[2] = {{seq_a, len_seq_a, nullptr, dmx_a, cols_a, nullptr, nullptr}, {seq_b, len_seq_b, nullptr, dmx_b, cols_b, nullptr, nullptr}};
    return dense_driver(c, cfg, sd, rows_a, wf_index, out);
}

/* from_dmxs with ragged rows: the reference takes Vec<Vec<f64>> and sorts each row with a PREFIX of seq (utils.rs:25-39), so rows
 * may be shorter than seq and differ in length.  dmx_x is the row-major [rows][cols_x] matrix padded with anything; row r of
 * side x has row_len_x[r] (1 .. cols_x) real entries.  Entries and categories beyond a row's length are never looked at. */
extern "C" int lchd_from_dmxs_ragged(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b,
                                     int64_t len_seq_b, const double* dmx_a, int64_t rows_a, int64_t cols_a, const int32_t* row_len_a,
                                     const double* dmx_b, int64_t rows_b, int64_t cols_b, const int32_t* row_len_b, const int32_t* wf_index,
                                     double* out) {
    CTX_LOCK(c);
    if (!c) return fail(LCHD_EVALUE, "null context");
    if (rows_a != rows_b)  // src/locohd.rs:420-428
        return fail(LCHD_EVALUE, "Expected matrices with the same length, got lengths %lld and %lld!", (long long)rows_a, (long long)rows_b);
    if (!row_len_a || !row_len_b) return fail(LCHD_EVALUE, "null row-length array");
    const DenseHostSide sd[2] = {{seq_a, len_seq_a, nullptr, dmx_a, cols_a, row_len_a, nullptr}, {seq_b, len_seq_b, nullptr, dmx_b, cols_b, row_len_b, nullptr}};
    return dense_driver(c, cfg, sd, rows_a, wf_index, out);
}

extern "C" int lchd_from_anchors(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const double* dists_a,
                                 int64_t len_dists_a, const int32_t* seq_b, int64_t len_seq_b, const double* dists_b,
                                 int64_t len_dists_b, int32_t wf_index, double* out) {
    CTX_LOCK(c);
    if (!c) return fail(LCHD_EVALUE, "null context");
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    CTX_GUARD(c);
    if (int rc = lchd_ctx_set_config(c, cfg)) return rc;
    if (wf_index < 0 || wf_index >= cfg->n_weight_functions) return fail(LCHD_EVALUE, "weight-function index out of range");
    c->last_valid = c->last_sweep_valid = false;
    // src/locohd.rs:70-77
    if (len_seq_a != len_dists_a || len_seq_b != len_dists_b) return fail(LCHD_EVALUE, "Lists seq and dists must have equal lengths!");
    if (len_seq_a == 0 || len_seq_b == 0) return fail(LCHD_EPANIC, "index out of bounds: the len is 0 but the index is 0");
    if (dists_a[0] != 0.0 || dists_b[0] != 0.0) return fail(LCHD_EVALUE, "The dists list must start with a distance of 0!");
    // environments of more than 65 535 points: the 64-bit-count form of the wide sweep (8-bit category ids, 24-bit lengths)
    if ((len_seq_a > 65535 || len_seq_b > 65535) && (cfg->n_categories > kMaxCategories || len_seq_a >= (1 << 24) || len_seq_b >= (1 << 24)))
        return fail(LCHD_EUNSUPPORTED, "environments of more than 65535 points are supported with at most %d categories and fewer than 2^24 points", kMaxCategories);
    bool ascending = true;  // (the reference never checks: lists that do not ascend take the literal walk of its loop, below)
    for (int side = 0; side < 2; ++side) {
        const double* d = side ? dists_b : dists_a;
        const int64_t n = side ? len_dists_b : len_dists_a;
        for (int64_t i = 0; i < n; ++i) {
            if (std::isnan(d[i])) return fail(LCHD_EPANIC, "internal error: entered unreachable code (NaN distance)");
            if (d[i] < 0.0) return fail(LCHD_EVALUE, "Invalid input value: %g. All values must be non-negative!", d[i]);
            if (i && d[i] < d[i - 1]) ascending = false;
        }
    }
    if (!ascending && (len_seq_a > (1 << 24) || len_seq_b > (1 << 24)))
        return fail(LCHD_EUNSUPPORTED, "lists whose distances do not ascend are walked by one lane: at most 2^24 points each");
    // pmf.rs:38-42: every point of both lists enters a PMF.  (The environment kernels make this check for the other entry
    // points; here the lists go to the sweep kernel as they are, and that kernel does not test categories.)
    for (int side = 0; side < 2; ++side) {
        const int32_t* q = side ? seq_b : seq_a;
        const int64_t n = side ? len_seq_b : len_seq_a;
        for (int64_t i = 0; i < n; ++i)
            if (q[i] < 0 || q[i] >= cfg->n_categories) return fail(LCHD_EVALUE, "Category not found!");
    }
    // The two lists, the weight-function index and the score travel through the context's pinned staging block: ONE
    // asynchronous copy on the context's stream in (ordered with everything else on that stream), the score is stored by the
    // sweep kernel straight into the pinned block.
    const size_t na = (size_t)len_seq_a, nb = (size_t)len_seq_b;
    size_t off = 0;
    auto take = [&](size_t bytes) { off = (off + 255) & ~size_t(255); const size_t o = off; off += bytes; return o; };
    const bool cat16 = cfg->n_categories > kMaxCategories;  // 16-bit category ids in the two lists
    const size_t cb_ = cat16 ? 2 : 1;
    const size_t o_ka = take(8 * na), o_kb = take(8 * nb), o_ca = take(cb_ * na), o_cb = take(cb_ * nb), o_la = take(4), o_lb = take(4), o_wf = take(4);
    const size_t in_bytes = off;
    const size_t o_meta = take(sizeof(int4)), o_out = take(sizeof(double));
    if (int rc = grow_io(c, off)) return rc;
    auto stage = [&](size_t o_k, size_t o_c, size_t o_l, const int32_t* seq, const double* d, size_t n) {
        uint64_t* k = reinterpret_cast<uint64_t*>(c->h_io + o_k);
        uint8_t* c8 = reinterpret_cast<uint8_t*>(c->h_io + o_c);
        uint16_t* c16 = reinterpret_cast<uint16_t*>(c->h_io + o_c);
        for (size_t i = 0; i < n; ++i) {
            const double v = d[i] + 0.0;  // -0.0 -> +0.0
            memcpy(&k[i], &v, 8);
            if (cat16) c16[i] = (uint16_t)seq[i]; else c8[i] = (uint8_t)seq[i];  // inside [0, n_categories): checked above
        }
        const int32_t len = (int32_t)n;
        memcpy(c->h_io + o_l, &len, 4);
    };
    stage(o_ka, o_ca, o_la, seq_a, dists_a, na);
    stage(o_kb, o_cb, o_lb, seq_b, dists_b, nb);
    memcpy(c->h_io + o_wf, &wf_index, 4);
    EnvStore ea{}, eb{};
    ea.key = reinterpret_cast<uint64_t*>(c->d_io + o_ka); ea.cat = reinterpret_cast<uint8_t*>(c->d_io + o_ca);
    ea.len = reinterpret_cast<int32_t*>(c->d_io + o_la); ea.stride = len_seq_a;
    eb.key = reinterpret_cast<uint64_t*>(c->d_io + o_kb); eb.cat = reinterpret_cast<uint8_t*>(c->d_io + o_cb);
    eb.len = reinterpret_cast<int32_t*>(c->d_io + o_lb); eb.stride = len_seq_b;
    ea.cat16 = eb.cat16 = cat16 ? 1 : 0;
    hipStream_t s = c->stream;
    if (int rc = begin_pass(c)) return rc;
    c->status_dirty = true;
    HIP_TRY(hipMemcpyAsync(c->d_io, c->h_io, in_bytes, hipMemcpyHostToDevice, s));
    mark(c, 2);
    mark(c, 3);
    double* h_out = reinterpret_cast<double*>(c->h_io + o_out);
    if (!ascending) {
        // src/locohd.rs:97-221 on lists that do not ascend: no sort-based kernel computes what that loop computes; one lane walks it
        c->status_dirty = false;
        if (cfg->n_categories > 2000)
            return fail(LCHD_EUNSUPPORTED, "lists whose distances do not ascend are walked with the count vectors in LDS: at most 2000 categories (got %d)",
                        cfg->n_categories);
        launch_anchors_literal(s, c->d_cfg, cfg->n_categories, ea, eb, (int)len_seq_a, (int)len_seq_b, wf_index, h_out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
        *out = *h_out;
        return LCHD_OK;
    }
    // a single pair: its weight-function index travels as a 1-element device array only when it is not 0
    int rc = sweep_rows(c, ea, eb, wf_index != 0 ? reinterpret_cast<const int32_t*>(c->d_io + o_wf) : nullptr, 1, h_out,
                        reinterpret_cast<int4*>(c->d_io + o_meta), DRV_ANCHORS);
    if (!rc) *out = *h_out;
    return rc;
}

// ------------------------------------------------------------------------------------------------
// dense ensembles (python_codes/ensembles/compare_ensembles.py:277-296: from_dmxs(seq, seq, dmx[i], dmx[j]) for every pair i < j
// of M structures of one topology).  The n dense rows of a structure are the same in all M - 1 of its comparisons: they are
// sorted ONCE into an environment store of resident structures (slot s: rows [s * n, (s + 1) * n)), and a structure pair is n
// sweep records over that store (lchd_ensemble.hip).  The row sort is the one from_dmxs uses (k_env_rows2 / k_env_rows on
// distance rows materialised by k_ens_dist), the sweep the launch_sweep family of the context's mode, so a record's score is
// the one from_coords / from_dmxs computes for that row (bit for bit in deterministic mode).
// Blocking: when the store of all M structures does not fit the free HBM, B slots are split into two halves of B / 2
// structures; block bi is built into the first half, every block bj > bi in turn into the second, and the pairs between the
// two resident blocks are swept -- block bi's rows are built once, block bj's once per bi < bj.
// ------------------------------------------------------------------------------------------------
constexpr int64_t kEnsRecords = (int64_t)1 << 22;   // sweep records per pass (anchors, weight-function index, pair record, score: 44 B each)
constexpr int64_t kEnsDistBytes = (int64_t)1 << 30; // distance rows materialised for one row-sort launch

static int ens_sweep(lchd_ctx* c, const EnvStore& st, const int64_t* anchors, const uint32_t* slots, int64_t n_slots, const int32_t* wf_rec,
                     int64_t q, double* out, int4* meta) {
    SweepArgs sw{};
    fill_sweep_args(c, sw);
    sw.env_a = sw.env_b = st;
    sw.anchors = anchors;
    sw.slot_a = sw.slot_b = slots;
    sw.n_slot_a = sw.n_slot_b = n_slots;
    sw.wf_index = wf_rec;
    sw.n_pairs = q;
    sw.out = out;
    sw.meta = meta;
    if (!launch_sweep(c->stream, c->tune, c->h_cfg.n_categories, c->hellinger2, c->unit_weights, c->wf_pow, 0, sw).ok)
        return fail(LCHD_EDEVICE, "internal error: the sweep launch set would not give every pair exactly one kernel");
    HIP_TRY(hipGetLastError());
    c->status_dirty = false;  // the record pass resets the device status
    uint32_t f = 0;
    if (int rc = wait_pass(c, &f)) return rc;
    return status_to_rc(f, DRV_DMXS);
}

// src: the rows of all M structures, [M * n][n] -- the coordinates of a regular batch (view: the topology's categories over the batch's
// coordinate arrays; open with as_rows, or in its cells) or given HOST rows; pairs: host [P][2] structure indices (validated);
// d_wf: DEVICE [n] or null; d_out: DEVICE [P][n]
static int ensemble_core(lchd_ctx* c, const RowSource& src, int64_t n, int64_t M, const std::vector<int32_t>& pairs, const int32_t* d_wf,
                         double* d_out) {
    const int64_t P = (int64_t)pairs.size() / 2;
    c->last_valid = c->last_sweep_valid = false;
    c->last_dense_valid = false;
    if (P == 0 || n == 0) return LCHD_OK;
    // (a call that cannot be repeated: k_env_rows2 up to its one-segment limit, longer rows through k_env_rows, which needs no retry)
    const lchd_dense_query query = dense_query(c, n, n, true, false, 0, true);
    const lchd_dense_plan dplan = plan_dense(query);
    const bool cat16 = query.cat16 != 0;
    if (dplan.unsupported) return fail_dense_rows(n);
    c->last_dense = lchd_dense_record{};
    c->last_dense.plan = dplan;
    c->last_dense.attempts = 1;
    const int64_t cap = next_pow2_host(n);
    const size_t cat_bytes = cat16 ? 2 : 1;
    const bool rows2 = dplan.path == LCHD_DENSE_ROWS2;
    const int64_t dist_structs = std::max<int64_t>(1, std::min<int64_t>(M, kEnsDistBytes / (8 * n * n)));
    const int64_t pass_pairs = std::max<int64_t>(1, std::min<int64_t>(P, kEnsRecords / n));
    const int64_t q_cap = pass_pairs * n;
    const size_t slot_bytes = (size_t)n * cap * (8 + cat_bytes) + (size_t)n * 8 + 1024;  // keys, categories, length, identity map, alignment
    const size_t fixed = (size_t)(dist_structs * n + 1) * n * 8 + (size_t)q_cap * (16 + 4 + 16 + 8) + (size_t)P * 16 + slot_bytes + (16 << 20);
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t budget = free_b / 10 * 8;
    int64_t fit = budget > fixed ? (int64_t)((budget - fixed) / slot_bytes) : 0;
    if (c->tune.ensemble_block > 0) fit = std::min<int64_t>(fit, c->tune.ensemble_block);
    int64_t slots, half;  // store slots; structures per block (== M: one block)
    if (fit >= M) {
        slots = half = M;
    } else {
        half = fit / 2;
        if (half < 1)
            return fail(LCHD_EUNSUPPORTED, "the ensemble call needs the sorted rows of two structures (%zu bytes) resident, but only %zu of %zu bytes "
                                           "of device memory are free", fixed + 2 * slot_bytes, free_b, total_b);
        slots = 2 * half;
    }
    if (slots * n >= ((int64_t)1 << 31)) return fail(LCHD_EUNSUPPORTED, "%lld resident rows exceed the 2^31 environment slots of a pass", (long long)(slots * n));
    // one device block for the call, released on every path out
    EnvStore st{};
    double *w = nullptr, *tmp = nullptr;
    int64_t* anchors = nullptr;
    int32_t* wf_rec = nullptr;
    int4 *meta = nullptr, *plan = nullptr;
    uint32_t* iota = nullptr;
    char* blk = nullptr;
    size_t blk_bytes = 0;
    for (int dry = 1; dry >= 0; --dry) {
        Arena ar(blk, blk_bytes, dry != 0);
        st = carve_row_store(ar, slots * n + 1, cap, 1, cat16);  // (+1 row: the odd row of a row-sort launch, below)
        iota = ar.take<uint32_t>((size_t)(slots * n));
        w = take_rows(ar, src, dist_structs * n);
        anchors = ar.take<int64_t>((size_t)q_cap * 2);
        wf_rec = d_wf ? ar.take<int32_t>((size_t)q_cap) : nullptr;
        meta = ar.take<int4>((size_t)q_cap);
        tmp = ar.take<double>((size_t)q_cap);
        plan = ar.take<int4>((size_t)P);
        if (dry) {
            blk_bytes = ar.off + 256;
            if (hipMalloc(&blk, blk_bytes) != hipSuccess) {
                (void)hipGetLastError();
                return fail(LCHD_EUNSUPPORTED, "the ensemble call needs %zu bytes of device memory; %zu of %zu are free", blk_bytes, free_b, total_b);
            }
        }
    }
    struct Release {
        lchd_ctx* c;
        char* p;
        ~Release() { (void)hipStreamSynchronize(c->stream); (void)hipFree(p); }
    } release{c, blk};
    st.cdf_keys = (c->h_cfg.n_wf == 1 && !c->tune.no_cdf_keys) ? 1 : 0;
    hipStream_t s = c->stream;
    launch_ens_iota(s, iota, slots * n);
    auto rows_of = [&](int64_t slot) {  // the store seen from row slot * n on
        EnvStore e = st;
        e.key += slot * n * cap;
        e.cat += slot * n * cap * (int64_t)cat_bytes;
        e.len += slot * n;
        return e;
    };
    // structures [s0, s0 + cnt) into slots [slot0, slot0 + cnt)
    auto build = [&](int64_t slot0, int64_t s0, int64_t cnt) -> int {
        for (int64_t k0 = 0; k0 < cnt; k0 += dist_structs) {
            const int64_t kc = std::min(dist_structs, cnt - k0), rows = kc * n;
            const double* dmx = nullptr;
            if (int rc = produce_rows(c, src, (s0 + k0) * n, rows, w, dmx)) return rc;
            const EnvStore e0 = rows_of(slot0 + k0);
            bool ok;
            if (rows2) {  // both halves of the launch: rows [0, h) and [h, 2h); an odd last row goes with the store's spare row
                const int64_t h = rows / 2;
                EnvStore e1 = e0;
                e1.key += h * cap; e1.cat += h * cap; e1.len += h;
                ok = launch_env_rows2(s, dplan, c->d_cfg, RowSide{src.view, dmx, n, n, 0.0, e0, nullptr}, RowSide{src.view, dmx + h * n, n, n, 0.0, e1, nullptr}, h,
                                      c->d_status);
                if (ok && (rows & 1)) {
                    EnvStore el = e0, spare = st;
                    el.key += (rows - 1) * cap; el.cat += (rows - 1) * cap; el.len += rows - 1;
                    spare.key += slots * n * cap; spare.cat += slots * n * cap; spare.len += slots * n;
                    const double* last = dmx + (rows - 1) * n;
                    ok = launch_env_rows2(s, dplan, c->d_cfg, RowSide{src.view, last, n, n, 0.0, el, nullptr}, RowSide{src.view, last, n, n, 0.0, spare, nullptr}, 1,
                                          c->d_status);
                }
            } else {
                ok = launch_env_rows(s, dplan.rows[0], c->d_cfg, src.view, dmx, n, rows, n, 0.0, e0, c->d_status);
            }
            if (!ok) return fail(LCHD_EUNSUPPORTED, "no dense environment kernel for rows of %lld points", (long long)n);
        }
        if (c->deterministic) {  // one order among equal keys, as deterministic from_coords / from_dmxs
            const EnvStore e = rows_of(slot0);
            launch_env_canon(s, e, e, cnt * n, 0, nullptr);
            c->last_dense.canon = 1;
        }
        HIP_TRY(hipGetLastError());
        return LCHD_OK;
    };
    // pairs grouped by the (lower, upper) block pair they need resident
    const int64_t n_blk = (M + half - 1) / half;
    std::vector<int64_t> order((size_t)P);
    for (int64_t p = 0; p < P; ++p) order[(size_t)p] = p;
    auto key_of = [&](int64_t p) {
        const int64_t bi = pairs[2 * p] / half, bj = pairs[2 * p + 1] / half;
        return std::min(bi, bj) * n_blk + std::max(bi, bj);
    };
    if (n_blk > 1) std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return key_of(x) < key_of(y); });
    std::vector<int4> h_plan((size_t)P);
    int64_t held[2] = {-1, -1};  // block resident in each half
    for (int64_t g0 = 0; g0 < P;) {
        const int64_t key = key_of(order[(size_t)g0]);
        int64_t g1 = g0;
        while (g1 < P && key_of(order[(size_t)g1]) == key) ++g1;
        const int64_t bi = key / n_blk, bj = key % n_blk;
        auto slot_of = [&](int32_t sidx) -> int32_t {
            const int64_t b = sidx / half;
            return (int32_t)((b == bi ? 0 : half) + (sidx - b * half));
        };
        for (int64_t g = g0; g < g1; ++g) {
            const int64_t p = order[(size_t)g];
            h_plan[(size_t)g] = make_int4(slot_of(pairs[2 * p]), slot_of(pairs[2 * p + 1]), (int)p, 0);
        }
        if (int rc = begin_pass(c)) return rc;
        c->status_dirty = true;  // until the record pass has been enqueued (ens_sweep)
        if (held[0] != bi) {
            if (int rc = build(0, bi * half, std::min(half, M - bi * half))) return rc;
            held[0] = bi;
        }
        if (bj != bi && held[1] != bj) {
            if (int rc = build(half, bj * half, std::min(half, M - bj * half))) return rc;
            held[1] = bj;
        }
        HIP_TRY(hipMemcpyAsync(plan + g0, h_plan.data() + g0, sizeof(int4) * (size_t)(g1 - g0), hipMemcpyHostToDevice, s));
        for (int64_t k0 = g0; k0 < g1; k0 += pass_pairs) {
            const int64_t kc = std::min(pass_pairs, g1 - k0);
            if (k0 != g0) {
                if (int rc = begin_pass(c)) return rc;
                c->status_dirty = true;
            }
            launch_ens_records(s, plan + k0, kc, (int32_t)n, d_wf, anchors, wf_rec);
            if (int rc = ens_sweep(c, st, anchors, iota, slots * n, wf_rec, kc * n, tmp, meta)) return rc;
            c->last_dense.n_bitonic += c->h_status->n_bitonic;  // (rows of the row-sort launches since the previous record pass)
            launch_ens_scatter(s, tmp, plan + k0, kc, (int32_t)n, d_out);
        }
        g0 = g1;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    c->last_dense_valid = true;
    return LCHD_OK;
}

// d_pairs: DEVICE [n_pairs][2] or null (every i < j, i outer); excluded columns: DEVICE CSR or null.  Copies the (small) pair and
// exclusion lists to the host to validate them and to plan the blocks; the P * n records are made on the device.
// cells: the cell fields of a periodic call's source (min_image_ensemble), or null.
static int ensemble_coords_dev(lchd_ctx* c, lchd_cloud* cl, const int32_t* d_pairs, int64_t n_pairs, const int32_t* d_excl_start,
                               const int32_t* d_excl_idx, const int32_t* d_wf_index, const RowSource* cells, double* d_out) {
    if (!c->cfg_set) return fail(LCHD_EVALUE, "lchd_ctx_set_config has not been called");
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    if (!cl->sid || cl->struct_size <= 0 || cl->n != (int64_t)cl->n_struct * cl->struct_size)
        return fail(LCHD_EVALUE, "the ensemble call takes a regular batch (structures of equal size stored one after the other: "
                                 "lchd_cloud_create_batch or a frames buffer)");
    if (n_pairs < 0) return fail(LCHD_EVALUE, "negative number of structure pairs");
    CTX_GUARD(c);
    const int64_t n = cl->struct_size, M = cl->n_struct;
    if (!d_pairs && n_pairs != M * (M - 1) / 2)
        return fail(LCHD_EVALUE, "without a pair list the call scores all %lld pairs i < j of %lld structures (got n_pairs = %lld)",
                    (long long)(M * (M - 1) / 2), (long long)M, (long long)n_pairs);
    if (n_pairs > 0 && !d_out) return fail(LCHD_EVALUE, "null score pointer");
    if (int rc = resolve_bbox(c, cl)) return rc;  // (a frames buffer: waits for its upload, rejects non-finite coordinates)
    std::vector<int32_t> pairs((size_t)n_pairs * 2);
    if (d_pairs) {
        if (n_pairs) HIP_TRY(hipMemcpyAsync(pairs.data(), d_pairs, sizeof(int32_t) * pairs.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (int64_t p = 0; p < n_pairs; ++p)
            for (int k = 0; k < 2; ++k)
                if (pairs[2 * p + k] < 0 || pairs[2 * p + k] >= M)
                    return fail(LCHD_EVALUE, "structure pair %lld refers to structure %d of %lld", (long long)p, pairs[2 * p + k], (long long)M);
    } else {
        size_t k = 0;
        for (int32_t i = 0; i < M; ++i)
            for (int32_t j = i + 1; j < M; ++j) { pairs[k++] = i; pairs[k++] = j; }
    }
    if (d_excl_start || d_excl_idx) {
        if (!d_excl_start || !d_excl_idx) return fail(LCHD_EVALUE, "the exclusion list needs both its row starts and its column indices");
        std::vector<int32_t> xs((size_t)n + 1);
        HIP_TRY(hipMemcpyAsync(xs.data(), d_excl_start, sizeof(int32_t) * xs.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (xs[0] != 0) return fail(LCHD_EVALUE, "the exclusion list's row starts must begin with 0");
        for (int64_t r = 0; r < n; ++r)
            if (xs[(size_t)r + 1] < xs[(size_t)r]) return fail(LCHD_EVALUE, "the exclusion list's row starts must not decrease");
        std::vector<int32_t> xi((size_t)xs[(size_t)n]);
        if (!xi.empty()) {
            HIP_TRY(hipMemcpyAsync(xi.data(), d_excl_idx, sizeof(int32_t) * xi.size(), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        for (size_t e = 0; e < xi.size(); ++e)
            if (xi[e] < 0 || xi[e] >= n) return fail(LCHD_EVALUE, "excluded column %d is outside [0, %lld)", xi[e], (long long)n);
    }
    RowSource src = cells ? *cells : RowSource{};  // (open: COORDS)
    src.view = cl->view(c->h_cfg.n_categories > kMaxCategories);  // (every structure carries the topology's categories: structure 0's are read)
    src.view.n = (int32_t)n;
    src.view.sid = nullptr;
    src.view.n_struct = 1;
    src.view.struct_size = 0;
    src.cols = n;
    src.as_rows = true;
    src.excl_start = d_excl_start;
    src.excl_idx = d_excl_idx;
    return ensemble_core(c, src, n, M, pairs, d_wf_index, d_out);
}
extern "C" int lchd_ensemble_from_coords_dev(lchd_ctx* c, lchd_cloud* cl, const int32_t* d_pairs, int64_t n_pairs, const int32_t* d_excl_start,
                                             const int32_t* d_excl_idx, const int32_t* d_wf_index, double* d_out) {
    CTX_LOCK(c);
    if (!c || !cl) return fail(LCHD_EVALUE, "null argument");
    return ensemble_coords_dev(c, cl, d_pairs, n_pairs, d_excl_start, d_excl_idx, d_wf_index, nullptr, d_out);
}

static int ens_check_pairs(const int32_t* pairs, int64_t n_pairs, int64_t M) {
    if (n_pairs < 0) return fail(LCHD_EVALUE, "negative number of structure pairs");
    if (n_pairs > 0 && !pairs) return LCHD_OK;
    for (int64_t p = 0; pairs && p < n_pairs; ++p)
        for (int k = 0; k < 2; ++k)
            if (pairs[2 * p + k] < 0 || pairs[2 * p + k] >= M)
                return fail(LCHD_EVALUE, "structure pair %lld refers to structure %d of %lld", (long long)p, pairs[2 * p + k], (long long)M);
    return LCHD_OK;
}

// device copies of a host call's arrays, released on every path out
struct EnsDevBufs {
    std::vector<void*> p;
    ~EnsDevBufs() { for (void* q : p) (void)hipFree(q); }
    template <class T>
    int put(const T* h, size_t count, T** d) {
        *d = nullptr;
        if (!count) return LCHD_OK;
        void* q = nullptr;
        HIP_TRY(hipMalloc(&q, sizeof(T) * count));
        p.push_back(q);
        if (h) HIP_TRY(hipMemcpy(q, h, sizeof(T) * count, hipMemcpyHostToDevice));
        *d = static_cast<T*>(q);
        return LCHD_OK;
    }
};

static int ensemble_coords_host(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq, int64_t n, const double* xyz, int64_t n_struct,
                                const int32_t* pairs, int64_t n_pairs, const int32_t* excl_start, const int32_t* excl_idx,
                                const int32_t* wf_index, const RowSource* cells, double* out) {
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    if (n < 0 || n_struct < 0) return fail(LCHD_EVALUE, "negative size");
    if (n_struct * n > ((int64_t)1 << 30)) return fail(LCHD_EUNSUPPORTED, "%lld atoms in all exceed a batch", (long long)(n_struct * n));
    CTX_GUARD(c);
    if (int rc = lchd_ctx_set_config(c, cfg)) return rc;
    if (int rc = check_wf_index(cfg, wf_index, n)) return rc;
    if (int rc = ens_check_pairs(pairs, n_pairs, n_struct)) return rc;
    const int64_t P = pairs ? n_pairs : n_struct * (n_struct - 1) / 2;
    if (!pairs && n_pairs != P)
        return fail(LCHD_EVALUE, "without a pair list the call scores all %lld pairs i < j of %lld structures (got n_pairs = %lld)", (long long)P,
                    (long long)n_struct, (long long)n_pairs);
    c->last_valid = c->last_sweep_valid = false;
    if (P == 0 || n == 0) return LCHD_OK;
    if (!(excl_start == nullptr) != !(excl_idx == nullptr)) return fail(LCHD_EVALUE, "the exclusion list needs both its row starts and its column indices");
    std::vector<int32_t> cat((size_t)(n_struct * n)), sid((size_t)(n_struct * n));
    for (int64_t k = 0; k < n_struct; ++k)
        for (int64_t i = 0; i < n; ++i) { cat[(size_t)(k * n + i)] = seq[i]; sid[(size_t)(k * n + i)] = (int32_t)k; }
    lchd_cloud* cl = nullptr;
    if (int rc = lchd_cloud_create_batch(c, xyz, cat.data(), nullptr, sid.data(), n_struct * n, (int32_t)n_struct, &cl)) return rc;
    struct Drop { lchd_ctx* c; lchd_cloud* cl; ~Drop() { lchd_cloud_destroy(c, cl); } } drop{c, cl};
    EnsDevBufs bufs;
    int32_t *d_pairs = nullptr, *d_xs = nullptr, *d_xi = nullptr, *d_wf = nullptr;
    double* d_out = nullptr;
    if (int rc = bufs.put(pairs, (size_t)(pairs ? 2 * n_pairs : 0), &d_pairs)) return rc;
    if (excl_start) {
        if (excl_start[0] != 0 || excl_start[n] < excl_start[0]) return fail(LCHD_EVALUE, "the exclusion list's row starts must begin with 0 and not decrease");
        if (int rc = bufs.put(excl_start, (size_t)n + 1, &d_xs)) return rc;
        if (int rc = bufs.put(excl_start[n] ? excl_idx : nullptr, (size_t)std::max<int32_t>(excl_start[n], 1), &d_xi)) return rc;
    }
    if (int rc = bufs.put(wf_index, (size_t)(wf_index ? n : 0), &d_wf)) return rc;
    if (int rc = bufs.put<double>(nullptr, (size_t)(P * n), &d_out)) return rc;
    if (int rc = ensemble_coords_dev(c, cl, d_pairs, P, d_xs, d_xi, d_wf, cells, d_out)) return rc;
    HIP_TRY(hipMemcpy(out, d_out, sizeof(double) * (size_t)(P * n), hipMemcpyDeviceToHost));
    return LCHD_OK;
}
extern "C" int lchd_ensemble_from_coords(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq, int64_t n, const double* xyz, int64_t n_struct,
                                         const int32_t* pairs, int64_t n_pairs, const int32_t* excl_start, const int32_t* excl_idx,
                                         const int32_t* wf_index, double* out) {
    CTX_LOCK(c);
    if (!c) return fail(LCHD_EVALUE, "null context");
    return ensemble_coords_host(c, cfg, seq, n, xyz, n_struct, pairs, n_pairs, excl_start, excl_idx, wf_index, nullptr, out);
}

extern "C" int lchd_ensemble_from_dmxs(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq, int64_t n, const double* dmx, int64_t n_struct,
                                       const int32_t* pairs, int64_t n_pairs, const int32_t* wf_index, double* out) {
    CTX_LOCK(c);
    if (!c) return fail(LCHD_EVALUE, "null context");
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    if (n < 0 || n_struct < 0) return fail(LCHD_EVALUE, "negative size");
    CTX_GUARD(c);
    if (int rc = lchd_ctx_set_config(c, cfg)) return rc;
    if (int rc = check_wf_index(cfg, wf_index, n)) return rc;
    if (int rc = ens_check_pairs(pairs, n_pairs, n_struct)) return rc;
    const int64_t P = pairs ? n_pairs : n_struct * (n_struct - 1) / 2;
    if (!pairs && n_pairs != P)
        return fail(LCHD_EVALUE, "without a pair list the call scores all %lld pairs i < j of %lld structures (got n_pairs = %lld)", (long long)P,
                    (long long)n_struct, (long long)n_pairs);
    c->last_valid = c->last_sweep_valid = false;
    if (P == 0 || n == 0) return LCHD_OK;
    std::vector<int32_t> hp((size_t)P * 2);
    if (pairs) {
        std::copy(pairs, pairs + 2 * P, hp.begin());
    } else {
        size_t k = 0;
        for (int32_t i = 0; i < n_struct; ++i)
            for (int32_t j = i + 1; j < n_struct; ++j) { hp[k++] = i; hp[k++] = j; }
    }
    lchd_cloud* cl = nullptr;  // the topology's categories (no coordinates: the rows are given)
    if (int rc = lchd_cloud_create(c, nullptr, seq, nullptr, n, &cl)) return rc;
    struct Drop { lchd_ctx* c; lchd_cloud* cl; ~Drop() { lchd_cloud_destroy(c, cl); } } drop{c, cl};
    EnsDevBufs bufs;
    int32_t* d_wf = nullptr;
    double* d_out = nullptr;
    if (int rc = bufs.put(wf_index, (size_t)(wf_index ? n : 0), &d_wf)) return rc;
    if (int rc = bufs.put<double>(nullptr, (size_t)(P * n), &d_out)) return rc;
    RowSource src{};
    src.kind = RowSource::HOST_ROWS;
    src.view = cl->view(cfg->n_categories > kMaxCategories);
    src.cols = n;
    src.m = dmx;
    if (int rc = ensemble_core(c, src, n, n_struct, hp, d_wf, d_out)) return rc;
    HIP_TRY(hipMemcpy(out, d_out, sizeof(double) * (size_t)(P * n), hipMemcpyDeviceToHost));
    return LCHD_OK;
}

// ------------------------------------------------------------------------------------------------
// dense calls in periodic cells (minimum image): the cells are reduced on the host and travel in the call's row sources (RowSource),
// whose rows launch_min_image_rows then materialises (produce_rows)
// ------------------------------------------------------------------------------------------------
// The cells of a call's sides, reduced: cell[k] = &rec[k], or null for an open side.  by_side: a refusal names cell k (else cell 0).
static int reduce_cells(const double* const* cells, int sides, bool by_side, MinImageCell* rec, const MinImageCell** cell) {
    for (int k = 0; k < 2; ++k) cell[k] = nullptr;
    for (int k = 0; k < sides; ++k)
        if (cells[k]) {
            if (int rc = min_image_record(cells[k], by_side ? k : 0, rec[k])) return rc;
            cell[k] = &rec[k];
        }
    return LCHD_OK;
}
// "cells" of lchd_ctx_last_ms after a periodic single-pair call: the row producers of both sides (events 0 and 1 of dense_pass)
static void min_image_time(lchd_ctx* c) {
    float t = -1.f;
    if (c->timing && hipEventElapsedTime(&t, c->ev[0], c->ev[1]) == hipSuccess) c->ms[PH_CELLS] = t;
}

extern "C" int lchd_from_coords_periodic_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int32_t* d_wf_index, const double* cell_a,
                                             const double* cell_b, double* d_out) {
    CTX_LOCK(c);
    if (!c || !a || !b) return fail(LCHD_EVALUE, "null argument");
    if (!cell_a && !cell_b) return coords_dev(c, a, b, d_wf_index, kNoCells, d_out);  // the open call
    const double* const cells[2] = {cell_a, cell_b};
    MinImageCell rec[2];
    const MinImageCell* cell[2];
    if (int rc = reduce_cells(cells, 2, true, rec, cell)) return rc;
    if (a->images || b->images) return fail(LCHD_EVALUE, "a periodic dense call takes the structures themselves, not their image clouds");
    CTX_GUARD(c);
    if (int rc = resolve_bbox(c, a)) return rc;  // (rejects non-finite coordinates of a buffer filled on the device)
    if (int rc = resolve_bbox(c, b)) return rc;
    const int rc = coords_dev(c, a, b, d_wf_index, cell, d_out);
    if (!rc) min_image_time(c);
    return rc;
}

extern "C" int lchd_from_coords_periodic(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b,
                                         int64_t len_seq_b, const double* xyz_a, int64_t n_a, const double* xyz_b, int64_t n_b,
                                         const int32_t* wf_index, const double* cell_a, const double* cell_b, double* out) {
    CTX_LOCK(c);
    if (!c) return fail(LCHD_EVALUE, "null context");
    const double* const cells[2] = {cell_a, cell_b};
    MinImageCell rec[2];
    const MinImageCell* cell[2];
    if (int rc = reduce_cells(cells, 2, true, rec, cell)) return rc;
    const int rc = coords_host(c, cfg, seq_a, len_seq_a, seq_b, len_seq_b, xyz_a, n_a, xyz_b, n_b, wf_index, cell, out);
    if (!rc && (cell_a || cell_b)) min_image_time(c);
    return rc;
}

// cells: HOST [n_cells][9], n_cells = 1 or the number of structures.  Fills the cell fields of `src`; per-structure records go to the
// device through `bufs`.
static int min_image_ensemble(const double* cells, int32_t n_cells, int64_t n_struct, RowSource& src, EnsDevBufs& bufs) {
    if (!cells || (n_cells != 1 && n_cells != n_struct))
        return fail(LCHD_EVALUE, "%d cells given for %lld structures (pass one cell, or one per structure)", cells ? n_cells : 0, (long long)n_struct);
    std::vector<MinImageCell> recs((size_t)n_cells);
    src.kind = RowSource::CELL;
    src.all_diagonal = true;
    for (int32_t k = 0; k < n_cells; ++k) {
        if (int rc = min_image_record(cells + 9 * (size_t)k, k, recs[(size_t)k])) return rc;
        if (recs[(size_t)k].v[18] == 0.0) src.all_diagonal = false;
    }
    src.cell = recs[0];
    if (n_cells > 1) {
        double* d = nullptr;
        if (int rc = bufs.put(recs[0].v, (size_t)n_cells * kMinImageRecord, &d)) return rc;
        src.d_cells = d;
    }
    return LCHD_OK;
}

extern "C" int lchd_ensemble_from_coords_periodic_dev(lchd_ctx* c, lchd_cloud* cl, const int32_t* d_pairs, int64_t n_pairs,
                                                      const int32_t* d_excl_start, const int32_t* d_excl_idx, const int32_t* d_wf_index,
                                                      const double* cells, int32_t n_cells, double* d_out) {
    CTX_LOCK(c);
    if (!c || !cl) return fail(LCHD_EVALUE, "null argument");
    if (cl->images) return fail(LCHD_EVALUE, "a periodic dense call takes the structures themselves, not their image clouds");
    CTX_GUARD(c);
    RowSource src{};
    EnsDevBufs bufs;
    if (int rc = min_image_ensemble(cells, n_cells, cl->n_struct, src, bufs)) return rc;
    return ensemble_coords_dev(c, cl, d_pairs, n_pairs, d_excl_start, d_excl_idx, d_wf_index, &src, d_out);
}

extern "C" int lchd_ensemble_from_coords_periodic(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq, int64_t n, const double* xyz,
                                                  int64_t n_struct, const int32_t* pairs, int64_t n_pairs, const int32_t* excl_start,
                                                  const int32_t* excl_idx, const int32_t* wf_index, const double* cells, int32_t n_cells,
                                                  double* out) {
    CTX_LOCK(c);
    if (!c) return fail(LCHD_EVALUE, "null context");
    CTX_GUARD(c);
    RowSource src{};
    EnsDevBufs bufs;
    if (int rc = min_image_ensemble(cells, n_cells, n_struct, src, bufs)) return rc;
    return ensemble_coords_host(c, cfg, seq, n, xyz, n_struct, pairs, n_pairs, excl_start, excl_idx, wf_index, &src, out);
}

// ------------------------------------------------------------------------------------------------
// profile calls (additive, not in the reference): local composition, radial score profiles, score attribution by category
// ------------------------------------------------------------------------------------------------
// A profile call builds the environments of a list of anchors (composition) or anchor pairs (radial, attribution) with the builders of
// the scoring passes (build_prims_store; dense rows: carve_row_store + produce_rows + k_env_rows) and hands the stores to its consumer's
// kernel instead of a sweep.  It plans with neutral hints and leaves the context's hints alone: the scoring passes before and after it
// pick their kernels as if it had not run.  The record of the last scoring pass's arrays goes (the arena is laid out anew); the sweep
// record, host data, stands across a radial or an attribution call, while a composition call clears it with the other.
extern "C" int lchd_radial_validate(const double* edges, int32_t n_edges) {
    if (!edges) return fail(LCHD_EVALUE, "null edges");
    if (n_edges < 2) return fail(LCHD_EVALUE, "a radial profile needs at least 2 edges (one bin), got %d", n_edges);
    if (n_edges > kRadialMaxBins + 1) return fail(LCHD_EVALUE, "a radial profile takes at most %d edges (%d bins), got %d", kRadialMaxBins + 1, kRadialMaxBins, n_edges);
    for (int32_t k = 0; k < n_edges; ++k) {
        const double e = edges[k];
        if (std::isnan(e) || e < 0.0) return fail(LCHD_EVALUE, "edge %d is %g: edges are distances >= 0", k, e);
        if (std::isinf(e) && k + 1 < n_edges) return fail(LCHD_EVALUE, "edge %d is +inf: only the last edge may be", k);
        if (k && !(e > edges[k - 1])) return fail(LCHD_EVALUE, "edge %d (%g) does not exceed edge %d (%g): edges ascend strictly", k, e, k - 1, edges[k - 1]);
    }
    return LCHD_OK;
}
// The consumer of a profile pass's stores: the profile kernel on ONE store (sides == 1: composition, lchd_profile.hip), or, on two
// stores and the pair records of k_pair_meta, the radial kernel (edges.n >= 2), the attribution kernel (edges.n == 0) or the
// category-gradient kernel (weights).  Everything
// up to the consumer's launch is one code path; it asks which consumer it serves in the three helpers below, in consumer_list_limit,
// in consumer_drop_records and where consumer_prims_pass fills a one-sided query; what else differs is data of the descriptor.
struct PairConsumer {
    RadialEdges edges;  // n >= 2: a radial profile
    const char* what;   // in messages: "a composition profile" / "a radial profile" / "an attribution" / ...
    const char* call;   // "composition" / "radial" / "attribution"
    const char* items;  // what its list holds: "anchors" / "anchor pairs"
    int sides;          // structures (stores) of a call, columns of its list: 1 composition, 2 the others
    bool records;       // its kernel reads the pair records of k_pair_meta (a dense pass carves them)
    int width;          // > 0: a sensitivity call with rows of this many slots
    SensitivityOut sens;  // ... and its DEVICE outputs, or all null: they are carved from the pass's one output block (sens_carve)
    int resolve;        // ... and what runs behind its kernel: kSensPlain nothing; kSensImages launch_sens_resolve, which resolves members
                        // of image clouds to source atoms (image and disp outputs); kSensMinImage launch_sens_min_image_disp on dense rows
                        // from coordinates (disp outputs alone)
    bool weights;       // a category-weight gradient: the attribution call's pass and row, the other kernel (lchd_category_gradient.hip)
    bool wgrad;         // a weight-function gradient: the sensitivity call's pass and lists (width = the longest list there is: none is too
                        // long for it), the other kernel (lchd_weight_gradient.hip) and rows of 1 + lchd_ctx::wf_np_max doubles
};
enum { kSensPlain = 0, kSensImages = 1, kSensMinImage = 2 };
static const PairConsumer kComposition{{}, "a composition profile", "composition", "anchors", 1, false};
static const PairConsumer kAttribution{{}, "an attribution", "attribution", "anchor pairs", 2, true};
static const PairConsumer kCategoryGradient{{}, "a category-weight gradient", "category gradient", "anchor pairs", 2, true, 0, {}, 0, true};
static PairConsumer radial_consumer(const double* edges, int32_t n_edges) {
    PairConsumer use{{}, "a radial profile", "radial", "anchor pairs", 2, true};
    use.edges.n = n_edges;
    for (int32_t k = 0; k < n_edges; ++k) use.edges.e[k] = edges[k];
    return use;
}
static PairConsumer sensitivity_consumer(int32_t width, const SensitivityOut& out, int resolve = kSensPlain) {
    PairConsumer use{{}, "a sensitivity call", "sensitivity", "anchor pairs", 2, true};
    use.width = width;
    use.sens = out;
    use.resolve = resolve;
    return use;
}
static PairConsumer weight_gradient_consumer() {
    PairConsumer use{{}, "a weight-function gradient", "weight gradient", "anchor pairs", 2, true};
    use.width = kRadialMaxPoints;
    use.wgrad = true;
    return use;
}
// doubles per pair of a sensitivity call's block: the nine arrays, behind them the two disp rows of a call that resolves, and behind
// those the two image rows of kSensImages
static size_t sens_row(int w, int resolve) {
    return 5 * (size_t)w + 2 + (resolve ? 6 * (size_t)w : 0) + (resolve == kSensImages ? (2 * (size_t)w + 7) / 8 : 0);
}
// A sensitivity call's outputs as ONE block of n * sens_row doubles (host or device): scores | g_a | g_b | dist_a | dist_b | idx_a | idx_b |
// count_a | count_b [| disp_a | disp_b [| image_a | image_b]] -- what the host call moves in one copy.
static SensitivityOut sens_carve(double* blk, int64_t n, int w, int resolve = kSensPlain) {
    const size_t nw = (size_t)n * (size_t)w;
    SensitivityOut o{};
    o.scores = blk;
    o.g_a = blk + n; o.g_b = o.g_a + nw; o.dist_a = o.g_b + nw; o.dist_b = o.dist_a + nw;
    o.idx_a = reinterpret_cast<int32_t*>(o.dist_b + nw); o.idx_b = o.idx_a + nw;
    o.count_a = o.idx_b + nw; o.count_b = o.count_a + n;
    if (resolve) { o.disp_a = blk + (size_t)n * (5 * (size_t)w + 2); o.disp_b = o.disp_a + 3 * nw; }
    if (resolve == kSensImages) { o.image_a = reinterpret_cast<int8_t*>(o.disp_b + 3 * nw); o.image_b = o.image_a + nw; }
    return o;
}
// doubles per entry in the consumer's output: the bins / the categories of the context's configuration / a sensitivity call's block
static size_t consumer_row(const lchd_ctx* c, const PairConsumer& use) {
    if (use.wgrad) return 1 + (size_t)c->wf_np_max;  // scores[P] | grad[P][NP]
    if (use.width) return sens_row(use.width, use.resolve);
    return use.edges.n ? (size_t)use.edges.n - 1 : (size_t)c->h_cfg.n_categories;
}
static int consumer_limits(const lchd_ctx* c, const PairConsumer& use) {
    static const char* names[4] = {"Hellinger", "Kolmogorov-Smirnov", "Kullback-Leibler", "Renyi"};
    if (use.sides == 1) return LCHD_OK;  // a composition has no distance, and its kernel takes every category count
    const int most = use.width ? kSensitivityMaxCategories : (use.edges.n ? kWideCategories : kAttributionMaxCategories);
    if (use.weights && c->h_cfg.sd_kind != SD_HELLINGER && c->h_cfg.sd_kind != SD_KL)
        return fail(LCHD_EUNSUPPORTED, "a category-weight gradient is implemented for the Hellinger and Kullback-Leibler distances; not for the %s distance",
                    names[c->h_cfg.sd_kind & 3]);
    if (!use.edges.n && !use.width && !use.weights && c->h_cfg.sd_kind != SD_HELLINGER)
        return fail(LCHD_EUNSUPPORTED, "an attribution splits the Hellinger distance over the categories; the %s distance is no sum of per-category terms",
                    names[c->h_cfg.sd_kind & 3]);
    if (c->h_cfg.n_categories > most)
        return fail(LCHD_EUNSUPPORTED, "%s takes at most %d categories (got %d)", use.what, most, c->h_cfg.n_categories);
    if (use.wgrad && c->wf_np_max > kWeightGradientMaxParams)
        return fail(LCHD_EUNSUPPORTED, "%s takes weight functions of at most %d parameters (got %d)", use.what, kWeightGradientMaxParams, c->wf_np_max);
    if (use.wgrad && c->wf_finf_off)
        return fail(LCHD_EVALUE, "%s needs F(+inf) = 1 whatever the parameters: a degenerate dagum (A = 0) is refused", use.what);
    return LCHD_OK;
}
// The consumer's kernel behind a finished store build (stream order), with what hands the status over: the record pass (k_pair_meta)
// in front of a pair kernel, launch_profile_publish behind the profile kernel.  sw: the stores, the list and its slots.
// A sensitivity call's indexed lists (c->d_indexed).  cells: the thresholded build from the prologue's cell lists and anchor records,
// launched behind the record pass; null: the lists of dense rows, which launch_rows_indexed built in front of it.
struct SensLists {
    IndexedStore env[2];
    const IndexedArgs* cells;
    lchd_cloud* cl[2];  // the clouds the lists index (read when the consumer resolves image clouds)
    const struct RowSource* rows;  // [2] the row sources of a dense pass (read by kSensMinImage: coordinates and cells), or null
};
static int consumer_enqueue(lchd_ctx* c, SweepArgs& sw, const PairConsumer& use, double* d_out, const SensLists* lists = nullptr) {
    const int n_wf = c->h_cfg.n_wf;
    hipStream_t s = c->stream;
    if (use.sides == 1) {
        ProfileArgs pa{};
        pa.cfg = c->d_cfg; pa.env = sw.env_a; pa.anchors = sw.anchors; pa.slot = sw.slot_a; pa.n_atoms = sw.n_slot_a; pa.wf_index = sw.wf_index;
        pa.n = sw.n_pairs; pa.out = d_out; pa.hst = c->h_status; pa.n_categories = c->h_cfg.n_categories;
        launch_profile(s, pa);
        launch_profile_publish(s, c->d_status, c->h_status, c->seq);
        return LCHD_OK;
    }
    if (int rc = grow_block(c->d_radial_bounds, c->radial_bounds_cap, sizeof(double) * (size_t)n_wf * (size_t)use.edges.n)) return rc;
    fill_sweep_args(c, sw);
    launch_pair_meta(s, sw);
    bool launched;
    if (use.wgrad) {
        WeightGradientArgs wa{};
        wa.sw = sw;
        wa.env_a = lists->env[0];
        wa.env_b = lists->env[1];
        wa.n_categories = c->h_cfg.n_categories;
        wa.width = c->wf_np_max;
        wa.scores = d_out;
        wa.grad = d_out + sw.n_pairs;
        launched = (!lists->cells || launch_env_indexed(s, *lists->cells)) && launch_weight_gradient(s, wa);
    } else if (use.width) {
        SensitivityArgs sa{};
        sa.sw = sw;
        sa.env_a = lists->env[0];
        sa.env_b = lists->env[1];
        sa.n_categories = c->h_cfg.n_categories;
        sa.width = use.width;
        sa.out = use.sens.scores ? use.sens : sens_carve(d_out, sw.n_pairs, use.width, use.resolve);
        launched = (!lists->cells || launch_env_indexed(s, *lists->cells)) && launch_sensitivity(s, sa);
        if (launched && use.resolve == kSensMinImage) {
            SensDispArgs da{};
            const int32_t* const idx[2] = {sa.out.idx_a, sa.out.idx_b};
            double* const disp[2] = {sa.out.disp_a, sa.out.disp_b};
            for (int k = 0; k < 2; ++k) {
                const RowSource& src = lists->rows[k];
                SensDispSide& S = da.s[k];
                S.x = src.view.x; S.y = src.view.y; S.z = src.view.z; S.n = src.view.n;
                S.idx = idx[k]; S.disp = disp[k];
                S.kind = src.kind == RowSource::CELL ? (src.all_diagonal ? 1 : 2) : 0;
                if (S.kind) S.cell = src.cell;
            }
            da.rows = sw.n_pairs; da.width = use.width;
            launched = launch_sens_min_image_disp(s, da);
        } else if (launched && use.resolve == kSensImages) {
            SensResolveArgs ra{};
            int32_t* const idx[2] = {sa.out.idx_a, sa.out.idx_b};
            int8_t* const image[2] = {sa.out.image_a, sa.out.image_b};
            double* const disp[2] = {sa.out.disp_a, sa.out.disp_b};
            for (int k = 0; k < 2; ++k) {
                lchd_cloud* const cl = lists->cl[k];
                ra.s[k] = SensResolveSide{cl->x, cl->y, cl->z, cl->n, cl->images ? cl->d_img_origin : nullptr, cl->images ? cl->d_img_code : nullptr,
                                          idx[k], image[k], disp[k]};
            }
            ra.anchors = sw.anchors; ra.n_pairs = sw.n_pairs; ra.width = use.width;
            launched = launch_sens_resolve(s, ra);
        }
    } else if (use.edges.n) {
        launch_radial_bounds(s, c->d_cfg, n_wf, use.edges, reinterpret_cast<double*>(c->d_radial_bounds));
        RadialArgs ra{};
        ra.sw = sw;
        ra.bounds = reinterpret_cast<const double*>(c->d_radial_bounds);
        ra.n_bins = use.edges.n - 1;
        ra.n_categories = c->h_cfg.n_categories;
        ra.out = d_out;
        launched = launch_radial(s, c->hellinger2 && c->unit_weights && !c->tune.force_generic, ra);
    } else if (use.weights) {
        CategoryGradientArgs ga{};
        ga.sw = sw;
        ga.n_categories = c->h_cfg.n_categories;
        ga.out = d_out;
        launched = launch_category_gradient(s, c->h_cfg.sd_kind, c->hellinger2, ga);
    } else {
        AttributionArgs aa{};
        aa.sw = sw;
        aa.n_categories = c->h_cfg.n_categories;
        aa.out = d_out;
        launched = launch_attribution(s, c->hellinger2, c->unit_weights, aa);
    }
    if (!launched) return fail(LCHD_EDEVICE, "internal error: the %s kernel rejected its launch configuration", use.call);
    return LCHD_OK;
}
// The longest list of one thresholded call.
static int consumer_list_limit(const PairConsumer& use, int64_t n) {
    if (use.sides == 1) {
        if (n > (int64_t)0x3FFFFFFF) return fail(LCHD_EUNSUPPORTED, "more than 2^30 - 1 anchors in one call (%lld): split the list", (long long)n);
        return LCHD_OK;
    }
    if (n > (int64_t)0x7FFFFFFF / kRadialMaxBins) return fail(LCHD_EUNSUPPORTED, "more than %d anchor pairs in one %s call (%lld): split the list", 0x7FFFFFFF / kRadialMaxBins, use.call, (long long)n);
    return LCHD_OK;
}
// A composition call drops both records of the last scoring pass where it starts; the pair consumers keep the sweep record (below).
static void consumer_drop_records(lchd_ctx* c, const PairConsumer& use) {
    if (use.sides == 1) c->last_valid = c->last_sweep_valid = false;
}

struct ConsumerRequest {
    lchd_cloud* cl[2];       // [use.sides]
    const int64_t* anchors;  // DEVICE [n][use.sides]
    const int32_t* wf;       // DEVICE [n] or null
    int64_t n;
    double thr;
    const PairConsumer& use;
    double* out;             // DEVICE [n][consumer_row]
};
// One thresholded pass with slots of `cap` points: enqueued, waited for; *flags_out = its status words.
static int consumer_prims_pass(lchd_ctx* c, const ConsumerRequest& R, int cap, uint32_t* flags_out) {
    const int sides = R.use.sides;
    lchd_cloud *a = R.cl[0], *b = R.cl[sides - 1];
    const int n_wf = c->h_cfg.n_wf;
    PassQuery q;
    q.n_a = a->n; q.n_b = b->n; q.n_pairs = R.n;
    q.same_object = a == b;  // (one side: the pair list is (i, i), both columns share one cell list, one set of slots, one store)
    q.has_wf_index = R.wf != nullptr;
    q.cap = cap;
    q.n_categories = c->h_cfg.n_categories; q.n_wf = n_wf;
    q.deterministic = c->deterministic; q.tag_mode = c->h_cfg.tag_mode;
    q.tune = c->tune;
    if (sides == 1) q.tune.no_share = false;
    PassPlan plan = plan_pass(q);
    // the consumer's kernel reads F keys whatever the dictionary's size or the environment kernel: set 0 keeps what the environment kernel
    // writes (one function: its F values; a dictionary: the distances), k_env_key_sets fills one set per function behind it
    plan.dict_sets = n_wf > 1;
    plan.key_sets = n_wf > 1 ? n_wf + 1 : 1;
    plan.pre_words = 0;
    // a sensitivity call: the indexed lists of both sides, slots and stride as the scoring stores', in a block of their own
    IndexedArgs ix{};
    if (R.use.width) {
        const int64_t ne[2] = {plan.max_env_a, plan.same ? 0 : plan.max_env_b}, na[2] = {a->n, b->n};
        size_t off[2][5], need = 0;
        for (int k = 0; k < 2; ++k) {
            const size_t pts = (size_t)ne[k] * (size_t)cap;
            const size_t bytes[5] = {4 * (size_t)na[k], 4 * (size_t)ne[k], 8 * pts, 4 * pts, pts};  // atom_of, len, dist, idx, cat
            for (int j = 0; j < 5; ++j) { off[k][j] = need; need = (need + bytes[j] + 255) & ~size_t(255); }
        }
        if (int rc = grow_block(c->d_indexed, c->indexed_cap, need + 256)) return rc;
        for (int k = 0; k < 2; ++k) {
            IndexedSide& S = ix.s[k];
            S.max_envs = ne[k];
            S.n = (int32_t)na[k];
            S.atom_of = reinterpret_cast<uint32_t*>(c->d_indexed + off[k][0]);
            S.env.len = reinterpret_cast<int32_t*>(c->d_indexed + off[k][1]);
            S.env.dist = reinterpret_cast<double*>(c->d_indexed + off[k][2]);
            S.env.idx = reinterpret_cast<uint32_t*>(c->d_indexed + off[k][3]);
            S.env.cat = reinterpret_cast<uint8_t*>(c->d_indexed + off[k][4]);
            S.env.stride = cap;
        }
    }
    PrimsStore st;
    const int built = sides == 1 ? build_prims_store(c, a, a, nullptr, R.anchors, R.n, R.thr, q, plan, st)
                                 : build_prims_store(c, a, b, R.anchors, nullptr, R.n, R.thr, q, plan, st);
    if (st.begun) ++c->n_passes;
    if (built) return built;
    hipStream_t s = c->stream;
    SweepArgs sw{};
    sw.env_a = st.env[0];
    sw.env_b = st.env[plan.same ? 0 : 1];
    sw.anchors = R.anchors;
    sw.slot_a = st.pb.a.slot;
    sw.slot_b = plan.same ? st.pb.a.slot : (plan.per_pair ? nullptr : st.pb.b.slot);
    sw.n_slot_a = a->n;
    sw.n_slot_b = b->n;
    sw.wf_index = R.wf;
    sw.n_pairs = R.n;
    sw.meta = st.pb.pair_meta;
    if (R.use.width) {
        ix.cfg = c->d_cfg; ix.thr = R.thr; ix.reach = plan.reach; ix.tag_list = plan.tag_list ? 1 : 0; ix.st = c->d_status;
        const SideBufs* sb[2] = {&st.pb.a, &st.pb.b};
        for (int k = 0; k < 2; ++k) {
            GridView g{};
            const GridPlan& gp = st.grid[k];
            for (int q3 = 0; q3 < 3; ++q3) { g.min[q3] = gp.min[q3]; g.inv[q3] = gp.inv[q3]; g.cell[q3] = 1.0 / gp.inv[q3]; g.dim[q3] = gp.dim[q3]; }
            g.n_cells = gp.n_cells; g.cell_start = sb[k]->cell_start; g.rec = sb[k]->rec; g.pos_of = sb[k]->pos_of;
            ix.s[k].g = g;
            ix.s[k].uniq = sb[k]->uniq;
        }
    }
    const SensLists lists{{ix.s[0].env, ix.s[1].max_envs > 0 ? ix.s[1].env : ix.s[0].env}, &ix, {a, b}};  // (both sides one object: one set of lists)
    if (int rc = consumer_enqueue(c, sw, R.use, R.out, R.use.width ? &lists : nullptr)) return rc;
    mark(c, 4);
    for (int k = 0; k < sides; ++k)
        if (R.cl[k]->ev_used) { HIP_TRY(hipEventRecord(R.cl[k]->ev_used, s)); R.cl[k]->used_valid = true; }
    HIP_TRY(hipGetLastError());
    c->status_dirty = false;  // the record pass / launch_profile_publish leaves the device status clean
    if (int rc = wait_pass(c, flags_out)) return rc;
    collect_times(c, 0, 4);
    return LCHD_OK;
}

// The thresholded, device-resident call of a consumer (lchd_{composition,radial,attribution}_primitives_dev); cl: [use.sides].
static int consumer_primitives_dev(lchd_ctx* c, lchd_cloud* const* cl, const int64_t* d_anchors, const int32_t* d_wf_index, int64_t n, double thr,
                                   const PairConsumer& use, double* d_out) {
    CTX_LOCK(c);
    lchd_cloud *a = cl[0], *b = cl[use.sides - 1];
    if (!c->cfg_set) return fail(LCHD_EVALUE, "lchd_ctx_set_config has not been called");
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    consumer_drop_records(c, use);
    if (int rc = consumer_limits(c, use)) return rc;
    if (n <= 0) return LCHD_OK;
    if (!d_anchors || !d_out) return fail(LCHD_EVALUE, "null anchor / output pointer");
    if (int rc = consumer_list_limit(use, n)) return rc;
    if (!(thr > 0.0)) return fail(LCHD_EPANIC, "index out of bounds: threshold_distance = %g leaves every environment empty", thr);
    if (a->n == 0 || b->n == 0) return fail(LCHD_EPANIC, "index out of bounds: %s given for an empty structure", use.items);
    if (thr > a->reach || thr > b->reach)
        return fail(LCHD_EVALUE, "threshold_distance = %g is beyond the reach %g the periodic images were built with", thr, std::min(a->reach, b->reach));
    if (!std::isfinite(thr)) thr = 1.7e308;
    CTX_GUARD(c);
    for (int k = 0; k < use.sides; ++k)
        if (int rc = resolve_bbox(c, cl[k])) return rc;
    if (use.resolve == kSensImages)  // (the origin maps the resolve step reads: built here, on the stream in front of the pass, if the last build left none)
        for (int k = 0; k < use.sides; ++k)
            if (cl[k]->images) if (int rc = images_origin(c, cl[k])) return rc;
    const bool keep_sweep_record = c->last_sweep_valid;  // (host data: the record of the last scoring pass stands)
    c->last_valid = false;                               // (its arrays do not: the arena is laid out anew)
    const ConsumerRequest R{{a, b}, d_anchors, d_wf_index, n, thr, use, d_out};
    // The retry ladder: an environment that did not fit its slot repeats the WHOLE pass with slots that hold the largest one reported (a
    // candidate-table overflow of k_env_group reports a bound; k_env_cells then counts).  Every row is written again: a row's bits do
    // not depend on the slot size.
    auto ladder = [&]() -> int {
        int cap = kEnvGroupCap;
        for (int attempt = 0; attempt < 8; ++attempt) {
            uint32_t f = 0;
            if (int rc = consumer_prims_pass(c, R, cap, &f)) return rc;
            const HostStatus h = *c->h_status;
            if ((f & ST_BAD_ANCHOR) || !(f & ST_ENV_OVERFLOW)) {
                if (int rc = status_to_rc(f & ~(uint32_t)ST_ENV_OVERFLOW, DRV_PRIMS)) return rc;
                if (use.width && !use.wgrad) {  // (the record pass publishes the longest environment among the pairs: the row width the call takes)
                    c->sens_needed = (int64_t)h.max_env;
                    if (h.max_env > (uint32_t)use.width)
                        return fail(LCHD_EVALUE, "row width %d is too small: the longest environment of these pairs holds %u points (lchd_sensitivity_needed_width)",
                                    use.width, h.max_env);
                }
                return LCHD_OK;
            }
            const int64_t want = std::max<int64_t>(std::max<int64_t>(h.max_env, h.max_bound / 3), cap + 1);
            if (h.max_env > (uint32_t)kRadialMaxPoints || cap > kRadialMaxPoints)
                return fail(LCHD_EUNSUPPORTED, "an environment holds %u points; %s takes at most %d", h.max_env, use.what, kRadialMaxPoints);
            cap = std::min(next_pow2_host(want), kRadialMaxPoints + 1);
        }
        return fail(LCHD_EDEVICE, "environment capacity retry did not converge");
    };
    const int rc = ladder();
    if (keep_sweep_record) c->last_sweep_valid = true;  // (a grown workspace drops both records; this one is host data)
    return rc;
}

// One structure of a thresholded host call, as lchd_from_primitives takes it, optionally in an orthorhombic box or a triclinic cell.
struct ProfilePrimsSide {
    const double* xyz;
    const int32_t *cat, *tag;
    int64_t n;
    const double *box, *cell;
};
// ... and from host arrays (lchd_{composition,radial,attribution}_primitives[_periodic]); sd: [use.sides].  Every structure goes to the
// device as a cloud of its own, a periodic one is replaced by its image cloud (reach = the threshold), and the call is the one above.
// The caller has checked c and cfg.
static int consumer_primitives_host(lchd_ctx* c, const lchd_config* cfg, const ProfilePrimsSide* sd, const int64_t* anchors, const int32_t* wf_index,
                                    int64_t n, double thr, const PairConsumer& use, double* out) {
    CTX_LOCK(c);
    const int sides = use.sides;
    for (int k = 0; k < sides; ++k)
        if (sd[k].box && sd[k].cell)
            return fail(LCHD_EVALUE, "a box and a cell were both given: a structure has one periodic box or one periodic cell");
    if (int rc = check_wf_index(cfg, wf_index, n)) return rc;
    for (int k = 0; k < sides; ++k)
        if (sd[k].n < 0 || sd[k].n > ((int64_t)1 << 27)) return fail(LCHD_EUNSUPPORTED, "structure size out of range");
    for (int k = 0; k < sides; ++k)
        if (sd[k].box) if (int rc = lchd_box_validate(sd[k].box, 1, thr)) return rc;
    for (int k = 0; k < sides; ++k)
        if (sd[k].cell) if (int rc = lchd_cell_validate(sd[k].cell, 1, thr)) return rc;
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    if (n > 0 && (!anchors || !out)) return fail(LCHD_EVALUE, "null anchor / output pointer");
    for (int64_t p = 0; p < n; ++p)  // (an index beyond the structure would name a ghost atom of an image cloud)
        for (int k = 0; k < sides; ++k)
            if (anchors[sides * p + k] < 0 || anchors[sides * p + k] >= sd[k].n)
                return fail(LCHD_EPANIC, "index out of bounds: an anchor index is outside its structure (src/locohd.rs:521)");
    CTX_GUARD(c);
    if (int rc = lchd_ctx_set_config(c, cfg)) return rc;
    if (n <= 0) return LCHD_OK;
    HostTemps t(c);
    lchd_cloud** const img = t.clouds;       // [sides] image clouds, destroyed before
    lchd_cloud** const own = t.clouds + 2;   // [sides] the structures themselves
    char*& d_blk = t.d_blk;
    const size_t K = consumer_row(c, use);
    const size_t o_wf = sizeof(int64_t) * (size_t)sides * (size_t)n, o_out = (o_wf + sizeof(int32_t) * (size_t)n + 255) & ~size_t(255);
    auto run = [&]() -> int {
        for (int k = 0; k < sides; ++k)
            if (int rc = lchd_cloud_create(c, sd[k].xyz, sd[k].cat, sd[k].tag, sd[k].n, &own[k])) return rc;
        for (int k = 0; k < sides; ++k)
            if (sd[k].box) if (int rc = lchd_cloud_create_images(c, own[k], sd[k].box, 1, thr, &img[k])) return rc;
        for (int k = 0; k < sides; ++k)
            if (sd[k].cell) if (int rc = lchd_cloud_create_images_cell(c, own[k], sd[k].cell, 1, thr, &img[k])) return rc;
        HIP_TRY(hipMalloc(&d_blk, o_out + sizeof(double) * (size_t)n * K));
        HIP_TRY(hipMemcpy(d_blk, anchors, o_wf, hipMemcpyHostToDevice));
        if (wf_index) HIP_TRY(hipMemcpy(d_blk + o_wf, wf_index, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
        lchd_cloud* cl[2] = {nullptr, nullptr};
        for (int k = 0; k < sides; ++k) cl[k] = img[k] ? img[k] : own[k];
        if (int rc = consumer_primitives_dev(c, cl, reinterpret_cast<const int64_t*>(d_blk),
                                             wf_index ? reinterpret_cast<const int32_t*>(d_blk + o_wf) : nullptr, n, thr, use,
                                             reinterpret_cast<double*>(d_blk + o_out)))
            return rc;
        HIP_TRY(hipMemcpy(out, d_blk + o_out, sizeof(double) * (size_t)n * K, hipMemcpyDeviceToHost));
        return LCHD_OK;
    };
    return t.rc = run();
}

// Dense rows: entry r = row r of every side (composition: of the one structure).  Row r is the whole structure seen from atom r
// (from_coords) or the given distance row r (from_dmxs).  src[k]: the side's coordinates (an open side is read in place, whatever the
// other side is) or DEVICE rows.  Every side goes through k_env_rows, which materialises the store
// (the fused sort-and-sweep kernel never writes one).  A sensitivity call also builds the indexed lists of both sides' rows
// (launch_rows_indexed, from the same rows or coordinates) for its kernel; the stores still feed the record pass.  src: [use.sides].
static int consumer_dense(lchd_ctx* c, const RowSource* src, int64_t rows, const int32_t* d_wf, const PairConsumer& use, double* d_out) {
    const int sides = use.sides;
    const int n_wf = c->h_cfg.n_wf;
    const bool cat16 = c->h_cfg.n_categories > kMaxCategories;
    const size_t sets = n_wf > 1 ? (size_t)n_wf + 1 : 1;  // (a dictionary: set 0 and one set per function, filled below)
    int cap[2] = {0, 0};
    EnvStore e[2] = {};
    double* w[2] = {nullptr, nullptr};
    const double* d_m[2] = {nullptr, nullptr};
    int4* d_meta = nullptr;
    // the consumers always take the per-side k_env_rows, never k_env_rows2 or the fused kernel, and have no retry
    lchd_dense_plan plan{};
    plan.path = LCHD_DENSE_ROWS;
    for (int k = 0; k < sides; ++k) {
        cap[k] = next_pow2_host(src[k].cols);
        if (!plan_dense_rows_side(cap[k], src[k].cols, cat16, plan.rows[k])) return fail(LCHD_EUNSUPPORTED, "no dense environment kernel for this row length");
    }
    for (int dry = 1; dry >= 0; --dry) {
        Arena ar(dry ? nullptr : c->ws, dry ? 0 : c->ws_cap, dry != 0);
        for (int k = 0; k < sides; ++k) e[k] = carve_row_store(ar, rows, cap[k], sets, cat16);
        if (use.records) d_meta = ar.take<int4>((size_t)rows);
        for (int k = 0; k < sides; ++k) w[k] = take_rows(ar, src[k], rows);
        if (dry) if (int rc = ensure_ws(c, ar.off + 4096)) return rc;
    }
    for (int k = 0; k < sides; ++k) e[k].cdf_keys = n_wf == 1 ? 1 : 0;  // (LCHD_NO_CDF_KEYS is the scoring passes' hook)
    // a sensitivity call: one indexed-list block per side, slots of the scoring stores' stride, in the block of the thresholded call
    // (grow-only, outside the arena): 13 bytes per padded point and side
    RowsIndexedArgs rx{};
    if (use.width) {
        size_t off[2][4], need = 0;
        for (int k = 0; k < 2; ++k) {
            const size_t pts = (size_t)rows * (size_t)cap[k];
            const size_t bytes[4] = {4 * (size_t)rows, 8 * pts, 4 * pts, pts};  // len, dist, idx, cat
            for (int j = 0; j < 4; ++j) { off[k][j] = need; need = (need + bytes[j] + 255) & ~size_t(255); }
        }
        if (int rc = grow_block(c->d_indexed, c->indexed_cap, need + 256)) return rc;
        rx.cfg = c->d_cfg; rx.rows = rows; rx.st = c->d_status;
        for (int k = 0; k < 2; ++k) {
            RowsIndexedSide& S = rx.s[k];
            S.c = src[k].view;
            S.ld = src[k].cols;
            S.cols = (int32_t)src[k].cols;
            S.env.len = reinterpret_cast<int32_t*>(c->d_indexed + off[k][0]);
            S.env.dist = reinterpret_cast<double*>(c->d_indexed + off[k][1]);
            S.env.idx = reinterpret_cast<uint32_t*>(c->d_indexed + off[k][2]);
            S.env.cat = reinterpret_cast<uint8_t*>(c->d_indexed + off[k][3]);
            S.env.stride = cap[k];
        }
    }
    hipStream_t s = c->stream;
    if (int rc = begin_pass(c)) return rc;
    c->status_dirty = true;
    mark(c, 0);
    for (int k = 0; k < sides; ++k)
        if (int rc = produce_rows(c, src[k], 0, rows, w[k], d_m[k])) return rc;
    mark(c, 1);
    // (between events 1 and 2, which nothing else of a dense pass separates: lchd_ctx_last_ms "anchors" is the list build's time)
    if (use.width) {
        for (int k = 0; k < 2; ++k) rx.s[k].dmx = d_m[k];
        if (!launch_rows_indexed(s, rx)) return fail(LCHD_EDEVICE, "internal error: the indexed-list kernel rejected its launch configuration");
    }
    mark(c, 2);
    int32_t canon = 0;  // (not recorded: a consumer call leaves c->last_dense, and last_sweep_valid, as it found them)
    if (!sort_rows(c, plan, sides, src, d_m, e, rows, &canon)) return fail(LCHD_EUNSUPPORTED, "no dense environment kernel for this row length");
    if (n_wf > 1) {
        launch_profile_rows(s, c->d_status, rows);  // (the key-set kernel walks DeviceStatus::n_unique[0] rows of its first store)
        for (int k = 0; k < sides; ++k) launch_env_key_sets(s, c->d_cfg, e[k], e[k], n_wf, rows, c->d_status);
        for (int k = 0; k < sides; ++k) {
            e[k].key += e[k].set_stride;
            e[k].cdf_keys = n_wf;
        }
    }
    mark(c, 3);
    SweepArgs sw{};
    sw.env_a = e[0];
    sw.env_b = e[sides - 1];
    sw.wf_index = d_wf;
    sw.n_pairs = rows;
    sw.meta = d_meta;
    const SensLists lists{{rx.s[0].env, rx.s[1].env}, nullptr, {nullptr, nullptr}, src};
    if (int rc = consumer_enqueue(c, sw, use, d_out, use.width ? &lists : nullptr)) return rc;
    mark(c, 4);
    HIP_TRY(hipGetLastError());
    c->status_dirty = false;
    uint32_t f = 0;
    if (int rc = wait_pass(c, &f)) return rc;
    collect_times(c, 0, 4);
    return status_to_rc(f, DRV_DMXS);
}
static int consumer_dense_check(lchd_ctx* c, const PairConsumer& use, const int64_t* cols) {
    if (int rc = consumer_limits(c, use)) return rc;
    bool over = false;
    for (int k = 0; k < use.sides; ++k) over = over || cols[k] > kRadialMaxPoints;
    if (!over) {
        if (!use.width || use.wgrad) return LCHD_OK;
        // every column is a member: the rows of a dense sensitivity call are as long as the longer side's
        const int64_t longest = std::max(cols[0], cols[1]);
        c->sens_needed = longest;
        if (use.width < longest)
            return fail(LCHD_EVALUE, "row width %d is too small: the longest row of these matrices holds %lld points (lchd_sensitivity_needed_width)",
                        use.width, (long long)longest);
        return LCHD_OK;
    }
    char got[64];
    int len = 0;
    for (int k = 0; k < use.sides; ++k) len += snprintf(got + len, sizeof got - (size_t)len, k ? " / %lld" : "%lld", (long long)cols[k]);
    return fail(LCHD_EUNSUPPORTED, "%s takes dense rows of at most %d points (got %s)", use.what, kRadialMaxPoints, got);
}

// The dense, device-resident call of a consumer (lchd_{composition,radial,attribution}_coords_dev); cl, cells: [use.sides].
static int consumer_coords_dev(lchd_ctx* c, lchd_cloud* const* cl, const int32_t* d_wf_index, const double* const* cells, const PairConsumer& use,
                               double* d_out) {
    CTX_LOCK(c);
    const int sides = use.sides;
    lchd_cloud *a = cl[0], *b = cl[sides - 1];
    if (!c->cfg_set) return fail(LCHD_EVALUE, "lchd_ctx_set_config has not been called");
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    if (a->sid || b->sid) return fail(LCHD_EVALUE, "from_coords takes single structures, not batches");
    for (int k = 0; k < sides; ++k)
        if (cells[k] && cl[k]->images) return fail(LCHD_EVALUE, "a periodic dense call takes the structures themselves, not their image clouds");
    if (a->n != b->n)
        return fail(LCHD_EVALUE, "Expected matrices with the same length, got lengths %lld and %lld!", (long long)a->n, (long long)b->n);
    MinImageCell rec[2];
    const MinImageCell* cell[2];
    if (int rc = reduce_cells(cells, sides, false, rec, cell)) return rc;
    consumer_drop_records(c, use);
    if (a->n == 0) return LCHD_OK;
    if (!d_out) return fail(LCHD_EVALUE, "null output pointer");
    const int64_t cols[2] = {a->n, b->n};
    if (int rc = consumer_dense_check(c, use, cols)) return rc;
    CTX_GUARD(c);
    for (int k = 0; k < sides; ++k)
        if (int rc = resolve_bbox(c, cl[k])) return rc;
    const bool keep_sweep_record = c->last_sweep_valid;
    c->last_valid = false;
    const bool cat16 = c->h_cfg.n_categories > kMaxCategories;
    RowSource src[2] = {};
    for (int k = 0; k < sides; ++k) src[k] = cloud_source(*cl[k], cat16, cols[k], cell[k]);
    const int rc = consumer_dense(c, src, a->n, d_wf_index, use, d_out);
    if (keep_sweep_record) c->last_sweep_valid = true;
    return rc;
}

// One side of a dense host call: coordinates (xyz set, dmx null; optional cell) or given rows (dmx [rows][cols], xyz null).
struct ProfileDenseSide {
    const int32_t* seq;
    int64_t len_seq;
    const double *xyz, *dmx;
    int64_t cols;
    const double* cell;
};
// ... and from host arrays (lchd_{composition,radial,attribution}_{coords,dmx[s]}); sd: [use.sides].  The caller has checked c and cfg.
static int consumer_dense_host(lchd_ctx* c, const lchd_config* cfg, const ProfileDenseSide* sd, int64_t rows, const int32_t* wf_index,
                               const PairConsumer& use, double* out) {
    CTX_LOCK(c);
    const int sides = use.sides;
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    const double* const cells[2] = {sd[0].cell, sides > 1 ? sd[1].cell : nullptr};
    MinImageCell rec[2];
    const MinImageCell* cell[2];
    if (int rc = reduce_cells(cells, sides, false, rec, cell)) return rc;
    CTX_GUARD(c);
    if (int rc = lchd_ctx_set_config(c, cfg)) return rc;
    if (int rc = check_wf_index(cfg, wf_index, rows)) return rc;
    consumer_drop_records(c, use);
    if (rows == 0) return LCHD_OK;
    int64_t cols[2] = {0, 0};
    bool longer = false, empty = false, null_side = false;
    for (int k = 0; k < sides; ++k) {
        cols[k] = sd[k].cols;
        longer = longer || sd[k].cols > sd[k].len_seq;
        empty = empty || sd[k].cols == 0;
        null_side = null_side || (!sd[k].xyz && !sd[k].dmx);
    }
    if (longer) return fail(LCHD_EPANIC, "index out of bounds: a distance row is longer than its seq");
    if (empty) return fail(LCHD_EPANIC, "index out of bounds: empty distance row (src/locohd.rs:74)");
    if (int rc = consumer_dense_check(c, use, cols)) return rc;
    if (!out || null_side) return fail(LCHD_EVALUE, "null pointer");
    const bool keep_sweep_record = c->last_sweep_valid;
    c->last_valid = false;
    HostTemps t(c);
    char*& d_blk = t.d_blk;
    const size_t K = consumer_row(c, use);
    size_t o_m[2] = {0, 0}, o_wf = 0;  // the given rows of every side, 256-byte aligned, then the weight-function indices
    for (int k = 0; k < sides; ++k) {
        o_m[k] = o_wf;
        if (sd[k].dmx) o_wf = (o_wf + sizeof(double) * (size_t)rows * (size_t)sd[k].cols + 255) & ~size_t(255);
    }
    const size_t o_out = (o_wf + sizeof(int32_t) * (size_t)rows + 255) & ~size_t(255);
    auto run = [&]() -> int {
        RowSource src[2] = {};
        for (int k = 0; k < sides; ++k)  // (given rows: the cloud carries the categories alone)
            if (int rc = lchd_cloud_create(c, sd[k].xyz, sd[k].seq, nullptr, sd[k].cols, &t.clouds[k])) return rc;
        HIP_TRY(hipMalloc(&d_blk, o_out + sizeof(double) * (size_t)rows * K));
        for (int k = 0; k < sides; ++k) {
            src[k] = cloud_source(*t.clouds[k], cfg->n_categories > kMaxCategories, cols[k], cell[k]);
            if (sd[k].dmx) {  // (the call's block holds them: rows on the device for the pass)
                HIP_TRY(hipMemcpy(d_blk + o_m[k], sd[k].dmx, sizeof(double) * (size_t)rows * (size_t)sd[k].cols, hipMemcpyHostToDevice));
                src[k].kind = RowSource::DEVICE_ROWS;
                src[k].m = reinterpret_cast<const double*>(d_blk + o_m[k]);
            }
        }
        if (wf_index) HIP_TRY(hipMemcpy(d_blk + o_wf, wf_index, sizeof(int32_t) * (size_t)rows, hipMemcpyHostToDevice));
        if (int rc = consumer_dense(c, src, rows, wf_index ? reinterpret_cast<const int32_t*>(d_blk + o_wf) : nullptr, use,
                                    reinterpret_cast<double*>(d_blk + o_out)))
            return rc;
        HIP_TRY(hipMemcpy(out, d_blk + o_out, sizeof(double) * (size_t)rows * K, hipMemcpyDeviceToHost));
        return LCHD_OK;
    };
    t.rc = run();
    if (keep_sweep_record) c->last_sweep_valid = true;
    return t.rc;
}
// from_coords' argument rule (the pair consumers)
static int coords_lengths(const double* xyz_a, int64_t n_a, const double* xyz_b, int64_t n_b) {
    if (n_a != n_b)  // src/locohd.rs:420-428 via :472-475
        return fail(LCHD_EVALUE, "Expected matrices with the same length, got lengths %lld and %lld!", (long long)n_a, (long long)n_b);
    if (n_a > 0 && (!xyz_a || !xyz_b)) return fail(LCHD_EVALUE, "null pointer");
    return LCHD_OK;
}

// ---- the entry points: argument adapters ----------------------------------------------------------------------------
// local composition profiles: one structure, one list of anchors, rows of n_categories doubles
extern "C" int lchd_composition_primitives_dev(lchd_ctx* c, lchd_cloud* cl, const int64_t* d_anchors, const int32_t* d_wf_index,
                                               int64_t n_anchors, double thr, double* d_out) {
    if (!c || !cl) return fail(LCHD_EVALUE, "null argument");
    return consumer_primitives_dev(c, &cl, d_anchors, d_wf_index, n_anchors, thr, kComposition, d_out);
}
extern "C" int lchd_composition_primitives_periodic(lchd_ctx* c, const lchd_config* cfg, const double* xyz, const int32_t* cat,
                                                    const int32_t* tag, int64_t n, const int64_t* anchors, const int32_t* wf_index,
                                                    int64_t n_anchors, double thr, const double* box, const double* cell, double* out) {
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    const ProfilePrimsSide sd{xyz, cat, tag, n, box, cell};
    return consumer_primitives_host(c, cfg, &sd, anchors, wf_index, n_anchors, thr, kComposition, out);
}
extern "C" int lchd_composition_primitives(lchd_ctx* c, const lchd_config* cfg, const double* xyz, const int32_t* cat, const int32_t* tag,
                                           int64_t n, const int64_t* anchors, const int32_t* wf_index, int64_t n_anchors, double thr,
                                           double* out) {
    return lchd_composition_primitives_periodic(c, cfg, xyz, cat, tag, n, anchors, wf_index, n_anchors, thr, nullptr, nullptr, out);
}
extern "C" int lchd_composition_coords_dev(lchd_ctx* c, lchd_cloud* cl, const int32_t* d_wf_index, const double* cell, double* d_out) {
    if (!c || !cl) return fail(LCHD_EVALUE, "null argument");
    return consumer_coords_dev(c, &cl, d_wf_index, &cell, kComposition, d_out);
}
extern "C" int lchd_composition_coords(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq, int64_t len_seq, const double* xyz, int64_t n,
                                       const int32_t* wf_index, const double* cell, double* out) {
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    const ProfileDenseSide sd{seq, len_seq, xyz, nullptr, n, cell};
    return consumer_dense_host(c, cfg, &sd, n, wf_index, kComposition, out);
}
extern "C" int lchd_composition_dmx(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq, int64_t len_seq, const double* dmx, int64_t rows,
                                    int64_t cols, const int32_t* wf_index, double* out) {
    if (rows > 0 && !dmx) return fail(LCHD_EVALUE, "null pointer");
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    const ProfileDenseSide sd{seq, len_seq, nullptr, dmx, cols, nullptr};
    return consumer_dense_host(c, cfg, &sd, rows, wf_index, kComposition, out);
}

// the pair consumers: two structures, one list of anchor pairs.  edges null: attribution (rows of n_categories doubles), else the
// radial profile over these edges (rows of n_edges - 1 doubles); each entry point validates its edges where it did before the merge.
static int pair_primitives_host(lchd_ctx* c, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a, const int32_t* tag_a, int64_t n_a,
                                const double* xyz_b, const int32_t* cat_b, const int32_t* tag_b, int64_t n_b, const int64_t* anchors,
                                const int32_t* wf_index, int64_t n_pairs, double thr, const double* box_a, const double* cell_a,
                                const double* box_b, const double* cell_b, const PairConsumer& use, double* out) {
    const ProfilePrimsSide sd[2] = {{xyz_a, cat_a, tag_a, n_a, box_a, cell_a}, {xyz_b, cat_b, tag_b, n_b, box_b, cell_b}};
    return consumer_primitives_host(c, cfg, sd, anchors, wf_index, n_pairs, thr, use, out);
}
static int pair_dense_host(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b, int64_t len_seq_b,
                           const double* xyz_a, const double* xyz_b, const double* dmx_a, const double* dmx_b, int64_t rows, int64_t cols_a,
                           int64_t cols_b, const int32_t* wf_index, const double* cell_a, const double* cell_b, const PairConsumer& use,
                           double* out) {
    const ProfileDenseSide sd[2] = {{seq_a, len_seq_a, xyz_a, dmx_a, cols_a, cell_a}, {seq_b, len_seq_b, xyz_b, dmx_b, cols_b, cell_b}};
    return consumer_dense_host(c, cfg, sd, rows, wf_index, use, out);
}

extern "C" int lchd_radial_primitives_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int64_t* d_anchors, const int32_t* d_wf_index,
                                          int64_t n_pairs, double thr, const double* edges, int32_t n_edges, double* d_out) {
    if (!c || !a || !b) return fail(LCHD_EVALUE, "null argument");
    if (int rc = lchd_radial_validate(edges, n_edges)) return rc;
    lchd_cloud* const cl[2] = {a, b};
    return consumer_primitives_dev(c, cl, d_anchors, d_wf_index, n_pairs, thr, radial_consumer(edges, n_edges), d_out);
}
extern "C" int lchd_radial_primitives(lchd_ctx* c, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a, const int32_t* tag_a,
                                      int64_t n_a, const double* xyz_b, const int32_t* cat_b, const int32_t* tag_b, int64_t n_b,
                                      const int64_t* anchors, const int32_t* wf_index, int64_t n_pairs, double thr, const double* box_a,
                                      const double* cell_a, const double* box_b, const double* cell_b, const double* edges, int32_t n_edges,
                                      double* out) {
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    if (int rc = lchd_radial_validate(edges, n_edges)) return rc;
    return pair_primitives_host(c, cfg, xyz_a, cat_a, tag_a, n_a, xyz_b, cat_b, tag_b, n_b, anchors, wf_index, n_pairs, thr, box_a, cell_a, box_b,
                                cell_b, radial_consumer(edges, n_edges), out);
}
extern "C" int lchd_radial_coords_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int32_t* d_wf_index, const double* cell_a,
                                      const double* cell_b, const double* edges, int32_t n_edges, double* d_out) {
    if (!c || !a || !b) return fail(LCHD_EVALUE, "null argument");
    if (int rc = lchd_radial_validate(edges, n_edges)) return rc;
    lchd_cloud* const cl[2] = {a, b};
    const double* const cells[2] = {cell_a, cell_b};
    return consumer_coords_dev(c, cl, d_wf_index, cells, radial_consumer(edges, n_edges), d_out);
}
extern "C" int lchd_radial_coords(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b,
                                  int64_t len_seq_b, const double* xyz_a, int64_t n_a, const double* xyz_b, int64_t n_b, const int32_t* wf_index,
                                  const double* cell_a, const double* cell_b, const double* edges, int32_t n_edges, double* out) {
    if (int rc = coords_lengths(xyz_a, n_a, xyz_b, n_b)) return rc;
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    if (int rc = lchd_radial_validate(edges, n_edges)) return rc;
    return pair_dense_host(c, cfg, seq_a, len_seq_a, seq_b, len_seq_b, xyz_a, xyz_b, nullptr, nullptr, n_a, n_a, n_b, wf_index, cell_a, cell_b,
                           radial_consumer(edges, n_edges), out);
}
extern "C" int lchd_radial_dmxs(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b,
                                int64_t len_seq_b, const double* dmx_a, const double* dmx_b, int64_t rows, int64_t cols_a, int64_t cols_b,
                                const int32_t* wf_index, const double* edges, int32_t n_edges, double* out) {
    if (rows > 0 && (!dmx_a || !dmx_b)) return fail(LCHD_EVALUE, "null pointer");
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    if (int rc = lchd_radial_validate(edges, n_edges)) return rc;
    return pair_dense_host(c, cfg, seq_a, len_seq_a, seq_b, len_seq_b, nullptr, nullptr, dmx_a, dmx_b, rows, cols_a, cols_b, wf_index, nullptr, nullptr,
                           radial_consumer(edges, n_edges), out);
}

// score attribution by category: the radial calls with the other consumer; the stores and records go to launch_attribution
// (lchd_attribution.hip).  Hellinger distances only.
extern "C" int lchd_attribution_primitives_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int64_t* d_anchors, const int32_t* d_wf_index,
                                               int64_t n_pairs, double thr, double* d_out) {
    if (!c || !a || !b) return fail(LCHD_EVALUE, "null argument");
    lchd_cloud* const cl[2] = {a, b};
    return consumer_primitives_dev(c, cl, d_anchors, d_wf_index, n_pairs, thr, kAttribution, d_out);
}
extern "C" int lchd_attribution_primitives(lchd_ctx* c, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a, const int32_t* tag_a,
                                           int64_t n_a, const double* xyz_b, const int32_t* cat_b, const int32_t* tag_b, int64_t n_b,
                                           const int64_t* anchors, const int32_t* wf_index, int64_t n_pairs, double thr, const double* box_a,
                                           const double* cell_a, const double* box_b, const double* cell_b, double* out) {
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    return pair_primitives_host(c, cfg, xyz_a, cat_a, tag_a, n_a, xyz_b, cat_b, tag_b, n_b, anchors, wf_index, n_pairs, thr, box_a, cell_a, box_b,
                                cell_b, kAttribution, out);
}
extern "C" int lchd_attribution_coords_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int32_t* d_wf_index, const double* cell_a,
                                           const double* cell_b, double* d_out) {
    if (!c || !a || !b) return fail(LCHD_EVALUE, "null argument");
    lchd_cloud* const cl[2] = {a, b};
    const double* const cells[2] = {cell_a, cell_b};
    return consumer_coords_dev(c, cl, d_wf_index, cells, kAttribution, d_out);
}
extern "C" int lchd_attribution_coords(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b,
                                       int64_t len_seq_b, const double* xyz_a, int64_t n_a, const double* xyz_b, int64_t n_b,
                                       const int32_t* wf_index, const double* cell_a, const double* cell_b, double* out) {
    if (int rc = coords_lengths(xyz_a, n_a, xyz_b, n_b)) return rc;
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    return pair_dense_host(c, cfg, seq_a, len_seq_a, seq_b, len_seq_b, xyz_a, xyz_b, nullptr, nullptr, n_a, n_a, n_b, wf_index, cell_a, cell_b,
                           kAttribution, out);
}
extern "C" int lchd_attribution_dmxs(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b,
                                     int64_t len_seq_b, const double* dmx_a, const double* dmx_b, int64_t rows, int64_t cols_a, int64_t cols_b,
                                     const int32_t* wf_index, double* out) {
    if (rows > 0 && (!dmx_a || !dmx_b)) return fail(LCHD_EVALUE, "null pointer");
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    return pair_dense_host(c, cfg, seq_a, len_seq_a, seq_b, len_seq_b, nullptr, nullptr, dmx_a, dmx_b, rows, cols_a, cols_b, wf_index, nullptr, nullptr,
                           kAttribution, out);
}

// category-weight gradients: the attribution calls with the fourth consumer; the stores and records go to launch_category_gradient
// (lchd_category_gradient.hip).  Hellinger and Kullback-Leibler distances.
extern "C" int lchd_category_gradient_primitives_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int64_t* d_anchors, const int32_t* d_wf_index,
                                                     int64_t n_pairs, double thr, double* d_out) {
    if (!c || !a || !b) return fail(LCHD_EVALUE, "null argument");
    lchd_cloud* const cl[2] = {a, b};
    return consumer_primitives_dev(c, cl, d_anchors, d_wf_index, n_pairs, thr, kCategoryGradient, d_out);
}
extern "C" int lchd_category_gradient_primitives(lchd_ctx* c, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a,
                                                 const int32_t* tag_a, int64_t n_a, const double* xyz_b, const int32_t* cat_b, const int32_t* tag_b,
                                                 int64_t n_b, const int64_t* anchors, const int32_t* wf_index, int64_t n_pairs, double thr,
                                                 const double* box_a, const double* cell_a, const double* box_b, const double* cell_b, double* out) {
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    return pair_primitives_host(c, cfg, xyz_a, cat_a, tag_a, n_a, xyz_b, cat_b, tag_b, n_b, anchors, wf_index, n_pairs, thr, box_a, cell_a, box_b,
                                cell_b, kCategoryGradient, out);
}
extern "C" int lchd_category_gradient_coords_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int32_t* d_wf_index, const double* cell_a,
                                                 const double* cell_b, double* d_out) {
    if (!c || !a || !b) return fail(LCHD_EVALUE, "null argument");
    lchd_cloud* const cl[2] = {a, b};
    const double* const cells[2] = {cell_a, cell_b};
    return consumer_coords_dev(c, cl, d_wf_index, cells, kCategoryGradient, d_out);
}
extern "C" int lchd_category_gradient_coords(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b,
                                             int64_t len_seq_b, const double* xyz_a, int64_t n_a, const double* xyz_b, int64_t n_b,
                                             const int32_t* wf_index, const double* cell_a, const double* cell_b, double* out) {
    if (int rc = coords_lengths(xyz_a, n_a, xyz_b, n_b)) return rc;
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    return pair_dense_host(c, cfg, seq_a, len_seq_a, seq_b, len_seq_b, xyz_a, xyz_b, nullptr, nullptr, n_a, n_a, n_b, wf_index, cell_a, cell_b,
                           kCategoryGradient, out);
}
extern "C" int lchd_category_gradient_dmxs(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b,
                                           int64_t len_seq_b, const double* dmx_a, const double* dmx_b, int64_t rows, int64_t cols_a,
                                           int64_t cols_b, const int32_t* wf_index, double* out) {
    if (rows > 0 && (!dmx_a || !dmx_b)) return fail(LCHD_EVALUE, "null pointer");
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    return pair_dense_host(c, cfg, seq_a, len_seq_a, seq_b, len_seq_b, nullptr, nullptr, dmx_a, dmx_b, rows, cols_a, cols_b, wf_index, nullptr, nullptr,
                           kCategoryGradient, out);
}

// neighbour sensitivities: every statistical distance.  The thresholded pass is the attribution call's with the indexed lists (built from
// the pass's cell lists) and k_sensitivity (lchd_sensitivity.hip) behind the record pass; periodic boxes, cells and image clouds only in
// the calls that resolve the members (lchd_sensitivity_images_dev / _primitives_periodic: k_sens_resolve_images behind the two).
// A host call's pass writes ONE block (sens_carve) in the layout of `resolve`, which `pass` receives with that value: the consumer and
// the copy back carve the same block.  The HOST arrays of `o` are filled from it: the nine, and the disp (and image) arrays of a
// resolving call.
template <class Pass>
static int sens_host_call(int64_t n_pairs, int32_t width, int resolve, const SensitivityOut& o, Pass&& pass) {
    const size_t n = n_pairs > 0 ? (size_t)n_pairs : 0, nw = n * (size_t)width;
    double* blk = n ? static_cast<double*>(malloc(sizeof(double) * n * sens_row(width, resolve))) : nullptr;
    if (n && !blk) return fail(LCHD_EUNSUPPORTED, "no host memory for the outputs of %lld pairs", (long long)n_pairs);
    const int rc = pass(blk, resolve);
    if (rc == LCHD_OK && n) {
        const SensitivityOut b = sens_carve(blk, n_pairs, width, resolve);
        memcpy(o.scores, b.scores, 8 * n);
        memcpy(o.g_a, b.g_a, 8 * nw); memcpy(o.g_b, b.g_b, 8 * nw);
        memcpy(o.dist_a, b.dist_a, 8 * nw); memcpy(o.dist_b, b.dist_b, 8 * nw);
        memcpy(o.idx_a, b.idx_a, 4 * nw); memcpy(o.idx_b, b.idx_b, 4 * nw);
        memcpy(o.count_a, b.count_a, 4 * n); memcpy(o.count_b, b.count_b, 4 * n);
        if (resolve) { memcpy(o.disp_a, b.disp_a, 24 * nw); memcpy(o.disp_b, b.disp_b, 24 * nw); }
        if (resolve == kSensImages) { memcpy(o.image_a, b.image_a, nw); memcpy(o.image_b, b.image_b, nw); }
    }
    free(blk);
    return rc;
}
static int sens_args(lchd_ctx* c, int64_t n_pairs, int32_t width) {
    if (c) c->sens_needed = 0;
    if (width < 1 || width > kRadialMaxPoints) return fail(LCHD_EVALUE, "row width %d is outside 1 .. %d", width, kRadialMaxPoints);
    if (n_pairs > 0 && (size_t)n_pairs > ((size_t)1 << 40) / (5 * (size_t)width + 2))
        return fail(LCHD_EUNSUPPORTED, "%lld pairs with rows of %d slots exceed 8 TiB of output: split the list", (long long)n_pairs, width);
    return LCHD_OK;
}
extern "C" int lchd_sensitivity_primitives_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int64_t* d_anchors, const int32_t* d_wf_index,
                                               int64_t n_pairs, double thr, int32_t width, double* d_scores, int32_t* d_count_a, int32_t* d_idx_a,
                                               double* d_dist_a, double* d_g_a, int32_t* d_count_b, int32_t* d_idx_b, double* d_dist_b,
                                               double* d_g_b) {
    if (!c || !a || !b) return fail(LCHD_EVALUE, "null argument");
    if (int rc = sens_args(c, n_pairs, width)) return rc;
    if (n_pairs > 0 && (!d_scores || !d_count_a || !d_idx_a || !d_dist_a || !d_g_a || !d_count_b || !d_idx_b || !d_dist_b || !d_g_b))
        return fail(LCHD_EVALUE, "null output pointer");
    if (a->images || b->images) return fail(LCHD_EUNSUPPORTED, "a sensitivity call takes the structures themselves, not periodic image clouds");
    SensitivityOut o{};
    o.scores = d_scores; o.count_a = d_count_a; o.count_b = d_count_b; o.idx_a = d_idx_a; o.idx_b = d_idx_b;
    o.dist_a = d_dist_a; o.dist_b = d_dist_b; o.g_a = d_g_a; o.g_b = d_g_b;
    lchd_cloud* const cl[2] = {a, b};
    return consumer_primitives_dev(c, cl, d_anchors, d_wf_index, n_pairs, thr, sensitivity_consumer(width, o), d_scores);
}
extern "C" int lchd_sensitivity_primitives(lchd_ctx* c, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a, const int32_t* tag_a,
                                           int64_t n_a, const double* xyz_b, const int32_t* cat_b, const int32_t* tag_b, int64_t n_b,
                                           const int64_t* anchors, const int32_t* wf_index, int64_t n_pairs, double thr, int32_t width,
                                           double* scores, int32_t* count_a, int32_t* idx_a, double* dist_a, double* g_a, int32_t* count_b,
                                           int32_t* idx_b, double* dist_b, double* g_b) {
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    if (int rc = sens_args(c, n_pairs, width)) return rc;
    if (n_pairs > 0 && (!scores || !count_a || !idx_a || !dist_a || !g_a || !count_b || !idx_b || !dist_b || !g_b))
        return fail(LCHD_EVALUE, "null output pointer");
    const SensitivityOut o{scores, count_a, count_b, idx_a, idx_b, dist_a, dist_b, g_a, g_b};
    return sens_host_call(n_pairs, width, kSensPlain, o, [&](double* blk, int resolve) {
        return pair_primitives_host(c, cfg, xyz_a, cat_a, tag_a, n_a, xyz_b, cat_b, tag_b, n_b, anchors, wf_index, n_pairs, thr, nullptr, nullptr,
                                    nullptr, nullptr, sensitivity_consumer(width, SensitivityOut{}, resolve), blk);
    });
}
extern "C" int64_t lchd_sensitivity_needed_width(lchd_ctx* c) { return c ? c->sens_needed : 0; }

// ... that name source atoms: the same pass on clouds of which any may be an image cloud, then k_sens_resolve_images on both sides' rows.
extern "C" int lchd_sensitivity_images_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int64_t* d_anchors, const int32_t* d_wf_index,
                                           int64_t n_pairs, double thr, int32_t width, double* d_scores, int32_t* d_count_a, int32_t* d_idx_a,
                                           int8_t* d_image_a, double* d_dist_a, double* d_g_a, double* d_disp_a, int32_t* d_count_b,
                                           int32_t* d_idx_b, int8_t* d_image_b, double* d_dist_b, double* d_g_b, double* d_disp_b) {
    if (!c || !a || !b) return fail(LCHD_EVALUE, "null argument");
    if (int rc = sens_args(c, n_pairs, width)) return rc;
    if (n_pairs > 0 && (!d_scores || !d_count_a || !d_idx_a || !d_image_a || !d_dist_a || !d_g_a || !d_disp_a || !d_count_b || !d_idx_b ||
                        !d_image_b || !d_dist_b || !d_g_b || !d_disp_b))
        return fail(LCHD_EVALUE, "null output pointer");
    const SensitivityOut o{d_scores, d_count_a, d_count_b, d_idx_a, d_idx_b, d_dist_a, d_dist_b, d_g_a, d_g_b, d_disp_a, d_disp_b, d_image_a, d_image_b};
    lchd_cloud* const cl[2] = {a, b};
    return consumer_primitives_dev(c, cl, d_anchors, d_wf_index, n_pairs, thr, sensitivity_consumer(width, o, kSensImages), d_scores);
}
extern "C" int lchd_sensitivity_primitives_periodic(lchd_ctx* c, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a,
                                                    const int32_t* tag_a, int64_t n_a, const double* xyz_b, const int32_t* cat_b,
                                                    const int32_t* tag_b, int64_t n_b, const int64_t* anchors, const int32_t* wf_index,
                                                    int64_t n_pairs, double thr, int32_t width, const double* box_a, const double* cell_a,
                                                    const double* box_b, const double* cell_b, double* scores, int32_t* count_a,
                                                    int32_t* idx_a, int8_t* image_a, double* dist_a, double* g_a, double* disp_a,
                                                    int32_t* count_b, int32_t* idx_b, int8_t* image_b, double* dist_b, double* g_b,
                                                    double* disp_b) {
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    if (int rc = sens_args(c, n_pairs, width)) return rc;
    if (n_pairs > 0 && (!scores || !count_a || !idx_a || !image_a || !dist_a || !g_a || !disp_a || !count_b || !idx_b || !image_b || !dist_b ||
                        !g_b || !disp_b))
        return fail(LCHD_EVALUE, "null output pointer");
    const SensitivityOut o{scores, count_a, count_b, idx_a, idx_b, dist_a, dist_b, g_a, g_b, disp_a, disp_b, image_a, image_b};
    return sens_host_call(n_pairs, width, kSensImages, o, [&](double* blk, int resolve) {
        return pair_primitives_host(c, cfg, xyz_a, cat_a, tag_a, n_a, xyz_b, cat_b, tag_b, n_b, anchors, wf_index, n_pairs, thr, box_a, cell_a,
                                    box_b, cell_b, sensitivity_consumer(width, SensitivityOut{}, resolve), blk);
    });
}

// ... and of dense rows: the attribution calls of the same name with the other consumer.  consumer_dense builds the indexed lists of
// both sides' rows (launch_rows_indexed) next to the scoring stores, which stay in front of the record pass: its records, status
// hand-over and checks are the attribution call's.  Every column is a member, so rows are max(cols_a, cols_b) wide at least.
extern "C" int lchd_sensitivity_coords_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int32_t* d_wf_index, int32_t width, double* d_scores,
                                           int32_t* d_count_a, int32_t* d_idx_a, double* d_dist_a, double* d_g_a, int32_t* d_count_b,
                                           int32_t* d_idx_b, double* d_dist_b, double* d_g_b) {
    if (!c || !a || !b) return fail(LCHD_EVALUE, "null argument");
    if (int rc = sens_args(c, a->n, width)) return rc;
    if (a->n > 0 && (!d_scores || !d_count_a || !d_idx_a || !d_dist_a || !d_g_a || !d_count_b || !d_idx_b || !d_dist_b || !d_g_b))
        return fail(LCHD_EVALUE, "null output pointer");
    if (a->images || b->images) return fail(LCHD_EUNSUPPORTED, "a sensitivity call takes the structures themselves, not periodic image clouds");
    const SensitivityOut o{d_scores, d_count_a, d_count_b, d_idx_a, d_idx_b, d_dist_a, d_dist_b, d_g_a, d_g_b};
    lchd_cloud* const cl[2] = {a, b};
    const double* const cells[2] = {nullptr, nullptr};
    return consumer_coords_dev(c, cl, d_wf_index, cells, sensitivity_consumer(width, o), d_scores);
}
extern "C" int lchd_sensitivity_coords(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b,
                                       int64_t len_seq_b, const double* xyz_a, const double* xyz_b, int64_t n, const int32_t* wf_index,
                                       int32_t width, double* scores, int32_t* count_a, int32_t* idx_a, double* dist_a, double* g_a,
                                       int32_t* count_b, int32_t* idx_b, double* dist_b, double* g_b) {
    if (int rc = coords_lengths(xyz_a, n, xyz_b, n)) return rc;
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    if (int rc = sens_args(c, n, width)) return rc;
    if (n > 0 && (!scores || !count_a || !idx_a || !dist_a || !g_a || !count_b || !idx_b || !dist_b || !g_b))
        return fail(LCHD_EVALUE, "null output pointer");
    const SensitivityOut o{scores, count_a, count_b, idx_a, idx_b, dist_a, dist_b, g_a, g_b};
    return sens_host_call(n, width, kSensPlain, o, [&](double* blk, int resolve) {
        return pair_dense_host(c, cfg, seq_a, len_seq_a, seq_b, len_seq_b, xyz_a, xyz_b, nullptr, nullptr, n, n, n, wf_index, nullptr, nullptr,
                               sensitivity_consumer(width, SensitivityOut{}, resolve), blk);
    });
}
// ... in periodic cells (minimum image): the same two calls with the reduced cells in the row sources, and k_sens_min_image_disp behind
// k_sensitivity for the displacement of every member -- the direction a minimum-image row, which stores |w| alone, does not carry.
extern "C" int lchd_sensitivity_coords_periodic_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int32_t* d_wf_index, const double* cell_a,
                                                    const double* cell_b, int32_t width, double* d_scores, int32_t* d_count_a, int32_t* d_idx_a,
                                                    double* d_dist_a, double* d_g_a, int32_t* d_count_b, int32_t* d_idx_b, double* d_dist_b,
                                                    double* d_g_b, double* d_disp_a, double* d_disp_b) {
    if (!c || !a || !b) return fail(LCHD_EVALUE, "null argument");
    if (int rc = sens_args(c, a->n, width)) return rc;
    if (a->n > 0 && (!d_scores || !d_count_a || !d_idx_a || !d_dist_a || !d_g_a || !d_count_b || !d_idx_b || !d_dist_b || !d_g_b || !d_disp_a ||
                     !d_disp_b))
        return fail(LCHD_EVALUE, "null output pointer");
    if (a->images || b->images) return fail(LCHD_EUNSUPPORTED, "a sensitivity call takes the structures themselves, not periodic image clouds");
    SensitivityOut o{d_scores, d_count_a, d_count_b, d_idx_a, d_idx_b, d_dist_a, d_dist_b, d_g_a, d_g_b};
    o.disp_a = d_disp_a; o.disp_b = d_disp_b;
    lchd_cloud* const cl[2] = {a, b};
    const double* const cells[2] = {cell_a, cell_b};
    return consumer_coords_dev(c, cl, d_wf_index, cells, sensitivity_consumer(width, o, kSensMinImage), d_scores);
}
extern "C" int lchd_sensitivity_coords_periodic(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b,
                                                int64_t len_seq_b, const double* xyz_a, const double* xyz_b, int64_t n, const int32_t* wf_index,
                                                const double* cell_a, const double* cell_b, int32_t width, double* scores, int32_t* count_a,
                                                int32_t* idx_a, double* dist_a, double* g_a, int32_t* count_b, int32_t* idx_b, double* dist_b,
                                                double* g_b, double* disp_a, double* disp_b) {
    if (int rc = coords_lengths(xyz_a, n, xyz_b, n)) return rc;
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    if (int rc = sens_args(c, n, width)) return rc;
    if (n > 0 && (!scores || !count_a || !idx_a || !dist_a || !g_a || !count_b || !idx_b || !dist_b || !g_b || !disp_a || !disp_b))
        return fail(LCHD_EVALUE, "null output pointer");
    SensitivityOut o{scores, count_a, count_b, idx_a, idx_b, dist_a, dist_b, g_a, g_b};
    o.disp_a = disp_a; o.disp_b = disp_b;
    return sens_host_call(n, width, kSensMinImage, o, [&](double* blk, int resolve) {
        return pair_dense_host(c, cfg, seq_a, len_seq_a, seq_b, len_seq_b, xyz_a, xyz_b, nullptr, nullptr, n, n, n, wf_index, cell_a, cell_b,
                               sensitivity_consumer(width, SensitivityOut{}, resolve), blk);
    });
}
extern "C" int lchd_sensitivity_dmxs(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b,
                                     int64_t len_seq_b, const double* dmx_a, const double* dmx_b, int64_t rows, int64_t cols_a, int64_t cols_b,
                                     const int32_t* wf_index, int32_t width, double* scores, int32_t* count_a, int32_t* idx_a, double* dist_a,
                                     double* g_a, int32_t* count_b, int32_t* idx_b, double* dist_b, double* g_b) {
    if (rows > 0 && (!dmx_a || !dmx_b)) return fail(LCHD_EVALUE, "null pointer");
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    if (int rc = sens_args(c, rows, width)) return rc;
    if (rows > 0 && (!scores || !count_a || !idx_a || !dist_a || !g_a || !count_b || !idx_b || !dist_b || !g_b))
        return fail(LCHD_EVALUE, "null output pointer");
    const SensitivityOut o{scores, count_a, count_b, idx_a, idx_b, dist_a, dist_b, g_a, g_b};
    return sens_host_call(rows, width, kSensPlain, o, [&](double* blk, int resolve) {
        return pair_dense_host(c, cfg, seq_a, len_seq_a, seq_b, len_seq_b, nullptr, nullptr, dmx_a, dmx_b, rows, cols_a, cols_b, wf_index, nullptr,
                               nullptr, sensitivity_consumer(width, SensitivityOut{}, resolve), blk);
    });
}

// weight-function gradients: the sensitivity calls of the same name with the sixth consumer -- the same plan, list builders and record
// pass, no row width from the caller (the lists are as wide as the pass needs), k_weight_gradient (lchd_weight_gradient.hip) behind them.
// out: ONE block, scores[P] | grad[P][NP], NP = the most parameters of any weight function of the configuration
// (lchd_weight_gradient_width once the context holds it).  Open structures only.
extern "C" int32_t lchd_weight_gradient_width(lchd_ctx* c) { return c && c->cfg_set ? c->wf_np_max : 0; }
static const char* const kWgradOpen = "a weight-function gradient takes the structures themselves, not periodic image clouds";
extern "C" int lchd_weight_gradient_primitives_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int64_t* d_anchors, const int32_t* d_wf_index,
                                                   int64_t n_pairs, double thr, double* d_out) {
    if (!c || !a || !b) return fail(LCHD_EVALUE, "null argument");
    if (n_pairs > 0 && !d_out) return fail(LCHD_EVALUE, "null output pointer");
    if (a->images || b->images) return fail(LCHD_EUNSUPPORTED, "%s", kWgradOpen);
    lchd_cloud* const cl[2] = {a, b};
    return consumer_primitives_dev(c, cl, d_anchors, d_wf_index, n_pairs, thr, weight_gradient_consumer(), d_out);
}
extern "C" int lchd_weight_gradient_primitives(lchd_ctx* c, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a, const int32_t* tag_a,
                                               int64_t n_a, const double* xyz_b, const int32_t* cat_b, const int32_t* tag_b, int64_t n_b,
                                               const int64_t* anchors, const int32_t* wf_index, int64_t n_pairs, double thr, double* out) {
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    if (n_pairs > 0 && !out) return fail(LCHD_EVALUE, "null output pointer");
    return pair_primitives_host(c, cfg, xyz_a, cat_a, tag_a, n_a, xyz_b, cat_b, tag_b, n_b, anchors, wf_index, n_pairs, thr, nullptr, nullptr,
                                nullptr, nullptr, weight_gradient_consumer(), out);
}
extern "C" int lchd_weight_gradient_coords_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int32_t* d_wf_index, double* d_out) {
    if (!c || !a || !b) return fail(LCHD_EVALUE, "null argument");
    if (a->n > 0 && !d_out) return fail(LCHD_EVALUE, "null output pointer");
    if (a->images || b->images) return fail(LCHD_EUNSUPPORTED, "%s", kWgradOpen);
    lchd_cloud* const cl[2] = {a, b};
    const double* const cells[2] = {nullptr, nullptr};
    return consumer_coords_dev(c, cl, d_wf_index, cells, weight_gradient_consumer(), d_out);
}
extern "C" int lchd_weight_gradient_coords(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b,
                                           int64_t len_seq_b, const double* xyz_a, const double* xyz_b, int64_t n, const int32_t* wf_index,
                                           double* out) {
    if (int rc = coords_lengths(xyz_a, n, xyz_b, n)) return rc;
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    if (n > 0 && !out) return fail(LCHD_EVALUE, "null output pointer");
    return pair_dense_host(c, cfg, seq_a, len_seq_a, seq_b, len_seq_b, xyz_a, xyz_b, nullptr, nullptr, n, n, n, wf_index, nullptr, nullptr,
                           weight_gradient_consumer(), out);
}
extern "C" int lchd_weight_gradient_dmxs(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b,
                                         int64_t len_seq_b, const double* dmx_a, const double* dmx_b, int64_t rows, int64_t cols_a, int64_t cols_b,
                                         const int32_t* wf_index, double* out) {
    if (rows > 0 && (!dmx_a || !dmx_b)) return fail(LCHD_EVALUE, "null pointer");
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    if (rows > 0 && !out) return fail(LCHD_EVALUE, "null output pointer");
    return pair_dense_host(c, cfg, seq_a, len_seq_a, seq_b, len_seq_b, nullptr, nullptr, dmx_a, dmx_b, rows, cols_a, cols_b, wf_index, nullptr,
                           nullptr, weight_gradient_consumer(), out);
}

// ------------------------------------------------------------------------------------------------
// cross-scoring: all anchors of one list against all anchors of another, in row tiles (include/loco_hd_hip.h, "cross-scoring")
// ------------------------------------------------------------------------------------------------
// A tile is tile_rows anchors of A against all of B: k_cross_pairs (lchd_cross.hip) writes its pair records into the context's cross
// block, lchd_from_primitives_dev scores them as it scores any list -- the context is held by this call, the owner re-enters -- and a
// nearest call reduces the tile's scores with k_nearest_rows.  Side B's environments are built again for every tile (about 0.16 ms per
// 10^4 anchors, against several ms of sweep for a tile of 5 10^6 pairs): no store outlives a pass.
extern "C" int lchd_cross_plan(int64_t n_a, int64_t n_b, int64_t budget_bytes, int64_t* tile_rows_out) {
    if (!tile_rows_out) return fail(LCHD_EVALUE, "null output pointer");
    *tile_rows_out = 0;
    if (n_a < 1 || n_b < 1 || budget_bytes < 0)
        return fail(LCHD_EVALUE, "a cross-scoring plan takes n_a >= 1, n_b >= 1 and a budget >= 0 (got %lld, %lld, %lld)", (long long)n_a,
                    (long long)n_b, (long long)budget_bytes);
    const int64_t rows = cross_plan_rows(n_a, n_b, budget_bytes);
    if (rows < 1) {
        if (n_b > kCrossMaxTilePairs)
            return fail(LCHD_EUNSUPPORTED, "one row of %lld anchor pairs exceeds the 2^31 - 1 pairs of a pass: split anchors_b", (long long)n_b);
        return fail(LCHD_EUNSUPPORTED, "one row of %lld anchor pairs takes %lld bytes of pair records, indices and scores; the budget is %lld",
                    (long long)n_b, (long long)(n_b * kCrossPairBytes), (long long)budget_bytes);
    }
    *tile_rows_out = rows;
    return LCHD_OK;
}

struct CrossRequest {
    lchd_cloud *a, *b;
    const int64_t *anchors_a, *anchors_b;  // DEVICE
    int64_t n_a, n_b;
    int32_t wf;          // -1: none
    double thr;
    int64_t tile_rows;   // 0: lchd_cross_plan
    int32_t k;           // 0: the cross form (the nearest entry points refuse a k < 1 before they get here)
    double* out;        // DEVICE: cross [n_a][n_b] / nearest scores [n_a][k]
    int32_t* cols;       // DEVICE: nearest [n_a][k]
};
// what needs no context: k and tile_rows against the list lengths
static int cross_args(int64_t n_a, int64_t n_b, int64_t tile_rows, bool nearest, int32_t k) {
    if (n_a < 0 || n_b < 0) return fail(LCHD_EVALUE, "negative anchor count");
    if (nearest && (k < 1 || k > kNearestMaxK || k > n_b))
        return fail(LCHD_EVALUE, "k = %d is outside 1 .. min(n_b, %d) with n_b = %lld", k, kNearestMaxK, (long long)n_b);
    if (tile_rows < 0) return fail(LCHD_EVALUE, "tile_rows = %lld is negative (0: planned from the free device memory)", (long long)tile_rows);
    if (tile_rows > 0 && n_b > 0 && std::min(tile_rows, std::max<int64_t>(n_a, 1)) > kCrossMaxTilePairs / n_b)
        return fail(LCHD_EVALUE, "tile_rows = %lld with n_b = %lld is a tile of more than 2^31 - 1 pairs", (long long)tile_rows, (long long)n_b);
    return LCHD_OK;
}
static int cross_core(lchd_ctx* c, const CrossRequest& R) {
    if (!c || !R.a || !R.b) return fail(LCHD_EVALUE, "null argument");
    if (int rc = cross_args(R.n_a, R.n_b, R.tile_rows, R.k != 0, R.k)) return rc;
    if (!c->cfg_set) return fail(LCHD_EVALUE, "lchd_ctx_set_config has not been called");
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    if (R.wf < -1 || R.wf >= c->h_cfg.n_wf) return fail(LCHD_EVALUE, "weight-function index %d out of range (-1: none)", R.wf);
    if (R.n_a == 0 || R.n_b == 0) return LCHD_OK;
    if (!R.anchors_a || !R.anchors_b || !R.out || (R.k && !R.cols)) return fail(LCHD_EVALUE, "null anchor / output pointer");
    CTX_GUARD(c);
    int64_t rows = std::min(R.tile_rows, R.n_a);
    if (R.tile_rows == 0) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        // (the pass itself takes about as much per pair in its arena, next to the environment stores)
        if (int rc = lchd_cross_plan(R.n_a, R.n_b, (int64_t)(std::min<size_t>(free_b, (size_t)1 << 62) / 4), &rows)) return rc;
    }
    const size_t tile_pairs = (size_t)rows * (size_t)R.n_b;
    const size_t o_wf = 16 * tile_pairs, o_sc = (o_wf + 4 * tile_pairs + 255) & ~size_t(255);
    if (int rc = grow_block(c->d_cross, c->cross_cap, o_sc + (R.k ? 8 * tile_pairs : 0))) return rc;
    int64_t* d_pairs = reinterpret_cast<int64_t*>(c->d_cross);
    int32_t* d_wf = reinterpret_cast<int32_t*>(c->d_cross + o_wf);
    double* d_tile = reinterpret_cast<double*>(c->d_cross + o_sc);
    hipStream_t s = c->stream;
    for (int64_t r0 = 0; r0 < R.n_a; r0 += rows) {
        const int64_t tr = std::min(rows, R.n_a - r0);
        launch_cross_pairs(s, R.anchors_a, R.anchors_b, r0, tr, R.n_b, R.wf, d_pairs, d_wf);
        HIP_TRY(hipGetLastError());
        double* scores = R.k ? d_tile : R.out + (size_t)r0 * (size_t)R.n_b;  // (the cross form: the tile's scores go to their place)
        if (int rc = lchd_from_primitives_dev(c, R.a, R.b, d_pairs, R.wf >= 0 ? d_wf : nullptr, tr * R.n_b, R.thr, scores)) return rc;
        if (R.k) {
            launch_nearest_rows(s, d_tile, tr, R.n_b, R.k, R.out + (size_t)r0 * (size_t)R.k, R.cols + (size_t)r0 * (size_t)R.k);
            HIP_TRY(hipGetLastError());
        }
    }
    if (R.k) HIP_TRY(hipStreamSynchronize(s));  // the call returns with the outputs complete, as the scoring call does
    c->last_valid = false;  // (the anchors of the last pass live in the cross block, which the next cross call overwrites)
    return LCHD_OK;
}
extern "C" int lchd_cross_primitives_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int64_t* d_anchors_a, int64_t n_a,
                                         const int64_t* d_anchors_b, int64_t n_b, int32_t wf_index, double thr, int64_t tile_rows, double* d_out) {
    CTX_LOCK(c);
    return cross_core(c, CrossRequest{a, b, d_anchors_a, d_anchors_b, n_a, n_b, wf_index, thr, tile_rows, 0, d_out, nullptr});
}
extern "C" int lchd_nearest_primitives_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int64_t* d_anchors_a, int64_t n_a,
                                           const int64_t* d_anchors_b, int64_t n_b, int32_t wf_index, double thr, int64_t tile_rows, int32_t k,
                                           double* d_scores, int32_t* d_cols) {
    CTX_LOCK(c);
    if (int rc = cross_args(n_a, n_b, tile_rows, true, k)) return rc;
    return cross_core(c, CrossRequest{a, b, d_anchors_a, d_anchors_b, n_a, n_b, wf_index, thr, tile_rows, k, d_scores, d_cols});
}
// The host-array forms: both structures as temporary clouds, the anchors and the outputs in one temporary device block.  k == 0: cross.
static int cross_host(lchd_ctx* c, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a, const int32_t* tag_a, int64_t n_atoms_a,
                      const double* xyz_b, const int32_t* cat_b, const int32_t* tag_b, int64_t n_atoms_b, const int64_t* anchors_a, int64_t n_a,
                      const int64_t* anchors_b, int64_t n_b, int32_t wf_index, double thr, int64_t tile_rows, int32_t k, double* out,
                      int32_t* cols) {
    CTX_LOCK(c);
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    if (int rc = cross_args(n_a, n_b, tile_rows, k != 0, k)) return rc;
    if (wf_index < -1 || wf_index >= cfg->n_weight_functions) return fail(LCHD_EVALUE, "weight-function index %d out of range (-1: none)", wf_index);
    if (n_atoms_a < 0 || n_atoms_b < 0 || n_atoms_a > ((int64_t)1 << 30) || n_atoms_b > ((int64_t)1 << 30))
        return fail(LCHD_EUNSUPPORTED, "structure size out of range");
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    CTX_GUARD(c);
    if (int rc = lchd_ctx_set_config(c, cfg)) return rc;
    if (n_a == 0 || n_b == 0) return LCHD_OK;
    if (!anchors_a || !anchors_b || !out || (k && !cols)) return fail(LCHD_EVALUE, "null anchor / output pointer");
    const size_t width = k ? (size_t)k : (size_t)n_b;
    if ((size_t)n_a > ((size_t)1 << 40) / width) return fail(LCHD_EUNSUPPORTED, "%lld x %zu outputs exceed 8 TiB: split anchors_a", (long long)n_a, width);
    HostTemps t(c);
    const size_t o_b = 8 * (size_t)n_a, o_out = (o_b + 8 * (size_t)n_b + 255) & ~size_t(255), n_out = (size_t)n_a * width,
                 o_cols = o_out + 8 * n_out;
    auto run = [&]() -> int {
        if (int rc = lchd_cloud_create(c, xyz_a, cat_a, tag_a, n_atoms_a, &t.clouds[0])) return rc;
        if (int rc = lchd_cloud_create(c, xyz_b, cat_b, tag_b, n_atoms_b, &t.clouds[1])) return rc;
        if (hipMalloc(&t.d_blk, o_cols + (k ? 4 * n_out : 0)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(LCHD_EUNSUPPORTED, "no device memory for the %zu outputs of this call: split anchors_a", n_out);
        }
        HIP_TRY(hipMemcpy(t.d_blk, anchors_a, 8 * (size_t)n_a, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(t.d_blk + o_b, anchors_b, 8 * (size_t)n_b, hipMemcpyHostToDevice));
        const CrossRequest R{t.clouds[0], t.clouds[1], reinterpret_cast<const int64_t*>(t.d_blk), reinterpret_cast<const int64_t*>(t.d_blk + o_b),
                             n_a, n_b, wf_index, thr, tile_rows, k, reinterpret_cast<double*>(t.d_blk + o_out),
                             k ? reinterpret_cast<int32_t*>(t.d_blk + o_cols) : nullptr};
        if (int rc = cross_core(c, R)) return rc;
        HIP_TRY(hipMemcpy(out, t.d_blk + o_out, 8 * n_out, hipMemcpyDeviceToHost));
        if (k) HIP_TRY(hipMemcpy(cols, t.d_blk + o_cols, 4 * n_out, hipMemcpyDeviceToHost));
        return LCHD_OK;
    };
    t.rc = run();
    c->last_valid = false;  // the clouds of this call go away (`t` destroys them on return)
    c->pend.req.a = c->pend.req.b = nullptr;
    return t.rc;
}
extern "C" int lchd_cross_primitives(lchd_ctx* c, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a, const int32_t* tag_a,
                                     int64_t n_atoms_a, const double* xyz_b, const int32_t* cat_b, const int32_t* tag_b, int64_t n_atoms_b,
                                     const int64_t* anchors_a, int64_t n_a, const int64_t* anchors_b, int64_t n_b, int32_t wf_index, double thr,
                                     int64_t tile_rows, double* out) {
    return cross_host(c, cfg, xyz_a, cat_a, tag_a, n_atoms_a, xyz_b, cat_b, tag_b, n_atoms_b, anchors_a, n_a, anchors_b, n_b, wf_index, thr,
                      tile_rows, 0, out, nullptr);
}
extern "C" int lchd_nearest_primitives(lchd_ctx* c, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a, const int32_t* tag_a,
                                       int64_t n_atoms_a, const double* xyz_b, const int32_t* cat_b, const int32_t* tag_b, int64_t n_atoms_b,
                                       const int64_t* anchors_a, int64_t n_a, const int64_t* anchors_b, int64_t n_b, int32_t wf_index, double thr,
                                       int64_t tile_rows, int32_t k, double* scores, int32_t* cols) {
    if (int rc = cross_args(n_a, n_b, tile_rows, true, k)) return rc;
    return cross_host(c, cfg, xyz_a, cat_a, tag_a, n_atoms_a, xyz_b, cat_b, tag_b, n_atoms_b, anchors_a, n_a, anchors_b, n_b, wf_index, thr,
                      tile_rows, k, scores, cols);
}

// ------------------------------------------------------------------------------------------------
// native coordinate gradients: the sensitivity lists reduced on the device (include/loco_hd_hip.h, "native coordinate gradients")
// ------------------------------------------------------------------------------------------------
// A thresholded call walks its pair list in tiles.  Per tile the sensitivity pass (lchd_sensitivity_primitives_dev, unchanged: the
// context is held by this call, the owner re-enters) writes its lists into the context's gradient block -- the scores go straight to
// the caller's array -- and k_grad_accumulate (lchd_gradient.hip) adds them into the exact accumulators of lchd_exact_sum.h.  A tile
// is added only after its pass has succeeded: a pass that reports too small a width is repeated at lchd_sensitivity_needed_width first.
// The dense form is one tile of lchd_sensitivity_coords_dev with the row's atom as the anchor.  k_grad_finish rounds once at the end.
static int64_t grad_pair_bytes(int32_t width, int resolve = kSensPlain) { return 8 * (int64_t)sens_row(width, resolve); }  // plain: 40 width + 16
constexpr int64_t kGradMaxAdds = (int64_t)1 << 31;  // additions a limb takes without carry propagation (lchd_exact_sum.h)
static int64_t grad_plan_tile(int64_t n_pairs, int32_t width, int resolve, int64_t budget_bytes) {
    return std::max<int64_t>(1, std::min(budget_bytes / grad_pair_bytes(width, resolve), n_pairs));
}

extern "C" int lchd_gradient_plan(int64_t n_pairs, int32_t width, int64_t budget_bytes, int64_t* tile_pairs_out) {
    if (!tile_pairs_out) return fail(LCHD_EVALUE, "null output pointer");
    *tile_pairs_out = 0;
    if (n_pairs < 1 || width < 1 || width > kRadialMaxPoints || budget_bytes < 0)
        return fail(LCHD_EVALUE, "a gradient plan takes n_pairs >= 1, a width in 1 .. %d and a budget >= 0 (got %lld, %d, %lld)", kRadialMaxPoints,
                    (long long)n_pairs, width, (long long)budget_bytes);
    *tile_pairs_out = grad_plan_tile(n_pairs, width, kSensPlain, budget_bytes);
    return LCHD_OK;
}
// ... for the wider rows of the periodic forms (resolve: LCHD_GRAD_PLAIN / _IMAGES / _MIN_IMAGE), with the call's slot rule in front: what
// a periodic call of these pairs at this width would refuse is refused here, with the same words.
extern "C" int lchd_gradient_plan_periodic(int64_t n_pairs, int32_t width, int32_t resolve, int64_t budget_bytes, int64_t* tile_pairs_out) {
    if (!tile_pairs_out) return fail(LCHD_EVALUE, "null output pointer");
    *tile_pairs_out = 0;
    if (n_pairs < 1 || width < 1 || width > kRadialMaxPoints || budget_bytes < 0 || resolve < kSensPlain || resolve > kSensMinImage)
        return fail(LCHD_EVALUE, "a gradient plan takes n_pairs >= 1, a width in 1 .. %d, a resolve mode in 0 .. 2 and a budget >= 0 (got %lld, %d, %d, %lld)",
                    kRadialMaxPoints, (long long)n_pairs, width, resolve, (long long)budget_bytes);
    if (n_pairs >= (kGradMaxAdds + width - 1) / width)
        return fail(LCHD_EUNSUPPORTED, "%lld pairs with rows of %d slots exceed the 2^31 additions an exact accumulator takes: split the list",
                    (long long)n_pairs, width);
    *tile_pairs_out = grad_plan_tile(n_pairs, width, resolve, budget_bytes);
    return LCHD_OK;
}
extern "C" int64_t lchd_gradient_strain_waves(void) { return 4 * (int64_t)kStrainMaxBlocks; }

struct GradRequest {
    lchd_cloud *a, *b;
    const int64_t* anchors;   // DEVICE [n_pairs][2]; null: the dense form (pair r = row r, n_pairs = size(a))
    const int32_t* wf;        // DEVICE or null
    int64_t n_pairs;
    double thr;
    const double* weights;    // DEVICE [n_pairs] or null
    int64_t tile_pairs;       // 0: lchd_gradient_plan
    double *scores, *grad_a, *grad_b;  // DEVICE
    // the periodic forms: which sensitivity call fills a tile.  kSensPlain: the two open calls, coordinates read by the accumulation;
    // kSensImages: lchd_sensitivity_images_dev (thresholded; any cloud may be an image cloud, gradients per source atom);
    // kSensMinImage: lchd_sensitivity_coords_periodic_dev (dense) with `cell`.  The last two accumulate from the lists' disp.
    int resolve = kSensPlain;
    const double* cell[2] = {nullptr, nullptr};   // HOST [9] or null: an open side (kSensMinImage)
    double* strain[2] = {nullptr, nullptr};       // DEVICE [9] each, both or neither (a resolving form)
};
static int grad_core(lchd_ctx* c, const GradRequest& R) {
    if (!c || !R.a || !R.b) return fail(LCHD_EVALUE, "null argument");
    const bool dense = R.anchors == nullptr;
    const int resolve = R.resolve;
    if (R.tile_pairs < 0) return fail(LCHD_EVALUE, "tile_pairs = %lld is negative (0: planned from the free device memory)", (long long)R.tile_pairs);
    if (R.n_pairs < 0) return fail(LCHD_EVALUE, "negative pair count");
    if (!R.strain[0] != !R.strain[1]) return fail(LCHD_EVALUE, "one strain pointer is null and the other is not: a call writes both tensors or neither");
    const bool strain = R.strain[0] != nullptr;
    if (!c->cfg_set) return fail(LCHD_EVALUE, "lchd_ctx_set_config has not been called");
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    if (resolve == kSensPlain && (R.a->images || R.b->images))
        return fail(LCHD_EUNSUPPORTED, "a native gradient call takes the structures themselves, not periodic image clouds");
    if (dense && R.a->n != R.b->n)
        return fail(LCHD_EVALUE, "Expected matrices with the same length, got lengths %lld and %lld!", (long long)R.a->n, (long long)R.b->n);
    if (dense && (R.a->sid || R.b->sid)) return fail(LCHD_EVALUE, "from_coords takes single structures, not batches");
    if (strain && (R.a->sid || R.b->sid))
        return fail(LCHD_EUNSUPPORTED, "a strain derivative belongs to one box or cell: a batch of structures has many (ask for gradients alone, or score one structure per call)");
    // (an image cloud's lists name source atoms: one gradient row per source atom)
    const int64_t n_at[2] = {resolve == kSensImages ? lchd_cloud_home_size(R.a) : R.a->n, resolve == kSensImages ? lchd_cloud_home_size(R.b) : R.b->n};
    if ((n_at[0] > 0 && !R.grad_a) || (n_at[1] > 0 && !R.grad_b) || (R.n_pairs > 0 && !R.scores)) return fail(LCHD_EVALUE, "null output pointer");
    if (dense && R.n_pairs > kRadialMaxPoints)
        return fail(LCHD_EUNSUPPORTED, "a sensitivity call takes dense rows of at most %d points (got %lld / %lld)", kRadialMaxPoints, (long long)n_at[0],
                    (long long)n_at[1]);
    CTX_GUARD(c);
    hipStream_t s = c->stream;
    // the accumulators: [status word, 256 bytes] | side A [n_a][3][limbs] | side B | strain [2][6][limbs]; zero between calls (the finish
    // kernels leave them so)
    const size_t side_bytes[2] = {(size_t)n_at[0] * 3 * LCHD_GRAD_LIMBS * 8, (size_t)n_at[1] * 3 * LCHD_GRAD_LIMBS * 8};
    const size_t acc_bytes = 256 + side_bytes[0] + side_bytes[1] + 2 * LCHD_STRAIN_LIMBS * 8;
    const bool grown = acc_bytes > c->grad_acc_cap;
    if (grown) HIP_TRY(hipStreamSynchronize(s));
    if (int rc = grow_block(c->d_grad_acc, c->grad_acc_cap, acc_bytes)) return rc;
    if (grown || c->grad_acc_dirty) HIP_TRY(hipMemsetAsync(c->d_grad_acc, 0, c->grad_acc_cap, s));
    c->grad_acc_dirty = true;
    uint32_t* const d_flag = reinterpret_cast<uint32_t*>(c->d_grad_acc);
    int64_t* const acc[2] = {reinterpret_cast<int64_t*>(c->d_grad_acc + 256), reinterpret_cast<int64_t*>(c->d_grad_acc + 256 + side_bytes[0])};
    int64_t* const strain_acc = reinterpret_cast<int64_t*>(c->d_grad_acc + 256 + side_bytes[0] + side_bytes[1]);

    int32_t width = dense ? (int32_t)std::max<int64_t>(R.n_pairs, 1) : std::min(std::max(128, c->grad_width), kRadialMaxPoints);
    int64_t tile = dense ? R.n_pairs : std::min(R.tile_pairs, R.n_pairs);
    const bool planned = !dense && R.tile_pairs == 0 && R.n_pairs > 0;
    size_t budget = 0;
    if (planned) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        budget = std::min<size_t>(free_b, (size_t)1 << 62) / 4;  // (the pass itself takes its stores and arena next to the lists)
        tile = grad_plan_tile(R.n_pairs, width, resolve, (int64_t)budget);
    }
    int64_t adds = 0;  // slots per side handed to the accumulation so far: what one accumulator's limbs can have received at the most
    for (int64_t p0 = 0; p0 < R.n_pairs;) {
        const int64_t tp = std::min(tile, R.n_pairs - p0);
        // (a dense row adds to its atoms once per row, far below the limit; the strain sums take every slot of the call)
        if ((!dense || strain) && adds + tp * (int64_t)width >= kGradMaxAdds)
            return fail(LCHD_EUNSUPPORTED, "%lld pairs with rows of %d slots exceed the 2^31 additions an exact accumulator takes: split the list",
                        (long long)R.n_pairs, width);
        const size_t lists = (size_t)tp * (size_t)grad_pair_bytes(width, resolve);
        if (lists > c->grad_cap) HIP_TRY(hipStreamSynchronize(s));  // (the block about to be freed may still be read)
        if (int rc = grow_block(c->d_grad, c->grad_cap, lists)) return rc;
        SensitivityOut o = sens_carve(reinterpret_cast<double*>(c->d_grad), tp, width, resolve);
        o.scores = R.scores + p0;
        const int32_t* wf = R.wf ? R.wf + p0 : nullptr;
        int rc;
        if (resolve == kSensImages)
            rc = lchd_sensitivity_images_dev(c, R.a, R.b, R.anchors + 2 * p0, wf, tp, R.thr, width, o.scores, o.count_a, o.idx_a, o.image_a, o.dist_a,
                                             o.g_a, o.disp_a, o.count_b, o.idx_b, o.image_b, o.dist_b, o.g_b, o.disp_b);
        else if (resolve == kSensMinImage)
            rc = lchd_sensitivity_coords_periodic_dev(c, R.a, R.b, wf, R.cell[0], R.cell[1], width, o.scores, o.count_a, o.idx_a, o.dist_a, o.g_a,
                                                      o.count_b, o.idx_b, o.dist_b, o.g_b, o.disp_a, o.disp_b);
        else if (dense)
            rc = lchd_sensitivity_coords_dev(c, R.a, R.b, wf, width, o.scores, o.count_a, o.idx_a, o.dist_a, o.g_a, o.count_b, o.idx_b, o.dist_b, o.g_b);
        else
            rc = lchd_sensitivity_primitives_dev(c, R.a, R.b, R.anchors + 2 * p0, wf, tp, R.thr, width, o.scores, o.count_a, o.idx_a, o.dist_a, o.g_a,
                                                 o.count_b, o.idx_b, o.dist_b, o.g_b);
        if (rc == LCHD_EVALUE && !dense && c->sens_needed > width) {  // too narrow: nothing of this tile has been added; once more, wider
            width = (int32_t)c->sens_needed;
            if (planned) tile = std::min(tile, grad_plan_tile(R.n_pairs, width, resolve, (int64_t)budget));
            continue;
        }
        if (rc) return rc;
        GradAccumArgs ga{};
        const lchd_cloud* const cl[2] = {R.a, R.b};
        for (int k = 0; k < 2; ++k) {
            GradSide& S = ga.s[k];
            S.idx = k ? o.idx_b : o.idx_a; S.dist = k ? o.dist_b : o.dist_a; S.g = k ? o.g_b : o.g_a;
            S.disp = k ? o.disp_b : o.disp_a;  // (null in the plain layout)
            S.x = cl[k]->x; S.y = cl[k]->y; S.z = cl[k]->z;
            S.n = n_at[k];
            S.acc = acc[k];
        }
        ga.weights = R.weights ? R.weights + p0 : nullptr;
        ga.n_pairs = tp;
        ga.width = width;
        ga.dense = dense ? 1 : 0;
        ga.flag = d_flag;
        if (!launch_grad_accumulate(s, ga)) return fail(LCHD_EDEVICE, "the gradient accumulation kernel rejected its launch configuration");
        if (strain && !launch_strain_accumulate(s, ga, strain_acc))
            return fail(LCHD_EDEVICE, "the strain accumulation kernel rejected its launch configuration");
        HIP_TRY(hipGetLastError());
        adds += tp * (int64_t)width;
        p0 += tp;
    }
    if (!dense) c->grad_width = width;
    if (!launch_grad_finish(s, acc[0], n_at[0], R.grad_a) || !launch_grad_finish(s, acc[1], n_at[1], R.grad_b) ||
        (strain && !launch_strain_finish(s, strain_acc, R.strain[0], R.strain[1])))
        return fail(LCHD_EDEVICE, "the gradient finish kernel rejected its launch configuration");
    HIP_TRY(hipGetLastError());
    uint32_t flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));  // the call returns with the outputs complete, as the sensitivity call does
    if (flag) HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof flag, s));
    c->grad_acc_dirty = false;
    if (flag) return fail(LCHD_EVALUE, "gradient contribution not finite or >= 2^63 (pair weights?)");
    return LCHD_OK;
}

extern "C" int lchd_gradient_primitives_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int64_t* d_anchors, const int32_t* d_wf_index,
                                            int64_t n_pairs, double thr, const double* d_pair_weights, int64_t tile_pairs, double* d_scores,
                                            double* d_grad_a, double* d_grad_b) {
    CTX_LOCK(c);
    if (n_pairs > 0 && !d_anchors) return fail(LCHD_EVALUE, "null anchor / output pointer");
    static const int64_t no_pairs[2] = {0, 0};  // (a non-null list marks the thresholded form; with no pairs it is never read)
    return grad_core(c, GradRequest{a, b, d_anchors ? d_anchors : no_pairs, d_wf_index, n_pairs, thr, d_pair_weights, tile_pairs, d_scores, d_grad_a,
                                    d_grad_b});
}
extern "C" int lchd_gradient_coords_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int32_t* d_wf_index, const double* d_pair_weights,
                                        double* d_scores, double* d_grad_a, double* d_grad_b) {
    CTX_LOCK(c);
    if (!c || !a || !b) return fail(LCHD_EVALUE, "null argument");
    return grad_core(c, GradRequest{a, b, nullptr, d_wf_index, a->n, 0.0, d_pair_weights, 0, d_scores, d_grad_a, d_grad_b});
}
// ... under periodic boundaries: the same tile loop on the lists of lchd_sensitivity_images_dev / lchd_sensitivity_coords_periodic_dev,
// accumulated from their displacements; with the strain tensors requested, k_strain_accumulate behind every tile's accumulation.
extern "C" int lchd_gradient_images_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int64_t* d_anchors, const int32_t* d_wf_index,
                                        int64_t n_pairs, double thr, const double* d_pair_weights, int64_t tile_pairs, double* d_scores,
                                        double* d_grad_a, double* d_grad_b, double* d_strain_a, double* d_strain_b) {
    CTX_LOCK(c);
    if (tile_pairs < 0) return fail(LCHD_EVALUE, "tile_pairs = %lld is negative (0: planned from the free device memory)", (long long)tile_pairs);
    if (!d_strain_a != !d_strain_b) return fail(LCHD_EVALUE, "one strain pointer is null and the other is not: a call writes both tensors or neither");
    if (!c || !a || !b) return fail(LCHD_EVALUE, "null argument");
    if (n_pairs > 0 && !d_anchors) return fail(LCHD_EVALUE, "null anchor / output pointer");
    static const int64_t no_pairs[2] = {0, 0};
    GradRequest R{a, b, d_anchors ? d_anchors : no_pairs, d_wf_index, n_pairs, thr, d_pair_weights, tile_pairs, d_scores, d_grad_a, d_grad_b};
    R.resolve = kSensImages;
    R.strain[0] = d_strain_a; R.strain[1] = d_strain_b;
    return grad_core(c, R);
}
extern "C" int lchd_gradient_coords_periodic_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int32_t* d_wf_index, const double* cell_a,
                                                 const double* cell_b, const double* d_pair_weights, double* d_scores, double* d_grad_a,
                                                 double* d_grad_b, double* d_strain_a, double* d_strain_b) {
    CTX_LOCK(c);
    if (!d_strain_a != !d_strain_b) return fail(LCHD_EVALUE, "one strain pointer is null and the other is not: a call writes both tensors or neither");
    if (!c || !a || !b) return fail(LCHD_EVALUE, "null argument");
    GradRequest R{a, b, nullptr, d_wf_index, a->n, 0.0, d_pair_weights, 0, d_scores, d_grad_a, d_grad_b};
    R.resolve = kSensMinImage;
    R.cell[0] = cell_a; R.cell[1] = cell_b;
    R.strain[0] = d_strain_a; R.strain[1] = d_strain_b;
    return grad_core(c, R);
}

// The host-array forms: both structures as temporary clouds; the list, the weights and the three outputs in one temporary device block.
struct GradHostArrays {
    const int64_t* anchors;   // null: the dense form
    const int32_t* wf;
    const double* weights;
    int64_t n_pairs, n_a, n_b;
    double thr;
    int64_t tile_pairs;
    double *scores, *grad_a, *grad_b;
    int resolve = kSensPlain;                    // as GradRequest
    const double* cell[2] = {nullptr, nullptr};
    double* strain[2] = {nullptr, nullptr};      // HOST [9] each, both or neither
};
static int grad_host(lchd_ctx* c, HostTemps& t, const GradHostArrays& H) {
    const size_t P = (size_t)H.n_pairs, na = (size_t)H.n_a, nb = (size_t)H.n_b;
    auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
    const size_t o_wf = up(H.anchors ? 16 * P : 0), o_w = up(o_wf + (H.wf ? 4 * P : 0)), o_sc = up(o_w + (H.weights ? 8 * P : 0)),
                 o_ga = up(o_sc + 8 * P), o_gb = up(o_ga + 24 * na), o_st = up(o_gb + 24 * nb), total = o_st + 2 * 72;
    if (!H.strain[0] != !H.strain[1]) return fail(LCHD_EVALUE, "one strain pointer is null and the other is not: a call writes both tensors or neither");
    if (hipMalloc(&t.d_blk, total ? total : 256) != hipSuccess) {
        (void)hipGetLastError();
        return fail(LCHD_EUNSUPPORTED, "no device memory for the %zu bytes of lists and outputs of this call", total);
    }
    if (H.anchors && P) HIP_TRY(hipMemcpy(t.d_blk, H.anchors, 16 * P, hipMemcpyHostToDevice));
    if (H.wf && P) HIP_TRY(hipMemcpy(t.d_blk + o_wf, H.wf, 4 * P, hipMemcpyHostToDevice));
    if (H.weights && P) HIP_TRY(hipMemcpy(t.d_blk + o_w, H.weights, 8 * P, hipMemcpyHostToDevice));
    static const int64_t no_pairs[2] = {0, 0};
    GradRequest R{t.clouds[0], t.clouds[1],
                        H.anchors ? (P ? reinterpret_cast<const int64_t*>(t.d_blk) : no_pairs) : nullptr,
                        H.wf ? reinterpret_cast<const int32_t*>(t.d_blk + o_wf) : nullptr, H.n_pairs, H.thr,
                        H.weights ? reinterpret_cast<const double*>(t.d_blk + o_w) : nullptr, H.tile_pairs,
                        reinterpret_cast<double*>(t.d_blk + o_sc), reinterpret_cast<double*>(t.d_blk + o_ga), reinterpret_cast<double*>(t.d_blk + o_gb)};
    R.resolve = H.resolve;
    for (int k = 0; k < 2; ++k) {
        R.cell[k] = H.cell[k];
        if (H.strain[k]) R.strain[k] = reinterpret_cast<double*>(t.d_blk + o_st + 72 * (size_t)k);
    }
    const int rc = grad_core(c, R);
    // (an out-of-range contribution fails the call behind complete outputs: the scores are valid and go back)
    const bool range = rc == LCHD_EVALUE && strstr(g_err, "gradient contribution") != nullptr;
    if (rc == LCHD_OK || range) {
        const std::string msg = g_err;
        if (P) HIP_TRY(hipMemcpy(H.scores, t.d_blk + o_sc, 8 * P, hipMemcpyDeviceToHost));
        if (na) HIP_TRY(hipMemcpy(H.grad_a, t.d_blk + o_ga, 24 * na, hipMemcpyDeviceToHost));
        if (nb) HIP_TRY(hipMemcpy(H.grad_b, t.d_blk + o_gb, 24 * nb, hipMemcpyDeviceToHost));
        for (int k = 0; k < 2; ++k)
            if (H.strain[k]) HIP_TRY(hipMemcpy(H.strain[k], t.d_blk + o_st + 72 * (size_t)k, 72, hipMemcpyDeviceToHost));
        if (rc) snprintf(g_err, sizeof g_err, "%s", msg.c_str());
    }
    return rc;
}

extern "C" int lchd_gradient_primitives(lchd_ctx* c, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a, const int32_t* tag_a,
                                        int64_t n_a, const double* xyz_b, const int32_t* cat_b, const int32_t* tag_b, int64_t n_b,
                                        const int64_t* anchors, const int32_t* wf_index, int64_t n_pairs, double thr, const double* pair_weights,
                                        int64_t tile_pairs, double* scores, double* grad_a, double* grad_b) {
    CTX_LOCK(c);
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    if (tile_pairs < 0) return fail(LCHD_EVALUE, "tile_pairs = %lld is negative (0: planned from the free device memory)", (long long)tile_pairs);
    if (n_pairs < 0) return fail(LCHD_EVALUE, "negative pair count");
    if (int rc = check_wf_index(cfg, wf_index, n_pairs)) return rc;
    if (n_a < 0 || n_b < 0 || n_a > ((int64_t)1 << 27) || n_b > ((int64_t)1 << 27)) return fail(LCHD_EUNSUPPORTED, "structure size out of range");
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    if ((n_pairs > 0 && (!anchors || !scores)) || (n_a > 0 && !grad_a) || (n_b > 0 && !grad_b)) return fail(LCHD_EVALUE, "null anchor / output pointer");
    CTX_GUARD(c);
    if (int rc = lchd_ctx_set_config(c, cfg)) return rc;
    static const int64_t no_pairs[2] = {0, 0};
    HostTemps t(c);
    auto run = [&]() -> int {
        if (int rc = lchd_cloud_create(c, xyz_a, cat_a, tag_a, n_a, &t.clouds[0])) return rc;
        if (int rc = lchd_cloud_create(c, xyz_b, cat_b, tag_b, n_b, &t.clouds[1])) return rc;
        return grad_host(c, t, GradHostArrays{anchors ? anchors : no_pairs, wf_index, pair_weights, n_pairs, n_a, n_b, thr, tile_pairs, scores, grad_a, grad_b});
    };
    t.rc = run();
    c->last_valid = false;  // the clouds of this call go away (`t` destroys them on return)
    c->pend.req.a = c->pend.req.b = nullptr;
    return t.rc;
}
extern "C" int lchd_gradient_coords(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b,
                                    int64_t len_seq_b, const double* xyz_a, const double* xyz_b, int64_t n, const int32_t* wf_index,
                                    const double* pair_weights, double* scores, double* grad_a, double* grad_b) {
    CTX_LOCK(c);
    if (n < 0) return fail(LCHD_EVALUE, "negative structure size");
    if (int rc = coords_lengths(xyz_a, n, xyz_b, n)) return rc;
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    CTX_GUARD(c);
    if (int rc = lchd_ctx_set_config(c, cfg)) return rc;
    if (int rc = check_wf_index(cfg, wf_index, n)) return rc;
    if (n == 0) return LCHD_OK;
    if (n > len_seq_a || n > len_seq_b) return fail(LCHD_EPANIC, "index out of bounds: a distance row is longer than its seq");
    if (!seq_a || !seq_b || !scores || !grad_a || !grad_b) return fail(LCHD_EVALUE, "null pointer");
    HostTemps t(c);
    auto run = [&]() -> int {
        if (int rc = lchd_cloud_create(c, xyz_a, seq_a, nullptr, n, &t.clouds[0])) return rc;
        if (int rc = lchd_cloud_create(c, xyz_b, seq_b, nullptr, n, &t.clouds[1])) return rc;
        return grad_host(c, t, GradHostArrays{nullptr, wf_index, pair_weights, n, n, n, 0.0, 0, scores, grad_a, grad_b});
    };
    t.rc = run();
    c->last_valid = false;
    c->pend.req.a = c->pend.req.b = nullptr;
    return t.rc;
}

// ... under periodic boundaries.  The thresholded form: the structures as clouds of their own, a side with a box or cell replaced by its
// image cloud (reach = the threshold) as lchd_sensitivity_primitives_periodic builds them, with that call's checks in its order.
extern "C" int lchd_gradient_primitives_periodic(lchd_ctx* c, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a,
                                                 const int32_t* tag_a, int64_t n_a, const double* xyz_b, const int32_t* cat_b,
                                                 const int32_t* tag_b, int64_t n_b, const int64_t* anchors, const int32_t* wf_index,
                                                 int64_t n_pairs, double thr, const double* box_a, const double* cell_a, const double* box_b,
                                                 const double* cell_b, const double* pair_weights, int64_t tile_pairs, double* scores,
                                                 double* grad_a, double* grad_b, double* strain_a, double* strain_b) {
    CTX_LOCK(c);
    // (what the arguments alone decide comes first: these need no context)
    if (tile_pairs < 0) return fail(LCHD_EVALUE, "tile_pairs = %lld is negative (0: planned from the free device memory)", (long long)tile_pairs);
    if (n_pairs < 0) return fail(LCHD_EVALUE, "negative pair count");
    if (!strain_a != !strain_b) return fail(LCHD_EVALUE, "one strain pointer is null and the other is not: a call writes both tensors or neither");
    const double* const box[2] = {box_a, box_b};
    const double* const cell[2] = {cell_a, cell_b};
    const int64_t n_at[2] = {n_a, n_b};
    for (int k = 0; k < 2; ++k)
        if (box[k] && cell[k])
            return fail(LCHD_EVALUE, "a box and a cell were both given: a structure has one periodic box or one periodic cell");
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    if (int rc = check_wf_index(cfg, wf_index, n_pairs)) return rc;
    if (n_a < 0 || n_b < 0 || n_a > ((int64_t)1 << 27) || n_b > ((int64_t)1 << 27)) return fail(LCHD_EUNSUPPORTED, "structure size out of range");
    for (int k = 0; k < 2; ++k)
        if (box[k]) if (int rc = lchd_box_validate(box[k], 1, thr)) return rc;
    for (int k = 0; k < 2; ++k)
        if (cell[k]) if (int rc = lchd_cell_validate(cell[k], 1, thr)) return rc;
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    if ((n_pairs > 0 && (!anchors || !scores)) || (n_a > 0 && !grad_a) || (n_b > 0 && !grad_b)) return fail(LCHD_EVALUE, "null anchor / output pointer");
    for (int64_t p = 0; p < n_pairs; ++p)  // (an index beyond the structure would name a ghost atom of an image cloud)
        for (int k = 0; k < 2; ++k)
            if (anchors[2 * p + k] < 0 || anchors[2 * p + k] >= n_at[k])
                return fail(LCHD_EPANIC, "index out of bounds: an anchor index is outside its structure (src/locohd.rs:521)");
    CTX_GUARD(c);
    if (int rc = lchd_ctx_set_config(c, cfg)) return rc;
    static const int64_t no_pairs[2] = {0, 0};
    HostTemps t(c);  // clouds[0 .. 1]: what the call runs on; clouds[2 .. 3]: the structures behind image clouds (destroyed after them)
    auto run = [&]() -> int {
        lchd_cloud* own[2] = {nullptr, nullptr};
        if (int rc = lchd_cloud_create(c, xyz_a, cat_a, tag_a, n_a, &own[0])) return rc;
        t.clouds[0] = own[0];
        if (int rc = lchd_cloud_create(c, xyz_b, cat_b, tag_b, n_b, &own[1])) return rc;
        t.clouds[1] = own[1];
        for (int k = 0; k < 2; ++k) {
            if (!box[k] && !cell[k]) continue;
            t.clouds[2 + k] = own[k];
            t.clouds[k] = nullptr;
            if (int rc = box[k] ? lchd_cloud_create_images(c, own[k], box[k], 1, thr, &t.clouds[k])
                                : lchd_cloud_create_images_cell(c, own[k], cell[k], 1, thr, &t.clouds[k]))
                return rc;
        }
        GradHostArrays H{anchors ? anchors : no_pairs, wf_index, pair_weights, n_pairs, n_a, n_b, thr, tile_pairs, scores, grad_a, grad_b};
        H.resolve = kSensImages;
        H.strain[0] = strain_a; H.strain[1] = strain_b;
        return grad_host(c, t, H);
    };
    t.rc = run();
    c->last_valid = false;  // the clouds of this call go away (`t` destroys them on return)
    c->pend.req.a = c->pend.req.b = nullptr;
    return t.rc;
}
// The dense form: lchd_gradient_coords with the cells of lchd_sensitivity_coords_periodic (row-major [9], NULL: an open side).
extern "C" int lchd_gradient_coords_periodic(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b,
                                             int64_t len_seq_b, const double* xyz_a, const double* xyz_b, int64_t n, const int32_t* wf_index,
                                             const double* cell_a, const double* cell_b, const double* pair_weights, double* scores,
                                             double* grad_a, double* grad_b, double* strain_a, double* strain_b) {
    CTX_LOCK(c);
    if (n < 0) return fail(LCHD_EVALUE, "negative structure size");
    if (int rc = coords_lengths(xyz_a, n, xyz_b, n)) return rc;
    if (!strain_a != !strain_b) return fail(LCHD_EVALUE, "one strain pointer is null and the other is not: a call writes both tensors or neither");
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    {
        const double* const cells[2] = {cell_a, cell_b};
        MinImageCell rec[2];
        const MinImageCell* cell[2];
        if (int rc = reduce_cells(cells, 2, false, rec, cell)) return rc;
    }
    CTX_GUARD(c);
    if (int rc = lchd_ctx_set_config(c, cfg)) return rc;
    if (int rc = check_wf_index(cfg, wf_index, n)) return rc;
    if (n == 0) {
        if (strain_a) for (int k = 0; k < 9; ++k) strain_a[k] = strain_b[k] = 0.0;
        return LCHD_OK;
    }
    if (n > len_seq_a || n > len_seq_b) return fail(LCHD_EPANIC, "index out of bounds: a distance row is longer than its seq");
    if (!seq_a || !seq_b || !scores || !grad_a || !grad_b) return fail(LCHD_EVALUE, "null pointer");
    HostTemps t(c);
    auto run = [&]() -> int {
        if (int rc = lchd_cloud_create(c, xyz_a, seq_a, nullptr, n, &t.clouds[0])) return rc;
        if (int rc = lchd_cloud_create(c, xyz_b, seq_b, nullptr, n, &t.clouds[1])) return rc;
        GradHostArrays H{nullptr, wf_index, pair_weights, n, n, n, 0.0, 0, scores, grad_a, grad_b};
        H.resolve = kSensMinImage;
        H.cell[0] = cell_a; H.cell[1] = cell_b;
        H.strain[0] = strain_a; H.strain[1] = strain_b;
        return grad_host(c, t, H);
    };
    t.rc = run();
    c->last_valid = false;
    c->pend.req.a = c->pend.req.b = nullptr;
    return t.rc;
}

// ------------------------------------------------------------------------------------------------
// reduced parameter gradients: sum_p v_p dS_p/dw_c and sum_p v_p dS_p/dtheta (include/loco_hd_hip.h, "reduced parameter gradients")
// ------------------------------------------------------------------------------------------------
// The tile loop of grad_core on the rows of the category-gradient / weight-gradient calls: per tile the unchanged per-pair pass
// (consumer_primitives_dev; dense: consumer_coords_dev, one tile) writes its rows into the context's gradient block, and
// k_param_accumulate (lchd_param_sum.hip) adds them, times the pair weights, into exact accumulators that share the block of the
// coordinate gradients' (status word in front, all zero between calls).  k_param_finish rounds once at the end.
// Bytes per pair of a tile: the row block (8 row_doubles) and what the thresholded pass carves per pair next to its stores (carve_pass:
// the 16-byte pair record and the 4-byte left-over list entry); the stores and indexed lists go with the anchors, not with the pairs.
constexpr int64_t kParamSumPassPairBytes = 16 + 4;
static int64_t param_sum_pair_bytes(int64_t row_doubles) { return 8 * row_doubles + kParamSumPassPairBytes; }
static int64_t param_sum_plan_tile(int64_t n_pairs, int64_t row_doubles, int64_t budget_bytes) {
    return std::max<int64_t>(1, std::min(budget_bytes / param_sum_pair_bytes(row_doubles), n_pairs));
}
extern "C" int lchd_param_sum_plan(int64_t n_pairs, int32_t row_doubles, int64_t budget_bytes, int64_t* tile_pairs_out) {
    if (!tile_pairs_out) return fail(LCHD_EVALUE, "null output pointer");
    *tile_pairs_out = 0;
    if (n_pairs < 1 || row_doubles < 1 || row_doubles > kParamSumMaxWidth + 1 || budget_bytes < 0)
        return fail(LCHD_EVALUE, "a parameter-sum plan takes n_pairs >= 1, rows of 1 .. %d doubles and a budget >= 0 (got %lld, %d, %lld)",
                    kParamSumMaxWidth + 1, (long long)n_pairs, row_doubles, (long long)budget_bytes);
    *tile_pairs_out = param_sum_plan_tile(n_pairs, row_doubles, budget_bytes);
    return LCHD_OK;
}

struct ParamSumRequest {
    bool wgrad;               // the weight form (rows scores | grad[NP], buckets = the weight functions); else the category form
    lchd_cloud *a, *b;
    const int64_t* anchors;   // DEVICE [n_pairs][2]; null: the dense form (pair r = row r, n_pairs = size(a))
    const int32_t* wf;        // DEVICE or null
    int64_t n_pairs;
    double thr;
    const double* cell[2];    // HOST [9] or null (the dense category form)
    const double* weights;    // DEVICE [n_pairs] or null
    int64_t tile_pairs;       // 0: lchd_param_sum_plan
    double* scores;           // DEVICE [n_pairs] (the weight form)
    double* out;              // DEVICE [C] / [n_wf][NP]
};
// *range (may be null): set when the call completed and then failed on an out-of-range term -- its scores are valid
static int param_sum_core(lchd_ctx* c, const ParamSumRequest& R, bool* range = nullptr) {
    if (range) *range = false;
    if (!c || !R.a || !R.b) return fail(LCHD_EVALUE, "null argument");
    const bool dense = R.anchors == nullptr;
    if (R.tile_pairs < 0) return fail(LCHD_EVALUE, "tile_pairs = %lld is negative (0: planned from the free device memory)", (long long)R.tile_pairs);
    if (R.n_pairs < 0) return fail(LCHD_EVALUE, "negative pair count");
    if (!c->cfg_set) return fail(LCHD_EVALUE, "lchd_ctx_set_config has not been called");
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    if (R.wgrad && (R.a->images || R.b->images)) return fail(LCHD_EUNSUPPORTED, "%s", kWgradOpen);
    const PairConsumer use = R.wgrad ? weight_gradient_consumer() : kCategoryGradient;
    if (int rc = consumer_limits(c, use)) return rc;
    if (R.n_pairs >= kGradMaxAdds)
        return fail(LCHD_EUNSUPPORTED, "%lld pairs exceed the 2^31 additions an exact accumulator takes: split the list", (long long)R.n_pairs);
    const int32_t W = R.wgrad ? c->wf_np_max : c->h_cfg.n_categories, buckets = R.wgrad ? c->h_cfg.n_wf : 1;
    const int64_t row = (int64_t)consumer_row(c, use), n_out = (int64_t)buckets * W;
    if (!R.out || (R.wgrad && R.n_pairs > 0 && !R.scores)) return fail(LCHD_EVALUE, "null output pointer");
    CTX_GUARD(c);
    hipStream_t s = c->stream;
    // the accumulators: [status word, 256 bytes] | [buckets][W][limbs]; zero between calls (the finish kernel leaves them so)
    const size_t acc_bytes = 256 + (size_t)n_out * LCHD_GRAD_LIMBS * 8;
    const bool grown = acc_bytes > c->grad_acc_cap;
    if (grown) HIP_TRY(hipStreamSynchronize(s));
    if (int rc = grow_block(c->d_grad_acc, c->grad_acc_cap, acc_bytes)) return rc;
    if (grown || c->grad_acc_dirty) HIP_TRY(hipMemsetAsync(c->d_grad_acc, 0, c->grad_acc_cap, s));
    c->grad_acc_dirty = true;
    uint32_t* const d_flag = reinterpret_cast<uint32_t*>(c->d_grad_acc);
    int64_t* const acc = reinterpret_cast<int64_t*>(c->d_grad_acc + 256);

    int64_t tile = dense ? R.n_pairs : std::min(R.tile_pairs, R.n_pairs);
    if (!dense && R.tile_pairs == 0 && R.n_pairs > 0) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        tile = param_sum_plan_tile(R.n_pairs, row, (int64_t)(std::min<size_t>(free_b, (size_t)1 << 62) / 4));  // (the stores take theirs next to the rows)
    }
    lchd_cloud* const cl[2] = {R.a, R.b};
    for (int64_t p0 = 0; p0 < R.n_pairs; p0 += tile) {
        const int64_t tp = std::min(tile, R.n_pairs - p0);
        const size_t rows_bytes = (size_t)tp * (size_t)row * 8;
        if (rows_bytes > c->grad_cap) HIP_TRY(hipStreamSynchronize(s));  // (the block about to be freed may still be read)
        if (int rc = grow_block(c->d_grad, c->grad_cap, rows_bytes)) return rc;
        double* const blk = reinterpret_cast<double*>(c->d_grad);
        const int32_t* const wf = R.wf ? R.wf + p0 : nullptr;
        if (int rc = dense ? consumer_coords_dev(c, cl, wf, R.cell, use, blk)
                           : consumer_primitives_dev(c, cl, R.anchors + 2 * p0, wf, tp, R.thr, use, blk))
            return rc;  // (nothing of this tile has been added)
        ParamSumArgs pa{};
        pa.rows = R.wgrad ? blk + tp : blk;  // (the weight form's block: scores[tp] | grad[tp][NP])
        pa.ld = W;
        pa.weights = R.weights ? R.weights + p0 : nullptr;
        pa.bucket = buckets > 1 ? wf : nullptr;  // (a dictionary without an index: every pair is scored with function 0, bucket 0)
        if (R.wgrad) { pa.scores_in = blk; pa.scores_out = R.scores + p0; }
        pa.acc = acc;
        pa.flag = d_flag;
        pa.n_pairs = tp;
        pa.width = W;
        pa.n_buckets = buckets;
        if (!launch_param_accumulate(s, pa, c->tune.param_sum_blocks))
            return fail(LCHD_EDEVICE, "the parameter-sum accumulation kernel rejected its launch configuration");
        HIP_TRY(hipGetLastError());
    }
    if (!launch_param_finish(s, acc, n_out, R.out)) return fail(LCHD_EDEVICE, "the parameter-sum finish kernel rejected its launch configuration");
    HIP_TRY(hipGetLastError());
    uint32_t flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));  // the call returns with the outputs complete, as the per-pair call does
    if (flag) HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof flag, s));
    c->grad_acc_dirty = false;
    if (flag && range) *range = true;
    if (flag) return fail(LCHD_EVALUE, "parameter gradient contribution not finite or >= 2^63 (pair weights?)");
    return LCHD_OK;
}

static const int64_t kNoPairs[2] = {0, 0};  // (a non-null list marks the thresholded form; with no pairs it is never read)
extern "C" int lchd_category_gradient_sum_primitives_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int64_t* d_anchors,
                                                         const int32_t* d_wf_index, int64_t n_pairs, double thr, const double* d_pair_weights,
                                                         int64_t tile_pairs, double* d_out) {
    CTX_LOCK(c);
    if (n_pairs > 0 && !d_anchors) return fail(LCHD_EVALUE, "null anchor / output pointer");
    return param_sum_core(c, ParamSumRequest{false, a, b, d_anchors ? d_anchors : kNoPairs, d_wf_index, n_pairs, thr, {nullptr, nullptr},
                                             d_pair_weights, tile_pairs, nullptr, d_out});
}
extern "C" int lchd_category_gradient_sum_coords_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int32_t* d_wf_index, const double* cell_a,
                                                     const double* cell_b, const double* d_pair_weights, double* d_out) {
    CTX_LOCK(c);
    if (!c || !a || !b) return fail(LCHD_EVALUE, "null argument");
    return param_sum_core(c, ParamSumRequest{false, a, b, nullptr, d_wf_index, a->n, 0.0, {cell_a, cell_b}, d_pair_weights, 0, nullptr, d_out});
}
extern "C" int lchd_weight_gradient_sum_primitives_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int64_t* d_anchors,
                                                       const int32_t* d_wf_index, int64_t n_pairs, double thr, const double* d_pair_weights,
                                                       int64_t tile_pairs, double* d_scores, double* d_out) {
    CTX_LOCK(c);
    if (n_pairs > 0 && !d_anchors) return fail(LCHD_EVALUE, "null anchor / output pointer");
    return param_sum_core(c, ParamSumRequest{true, a, b, d_anchors ? d_anchors : kNoPairs, d_wf_index, n_pairs, thr, {nullptr, nullptr},
                                             d_pair_weights, tile_pairs, d_scores, d_out});
}
extern "C" int lchd_weight_gradient_sum_coords_dev(lchd_ctx* c, lchd_cloud* a, lchd_cloud* b, const int32_t* d_wf_index,
                                                   const double* d_pair_weights, double* d_scores, double* d_out) {
    CTX_LOCK(c);
    if (!c || !a || !b) return fail(LCHD_EVALUE, "null argument");
    return param_sum_core(c, ParamSumRequest{true, a, b, nullptr, d_wf_index, a->n, 0.0, {nullptr, nullptr}, d_pair_weights, 0, d_scores, d_out});
}

// The host-array forms: the structures as temporary clouds (a periodic side of the thresholded category form replaced by its image
// cloud, as lchd_category_gradient_primitives does); the list, the weights and the outputs in one temporary device block.
struct ParamSumHostArrays {
    bool wgrad;
    const int64_t* anchors;   // null: the dense form
    const int32_t* wf;
    const double* weights;
    int64_t n_pairs;
    double thr;
    const double* cell[2];
    int64_t tile_pairs;
    double *scores, *out;     // HOST
};
static int param_sum_host(lchd_ctx* c, HostTemps& t, const ParamSumHostArrays& H) {
    const size_t P = (size_t)H.n_pairs;
    const size_t n_out = H.wgrad ? (size_t)c->h_cfg.n_wf * (size_t)c->wf_np_max : (size_t)c->h_cfg.n_categories;
    auto up = [](size_t v) { return (v + 255) & ~size_t(255); };
    const size_t o_wf = up(H.anchors ? 16 * P : 0), o_w = up(o_wf + (H.wf ? 4 * P : 0)), o_sc = up(o_w + (H.weights ? 8 * P : 0)),
                 o_out = up(o_sc + (H.wgrad ? 8 * P : 0)), total = o_out + 8 * n_out;
    if (hipMalloc(&t.d_blk, total ? total : 256) != hipSuccess) {
        (void)hipGetLastError();
        return fail(LCHD_EUNSUPPORTED, "no device memory for the %zu bytes of lists and outputs of this call", total);
    }
    if (H.anchors && P) HIP_TRY(hipMemcpy(t.d_blk, H.anchors, 16 * P, hipMemcpyHostToDevice));
    if (H.wf && P) HIP_TRY(hipMemcpy(t.d_blk + o_wf, H.wf, 4 * P, hipMemcpyHostToDevice));
    if (H.weights && P) HIP_TRY(hipMemcpy(t.d_blk + o_w, H.weights, 8 * P, hipMemcpyHostToDevice));
    const ParamSumRequest R{H.wgrad, t.clouds[0], t.clouds[1],
                            H.anchors ? (P ? reinterpret_cast<const int64_t*>(t.d_blk) : kNoPairs) : nullptr,
                            H.wf ? reinterpret_cast<const int32_t*>(t.d_blk + o_wf) : nullptr, H.n_pairs, H.thr, {H.cell[0], H.cell[1]},
                            H.weights ? reinterpret_cast<const double*>(t.d_blk + o_w) : nullptr, H.tile_pairs,
                            reinterpret_cast<double*>(t.d_blk + o_sc), reinterpret_cast<double*>(t.d_blk + o_out)};
    bool range = false;  // (an out-of-range term fails the call behind complete outputs: the scores are valid and go back)
    const int rc = param_sum_core(c, R, &range);
    if (rc == LCHD_OK || range) {
        const std::string msg = g_err;
        if (H.wgrad && P) HIP_TRY(hipMemcpy(H.scores, t.d_blk + o_sc, 8 * P, hipMemcpyDeviceToHost));
        if (n_out) HIP_TRY(hipMemcpy(H.out, t.d_blk + o_out, 8 * n_out, hipMemcpyDeviceToHost));
        if (rc) snprintf(g_err, sizeof g_err, "%s", msg.c_str());
    }
    return rc;
}
// the thresholded host forms, with the checks of consumer_primitives_host in its order
static int param_sum_primitives_host(lchd_ctx* c, const lchd_config* cfg, bool wgrad, const ProfilePrimsSide* sd, const int64_t* anchors,
                                     const int32_t* wf_index, int64_t n_pairs, double thr, const double* pair_weights, int64_t tile_pairs,
                                     double* scores, double* out) {
    CTX_LOCK(c);
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    if (tile_pairs < 0) return fail(LCHD_EVALUE, "tile_pairs = %lld is negative (0: planned from the free device memory)", (long long)tile_pairs);
    if (n_pairs < 0) return fail(LCHD_EVALUE, "negative pair count");
    for (int k = 0; k < 2; ++k)
        if (sd[k].box && sd[k].cell)
            return fail(LCHD_EVALUE, "a box and a cell were both given: a structure has one periodic box or one periodic cell");
    if (int rc = check_wf_index(cfg, wf_index, n_pairs)) return rc;
    for (int k = 0; k < 2; ++k)
        if (sd[k].n < 0 || sd[k].n > ((int64_t)1 << 27)) return fail(LCHD_EUNSUPPORTED, "structure size out of range");
    for (int k = 0; k < 2; ++k)
        if (sd[k].box) if (int rc = lchd_box_validate(sd[k].box, 1, thr)) return rc;
    for (int k = 0; k < 2; ++k)
        if (sd[k].cell) if (int rc = lchd_cell_validate(sd[k].cell, 1, thr)) return rc;
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    if (!out || (n_pairs > 0 && (!anchors || (wgrad && !scores)))) return fail(LCHD_EVALUE, "null anchor / output pointer");
    for (int64_t p = 0; p < n_pairs; ++p)  // (an index beyond the structure would name a ghost atom of an image cloud)
        for (int k = 0; k < 2; ++k)
            if (anchors[2 * p + k] < 0 || anchors[2 * p + k] >= sd[k].n)
                return fail(LCHD_EPANIC, "index out of bounds: an anchor index is outside its structure (src/locohd.rs:521)");
    CTX_GUARD(c);
    if (int rc = lchd_ctx_set_config(c, cfg)) return rc;
    HostTemps t(c);  // clouds[0 .. 1]: what the call runs on; clouds[2 .. 3]: the structures behind image clouds (destroyed after them)
    auto run = [&]() -> int {
        for (int k = 0; k < 2; ++k) {
            lchd_cloud* own = nullptr;
            if (int rc = lchd_cloud_create(c, sd[k].xyz, sd[k].cat, sd[k].tag, sd[k].n, &own)) return rc;
            t.clouds[k] = own;
            if (!sd[k].box && !sd[k].cell) continue;
            t.clouds[2 + k] = own;
            t.clouds[k] = nullptr;
            if (int rc = sd[k].box ? lchd_cloud_create_images(c, own, sd[k].box, 1, thr, &t.clouds[k])
                                   : lchd_cloud_create_images_cell(c, own, sd[k].cell, 1, thr, &t.clouds[k]))
                return rc;
        }
        return param_sum_host(c, t, ParamSumHostArrays{wgrad, anchors ? anchors : kNoPairs, wf_index, pair_weights, n_pairs, thr, {nullptr, nullptr},
                                                       tile_pairs, scores, out});
    };
    t.rc = run();
    c->last_valid = false;  // the clouds of this call go away (`t` destroys them on return)
    c->pend.req.a = c->pend.req.b = nullptr;
    return t.rc;
}
// ... and the dense ones, with the checks of consumer_dense_host in its order
static int param_sum_coords_host(lchd_ctx* c, const lchd_config* cfg, bool wgrad, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b,
                                 int64_t len_seq_b, const double* xyz_a, const double* xyz_b, int64_t n, const int32_t* wf_index,
                                 const double* cell_a, const double* cell_b, const double* pair_weights, double* scores, double* out) {
    CTX_LOCK(c);
    if (n < 0) return fail(LCHD_EVALUE, "negative structure size");
    if (!c || !cfg) return fail(LCHD_EVALUE, "null context / configuration");
    if (c->pend.active) return fail(LCHD_EVALUE, "an asynchronous call has not been finished (lchd_ctx_finish)");
    {
        const double* const cells[2] = {cell_a, cell_b};
        MinImageCell rec[2];
        const MinImageCell* cell[2];
        if (int rc = reduce_cells(cells, 2, false, rec, cell)) return rc;
    }
    CTX_GUARD(c);
    if (int rc = lchd_ctx_set_config(c, cfg)) return rc;
    if (int rc = check_wf_index(cfg, wf_index, n)) return rc;
    if (n > len_seq_a || n > len_seq_b) return fail(LCHD_EPANIC, "index out of bounds: a distance row is longer than its seq");
    if (!out || (n > 0 && (!seq_a || !seq_b || (wgrad && !scores)))) return fail(LCHD_EVALUE, "null pointer");
    if (n == 0) {  // (no rows: every sum is +0.0)
        const size_t n_out = wgrad ? (size_t)c->h_cfg.n_wf * (size_t)c->wf_np_max : (size_t)c->h_cfg.n_categories;
        for (size_t k = 0; k < n_out; ++k) out[k] = 0.0;
        return LCHD_OK;
    }
    HostTemps t(c);
    auto run = [&]() -> int {
        if (int rc = lchd_cloud_create(c, xyz_a, seq_a, nullptr, n, &t.clouds[0])) return rc;
        if (int rc = lchd_cloud_create(c, xyz_b, seq_b, nullptr, n, &t.clouds[1])) return rc;
        return param_sum_host(c, t, ParamSumHostArrays{wgrad, nullptr, wf_index, pair_weights, n, 0.0, {cell_a, cell_b}, 0, scores, out});
    };
    t.rc = run();
    c->last_valid = false;
    c->pend.req.a = c->pend.req.b = nullptr;
    return t.rc;
}

extern "C" int lchd_category_gradient_sum_primitives(lchd_ctx* c, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a,
                                                     const int32_t* tag_a, int64_t n_a, const double* xyz_b, const int32_t* cat_b,
                                                     const int32_t* tag_b, int64_t n_b, const int64_t* anchors, const int32_t* wf_index,
                                                     int64_t n_pairs, double thr, const double* box_a, const double* cell_a, const double* box_b,
                                                     const double* cell_b, const double* pair_weights, int64_t tile_pairs, double* out) {
    const ProfilePrimsSide sd[2] = {{xyz_a, cat_a, tag_a, n_a, box_a, cell_a}, {xyz_b, cat_b, tag_b, n_b, box_b, cell_b}};
    return param_sum_primitives_host(c, cfg, false, sd, anchors, wf_index, n_pairs, thr, pair_weights, tile_pairs, nullptr, out);
}
extern "C" int lchd_category_gradient_sum_coords(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b,
                                                 int64_t len_seq_b, const double* xyz_a, int64_t n_a, const double* xyz_b, int64_t n_b,
                                                 const int32_t* wf_index, const double* cell_a, const double* cell_b, const double* pair_weights,
                                                 double* out) {
    if (int rc = coords_lengths(xyz_a, n_a, xyz_b, n_b)) return rc;
    return param_sum_coords_host(c, cfg, false, seq_a, len_seq_a, seq_b, len_seq_b, xyz_a, xyz_b, n_a, wf_index, cell_a, cell_b, pair_weights,
                                 nullptr, out);
}
extern "C" int lchd_weight_gradient_sum_primitives(lchd_ctx* c, const lchd_config* cfg, const double* xyz_a, const int32_t* cat_a,
                                                   const int32_t* tag_a, int64_t n_a, const double* xyz_b, const int32_t* cat_b,
                                                   const int32_t* tag_b, int64_t n_b, const int64_t* anchors, const int32_t* wf_index,
                                                   int64_t n_pairs, double thr, const double* pair_weights, int64_t tile_pairs, double* scores,
                                                   double* out) {
    const ProfilePrimsSide sd[2] = {{xyz_a, cat_a, tag_a, n_a, nullptr, nullptr}, {xyz_b, cat_b, tag_b, n_b, nullptr, nullptr}};
    return param_sum_primitives_host(c, cfg, true, sd, anchors, wf_index, n_pairs, thr, pair_weights, tile_pairs, scores, out);
}
extern "C" int lchd_weight_gradient_sum_coords(lchd_ctx* c, const lchd_config* cfg, const int32_t* seq_a, int64_t len_seq_a, const int32_t* seq_b,
                                               int64_t len_seq_b, const double* xyz_a, const double* xyz_b, int64_t n, const int32_t* wf_index,
                                               const double* pair_weights, double* scores, double* out) {
    if (int rc = coords_lengths(xyz_a, n, xyz_b, n)) return rc;
    return param_sum_coords_host(c, cfg, true, seq_a, len_seq_a, seq_b, len_seq_b, xyz_a, xyz_b, n, wf_index, nullptr, nullptr, pair_weights,
                                 scores, out);
}
