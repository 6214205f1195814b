/*
 * loco_hd_hip.h -- C ABI of the MI355X-native LoCoHD scoring core (libloco_hd_hip.so).
 *
 * This is the drop-in boundary that replaces the reference's PyO3 extension module
 * `loco_hd.loco_hd` (/root/reference/src/lib.rs:9-17, Cargo.toml:6-9 `crate-type = ["cdylib"]`) for
 * the scoring path only.  Every entry point names the reference interface it replaces.  Signatures
 * use plain pointers and sizes only (no torch / pyo3 / C++ types); all functions return 0 on success
 * and a non-zero lchd_status otherwise, with the message available from lchd_last_error() on the
 * calling thread.  Status LCHD_EVALUE corresponds to the reference's PyValueError, LCHD_EPANIC to a
 * Rust panic (pyo3 PanicException) in the reference, LCHD_EDEVICE to a HIP failure / missing GPU and
 * LCHD_EUNSUPPORTED to an input the reference accepts but this build cannot run yet.  There is NO CPU
 * fallback: every scoring entry point launches HIP kernels on the context's device.
 *
 * Strings never cross the boundary: a category is the index the reference's HashMap would give it
 * (src/locohd.rs:312-316; -1 = "not in the map", src/locohd/pmf.rs:38-42), a tag is an interned
 * integer (equal strings <=> equal integers; only equality is ever used,
 * src/locohd/tag_pairing_rule.rs:49-75).  The caller owns every buffer; the library never frees or
 * retains caller memory beyond the call (mirrors the reference's copy-in / copy-out ownership).
 *
 * Threads: calls on one context are serialised.  Every entry point that takes an lchd_ctx holds the context for the whole call
 * (lchd_ctx_destroy excepted: no call may be in flight when it is called), so threads may share a context and each gets the
 * result, the status and the lchd_last_error() text of its own call; they simply run one after the other.  Between
 * lchd_from_primitives_dev_async and lchd_ctx_finish the context stays with the thread that enqueued the pass: that thread may
 * go on calling (a second async call is LCHD_EVALUE as before), a call from any other thread waits until the pass is finished
 * (any thread may call lchd_ctx_finish).  lchd_group_from_primitives and lchd_group_last_counts are serialised per group in the
 * same way.  For parallel throughput use one context (one LoCoHD instance) per thread.
 */
#ifndef LOCO_HD_HIP_H
#define LOCO_HD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    LCHD_OK = 0,
    LCHD_EVALUE = 1,       /* reference: ValueError */
    LCHD_EPANIC = 2,       /* reference: Rust panic */
    LCHD_EDEVICE = 3,      /* HIP error / no device */
    LCHD_EUNSUPPORTED = 4  /* valid for the reference, not (yet) for this build */
} lchd_status;

/* weight_function.rs:22-93 function_name */
typedef enum { LCHD_WF_HYPER_EXP = 0, LCHD_WF_DAGUM = 1, LCHD_WF_UNIFORM = 2, LCHD_WF_KUMARASWAMY = 3 } lchd_wf_kind;
/* pmf/statistical_distances.rs:80-85 distance_name */
typedef enum { LCHD_SD_HELLINGER = 0, LCHD_SD_KOLMOGOROV_SMIRNOV = 1, LCHD_SD_KULLBACK_LEIBLER = 2, LCHD_SD_RENYI = 3 } lchd_sd_kind;

/* One WeightFunction (weight_function.rs:6-17): kind + parameter vector. */
typedef struct {
    int32_t kind;         /* lchd_wf_kind */
    int32_t n_params;
    const double *params; /* [n_params] */
} lchd_weight_function;

/* The fields of `struct LoCoHD` (src/locohd.rs:42-55) that the scoring path reads. */
typedef struct {
    int32_t n_categories;            /* categories.len() (:312-316); this build: 1..65534 (16-bit ids on the device) */
    const double *category_weights;  /* [n_categories], all > 0 (:319-346) */
    int32_t n_weight_functions;      /* 1 for WeightFunctionOptions::Single, dict size for ::Multiple (:27-32) */
    const lchd_weight_function *weight_functions;
    int32_t sd_kind;                 /* lchd_sd_kind (:365-370) */
    int32_t sd_n_params;
    double sd_params[2];
    int32_t tag_mode;                /* 0 = WithoutList{accept_same}, 1 = WithList{...} (tag_pairing_rule.rs:5-21) */
    int32_t tag_accept_same;
    int32_t tag_accepted_pairs;
    int32_t tag_ordered;
    const int32_t *tag_pairs;        /* [n_tag_pairs][2] interned (anchor tag, neighbour tag) */
    int64_t n_tag_pairs;
} lchd_config;

typedef struct lchd_ctx lchd_ctx; /* opaque: device, stream, device workspace; replaces the rayon pool (:53,373-383) */

const char *lchd_last_error(void);
const char *lchd_version(void);

/* ---- host-side leaves (no GPU work; same arithmetic headers as the kernels) ------------------- */
/* WeightFunction::build validation, weight_function.rs:22-93 */
int lchd_wf_validate(int32_t kind, const double *params, int32_t n_params);
/* WeightFunction::integral_vec / integral_point, weight_function.rs:95-116: out[i] = CDF(x[i]); x<0 -> LCHD_EVALUE */
int lchd_wf_cdf(int32_t kind, const double *params, int32_t n_params, const double *x, int64_t n, double *out);
/* The density F' of the same weight function (additive): out[i] = w(x[i]); 0 for x < 0 and outside a bounded support. */
int lchd_wf_pdf(int32_t kind, const double *params, int32_t n_params, const double *x, int64_t n, double *out);
/* The parameter derivatives of the same weight function (additive): out[i][k] = dF/dtheta_k at x[i], k in the order of params, out
 * row-major [n][n_params]; x<0 -> LCHD_EVALUE.  Conventions: "weight-function gradients" below. */
int lchd_wf_cdf_grad(int32_t kind, const double *params, int32_t n_params, const double *x, int64_t n, double *out);
/* StatisticalDistance::build validation, statistical_distances.rs:96-121 */
int lchd_sd_validate(int32_t kind, int32_t n_params);
/* StatisticalDistance::run, statistical_distances.rs:123-142 */
int lchd_sd_run(int32_t kind, const double *params, const double *p1, const double *p2, int32_t n, double *out);
/* LoCoHD::build validation, src/locohd.rs:305-346 (n_given = len of the list passed, n_map = len after de-dup) */
int lchd_config_validate(int64_t n_categories_given, int64_t n_categories_map, const double *weights, int64_t n_weights);

/* ---- context ----------------------------------------------------------------------------------- */
/* device < 0 => current HIP device.  Fails with LCHD_EDEVICE when no GPU is usable. */
int lchd_ctx_create(int32_t device, lchd_ctx **out);
void lchd_ctx_destroy(lchd_ctx *ctx);
/* Launch everything on this hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = default stream.
 *
 * Streams (tests/test_gpu_streams.py and tests/cabi_streams.c are the executable form of this paragraph, except where it says
 * "not observable").  The stream may be a
 * non-blocking one.  lchd_ctx_set_stream first waits, on the host, for everything the context has queued on the stream it leaves,
 * so work of one context never runs on two streams at once; it is LCHD_EVALUE while an asynchronous pass is pending (the pass stays
 * intact).  DEVICE pointers passed to a *_dev / _async call (d_anchors, d_wf_index, d_pairs, d_excl_*, d_gathered, and d_out /
 * d_sel_* as outputs) are read and written IN STREAM ORDER on the context's stream: work queued on that stream in front of the
 * call (a kernel or hipMemcpyAsync that fills the pair list, a fill of d_out) is complete before the library touches them, and no
 * host synchronise is needed in between.  Two things must be COMPLETE AT CALL TIME instead: every HOST pointer (it is read before
 * the call returns; the caller may reuse it at once), and the pair list of lchd_shard_plan_dev, which is read on a side stream of
 * the context that is not ordered behind the context's stream.  "Complete on return" (lchd_from_primitives_dev,
 * lchd_from_coords_dev, lchd_ensemble_from_coords_dev, lchd_ctx_finish, lchd_unshard_scores_dev): the host has waited for the
 * context's stream, so d_out may be read from ANY stream or copied to the host without a further wait.
 * lchd_from_primitives_dev_async and lchd_shard_select_dev return with their work only queued: their outputs are ready in stream
 * order on the context's stream (the pass's: for everybody after lchd_ctx_finish).  Structures and configurations come from host
 * pointers (lchd_cloud_create*, lchd_cloud_set_coords, lchd_ctx_set_config): they are ordered behind what the context's stream
 * holds -- a pass queued earlier still sees the old contents -- and are complete on return.  A load into a frames buffer
 * (lchd_frames_load*) runs on ITS `hip_stream` (NULL = the context's stream) and is ordered (a) behind the work queued on that
 * stream before it, the producer of d_atom_xyz included, (b) behind the last pass that read the buffer, and (c) behind the previous
 * load of the same buffer (the host waits until the pinned staging block is free); it is refused (LCHD_EVALUE) while an unfinished
 * asynchronous pass uses the buffer.  Every later call that reads the buffer (a pass, the ensemble call, lchd_cloud_get_coords)
 * waits for the load, whatever stream it ran on -- on the host, because the frames' bounding box and non-finite flag are needed to
 * plan the pass --, and reports a non-finite coordinate of the loaded frames as LCHD_EVALUE.
 * What a caller can rely on, and what is belt and braces: of the load's orderings, (a) and (c) can be observed and are tested (for
 * (c): the previous load is complete when the next load's call returns).  (b) is not observable through this API: a load is refused
 * while a pass is pending, and lchd_ctx_finish has waited for the pass on the host before a load is accepted, so the load's stream
 * wait for the pass's event never has anything left to wait for.  The same holds for the stream wait a pass makes for the load's
 * event: the host wait in front of it has already covered it.  Both stream waits are kept for a later version in which the host
 * wait is dropped for passes that need no new grid; the guarantee callers get today is the host-side one. */
int lchd_ctx_set_stream(lchd_ctx *ctx, void *hip_stream);
/* Upload a LoCoHD configuration; later *_dev calls use it. (The host-pointer drivers below do this themselves.) */
int lchd_ctx_set_config(lchd_ctx *ctx, const lchd_config *cfg);

/* ---- the four reference drivers, host pointers in / host pointers out -------------------------- */
/* LoCoHD::from_anchors, src/locohd.rs:392-406 (+ stat_dist_integral :61-226).  wf_index selects
 * cfg->weight_functions[wf_index] (the shim resolves the key, :230-283).  len_* are passed separately so
 * the "Lists seq and dists must have equal lengths!" check (:70-73) lives behind the boundary. */
int lchd_from_anchors(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq_a, int64_t len_seq_a, const double *dists_a,
                      int64_t len_dists_a, const int32_t *seq_b, int64_t len_seq_b, const double *dists_b,
                      int64_t len_dists_b, int32_t wf_index, double *out);

/* LoCoHD::from_dmxs, src/locohd.rs:410-458.  dmx_x is row-major [rows_x][cols_x]; wf_index NULL or [rows]. */
int lchd_from_dmxs(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq_a, int64_t len_seq_a, const int32_t *seq_b,
                   int64_t len_seq_b, const double *dmx_a, int64_t rows_a, int64_t cols_a, const double *dmx_b,
                   int64_t rows_b, int64_t cols_b, const int32_t *wf_index, double *out);

/* The same with ragged rows (the reference's Vec<Vec<f64>> may hold rows of different lengths; utils.rs:25-39 sorts each row
 * with a prefix of seq): dmx_x is padded to [rows][cols_x], row r of side x has row_len_x[r] in 1..cols_x real entries; what lies
 * beyond a row's length -- matrix entries and seq categories alike -- is never looked at. */
int lchd_from_dmxs_ragged(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq_a, int64_t len_seq_a, const int32_t *seq_b,
                          int64_t len_seq_b, const double *dmx_a, int64_t rows_a, int64_t cols_a, const int32_t *row_len_a,
                          const double *dmx_b, int64_t rows_b, int64_t cols_b, const int32_t *row_len_b, const int32_t *wf_index,
                          double *out);

/* LoCoHD::from_coords, src/locohd.rs:463-476.  xyz_x is [n_x][3]; out is [n_a]. */
int lchd_from_coords(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq_a, int64_t len_seq_a, const int32_t *seq_b,
                     int64_t len_seq_b, const double *xyz_a, int64_t n_a, const double *xyz_b, int64_t n_b,
                     const int32_t *wf_index, double *out);

/* LoCoHD::from_primitives, src/locohd.rs:479-567.  Primitive atoms as SoA (xyz [n][3], category, tag);
 * anchors is [n_pairs][2] = (index into a, index into b); out[i] belongs to anchors[i] (order-preserving,
 * like the reference's indexed rayon collect). */
int lchd_from_primitives(lchd_ctx *ctx, const lchd_config *cfg, const double *xyz_a, const int32_t *cat_a,
                         const int32_t *tag_a, int64_t n_a, const double *xyz_b, const int32_t *cat_b,
                         const int32_t *tag_b, int64_t n_b, const int64_t *anchors, const int32_t *wf_index,
                         int64_t n_pairs, double threshold_distance, double *out);

/* ---- device-resident path (what bench.py and multi-structure callers use) --------------------- */
/* A primitive-atom structure resident in HBM as SoA (replaces the per-call Vec<PrimitiveAtom> clone at the
 * PyO3 boundary, src/locohd/primitive_atom.rs:4-16).  xyz/cat/tag are HOST pointers here. */
typedef struct lchd_cloud lchd_cloud;
int lchd_cloud_create(lchd_ctx *ctx, const double *xyz, const int32_t *cat, const int32_t *tag, int64_t n, lchd_cloud **out);
/* A BATCH of structures in one device object (additive; replaces a Python loop of from_primitives calls such as
 * python_codes/casp14/casp14_extend_with_locohd.py:42-88 or python_codes/trajectory_analyzer.py:112-120): the atoms of
 * all structures are concatenated, sid[i] in [0, n_struct) names the structure of atom i, and an environment only ever
 * contains atoms of its anchor's own structure.  Anchor indices are positions in the concatenated arrays, so one
 * lchd_from_primitives_dev call can score anchor pairs of many structure pairs (pass the same batch as `a` and `b`
 * for all-vs-all). */
int lchd_cloud_create_batch(lchd_ctx *ctx, const double *xyz, const int32_t *cat, const int32_t *tag, const int32_t *sid,
                            int64_t n, int32_t n_struct, lchd_cloud **out);
/* Atoms a cloud / batch / frames buffer currently holds (-1 for a null handle). */
int64_t lchd_cloud_size(const lchd_cloud *cloud);
/* Structures a cloud (1), batch or frames buffer (the frames loaded last) currently holds (-1 for a null handle). */
int32_t lchd_cloud_structures(const lchd_cloud *cloud);
/* Replace the coordinates of an existing cloud (MD frames: same atoms, new positions). Host pointer [n][3]. */
int lchd_cloud_set_coords(lchd_ctx *ctx, lchd_cloud *cloud, const double *xyz);
void lchd_cloud_destroy(lchd_ctx *ctx, lchd_cloud *cloud);

/* from_primitives with everything already on the device: d_anchors is a DEVICE pointer [n_pairs][2] int64,
 * d_wf_index a DEVICE pointer [n_pairs] int32 or NULL, d_out a DEVICE pointer [n_pairs] double.  Work is
 * enqueued on the context's stream; the call returns after the (tiny) status word has been read back, i.e.
 * d_out is complete on return.  Uses the configuration set by lchd_ctx_set_config. */
int lchd_from_primitives_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int64_t *d_anchors,
                             const int32_t *d_wf_index, int64_t n_pairs, double threshold_distance, double *d_out);

/* LoCoHD::from_coords (src/locohd.rs:463-476) with both structures already on the device: pair r = (atom r of a, atom r of
 * b), every environment is the whole structure (no threshold, no tag rule).  d_wf_index: DEVICE [n] int32 or NULL, d_out:
 * DEVICE [n] double, complete on return.  Uses the configuration set by lchd_ctx_set_config. */
int lchd_from_coords_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int32_t *d_wf_index, double *d_out);

/* Dense ensembles (python_codes/ensembles/compare_ensembles.py:277-296: from_dmxs(seq, seq, dmx[i], dmx[j]) for every pair i < j of M
 * structures of one topology), additive.  out[p][r] = from_coords(seq, seq, X[i_p], X[j_p])[r] for structure pair p = (i_p, j_p);
 * each structure's n dense rows are sorted once and reused by all of its pairs.
 *   cloud     a regular batch (lchd_cloud_create_batch of equal-sized structures stored one after the other, or a frames
 *             buffer): M = its structures, n = atoms per structure; the categories of structure 0 are the topology's
 *   d_pairs   DEVICE int32 [n_pairs][2] structure indices ((i, i), (j, i) and repeats allowed), or NULL: every i < j, i outer
 *             (n_pairs must then be M (M - 1) / 2)
 *   d_excl_start [n + 1], d_excl_idx [d_excl_start[n]]: DEVICE CSR of excluded columns per row, or both NULL; an excluded entry
 *             (r, c) counts as distance +inf in every structure (directional: list (c, r) as well for a symmetric ban)
 *   d_wf_index DEVICE int32 [n] (one weight function per row, as from_dmxs's w_func_keys) or NULL; d_out DEVICE double [n_pairs][n]
 * Uses the configuration of lchd_ctx_set_config; d_out is complete on return.  The environment store holds as many structures
 * as the free device memory allows; beyond that the structures are processed in blocks (rows of a block rebuilt per block pair). */
int lchd_ensemble_from_coords_dev(lchd_ctx *ctx, lchd_cloud *cloud, const int32_t *d_pairs, int64_t n_pairs,
                                  const int32_t *d_excl_start, const int32_t *d_excl_idx, const int32_t *d_wf_index, double *d_out);
/* The same from host arrays: xyz [n_struct][n][3], pairs [n_pairs][2] or NULL, excl_start / excl_idx or NULL, wf_index [n] or
 * NULL, out [n_pairs][n].  Uploads a temporary batch and calls the _dev form. */
int lchd_ensemble_from_coords(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq, int64_t n, const double *xyz, int64_t n_struct,
                              const int32_t *pairs, int64_t n_pairs, const int32_t *excl_start, const int32_t *excl_idx,
                              const int32_t *wf_index, double *out);
/* Given square distance matrices dmx [n_struct][n][n] (+inf allowed), out[p][r] = from_dmxs(seq, seq, dmx[i_p], dmx[j_p])[r]. */
int lchd_ensemble_from_dmxs(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq, int64_t n, const double *dmx, int64_t n_struct,
                            const int32_t *pairs, int64_t n_pairs, const int32_t *wf_index, double *out);

/* Split form of lchd_from_primitives_dev: _async enqueues the whole pass on the context's stream and returns without
 * waiting; lchd_ctx_finish waits, re-runs the pass with a larger environment capacity if one overflowed, and returns
 * the status.  Between the two calls the host is free (e.g. to stage the next batch of frames). */
int lchd_from_primitives_dev_async(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int64_t *d_anchors,
                                   const int32_t *d_wf_index, int64_t n_pairs, double threshold_distance, double *d_out);
int lchd_ctx_finish(lchd_ctx *ctx);

/* Trajectory frames (python_codes/trajectory_analyzer.py:97-119: same atoms, new coordinates per frame).  A frames
 * buffer is a batch cloud with room for `capacity_frames` copies of `tmpl`'s atoms (categories and tags replicated on
 * the device once).  lchd_frames_load copies a HOST block xyz[n_frames][n_atoms][3] into pinned staging, then enqueues
 * the H2D copy, the SoA unpack and the bounding-box reduction on `hip_stream` (NULL = the context's stream) and
 * returns; passes that use the buffer are ordered behind the upload with events, so uploading chunk k+1 on a second
 * stream overlaps the scoring of chunk k (use two buffers). */
int lchd_frames_create(lchd_ctx *ctx, const lchd_cloud *tmpl, int32_t capacity_frames, lchd_cloud **out);
int lchd_frames_load(lchd_ctx *ctx, lchd_cloud *frames, const double *xyz, int32_t n_frames, void *hip_stream);

/* Frames given as SOURCE atoms (the step in front of the scoring path): the reference converts every
 * frame on the host -- PrimitiveAssigner.assign_primitive_structure, loco_hd/atom_converter_utils.py:95-129, and its
 * MD variant python_codes/trajectory_analyzer.py:37-74 -- where each primitive atom is np.mean(atom_coords, axis=0) over
 * the float32 coordinates of the atoms its typing-scheme element matched.  The match (regexes on residue / atom names)
 * depends on the topology only, so the host resolves it once into a CSR map and the device evaluates the centroids
 * for every frame with np.mean's float32 arithmetic (sequential adds in member order, one division), bit for bit.
 *   src_start [n_primitive_atoms + 1], src_idx [src_start[n]] : primitive atom p <- source atoms src_idx[src_start[p]..src_start[p+1])
 *   atom_xyz  HOST float32 [n_frames][n_src_atoms][3]
 * lchd_frames_load_atoms has the stream / overlap semantics of lchd_frames_load. */
int lchd_frames_set_sources(lchd_ctx *ctx, lchd_cloud *frames, const int32_t *src_start, const int32_t *src_idx,
                            int64_t n_src_atoms);
int lchd_frames_load_atoms(lchd_ctx *ctx, lchd_cloud *frames, const float *atom_xyz, int32_t n_frames, void *hip_stream);
/* The same with the source atoms already in HBM (d_atom_xyz is a DEVICE pointer; no staging copy), and the duration of
 * the most recent conversion kernel of this buffer in ms (HIP events; <0 unless lchd_ctx_enable_timing is on). */
int lchd_frames_load_atoms_dev(lchd_ctx *ctx, lchd_cloud *frames, const float *d_atom_xyz, int32_t n_frames, void *hip_stream);
double lchd_frames_last_convert_ms(lchd_ctx *ctx, lchd_cloud *frames);
/* Coordinates of a cloud / frames buffer back on the host as [n][3] f64 (n must equal the atoms it holds). */
int lchd_cloud_get_coords(lchd_ctx *ctx, lchd_cloud *cloud, double *xyz_out, int64_t n);

/* ---- periodic boundaries (additive) ---------------------------------------------------------------
 * The reference searches an open system: KdTree::within_radius over the structure's own atoms (src/locohd.rs:504-528).  MD boxes are
 * periodic; the calls below extend that search to an ORTHORHOMBIC box (Lx, Ly, Lz), all edges finite and > 0.  With a box, the
 * environment of an anchor holds every periodic image of every atom of its structure whose distance to the anchor is < the
 * threshold (the same strict comparison of squared distances), the anchor itself always; an image passes or fails the tag rule as
 * its atom would (an image is a different atom with the same category and tag).  For a threshold <= L / 2 this is the minimum-image
 * convention; for L / 2 < threshold <= L an atom may enter through two images, as it would for a kd-tree over the replicated system.
 * Periodicity is resolved in front of the search: an IMAGE CLOUD holds the wrapped atoms of its source at their indices 0 .. n - 1
 * (anchor lists stay valid) and, behind them, the images ("ghosts") that lie within `reach` of the box; the cell lists, environment
 * and sweep kernels then run on it as on any other cloud.
 *   wrap    w = x - floor(x / L) * L per axis, and w = 0 if that rounds to L
 *   images  w + L is emitted iff w < reach, w - L iff w >= L - reach, each computed as that single f64 addition; a ghost is any
 *           combination of per-axis choices other than "all original" (up to 26 per atom), written in ascending image code
 *           cx + 3 cy + 9 cz (c = 0 original, 1 +L, 2 -L) behind the ghosts of the atoms in front: the cloud is a function of its input
 *   reach   threshold_distance <= reach <= min(Lx, Ly, Lz): one layer of images suffices and an anchor never meets its own image
 * Triclinic cells have calls of their own further down, the dense from_coords paths theirs behind those ("minimum-image dense rows");
 * device groups are out of scope. */
/* Host only, no device: LCHD_EVALUE for a non-finite or non-positive edge or reach, or reach > the smallest edge of a box. */
int lchd_box_validate(const double *boxes /* [n_boxes][3] */, int32_t n_boxes, double reach);
/* The image cloud of `src` -- a single structure, a batch (ragged included) or a frames buffer (the frames loaded last).  boxes: HOST
 * [n_boxes][3], n_boxes = 1 (one box for every structure) or the number of structures.  The work runs on the context's stream, behind
 * the source's pending upload (the events lchd_from_primitives_dev uses); the call reads ONE total back to size the output -- a small
 * synchronising copy -- and the ghosts are queued behind it.  The result is an ordinary lchd_cloud (its structures and structure ids
 * are the source's; destroy it with lchd_cloud_destroy) with two differences: lchd_from_primitives_dev / _async return LCHD_EVALUE for
 * a threshold_distance beyond its reach, and lchd_cloud_set_coords / lchd_frames_load* on it are LCHD_EVALUE.  A non-finite source
 * coordinate is LCHD_EVALUE. */
int lchd_cloud_create_images(lchd_ctx *ctx, lchd_cloud *src, const double *boxes, int32_t n_boxes, double reach, lchd_cloud **out);
/* Rebuild an image cloud in place from the current coordinates of `src` (trajectories: once per chunk).  Its arrays only grow.  Waits
 * for the context's stream (the last pass over the image cloud) and, like the call above, for the one total. */
int lchd_cloud_update_images(lchd_ctx *ctx, lchd_cloud *images, lchd_cloud *src, const double *boxes, int32_t n_boxes);
/* Atoms one workgroup of the image kernels covers: beyond it the exclusive scan of the ghost counts takes its two-level form. */
int32_t lchd_images_scan_span(void);
/* lchd_from_primitives in periodic boxes: box_a / box_b are HOST (Lx, Ly, Lz) of the two structures, NULL for a non-periodic side.
 * Uploads both structures, builds the image cloud of every side that has a box with reach = threshold_distance, and scores. */
int lchd_from_primitives_periodic(lchd_ctx *ctx, const lchd_config *cfg, const double *xyz_a, const int32_t *cat_a,
                                  const int32_t *tag_a, int64_t n_a, const double *xyz_b, const int32_t *cat_b,
                                  const int32_t *tag_b, int64_t n_b, const int64_t *anchors, const int32_t *wf_index,
                                  int64_t n_pairs, double threshold_distance, const double *box_a, const double *box_b, double *out);

/* ---- periodic boundaries in triclinic cells (additive) ---------------------------------------------
 * The siblings of the box calls above for a CELL of three lattice vectors a, b, c: a 3 x 3 row-major f64 matrix, row 0 = a.  Any
 * non-singular matrix is a cell: left-handed, not reduced, strongly skewed, not lower-triangular.  Lifetime, stream and error rules are
 * those of the box calls; an image cloud is a box cloud or a cell cloud from its creation on.
 *   widths  w_k = |det| / |cross product of the other two vectors|: the distance between the two faces of the cell that axis k joins.
 *           det = a . (b x c); every cross component is u1 v2 - u2 v1 (cyclic), every sum runs left to right, every norm is
 *           sqrt(x x + y y + z z): plain f64, nothing fused, so a caller can compute the very same numbers
 *   reach   threshold_distance <= reach <= min(w_0, w_1, w_2): a shift of 2 along axis k moves an atom of the cell at least w_k away
 *           from every point of the cell, so one layer of images (shifts in {-1, 0, 1}^3) is all there is, and an anchor never meets
 *           its own image (a non-zero lattice vector is at least min w long)
 *   wrap    f = x . cell^-1 (the inverse is computed on the host in f64), p = x - (floor(f_0) a + floor(f_1) b + floor(f_2) c); the
 *           wrapped originals keep the slots 0 .. n - 1
 *   images  with g = p . cell^-1: along axis k the image p + a_k exists iff g_k w_k < reach, the image p - a_k iff (1 - g_k) w_k <= reach.
 *           This slab rule is a superset of the images within `reach` of any point of the cell; the search measures real distances.
 *           A ghost is any combination of per-axis choices other than "all original" (up to 26 per atom), in ascending image code
 *           c0 + 3 c1 + 9 c2 (c = 0 original, 1 plus, 2 minus), as in a box
 *   ghosts  coordinate d of a ghost is p[d] + t[d], t[d] = (i a[d] + j b[d]) + k c[d] with i, j, k in {-1, 0, 1} held as doubles:
 *           plain f64 products and sums in exactly that order, no fused multiply-add.  A host that reads the wrapped originals back
 *           (lchd_cloud_get_coords) can therefore rebuild every ghost bit for bit. */
/* Host only, no device: LCHD_EVALUE for a non-finite entry, a singular cell (|det| not > 0, or below 1e-12 |a| |b| |c|), a reach that is
 * not finite and > 0, or a reach above the smallest width of a cell. */
int lchd_cell_validate(const double *cells /* [n_cells][9] */, int32_t n_cells, double reach);
/* lchd_cloud_create_images for cells: HOST [n_cells][9], n_cells = 1 (one cell for every structure) or the number of structures.
 * What an image cloud refuses (lchd_cloud_set_coords, lchd_frames_load*, a threshold beyond its reach) a cell cloud refuses too. */
int lchd_cloud_create_images_cell(lchd_ctx *ctx, lchd_cloud *src, const double *cells, int32_t n_cells, double reach, lchd_cloud **out);
/* lchd_cloud_update_images for a cloud made by the call above.  Updating a box cloud through this call, or a cell cloud through
 * lchd_cloud_update_images, is LCHD_EVALUE. */
int lchd_cloud_update_images_cell(lchd_ctx *ctx, lchd_cloud *images, lchd_cloud *src, const double *cells, int32_t n_cells);
/* lchd_from_primitives_periodic with cells: cell_a / cell_b are HOST [9] matrices of the two structures, NULL for a non-periodic side. */
int lchd_from_primitives_periodic_cell(lchd_ctx *ctx, const lchd_config *cfg, const double *xyz_a, const int32_t *cat_a,
                                       const int32_t *tag_a, int64_t n_a, const double *xyz_b, const int32_t *cat_b,
                                       const int32_t *tag_b, int64_t n_b, const int64_t *anchors, const int32_t *wf_index,
                                       int64_t n_pairs, double threshold_distance, const double *cell_a, const double *cell_b, double *out);

/* ---- minimum-image dense rows (additive) -------------------------------------------------------------
 * The dense calls (lchd_from_coords*, lchd_ensemble_from_coords*) in a periodic cell.  A dense row has no threshold, so it follows the
 * MINIMUM-IMAGE convention: every atom of the structure appears exactly once, at the distance of its nearest periodic image to the
 * row's atom; row length and categories do not change, entry r of row r is exactly 0.  This differs from the thresholded calls above,
 * where an atom beyond half an edge may enter an environment through two images.  A cell is the 3 x 3 matrix above (rows a, b, c), any
 * non-singular one (the singularity rule of lchd_cell_validate; no width condition, there is no reach); an orthorhombic box
 * (Lx, Ly, Lz) is the diagonal cell and takes the per-axis form.  Coordinates need not be wrapped; a non-finite one is LCHD_EVALUE.
 * The rows are materialised on the device (8 n^2 bytes per periodic structure of a single pair, in the context's workspace) in front
 * of the unchanged given-row sorts and sweeps, so a score is the one lchd_from_dmxs computes from these rows:
 *   d        = (row atom) - (column atom), per axis
 *   diagonal d_k = d_k - L_k * rint(d_k / L_k) (IEEE division, round to nearest even), distance = sqrt((dx dx + dy dy) + dz dz)
 *   other    with R / I = the reduced cell and its inverse from lchd_cell_reduce:  f_k = (dx I[0][k] + dy I[1][k]) + dz I[2][k],
 *            f_k = f_k - rint(f_k), v = (f_0 a + f_1 b) + f_2 c per component (a, b, c = the rows of R); for i, j, k in {-1, 0, 1}
 *            t = (i a + j b) + k c (the rule of the ghosts above), w = v + t, d2 = (wx wx + wy wy) + wz wz; distance = sqrt(min d2)
 * Plain f64, left to right, nothing fused: a caller can compute the very same rows. */
/* Host only, no device.  Minkowski-reduces a cell: `reduced` spans the same lattice (an integer combination of the rows of `cell` of
 * determinant +-1, each reduced vector evaluated as (T_0 a + T_1 b) + T_2 c from the caller's vectors), and no reduced vector gets
 * shorter by adding a {-1, 0, 1} combination of the other two -- then the nearest lattice translate of a displacement whose fractional
 * coordinates are wrapped to [-1/2, 1/2] is among the 27 shifts {-1, 0, 1}^3, which does not hold for an arbitrary cell.  `inverse` is
 * the inverse of `reduced` in the arithmetic of lchd_cell_validate (inverse[d][k] = (cross product of the other two vectors)[d] / det).
 * A diagonal cell is returned untouched with the inverse diag(1 / L).  LCHD_EVALUE for a non-finite entry or a singular cell. */
int lchd_cell_reduce(const double *cell /* [9] */, double *reduced /* [9] */, double *inverse /* [9] */);
/* lchd_from_coords in periodic cells: cell_a / cell_b are HOST [9] matrices of the two structures, NULL for an open side (its rows are
 * those of lchd_from_coords); with both NULL the call IS lchd_from_coords.  Row-length limits are those of lchd_from_dmxs; a workspace
 * that does not fit the device is LCHD_EUNSUPPORTED.  With lchd_ctx_enable_timing, "cells" of lchd_ctx_last_ms is the time of the row
 * producers of both sides. */
int lchd_from_coords_periodic(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq_a, int64_t len_seq_a, const int32_t *seq_b,
                              int64_t len_seq_b, const double *xyz_a, int64_t n_a, const double *xyz_b, int64_t n_b,
                              const int32_t *wf_index, const double *cell_a, const double *cell_b, double *out);
/* The same on two device-resident structures (lchd_from_coords_dev); the cells stay HOST pointers. */
int lchd_from_coords_periodic_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int32_t *d_wf_index, const double *cell_a,
                                  const double *cell_b, double *d_out);
/* lchd_ensemble_from_coords / _dev in periodic cells: cells is HOST [n_cells][9], n_cells = 1 (one cell for every structure) or the
 * number of structures (NPT).  Excluded entries count as +inf on top of the minimum-image rows; blocks rebuild their rows as before. */
int lchd_ensemble_from_coords_periodic(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq, int64_t n, const double *xyz,
                                       int64_t n_struct, const int32_t *pairs, int64_t n_pairs, const int32_t *excl_start,
                                       const int32_t *excl_idx, const int32_t *wf_index, const double *cells, int32_t n_cells, double *out);
int lchd_ensemble_from_coords_periodic_dev(lchd_ctx *ctx, lchd_cloud *cloud, const int32_t *d_pairs, int64_t n_pairs,
                                           const int32_t *d_excl_start, const int32_t *d_excl_idx, const int32_t *d_wf_index,
                                           const double *cells, int32_t n_cells, double *d_out);

/* ---- local composition profiles (additive, not in the reference) -------------------------------------
 * The quantity a LoCoHD score is the distance of: the weight-function-averaged local composition of ONE environment.  For an environment
 * sorted by distance, d_0 = 0 (the anchor) <= d_1 <= ... <= d_{n-1}, d_n = +inf, with categories c_k, category weights w and the CDF F of
 * the anchor's weight function:
 *   n_c(k) = #{ j <= k : c_j = c },   p_c(k) = w_c n_c(k) / sum_c' w_c' n_c'(k)   (the PMF the sweeps use between d_k and d_{k+1})
 *   P_c    = sum_{k = 0}^{n-1} (F(d_{k+1}) - F(d_k)) p_c(k)
 * out is row-major [entries][n_categories] f64, one row per anchor (or dense row) in the caller's order, categories in the order of
 * lchd_config; a row sums to F(inf) - F(0).  The environment is exactly the one the scoring call of the same name builds for the anchor:
 * strict radius test, tag pairing rule, the anchor itself, periodic images or minimum-image rows, errors for an atom whose type is not in
 * the category map (LCHD_EVALUE), anchors outside the structure (LCHD_EPANIC) -- the calls below run the same prologue and environment
 * kernels on ONE list of anchors (repeated anchors are built once) and hand the store to the profile kernel (lchd_profile.hip)
 * instead of a sweep.  With the Hellinger distance of exponent 1 (total variation), P_X = (F(inf) - F(0)) - score(this environment, a
 * lone anchor of category X): tests/test_composition_model.py and tests/test_gpu_composition.py pin the rows to the oracle that way.
 * Ties in distance carry zero weight, so P does not depend on tie order; under lchd_ctx_set_deterministic a row's bits are a function of
 * the anchor's environment and the configuration alone (not of the other anchors, the slot size a call ended up with, or earlier calls).
 * An environment that does not fit its slot repeats the pass with larger slots (every row is written again).  Limits: environments and
 * dense rows of at most 65 535 points (LCHD_EUNSUPPORTED beyond).  The calls take the context's lock and run on its stream like every
 * other entry point; device pointers follow the stream rules of lchd_from_primitives_dev (read and written in stream order, d_out
 * complete on return).  They leave the hints of the scoring passes alone: scores before and after a profile call are the same bits.
 * With lchd_ctx_enable_timing, "env" of lchd_ctx_last_ms is the environment build (key sets and tie canonicalisation included) and
 * "sweep" the profile kernel.  Device groups have no profile call. */
/* Thresholded, device-resident: `cloud` is a single structure, a batch, a frames buffer or an image cloud (periodic boxes / cells);
 * d_anchors DEVICE int64 [n_anchors] atom indices, d_wf_index DEVICE int32 [n_anchors] or NULL, d_out DEVICE f64 [n_anchors][n_categories].
 * Uses the configuration of lchd_ctx_set_config. */
int lchd_composition_primitives_dev(lchd_ctx *ctx, lchd_cloud *cloud, const int64_t *d_anchors, const int32_t *d_wf_index,
                                    int64_t n_anchors, double threshold_distance, double *d_out);
/* The same from host arrays (one structure, as one side of lchd_from_primitives); out HOST [n_anchors][n_categories]. */
int lchd_composition_primitives(lchd_ctx *ctx, const lchd_config *cfg, const double *xyz, const int32_t *cat, const int32_t *tag, int64_t n,
                                const int64_t *anchors, const int32_t *wf_index, int64_t n_anchors, double threshold_distance, double *out);
/* ... in an orthorhombic box (HOST [3]) or a triclinic cell (HOST [9]); at most one of the two, both NULL: the call above.  The rules of
 * lchd_from_primitives_periodic / _cell: reach = the threshold, which the box or cell must allow. */
int lchd_composition_primitives_periodic(lchd_ctx *ctx, const lchd_config *cfg, const double *xyz, const int32_t *cat, const int32_t *tag,
                                         int64_t n, const int64_t *anchors, const int32_t *wf_index, int64_t n_anchors,
                                         double threshold_distance, const double *box, const double *cell, double *out);
/* Dense rows (lchd_from_coords: row r is the whole structure seen from atom r; no threshold, no tag rule), device-resident single structure;
 * cell HOST [9] or NULL: minimum-image rows (lchd_cell_reduce, the row producer of lchd_from_coords_periodic).  d_out DEVICE [n][n_categories].
 * The rows go through the row kernels that materialise the store (never the fused sort-and-sweep kernel). */
int lchd_composition_coords_dev(lchd_ctx *ctx, lchd_cloud *cloud, const int32_t *d_wf_index, const double *cell, double *d_out);
/* The same from host arrays: seq [len_seq] categories, xyz [n][3]; out HOST [n][n_categories]. */
int lchd_composition_coords(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq, int64_t len_seq, const double *xyz, int64_t n,
                            const int32_t *wf_index, const double *cell, double *out);
/* Given distance rows (lchd_from_dmxs): dmx HOST row-major [rows][cols], +inf entries allowed, every row must hold a 0; wf_index [rows] or
 * NULL; out HOST [rows][n_categories]. */
int lchd_composition_dmx(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq, int64_t len_seq, const double *dmx, int64_t rows,
                         int64_t cols, const int32_t *wf_index, double *out);

/* ---- radial score profiles (additive, not in the reference) -------------------------------------------
 * A LoCoHD score is one number per anchor pair, S = integral of w(r) H(A(r), B(r)) dr.  A radial profile resolves that integrand over
 * distance bins.  Edges e_0 < e_1 < ... < e_K (K >= 1, e_0 >= 0, all finite except that e_K may be +inf, at most 64 bins).  For a pair
 * with merged breakpoints u_0 = 0 <= u_1 <= ... <= u_J (the distances of the points of both environments), u_{J+1} = +inf, and H_j the
 * statistical distance of the two PMFs between u_j and u_{j+1} -- exactly what the scoring call integrates, the anchors included:
 *   out[p][k] = sum_j H_j * max(0, min(F(u_{j+1}), F(e_{k+1})) - max(F(u_j), F(e_k)))
 * with F the CDF of the pair's weight function (wf_index picks it per pair, as in the scoring calls).  out is row-major [pairs][K] f64.
 *   - with e_0 = 0 and e_K = +inf a row sums to the pair's score
 *   - the last bin carries the tail (F(inf) - F(u_J)) H_J beyond the threshold when e_K = +inf, as the reference's definition does
 *   - a bin that does not overlap the weight function's support is exactly 0.0
 *   - mass below e_0 or above a finite e_K is dropped
 *   - ties have zero width: the result does not depend on tie order when H is finite
 * With bins on a fine grid and a uniform weight function the output is the integral of H per bin, and the score under ANY
 * piecewise-constant weight function on that grid is a dot product on the host: the pairs never need rescoring.
 * The environments are exactly those of the scoring call of the same name (strict radius test, tag pairing rule, periodic images or
 * minimum-image rows) and so are the errors (LCHD_EPANIC for an anchor outside its structure, LCHD_EVALUE for a type outside the
 * category map, ...), plus LCHD_EVALUE for bad edges.  The kernel (lchd_radial.hip) works in key space: the bin bounds F(e_k) are
 * computed on the device with the routine that writes the stores' keys, so a point at distance exactly e_k falls on the bound bit for
 * bit.  Every sum has a fixed shape and there are no floating-point atomics: under lchd_ctx_set_deterministic a row's bits depend on
 * the pair, the configuration and the edges alone.  An environment that does not fit its slot repeats the whole pass with larger slots.
 * Limits: at most 512 categories, environments and rows of at most 65 535 points (LCHD_EUNSUPPORTED beyond).  The calls take the
 * context's lock and run on its stream; device pointers follow the stream rules of lchd_from_primitives_dev (d_out complete on return).
 * They leave the hints of the scoring passes and lchd_ctx_last_sweep alone: scores before and after a radial call are the same bits.
 * With lchd_ctx_enable_timing, "env" of lchd_ctx_last_ms is the store build and "sweep" the pair records plus the radial kernel.
 * Device groups have no radial call. */
/* Host only, no device: LCHD_EVALUE for fewer than 2 or more than 65 edges, a negative or NaN edge, edges that do not ascend strictly,
 * +inf anywhere but last. */
int lchd_radial_validate(const double *edges, int32_t n_edges);
/* Thresholded, device-resident: a / b as lchd_from_primitives_dev takes them (single structures, batches, frames buffers, image
 * clouds); d_anchors DEVICE int64 [n_pairs][2], d_wf_index DEVICE int32 [n_pairs] or NULL, edges HOST [n_edges], d_out DEVICE f64
 * [n_pairs][n_edges - 1].  Uses the configuration of lchd_ctx_set_config. */
int lchd_radial_primitives_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int64_t *d_anchors, const int32_t *d_wf_index,
                               int64_t n_pairs, double threshold_distance, const double *edges, int32_t n_edges, double *d_out);
/* The same from host arrays (both sides as lchd_from_primitives).  box_x HOST [3] / cell_x HOST [9]: the periodic box or cell of a side
 * (at most one of the two per side, NULL: open), by the rules of lchd_from_primitives_periodic / _cell.  out HOST [n_pairs][n_edges - 1]. */
int lchd_radial_primitives(lchd_ctx *ctx, const lchd_config *cfg, const double *xyz_a, const int32_t *cat_a, const int32_t *tag_a, int64_t n_a,
                           const double *xyz_b, const int32_t *cat_b, const int32_t *tag_b, int64_t n_b, const int64_t *anchors,
                           const int32_t *wf_index, int64_t n_pairs, double threshold_distance, const double *box_a, const double *cell_a,
                           const double *box_b, const double *cell_b, const double *edges, int32_t n_edges, double *out);
/* Dense rows (lchd_from_coords: pair r = atom r of a against atom r of b, the environments are the whole structures), device-resident
 * single structures of equal size; cell_x HOST [9] or NULL: minimum-image rows.  d_out DEVICE [n][n_edges - 1].  The rows go through
 * the row kernels that materialise the stores (never the fused sort-and-sweep kernel). */
int lchd_radial_coords_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int32_t *d_wf_index, const double *cell_a, const double *cell_b,
                           const double *edges, int32_t n_edges, double *d_out);
/* The same from host arrays, as lchd_from_coords takes them; out HOST [n][n_edges - 1]. */
int lchd_radial_coords(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq_a, int64_t len_seq_a, const int32_t *seq_b, int64_t len_seq_b,
                       const double *xyz_a, int64_t n_a, const double *xyz_b, int64_t n_b, const int32_t *wf_index, const double *cell_a,
                       const double *cell_b, const double *edges, int32_t n_edges, double *out);
/* Given distance rows (lchd_from_dmxs): dmx_x HOST row-major [rows][cols_x], +inf entries allowed, every row must hold a 0; wf_index
 * [rows] or NULL; out HOST [rows][n_edges - 1]. */
int lchd_radial_dmxs(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq_a, int64_t len_seq_a, const int32_t *seq_b, int64_t len_seq_b,
                     const double *dmx_a, const double *dmx_b, int64_t rows, int64_t cols_a, int64_t cols_b, const int32_t *wf_index,
                     const double *edges, int32_t n_edges, double *out);

/* ---- score attribution by category (additive, not in the reference) -----------------------------------
 * Which categories carry a pair's score.  For the Hellinger distance with exponent e, between two merged breakpoints (the notation of
 * the radial profiles above) with a / b the two sides' weighted, normalised PMFs, anchors included:
 *   t_c = |a_c^(1/e) - b_c^(1/e)|^e      T = sum_c t_c      H = (T / 2)^(1/e)
 *   out[p][c] = sum_j (F(u_{j+1}) - F(u_j)) * H_j * t_{c,j} / T_j          (a piece with T_j = 0 adds 0 to every column)
 * out is row-major [pairs][n_categories] f64, categories in the order of lchd_config.
 *   - a row sums to the pair's score (the scoring call of the same name)
 *   - a pair of identical environments gives a row of exact zeros; swapping the sides leaves the row unchanged
 *   - a category neither environment holds has an exactly zero column
 *   - e = 2: t_c is the literal (sqrt a_c - sqrt b_c)^2 and H t_c / T = t_c / (2 H); e = 1 (total variation): 1/2 integral w |a_c - b_c| dr
 *   - this is not the difference of the two composition profiles: a swap at 4 A that is undone at 8 A cancels there, and counts here
 *     at every radius in between
 * Only the Hellinger distance is a sum of per-category terms: under Kolmogorov-Smirnov, Kullback-Leibler and Renyi configurations these
 * calls fail with LCHD_EUNSUPPORTED (the message names the distance); the scoring calls are untouched.
 * The calls are the radial calls without edges: the same environments, store builds, record pass, capacity repeats and errors
 * (LCHD_EPANIC for an anchor outside its structure, LCHD_EVALUE for a type outside the category map, a zero norm under category weights
 * or a weight-function index outside the dictionary, ...), the same stream and lock rules (d_out complete on return), and they too leave
 * the hints of the scoring passes and lchd_ctx_last_sweep alone.  The kernel (lchd_attribution.hip) keeps one accumulator per category
 * and lane and reduces them in lane order: no floating-point atomics, and under lchd_ctx_set_deterministic a row's bits depend on the
 * pair and the configuration alone.
 * Limits: at most 64 categories (LCHD_EUNSUPPORTED beyond; the accumulators of a wavefront live in the LDS), environments and rows of at
 * most 65 535 points.  Device groups have no attribution call. */
/* Thresholded, device-resident (lchd_radial_primitives_dev without edges); d_out DEVICE f64 [n_pairs][n_categories]. */
int lchd_attribution_primitives_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int64_t *d_anchors, const int32_t *d_wf_index,
                                    int64_t n_pairs, double threshold_distance, double *d_out);
/* The same from host arrays (lchd_radial_primitives without edges); out HOST [n_pairs][n_categories]. */
int lchd_attribution_primitives(lchd_ctx *ctx, const lchd_config *cfg, const double *xyz_a, const int32_t *cat_a, const int32_t *tag_a,
                                int64_t n_a, const double *xyz_b, const int32_t *cat_b, const int32_t *tag_b, int64_t n_b,
                                const int64_t *anchors, const int32_t *wf_index, int64_t n_pairs, double threshold_distance,
                                const double *box_a, const double *cell_a, const double *box_b, const double *cell_b, double *out);
/* Dense rows, device-resident single structures of equal size (lchd_radial_coords_dev without edges); d_out DEVICE [n][n_categories]. */
int lchd_attribution_coords_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int32_t *d_wf_index, const double *cell_a,
                                const double *cell_b, double *d_out);
/* The same from host arrays, as lchd_from_coords takes them; out HOST [n][n_categories]. */
int lchd_attribution_coords(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq_a, int64_t len_seq_a, const int32_t *seq_b,
                            int64_t len_seq_b, const double *xyz_a, int64_t n_a, const double *xyz_b, int64_t n_b, const int32_t *wf_index,
                            const double *cell_a, const double *cell_b, double *out);
/* Given distance rows (lchd_radial_dmxs without edges); out HOST [rows][n_categories]. */
int lchd_attribution_dmxs(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq_a, int64_t len_seq_a, const int32_t *seq_b,
                          int64_t len_seq_b, const double *dmx_a, const double *dmx_b, int64_t rows, int64_t cols_a, int64_t cols_b,
                          const int32_t *wf_index, double *out);

/* ---- category-weight gradients (additive, not in the reference) ----------------------------------------
 * The derivative of a pair's score with respect to the category_weights of the configuration: G[p][c] = dS_p / dw_c.  Between two merged
 * breakpoints u_j <= u_{j+1} (the notation of the radial profiles above; u_0 = 0, u_{J+1} = +inf), with nA_c / nB_c the category counts
 * of the piece (anchors included), p_c = w_c nA_c / sum_k w_k nA_k and q_c likewise from nB, D(p, q) the statistical distance,
 * x_c = p_c dD/dp_c and y_c = q_c dD/dq_c -- since w_c dp_k/dw_c = p_c (delta_kc - p_k):
 *   w_c dD/dw_c = x_c + y_c - p_c sum_k x_k - q_c sum_k y_k
 *   out[p][c]   = (1 / w_c) * sum_j (F(u_{j+1}) - F(u_j)) * (w_c dD/dw_c)_j
 * Hellinger, exponent e: d_c = p_c^(1/e) - q_c^(1/e), T = sum_c |d_c|^e, D = (T / 2)^(1/e),
 *   x_c = (D / (e T)) |d_c|^(e-1) sgn(d_c) p_c^(1/e)        y_c = -(D / (e T)) |d_c|^(e-1) sgn(d_c) q_c^(1/e)
 *   (e = 2: w_c dH/dw_c = (sqrt p_c - sqrt q_c)^2 / (4 H) - (p_c + q_c) H / 4)
 * Kullback-Leibler, epsilon (side A is the first argument, as in the scoring calls):
 *   x_c = p_c [ln((p_c + eps) / (q_c + eps)) + p_c / (p_c + eps)]        y_c = -p_c q_c / (q_c + eps)
 * Every term is finite at p_c = 0 or q_c = 0; nothing divides by a PMF entry.  Conventions:
 *   - a Hellinger piece with T = 0 adds 0 to every column (the distance has a kink there; 0 is the subgradient the attribution implies)
 *   - a category with d_c = 0 has x_c = y_c = 0 for every exponent (sgn 0 = 0)
 *   - a piece with F(u_{j+1}) - F(u_j) <= 0 adds nothing
 * so that
 *   - a category neither environment of a pair holds has an exactly zero column
 *   - two identical environments give a row of exact zeros under Hellinger; one category gives exact zeros
 *   - sum_c w_c out[p][c] = 0 up to rounding: the score is homogeneous of degree 0 in the weights
 * out is row-major [pairs][n_categories] f64, categories in the order of lchd_config.  Under Kolmogorov-Smirnov and Renyi configurations
 * these calls fail with LCHD_EUNSUPPORTED (the message names the distance); the scoring calls are untouched.
 * The calls are the attribution calls of the same name with another kernel (lchd_category_gradient.hip) behind the same pass: the same
 * environments, store builds, record pass, capacity repeats, errors (a NaN row for a weight-function index outside the dictionary, ...),
 * stream and lock rules, limits (64 categories, 65 535 points), and they too leave the hints of the scoring passes and
 * lchd_ctx_last_sweep alone.  One accumulator per category and lane, reduced in lane order: no floating-point atomics, a row's bits
 * depend on the stored pair and the configuration alone.  Device groups have no such call. */
/* Thresholded, device-resident; d_out DEVICE f64 [n_pairs][n_categories]. */
int lchd_category_gradient_primitives_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int64_t *d_anchors, const int32_t *d_wf_index,
                                          int64_t n_pairs, double threshold_distance, double *d_out);
/* The same from host arrays, open or periodic per side (box_* / cell_* as lchd_attribution_primitives); out HOST [n_pairs][n_categories]. */
int lchd_category_gradient_primitives(lchd_ctx *ctx, const lchd_config *cfg, const double *xyz_a, const int32_t *cat_a, const int32_t *tag_a,
                                      int64_t n_a, const double *xyz_b, const int32_t *cat_b, const int32_t *tag_b, int64_t n_b,
                                      const int64_t *anchors, const int32_t *wf_index, int64_t n_pairs, double threshold_distance,
                                      const double *box_a, const double *cell_a, const double *box_b, const double *cell_b, double *out);
/* Dense rows, device-resident single structures of equal size; d_out DEVICE [n][n_categories]. */
int lchd_category_gradient_coords_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int32_t *d_wf_index, const double *cell_a,
                                      const double *cell_b, double *d_out);
/* The same from host arrays, as lchd_from_coords takes them; out HOST [n][n_categories]. */
int lchd_category_gradient_coords(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq_a, int64_t len_seq_a, const int32_t *seq_b,
                                  int64_t len_seq_b, const double *xyz_a, int64_t n_a, const double *xyz_b, int64_t n_b,
                                  const int32_t *wf_index, const double *cell_a, const double *cell_b, double *out);
/* Given distance rows; out HOST [rows][n_categories]. */
int lchd_category_gradient_dmxs(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq_a, int64_t len_seq_a, const int32_t *seq_b,
                                int64_t len_seq_b, const double *dmx_a, const double *dmx_b, int64_t rows, int64_t cols_a, int64_t cols_b,
                                const int32_t *wf_index, double *out);

/* ---- neighbour sensitivities (additive, not in the reference) ------------------------------------------
 * Which members of the two environments carry a pair's score, and how it changes when one of them moves: the derivative of the score
 * with respect to the distance d of every environment member.  On the piecewise-constant integrand the sweeps walk,
 *   S = sum_j (F(u_{j+1}) - F(u_j)) * H_j          g = dS/dd = w(d) * (H- - H+)
 * with w = F' the density of the pair's weight function (lchd_wf_pdf) and H- / H+ the statistical distance on the piece that ends /
 * starts at the member.  With x the member's and x0 the anchor's coordinates, dS/dx = g (x - x0) / d and dS/dx0 = -g (x - x0) / d.
 *   - the derivative ignores members entering or leaving at the threshold: it is exact when the weight function's support ends at or
 *     inside the threshold (the default: uniform [3, 10] with threshold 10), else the derivative of the score at fixed membership
 *   - at exact ties it is one-sided: tied members are treated one at a time in list order
 *   - every statistical distance is supported (only values of H are needed); at most 64 categories, environments of at most 65 535 points
 * Every environment is returned as a list sorted ascending by (distance bits, atom index) with the anchor in slot 0 -- one defined
 * order among ties.  Per pair p and side, with K = width the caller's row width:
 *   count[p]     members, the anchor included (0: an unusable pair)
 *   idx[p][K]    atom index of every member (i32), padded with -1; for a batch the GLOBAL index (the position in the concatenated arrays,
 *                as the anchors are given), not the index within the member's structure
 *   dist[p][K]   its distance, padded with 0
 *   g[p][K]      dS/dd; 0 in slot 0 and in the padding.  A member at d == 0 other than the anchor has a g but no direction.
 *   scores[p]    the pair's score from the same walk (the scoring call of the same inputs, to rounding)
 * The pair of an out-of-range weight-function index has NaN scores and g rows, count 0, and the call fails as the attribution call does.
 * Row width: a call whose longest environment holds more than `width` points fails with LCHD_EVALUE (the message names the width it
 * takes) after one pass; lchd_sensitivity_needed_width then returns that width, and after a successful call the longest list.
 * Errors, stream and lock rules, capacity repeats and the untouched hints / lchd_ctx_last_sweep: as lchd_attribution_primitives(_dev).
 * The two thresholded calls right below refuse periodic boxes, cells and image clouds (LCHD_EUNSUPPORTED); lchd_sensitivity_images_dev and
 * lchd_sensitivity_primitives_periodic further down take them.  The dense forms are calls of their own.  Device groups have no
 * sensitivity call. */
int lchd_sensitivity_primitives_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int64_t *d_anchors, const int32_t *d_wf_index,
                                    int64_t n_pairs, double threshold_distance, int32_t width, double *d_scores, int32_t *d_count_a,
                                    int32_t *d_idx_a, double *d_dist_a, double *d_g_a, int32_t *d_count_b, int32_t *d_idx_b,
                                    double *d_dist_b, double *d_g_b);
/* The same from host arrays (the structures as lchd_attribution_primitives takes them, without boxes and cells); outputs HOST. */
int lchd_sensitivity_primitives(lchd_ctx *ctx, const lchd_config *cfg, const double *xyz_a, const int32_t *cat_a, const int32_t *tag_a,
                                int64_t n_a, const double *xyz_b, const int32_t *cat_b, const int32_t *tag_b, int64_t n_b,
                                const int64_t *anchors, const int32_t *wf_index, int64_t n_pairs, double threshold_distance, int32_t width,
                                double *scores, int32_t *count_a, int32_t *idx_a, double *dist_a, double *g_a, int32_t *count_b,
                                int32_t *idx_b, double *dist_b, double *g_b);
int64_t lchd_sensitivity_needed_width(lchd_ctx *ctx);
/* Under periodic boundaries: the same pass on clouds of which any may be an IMAGE CLOUD, with every member resolved to its source atom.
 * `a` / `b`: whatever lchd_sensitivity_primitives_dev takes, or the image clouds of such clouds, in any mix; threshold_distance <= reach
 * is checked as the scoring pass checks it.  Per pair and side, next to count / dist / g as above:
 *   idx[p][K]      the SOURCE atom of every member (i32, padded with -1; for a batch the global index): a ghost names the atom it is an
 *                  image of, so an atom that enters through two images appears twice
 *   image[p][K]    its image code (i8): 0 a home atom (or the padding, or a side that is no image cloud), else c0 + 3 c1 + 9 c2 of the
 *                  periodic section above (c: 0 original, 1 plus, 2 minus, per axis / lattice vector)
 *   disp[p][K][3]  (f64) x_img[member] - x_img[anchor] per axis, on the coordinates of the cloud the pass searched (an image cloud: the
 *                  wrapped originals and their ghosts): the very subtractions behind dist, so dist = sqrt(disp . disp) in the scoring
 *                  order; 0 in slot 0 and in the padding
 * dS/dx(source atom idx) += g disp / dist and dS/dx(anchor) -= the same.  A wrap is a translation by a lattice vector, so this is the
 * derivative with respect to the caller's own, unwrapped coordinates; no coordinates are needed to assemble it.  Not included: the
 * derivative with respect to the box or cell (virial).
 * List order: the one of the pass on the searched cloud -- ascending by (distance bits, index in that cloud) with the anchor first.  An
 * image cloud holds the wrapped originals first and the ghosts behind them by (source atom, image code), so among exact ties: home atoms
 * before ghosts, then the source index, then the image code.  The one-sided derivative at ties follows this order.
 * Width, lchd_sensitivity_needed_width, the NaN rows of a bad weight-function index, errors, stream and lock rules and capacity repeats:
 * as lchd_sensitivity_primitives_dev.  The origin map of an image cloud (lchd_cloud_image_origin) is built by the first such call after
 * the cloud was built or updated, one launch on the context's stream; scoring calls on image clouds never build it. */
int lchd_sensitivity_images_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int64_t *d_anchors, const int32_t *d_wf_index,
                                int64_t n_pairs, double threshold_distance, int32_t width, double *d_scores, int32_t *d_count_a,
                                int32_t *d_idx_a, int8_t *d_image_a, double *d_dist_a, double *d_g_a, double *d_disp_a, int32_t *d_count_b,
                                int32_t *d_idx_b, int8_t *d_image_b, double *d_dist_b, double *d_g_b, double *d_disp_b);
/* The same from host arrays; outputs HOST.  box_* HOST [3], cell_* HOST [9] (row 0 = a): at most one of the two per side, NULL = an open
 * side.  The image cloud of a periodic side is built with reach = threshold_distance and destroyed before the call returns, as
 * lchd_from_primitives_periodic(_cell) and lchd_radial_primitives do; an anchor index beyond its structure fails with their error. */
int lchd_sensitivity_primitives_periodic(lchd_ctx *ctx, const lchd_config *cfg, const double *xyz_a, const int32_t *cat_a,
                                         const int32_t *tag_a, int64_t n_a, const double *xyz_b, const int32_t *cat_b, const int32_t *tag_b,
                                         int64_t n_b, const int64_t *anchors, const int32_t *wf_index, int64_t n_pairs,
                                         double threshold_distance, int32_t width, const double *box_a, const double *cell_a,
                                         const double *box_b, const double *cell_b, double *scores, int32_t *count_a, int32_t *idx_a,
                                         int8_t *image_a, double *dist_a, double *g_a, double *disp_a, int32_t *count_b, int32_t *idx_b,
                                         int8_t *image_b, double *dist_b, double *g_b, double *disp_b);
/* The way back from a slot of an image cloud to its source: origin_out[o] (i32) = the source atom of slot o (origin[i] = i for the wrapped
 * originals), code_out[o] (i8) = its image code (0: an original), HOST arrays of n = lchd_cloud_size(images) entries.  LCHD_EVALUE for a
 * cloud that is no image cloud or another n.  Stream and lock rules of lchd_cloud_get_coords.  The map is built on the first request
 * after a build or update (lchd_cloud_create_images*, lchd_cloud_update_images*) and kept with the cloud until the next one. */
int lchd_cloud_image_origin(lchd_ctx *ctx, lchd_cloud *images, int32_t *origin_out, int8_t *code_out, int64_t n);
/* The source atoms of an image cloud (its slots 0 .. home - 1 hold them, wrapped); for any other cloud its own size. */
int64_t lchd_cloud_home_size(const lchd_cloud *cloud);
/* Dense rows (lchd_attribution_coords_dev / _coords / _dmxs with the sensitivity outputs): pair r = row r of both sides, and EVERY column
 * of a row is a member.  A dense row has no threshold, so no member enters or leaves: g is the whole derivative of the row's score with
 * respect to the row's entries, for any weight function, away from ties (one-sided there).
 *   - the list of a row is sorted ascending by (distance bits, column index) with NO forced anchor: slot 0 is the first of that order, the
 *     reference's stable co-sort of the row with seq -- for coordinates atom r itself, unless an atom of lower index sits on the same point
 *   - idx are column (atom) indices, count = cols of the side, dist the row's entries bit for bit (coordinates: the distances of
 *     lchd_from_coords, bit-identical to rows computed in its operation order)
 *   - `width` must reach max(cols_a, cols_b): a smaller one fails with LCHD_EVALUE before any pass; lchd_sensitivity_needed_width
 *     reports that length either way
 *   - rows are checked as the scoring calls check them (a negative or NaN entry, a row without a 0, a type outside the category map:
 *     LCHD_EVALUE with the scoring call's message)
 * Rows of up to LCHD_SENSITIVITY_ROWS_LDS_POINTS (padded) points are sorted in the LDS of one workgroup, longer ones (up to 65 535) in
 * place in device memory.  No ragged rows, no batches or image clouds; periodic cells in the two calls of the next section. */
#define LCHD_SENSITIVITY_ROWS_LDS_POINTS 8192
int lchd_sensitivity_coords_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int32_t *d_wf_index, int32_t width, double *d_scores,
                                int32_t *d_count_a, int32_t *d_idx_a, double *d_dist_a, double *d_g_a, int32_t *d_count_b,
                                int32_t *d_idx_b, double *d_dist_b, double *d_g_b);
int lchd_sensitivity_coords(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq_a, int64_t len_seq_a, const int32_t *seq_b,
                            int64_t len_seq_b, const double *xyz_a, const double *xyz_b, int64_t n, const int32_t *wf_index, int32_t width,
                            double *scores, int32_t *count_a, int32_t *idx_a, double *dist_a, double *g_a, int32_t *count_b,
                            int32_t *idx_b, double *dist_b, double *g_b);
int lchd_sensitivity_dmxs(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq_a, int64_t len_seq_a, const int32_t *seq_b,
                          int64_t len_seq_b, const double *dmx_a, const double *dmx_b, int64_t rows, int64_t cols_a, int64_t cols_b,
                          const int32_t *wf_index, int32_t width, double *scores, int32_t *count_a, int32_t *idx_a, double *dist_a,
                          double *g_a, int32_t *count_b, int32_t *idx_b, double *dist_b, double *g_b);

/* Dense rows in periodic cells (lchd_sensitivity_coords / _dev on the rows of "minimum-image dense rows"): cell_a / cell_b are HOST [9]
 * matrices or NULL for an open side, exactly as lchd_from_coords_periodic takes them (an orthorhombic box is its diagonal cell).  The
 * nine outputs are those of lchd_sensitivity_coords on the minimum-image rows: dist holds the minimum-image distances bit for bit, the
 * lists are sorted by (distance bits, atom index), scores are those of lchd_from_coords_periodic.  A minimum-image row stores a length
 * alone, and once an image is chosen the direction of a member is no longer x[member] - x[r]; so the call also returns
 *   disp[r][K][3]  (f64) the displacement from row atom r to the nearest image of member idx[r][k], 0 in the padding:  disp = -w with
 *                  d = x[r] - x[member] per axis and, in the arithmetic of the row producer (same operands, plain f64, left to right,
 *                  nothing fused),
 *                    an open side     w = d
 *                    a diagonal cell  w_k = d_k - L_k * rint(d_k / L_k)
 *                    any other cell   v from the wrapped fractional coordinates of d (R / I of lchd_cell_reduce, as above), then the
 *                                     27 candidates w = v + ((i a + j b) + k c), i outermost and k innermost: the chosen w is the FIRST
 *                                     candidate in that order with the smallest (wx wx + wy wy) + wz wz (an update on strict < only)
 *                  A negation is exact, so sqrt((dx dx + dy dy) + dz dz) of disp equals dist[r][k] bit for bit, on every side kind.
 *                  disp = -w also means that a zero component is -0.0 where w is +0.0: the row's own atom (d = +0.0) has disp
 *                  (-0.0, -0.0, -0.0), equal in value and not in bits to x[member] - x[r] = +0.0.  No gradient term is built from a
 *                  slot at distance 0.
 *                  Between two images at exactly the same distance (an atom half a cell away) the rule above decides; slot 0 is
 *                  computed like every other slot (the row atom itself: 0).
 * dS_r/dx(atom idx[r][k]) += g disp / dist and dS_r/dx(atom r) -= the same, for slots beyond 0 with dist > 0: the exact gradient of
 * the row's score with respect to the coordinates as given (wrapped or not), for any weight function.  The derivative with respect to
 * the cell (virial) is not part of it.  No image-code arrays: every atom appears once.  With both cells NULL the call is
 * lchd_sensitivity_coords plus disp.  Errors: those of lchd_sensitivity_coords (width below n: LCHD_EVALUE naming the width needed, more
 * than 65 535 points, batches, image clouds) and those of lchd_from_coords_periodic (a singular or non-finite cell, a non-finite
 * coordinate).  With lchd_ctx_enable_timing, "cells" of lchd_ctx_last_ms is the time of the row producers and "sweep" includes the
 * displacement kernel. */
int lchd_sensitivity_coords_periodic_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int32_t *d_wf_index, const double *cell_a,
                                         const double *cell_b, int32_t width, double *d_scores, int32_t *d_count_a, int32_t *d_idx_a,
                                         double *d_dist_a, double *d_g_a, int32_t *d_count_b, int32_t *d_idx_b, double *d_dist_b,
                                         double *d_g_b, double *d_disp_a, double *d_disp_b);
int lchd_sensitivity_coords_periodic(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq_a, int64_t len_seq_a, const int32_t *seq_b,
                                     int64_t len_seq_b, const double *xyz_a, const double *xyz_b, int64_t n, const int32_t *wf_index,
                                     const double *cell_a, const double *cell_b, int32_t width, double *scores, int32_t *count_a,
                                     int32_t *idx_a, double *dist_a, double *g_a, int32_t *count_b, int32_t *idx_b, double *dist_b,
                                     double *g_b, double *disp_a, double *disp_b);

/* ---- weight-function gradients (additive, not in the reference) ------------------------------------------
 * The derivative of a pair's score with respect to the parameters theta of the pair's weight function: how the score changes with which
 * radii count, and how much.  The environments do not depend on the weight function, so on the piecewise-constant integrand
 *   S           = sum_j (F(u_{j+1}) - F(u_j)) * H_j
 *   dS/dtheta_k = sum_j (G_k(u_{j+1}) - G_k(u_j)) * H_j                                            G_k = dF/dtheta_k
 *               = sum_members G_k(d_m) * (H- - H+) + G_k(inf) * H_last - G_k(0) * H_first          (summation by parts)
 * with H- / H+ the statistical distance on the piece that ends / starts at the member, as for the sensitivities.  This is the
 * derivative of the score as the scoring call computes it: no threshold caveat applies (a member entering or leaving at the threshold
 * does not move with theta).  G_k per family, parameters in the order of lchd_weight_function::params (lchd_wf_cdf_grad evaluates it):
 *   uniform (a, b)                 on a <= x <= b: (x - b) / (b - a)^2 and -(x - a) / (b - a)^2; 0 elsewhere
 *   kumaraswamy (x_min, x_max, alpha, beta)   0 outside [x_min, x_max]; inside, z = (x - x_min) / L, L = x_max - x_min:
 *                                  dF/dz = alpha beta z^(alpha-1) (1 - z^alpha)^(beta-1), dz/dx_min = -(1 - z) / L, dz/dx_max = -z / L,
 *                                  dF/dalpha = beta (1 - z^alpha)^(beta-1) z^alpha ln z, dF/dbeta = -(1 - z^alpha)^beta ln(1 - z^alpha)
 *   dagum (A, B, P)                t = (x / B)^-A: dF/dP = -F ln(1 + t), dF/dt = -P (1 + t)^(-P-1), dt/dA = -t ln(x / B), dt/dB = A t / B
 *   hyper_exp (a_1..a_n, b_1..b_n) N = sum a_i: dF/da_k = ((1 - F) - e^(-b_k x)) / N, dF/db_k = a_k x e^(-b_k x) / N
 * Conventions: x = +inf gives 0 in every family (so the G(inf) term vanishes); x = 0 gives the formula's value, 0 for a dagum; a product
 * of the form 0 * ln 0 is 0; where the limit is infinite (kumaraswamy's bounds with alpha < 1 at z = 0 or beta < 1 at z = 1, a set of
 * distances of measure zero) the value is 0, so every output is finite; a member exactly on a support bound of uniform / kumaraswamy
 * takes the inside branch as the CDF does -- the derivative is one-sided there, and only there.
 * Output: ONE block of n * (1 + NP) doubles, scores[n] | grad[n][NP] row-major, NP = the most parameters of any weight function of the
 * configuration (lchd_weight_gradient_width once the context holds the configuration; a host call sizes `out` from its cfg).  Row p
 * holds the derivatives with respect to the parameters of ITS weight function (wf_index[p]) in their order; the columns behind that
 * function's n_params are exact zeros.  scores[p] is the pair's score from the same walk, bit for bit the sensitivity call's.
 * A row and its score are NaN where the sensitivity call's rows are: an unusable pair, a category outside the configuration, a zero
 * norm, a weight-function index outside the dictionary -- with the same status and return code.
 * The calls are the sensitivity calls of the same name without the list outputs and without a row width (the lists are as wide as the
 * pass needs) and with another kernel (lchd_weight_gradient.hip) behind the same pass: arguments, errors, stream and lock rules, capacity
 * repeats and the untouched hints / lchd_ctx_last_sweep are theirs; lchd_sensitivity_needed_width is left alone.  Every statistical
 * distance; at most 64 categories, lists of at most 65 535 points, weight functions of at most 16 parameters (more: LCHD_EUNSUPPORTED);
 * a weight function whose F(+inf) is not 1 (a dagum with A = 0) fails with LCHD_EVALUE.  Open structures only: no boxes, cells or image
 * clouds (LCHD_EUNSUPPORTED), and device groups have no such call.  One register accumulator per parameter and lane, reduced once per
 * pair in lane order: no floating-point atomics, a row's bits depend on the stored pair and the configuration alone. */
int32_t lchd_weight_gradient_width(lchd_ctx *ctx);
/* Thresholded, device-resident (clouds as lchd_sensitivity_primitives_dev takes them); d_out DEVICE f64 [n_pairs * (1 + NP)]. */
int lchd_weight_gradient_primitives_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int64_t *d_anchors, const int32_t *d_wf_index,
                                        int64_t n_pairs, double threshold_distance, double *d_out);
/* The same from host arrays; out HOST [n_pairs * (1 + NP)]. */
int lchd_weight_gradient_primitives(lchd_ctx *ctx, const lchd_config *cfg, const double *xyz_a, const int32_t *cat_a, const int32_t *tag_a,
                                    int64_t n_a, const double *xyz_b, const int32_t *cat_b, const int32_t *tag_b, int64_t n_b,
                                    const int64_t *anchors, const int32_t *wf_index, int64_t n_pairs, double threshold_distance, double *out);
/* Dense rows, device-resident single structures of equal size n; d_out DEVICE [n * (1 + NP)]. */
int lchd_weight_gradient_coords_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int32_t *d_wf_index, double *d_out);
/* The same from host arrays, as lchd_sensitivity_coords takes them; out HOST [n * (1 + NP)]. */
int lchd_weight_gradient_coords(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq_a, int64_t len_seq_a, const int32_t *seq_b,
                                int64_t len_seq_b, const double *xyz_a, const double *xyz_b, int64_t n, const int32_t *wf_index, double *out);
/* Given distance rows, as lchd_sensitivity_dmxs takes them; out HOST [rows * (1 + NP)]. */
int lchd_weight_gradient_dmxs(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq_a, int64_t len_seq_a, const int32_t *seq_b,
                              int64_t len_seq_b, const double *dmx_a, const double *dmx_b, int64_t rows, int64_t cols_a, int64_t cols_b,
                              const int32_t *wf_index, double *out);

/* ---- native coordinate gradients (additive, not in the reference) ---------------------------------------
 * grad = sum_p v_p dS_p/dx over the pairs of a call, v the pair weights: the backward pass of a loss built from LoCoHD scores.  The lists
 * of the sensitivity calls above are reduced on the device and never reach the caller: a call returns scores, grad_a and grad_b alone.
 * The contribution of slot k >= 1 of pair p on one side is fixed, in IEEE float64 with no contraction:
 *
 *     use   = idx[p][k] >= 0  &&  dist[p][k] > 0  &&  isfinite(g[p][k])
 *     coef  = (v_p * g[p][k]) / dist[p][k]              (v_p = 1.0 without pair weights)
 *     step_c = coef * (x[m][c] - x[a][c])               m = idx[p][k]
 *     acc[m][c] += step_c ;  acc[a][c] += -step_c
 *
 * with idx / dist / g the lists of the sensitivity call of the same inputs and x the clouds' own coordinates.  The atom a is the anchor
 * idx[p][0] in the thresholded form and the row's own atom p in the dense form (not idx[p][0], which is a coincident atom of lower index
 * where one exists); slot 0 is skipped in both.
 * Every acc[atom][c] is an exact fixed-point accumulator: LCHD_GRAD_LIMBS little-endian int64 limbs, each carrying one 32-bit chunk of
 * trunc(step / q) with q = 2^LCHD_GRAD_QUANTUM_LOG2 (toward zero), added with 64-bit integer atomics; integer addition is associative,
 * so the limbs do not depend on the order of the adds.  grad[atom][c] is THE correctly rounded (nearest, ties to even) double of the
 * accumulated sum.  A gradient is therefore a function of the inputs alone: the same bits for every tile size, in default and
 * deterministic mode, on every run -- given the same lists, which the sensitivity pass produces bit-identically for every slot size.
 * A contribution must be finite and smaller than 2^LCHD_GRAD_LIMIT_LOG2 in magnitude: a call in which one was not completes and then
 * fails with LCHD_EVALUE ("gradient contribution not finite or >= 2^63 (pair weights?)"); its scores are valid, its gradients
 * unspecified, and the next call starts from clean accumulators.  Design constants: scores lie in [0, 1] and coordinates are in
 * Angstrom, so contributions are O(1) times the pair weight; 63 bits cover any sane weight, and 2^-192 is below the last bit of anything
 * a caller can observe.
 *   scores[p]     as the sensitivity call returns them, bit for bit (NaN for an unusable pair, which contributes nothing)
 *   grad_a/_b     [size(a)][3] / [size(b)][3] float64, every element written (0 for an atom no pair touches); for a batch the rows
 *                 follow the GLOBAL atom indices
 *   pair_weights  [n_pairs] float64 or NULL (ones)
 * The thresholded form walks the pair list in tiles of tile_pairs: per tile the pass of lchd_sensitivity_primitives_dev -- unchanged --
 * into a grow-only block of the context (40 width + 16 bytes per pair), then the accumulation; a tile is added only after its pass has
 * succeeded, and a pass that reports too small a row width is repeated at lchd_sensitivity_needed_width first.  tile_pairs: 0 =
 * lchd_gradient_plan on a quarter of the free device memory; > 0: that many pairs per tile, clamped to n_pairs; < 0: LCHD_EVALUE.
 * lchd_gradient_plan: pure host arithmetic, the largest tile in 1 .. n_pairs with tile (40 width + 16) <= budget_bytes (1 if not even
 * one pair fits: the allocation then decides); n_pairs < 1, a width outside 1 .. 65535 or a negative budget: LCHD_EVALUE.
 * A list of n_pairs pairs whose rows sum to 2^31 slots or more is LCHD_EUNSUPPORTED (the limbs' headroom): split it.
 * The dense form is one tile: the lists of lchd_sensitivity_coords_dev, the accumulation with a = the row, then the rounding.
 * Clouds, batches, errors, stream and lock rules: those of lchd_sensitivity_primitives_dev / lchd_sensitivity_coords_dev; the context
 * is held once for the whole call.  Image clouds are LCHD_EUNSUPPORTED, device groups have no gradient call; a block that cannot be
 * allocated is LCHD_EUNSUPPORTED like every other out-of-memory condition.  The calls return with their outputs complete. */
#define LCHD_GRAD_LIMBS 8
#define LCHD_GRAD_QUANTUM_LOG2 (-192)
#define LCHD_GRAD_LIMIT_LOG2 63
int lchd_gradient_plan(int64_t n_pairs, int32_t width, int64_t budget_bytes, int64_t *tile_pairs_out);
int lchd_gradient_primitives_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int64_t *d_anchors, const int32_t *d_wf_index,
                                 int64_t n_pairs, double threshold_distance, const double *d_pair_weights, int64_t tile_pairs,
                                 double *d_scores, double *d_grad_a, double *d_grad_b);
/* The same from host arrays (the structures as lchd_sensitivity_primitives takes them); outputs HOST. */
int lchd_gradient_primitives(lchd_ctx *ctx, const lchd_config *cfg, const double *xyz_a, const int32_t *cat_a, const int32_t *tag_a,
                             int64_t n_a, const double *xyz_b, const int32_t *cat_b, const int32_t *tag_b, int64_t n_b,
                             const int64_t *anchors, const int32_t *wf_index, int64_t n_pairs, double threshold_distance,
                             const double *pair_weights, int64_t tile_pairs, double *scores, double *grad_a, double *grad_b);
/* Dense rows of two device-resident structures of equal size n: d_wf_index / d_pair_weights DEVICE [n] or NULL, d_scores DEVICE [n]. */
int lchd_gradient_coords_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int32_t *d_wf_index, const double *d_pair_weights,
                             double *d_scores, double *d_grad_a, double *d_grad_b);
/* The same from host arrays, as lchd_sensitivity_coords takes them; grad_a / grad_b HOST [n][3]. */
int lchd_gradient_coords(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq_a, int64_t len_seq_a, const int32_t *seq_b,
                         int64_t len_seq_b, const double *xyz_a, const double *xyz_b, int64_t n, const int32_t *wf_index,
                         const double *pair_weights, double *scores, double *grad_a, double *grad_b);

/* ---- ... under periodic boundaries, and the strain derivative (additive) -----------------------------------
 * The same reduction on the lists of the periodic sensitivity calls, which carry every member's displacement disp[p][k] from its anchor
 * (an image cloud's member: to the image the pass saw; a minimum-image row: to the nearest image; an open side: x[m] - x[a]).  Per side,
 * with use, coef and the accumulators as above:
 *
 *     use   = k >= 1  &&  idx[p][k] >= 0  &&  dist[p][k] > 0  &&  isfinite(g[p][k])
 *     coef  = (v_p * g[p][k]) / dist[p][k]
 *     step_c = coef * disp[p][k][c]                                             (c = 0, 1, 2)
 *     grad[m][c] += step_c ;  grad[a][c] += -step_c                             m = idx[p][k] (a SOURCE atom), a = the anchor / the row's atom
 *     W[i][j]   += step_i * disp[p][k][j]      for i <= j only;  W[j][i] is a copy of W[i][j]
 *
 * every product one IEEE float64 operation, no contraction; grad has one row per source atom (lchd_cloud_home_size), so the terms of an
 * atom that enters an environment through two images, or as its own anchor's image, all meet in its row.  No coordinate is read.
 * W (strain_a / strain_b, double[9] row-major, one per side) is the STRAIN DERIVATIVE of L = sum_p v_p S_p: for x -> x (I + eps) applied
 * to a side's coordinates (rows) and its box or cell together, dL/d eps[i][j] = W[i][j].  It is symmetric by construction -- six exact
 * sums, each rounded once, the lower triangle copied -- and trace W = sum v g d.  It needs no image code, only disp, so it is defined for
 * an open side too.  From it, with h the cell (rows are the lattice vectors; a box is diag(Lx, Ly, Lz)):
 *     dL/dh at fixed FRACTIONAL coordinates  = inv(h)^T W                      (host arithmetic: loco_hd_amd.cell_gradient)
 *     dL/dh at fixed CARTESIAN coordinates   = inv(h)^T (W - sum_atoms x_atom^T (x) grad_atom)
 * The caveats of the sensitivity calls carry over: the thresholded form ignores members that enter or leave at the threshold, and every
 * form is one-sided at ties (and where a minimum-image member sits exactly half a cell away).
 * The six sums of a side are accumulators like any other (LCHD_GRAD_LIMBS limbs each, next to the per-atom ones), but every slot of a
 * call adds to them: k_strain_accumulate keeps them as integer partial sums in registers across a bounded grid and adds each wavefront's
 * totals once.  Bits: a function of the inputs alone, as the gradients'.
 *   strain_a/_b   both given or both NULL (one alone: LCHD_EVALUE); NULL: the strain kernel is not launched.  With a batch cloud on
 *                 either side a strain request is LCHD_EUNSUPPORTED (one tensor for many boxes has no meaning); gradients work as
 *                 lchd_sensitivity_images_dev takes batches.
 *   slot rule     with strain requested, a call whose slots per side (sum over tiles of tile_pairs x width) reach 2^31 is
 *                 LCHD_EUNSUPPORTED before anything of the offending tile is launched -- the dense form included (n >= 46341, beyond
 *                 the row limit today); without strain the rules above hold.
 * lchd_gradient_images_dev: lchd_gradient_primitives_dev on clouds of which any may be an image cloud, tiles from
 * lchd_sensitivity_images_dev (88 width + 16 + 8 ceil(width / 4) bytes per pair).  lchd_gradient_coords_periodic_dev: lchd_gradient_coords_dev
 * on minimum-image rows, cell_a / cell_b HOST [9] or NULL (an open side) as lchd_sensitivity_coords_periodic_dev takes them; with both
 * NULL the gradients equal lchd_gradient_coords_dev's bit for bit.  Errors of the periodic sensitivity calls pass through unchanged; the
 * out-of-range failure returns behind valid scores and leaves clean accumulators.
 * lchd_gradient_plan_periodic: lchd_gradient_plan for the rows of `resolve` (LCHD_GRAD_PLAIN: 40 width + 16 bytes per pair; _MIN_IMAGE:
 * 88 width + 16; _IMAGES: 8 ceil(width / 4) more), after the slot rule: n_pairs x width >= 2^31 is LCHD_EUNSUPPORTED; a resolve outside 0 .. 2: LCHD_EVALUE.
 * The plan assumes a strain request: a dense call WITHOUT strain is not bound by the slot rule, so the plan refuses LCHD_GRAD_MIN_IMAGE
 * shapes with n in 46341 .. 65535 that such a call takes (it is one tile and needs no plan).
 * lchd_gradient_strain_waves: the wavefronts of the strain kernel's largest grid (tests size their pair lists by it). */
#define LCHD_GRAD_PLAIN 0
#define LCHD_GRAD_IMAGES 1
#define LCHD_GRAD_MIN_IMAGE 2
int lchd_gradient_plan_periodic(int64_t n_pairs, int32_t width, int32_t resolve, int64_t budget_bytes, int64_t *tile_pairs_out);
int64_t lchd_gradient_strain_waves(void);
int lchd_gradient_images_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int64_t *d_anchors, const int32_t *d_wf_index,
                             int64_t n_pairs, double threshold_distance, const double *d_pair_weights, int64_t tile_pairs,
                             double *d_scores, double *d_grad_a, double *d_grad_b, double *d_strain_a, double *d_strain_b);
/* The same from host arrays, boxes and cells as lchd_sensitivity_primitives_periodic takes them; outputs HOST. */
int lchd_gradient_primitives_periodic(lchd_ctx *ctx, const lchd_config *cfg, const double *xyz_a, const int32_t *cat_a,
                                      const int32_t *tag_a, int64_t n_a, const double *xyz_b, const int32_t *cat_b, const int32_t *tag_b,
                                      int64_t n_b, const int64_t *anchors, const int32_t *wf_index, int64_t n_pairs,
                                      double threshold_distance, const double *box_a, const double *cell_a, const double *box_b,
                                      const double *cell_b, const double *pair_weights, int64_t tile_pairs, double *scores,
                                      double *grad_a, double *grad_b, double *strain_a, double *strain_b);
int lchd_gradient_coords_periodic_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int32_t *d_wf_index, const double *cell_a,
                                      const double *cell_b, const double *d_pair_weights, double *d_scores, double *d_grad_a,
                                      double *d_grad_b, double *d_strain_a, double *d_strain_b);
int lchd_gradient_coords_periodic(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq_a, int64_t len_seq_a, const int32_t *seq_b,
                                  int64_t len_seq_b, const double *xyz_a, const double *xyz_b, int64_t n, const int32_t *wf_index,
                                  const double *cell_a, const double *cell_b, const double *pair_weights, double *scores,
                                  double *grad_a, double *grad_b, double *strain_a, double *strain_b);

/* ---- reduced parameter gradients (additive, not in the reference) ------------------------------------------
 * out = sum_p v_p dS_p/dw_c and sum_p v_p dS_p/dtheta over the pairs of a call, v the pair weights: the backward pass of a loss over P
 * pairs with respect to parameters every pair shares.  The per-pair call of the same inputs (lchd_category_gradient_* / lchd_weight_gradient_*
 * above) produces rows row[p][0 .. W): W = n_categories for a category gradient, W = NP = lchd_weight_gradient_width for a weight gradient
 * (next to scores[p]).  They never reach the caller; the rule that reduces them is fixed, in IEEE float64 with no contraction:
 *
 *     use      = !isnan(row[p][0])              (an unusable pair's row is NaN in every column)
 *     term_k   = v_p * row[p][k]                (one multiplication; v_p = 1.0 without pair weights)
 *     acc[b][k] += term_k                       exact: lchd_xs_add of lchd_exact_sum.h (64-bit integer atomics, order-free)
 *     out[b][k] = lchd_xs_finish(acc[b][k])     THE correctly rounded double, once
 *
 *   category form   one bucket; out [n_categories].
 *   weight form     b = wf_index[p], or 0 without an index; out [n_weight_functions][NP] row-major: row f holds sum v_p dS_p/dtheta over the
 *                   pairs scored with function f, in that function's parameter order, exact zeros behind its n_params.  scores [n_pairs]
 *                   as the per-pair call returns them, bit for bit.
 *   out of range    a term that is not finite or >= 2^LCHD_GRAD_LIMIT_LOG2 in magnitude on a usable row (a NaN or infinite v_p is one such
 *                   case) adds nothing; the call completes and then fails with LCHD_EVALUE ("parameter gradient contribution not finite or
 *                   >= 2^63 (pair weights?)"): its scores are valid, its sums unspecified, the next call starts from clean accumulators --
 *                   the behaviour of lchd_gradient_*.  Terms below 2^LCHD_GRAD_QUANTUM_LOG2 are cut off toward zero, as there.
 *   pair_weights    [n_pairs] float64 or NULL (ones), for the thresholded and the dense forms.
 * The outputs are a function of the rows and weights alone: the same bits for every tile_pairs, in default and deterministic mode, on
 * every run -- given the same rows, which the per-pair passes produce bit-identically for every slot size.
 * The thresholded forms walk the pair list in tiles exactly as lchd_gradient_primitives_dev does: per tile the unchanged per-pair pass
 * into a grow-only block of the context, then the accumulation (lchd_param_sum.hip); a tile is added only after its pass has succeeded.
 * tile_pairs: 0 = lchd_param_sum_plan on a quarter of the free device memory; > 0: that many pairs per tile, clamped to n_pairs; < 0:
 * LCHD_EVALUE.  The dense forms are one tile.
 * lchd_param_sum_plan: pure host arithmetic, the largest tile in 1 .. n_pairs with tile * (8 row_doubles + 20) <= budget_bytes (1 if not
 * even one pair fits: the allocation then decides).  row_doubles is the per-pair call's row: n_categories for the category form, 1 + NP
 * for the weight form (its score travels with the row).  The 20 bytes are what the thresholded pass holds per pair next to the row: its
 * 16-byte pair record and a 4-byte list entry.  The formula is NOT the call's footprint: environment stores and indexed lists come on
 * top.  They are sized by the distinct anchors of a tile, not by its pairs (these passes plan with neutral hints, so a side-B store with one
 * slot per pair is taken only under the LCHD_PER_PAIR=1 test hook, where it adds a slot per pair below 2^22 pairs), and at 10^6 pairs of
 * two 10 k-atom clouds they were measured at about 180 - 290 MB next to 23 - 76 MB of rows: budget for them.  n_pairs < 1, row_doubles outside 1 .. 65 or a negative budget: LCHD_EVALUE.
 * A call of 2^31 pairs or more is LCHD_EUNSUPPORTED (the limbs' headroom): split it.
 * Clouds, batches, boxes and cells are accepted where the per-pair form accepts them; limits, errors, status reports, stream and lock
 * rules are those of the per-pair call of the same name (a weight-function index outside the dictionary fails the call as it fails that
 * one); the context is held once for the whole call.  The host-array category form keeps the box_* / cell_* arguments of
 * lchd_category_gradient_primitives; the weight forms are open structures only.  Given distance rows (dmxs) and device groups have no
 * such call.  The calls return with their outputs complete. */
int lchd_param_sum_plan(int64_t n_pairs, int32_t row_doubles, int64_t budget_bytes, int64_t *tile_pairs_out);
/* Thresholded, device-resident; d_pair_weights DEVICE [n_pairs] or NULL, d_out DEVICE f64 [n_categories]. */
int lchd_category_gradient_sum_primitives_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int64_t *d_anchors,
                                              const int32_t *d_wf_index, int64_t n_pairs, double threshold_distance,
                                              const double *d_pair_weights, int64_t tile_pairs, double *d_out);
/* The same from host arrays, open or periodic per side; out HOST [n_categories]. */
int lchd_category_gradient_sum_primitives(lchd_ctx *ctx, const lchd_config *cfg, const double *xyz_a, const int32_t *cat_a,
                                          const int32_t *tag_a, int64_t n_a, const double *xyz_b, const int32_t *cat_b, const int32_t *tag_b,
                                          int64_t n_b, const int64_t *anchors, const int32_t *wf_index, int64_t n_pairs,
                                          double threshold_distance, const double *box_a, const double *cell_a, const double *box_b,
                                          const double *cell_b, const double *pair_weights, int64_t tile_pairs, double *out);
/* Dense rows, device-resident single structures of equal size n; d_pair_weights DEVICE [n] or NULL, d_out DEVICE [n_categories]. */
int lchd_category_gradient_sum_coords_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int32_t *d_wf_index, const double *cell_a,
                                          const double *cell_b, const double *d_pair_weights, double *d_out);
/* The same from host arrays, as lchd_category_gradient_coords takes them; out HOST [n_categories]. */
int lchd_category_gradient_sum_coords(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq_a, int64_t len_seq_a, const int32_t *seq_b,
                                      int64_t len_seq_b, const double *xyz_a, int64_t n_a, const double *xyz_b, int64_t n_b,
                                      const int32_t *wf_index, const double *cell_a, const double *cell_b, const double *pair_weights,
                                      double *out);
/* Thresholded, device-resident; d_scores DEVICE [n_pairs], d_out DEVICE [n_weight_functions][NP]. */
int lchd_weight_gradient_sum_primitives_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int64_t *d_anchors, const int32_t *d_wf_index,
                                            int64_t n_pairs, double threshold_distance, const double *d_pair_weights, int64_t tile_pairs,
                                            double *d_scores, double *d_out);
/* The same from host arrays; scores HOST [n_pairs], out HOST [n_weight_functions][NP] (sized from cfg). */
int lchd_weight_gradient_sum_primitives(lchd_ctx *ctx, const lchd_config *cfg, const double *xyz_a, const int32_t *cat_a, const int32_t *tag_a,
                                        int64_t n_a, const double *xyz_b, const int32_t *cat_b, const int32_t *tag_b, int64_t n_b,
                                        const int64_t *anchors, const int32_t *wf_index, int64_t n_pairs, double threshold_distance,
                                        const double *pair_weights, int64_t tile_pairs, double *scores, double *out);
/* Dense rows, device-resident single structures of equal size n; d_scores DEVICE [n]. */
int lchd_weight_gradient_sum_coords_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int32_t *d_wf_index, const double *d_pair_weights,
                                        double *d_scores, double *d_out);
/* The same from host arrays, as lchd_weight_gradient_coords takes them. */
int lchd_weight_gradient_sum_coords(lchd_ctx *ctx, const lchd_config *cfg, const int32_t *seq_a, int64_t len_seq_a, const int32_t *seq_b,
                                    int64_t len_seq_b, const double *xyz_a, const double *xyz_b, int64_t n, const int32_t *wf_index,
                                    const double *pair_weights, double *scores, double *out);

/* ---- cross-scoring (additive, not in the reference) ------------------------------------------------------
 * Every anchor of one list against every anchor of another: which environments of B look like this environment of A.
 *   cross:   out[i][j] = the score lchd_from_primitives_dev gives the pair (anchors_a[i], anchors_b[j]) -- same threshold, configuration
 *            and tag rule; a row-major [n_a][n_b] matrix.
 *   nearest: per row i the k columns with the smallest (score, j), ascending in that key: scores[n_a][k] and cols[n_a][k] (i32 positions
 *            in anchors_b).  The secondary key j makes the order a function of the score matrix alone.  1 <= k <= min(n_b, 64).
 * anchors_a / anchors_b: [n_a] / [n_b] atom indices into side A / side B (for batches, frames buffers and image clouds: positions in the
 * concatenated arrays, as in lchd_from_primitives_dev); repeats are allowed on both sides.  wf_index: one weight function of the
 * configuration for the whole call, or -1: none (the pass runs without an index list, as lchd_from_primitives_dev with d_wf_index NULL).
 * No pair list exists on the host: the call walks A in tiles of tile_rows anchors, writes the [tile_rows * n_b][2] pair records of a tile
 * on the device (k_cross_pairs), scores them with the pass of lchd_from_primitives_dev -- unchanged, capacity repeats and the second pass
 * over overflowed environments included -- and, for nearest, reduces the tile's scores to k per row (k_nearest_rows, one wavefront per
 * row).  Rows never span tiles and a score does not depend on the tile it is computed in under lchd_ctx_set_deterministic, so both
 * results are then bit-identical for every tile_rows; nearest is always the exact selection on the scores its own passes computed.
 * tile_rows: 0 = lchd_cross_plan on a quarter of the free device memory; > 0: that many rows per tile (memory control, tests), clamped
 * to n_a; a tile of more than 2^31 - 1 pairs is LCHD_EVALUE, as is tile_rows < 0 and a k outside 1 .. min(n_b, 64).
 * Other errors: those lchd_from_primitives_dev gives for the same defect (an anchor outside its structure: LCHD_EPANIC, ...); with n_a
 * or n_b == 0 there is nothing to score and the cross form returns LCHD_OK, as that call does for no pairs.  Stream and lock rules as lchd_from_primitives_dev: the context is held once for the whole call, all work
 * runs on the context's stream, the call returns with the outputs complete.  Afterwards the context's hints and lchd_ctx_last_*
 * read-backs describe the last tile's pass. */
/* Pure host arithmetic, no device: the largest tile_rows in 1 .. n_a for which a tile's pair records (16 bytes per pair), weight-function
 * indices (4) and score scratch (8) fit in budget_bytes and the tile holds at most 2^31 - 1 pairs.  LCHD_EUNSUPPORTED if one row does not
 * fit (a row of more than 2^31 - 1 pairs included), LCHD_EVALUE for n_a < 1, n_b < 1, budget_bytes < 0 or a null output. */
int lchd_cross_plan(int64_t n_a, int64_t n_b, int64_t budget_bytes, int64_t *tile_rows_out);
/* anchors and outputs DEVICE; d_out: [n_a][n_b] doubles */
int lchd_cross_primitives_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int64_t *d_anchors_a, int64_t n_a,
                              const int64_t *d_anchors_b, int64_t n_b, int32_t wf_index, double threshold_distance, int64_t tile_rows,
                              double *d_out);
/* d_scores: [n_a][k] doubles, d_cols: [n_a][k] i32 */
int lchd_nearest_primitives_dev(lchd_ctx *ctx, lchd_cloud *a, lchd_cloud *b, const int64_t *d_anchors_a, int64_t n_a,
                                const int64_t *d_anchors_b, int64_t n_b, int32_t wf_index, double threshold_distance, int64_t tile_rows,
                                int32_t k, double *d_scores, int32_t *d_cols);
/* The same from host arrays (open structures, as lchd_from_primitives takes them): temporary clouds, then the _dev forms; outputs HOST. */
int lchd_cross_primitives(lchd_ctx *ctx, const lchd_config *cfg, const double *xyz_a, const int32_t *cat_a, const int32_t *tag_a, int64_t n_atoms_a,
                          const double *xyz_b, const int32_t *cat_b, const int32_t *tag_b, int64_t n_atoms_b, const int64_t *anchors_a,
                          int64_t n_a, const int64_t *anchors_b, int64_t n_b, int32_t wf_index, double threshold_distance, int64_t tile_rows,
                          double *out);
int lchd_nearest_primitives(lchd_ctx *ctx, const lchd_config *cfg, const double *xyz_a, const int32_t *cat_a, const int32_t *tag_a,
                            int64_t n_atoms_a, const double *xyz_b, const int32_t *cat_b, const int32_t *tag_b, int64_t n_atoms_b,
                            const int64_t *anchors_a, int64_t n_a, const int64_t *anchors_b, int64_t n_b, int32_t wf_index,
                            double threshold_distance, int64_t tile_rows, int32_t k, double *scores, int32_t *cols);

/* ---- multi-GPU ------------------------------------------------------------------------------------
 * The reference's parallelism lives INSIDE the core call: a thread pool that is a field of `LoCoHD` (src/locohd.rs:53,
 * 373-383) runs the anchor pairs of one call (:545-557, order-preserving collect).  The counterpart here is a GROUP of
 * devices inside one process: lchd_group_from_primitives has the signature and the semantics of lchd_from_primitives and
 * spreads the call's anchor pairs over the group's GPUs (both structures are replicated, pairs are binned by their side-A
 * anchor so that every device builds ~1/n of side A's environments, every device scores its bin concurrently, out[i] is
 * the score of anchors[i]).  A binding in any host language gets multi-GPU scoring from this one call; no torch, no MPI. */
typedef struct lchd_group lchd_group;
/* devices: HIP device ordinals (a device may be listed twice: two contexts on it); n_devices in [1, 64]. */
int lchd_group_create(const int32_t *devices, int32_t n_devices, lchd_group **out);
void lchd_group_destroy(lchd_group *group);
int32_t lchd_group_size(const lchd_group *group);
int lchd_group_from_primitives(lchd_group *group, const lchd_config *cfg, const double *xyz_a, const int32_t *cat_a,
                               const int32_t *tag_a, int64_t n_a, const double *xyz_b, const int32_t *cat_b,
                               const int32_t *tag_b, int64_t n_b, const int64_t *anchors, const int32_t *wf_index,
                               int64_t n_pairs, double threshold_distance, double *out);
/* Pairs the most recent lchd_group_from_primitives call gave to each device: counts_out[n_devices]. */
int lchd_group_last_counts(const lchd_group *group, int64_t *counts_out);

/* One process per GPU (torch.distributed / MPI style): every rank holds the whole pair list on its device and runs the
 * SAME deterministic partition (a pure function of the list, so no communication is needed to agree on it):
 *   bin(p) = floor(anchor_a(p) * 1024 / n_atoms_a),  rank(bin) = min(world - 1, floor(#pairs in lower bins * world / n_pairs)).
 * A list whose side-A partition is unbalanced (a rank would hold more than 1.25 n_pairs / world + 1 pairs: ONE reference anchor
 * against thousands, /root/reference/python_codes/kras_scan.py:46-52) is binned by its side-B anchors instead (n_atoms_b > 0),
 * and if that partition is unbalanced too (or n_atoms_b <= 0) cut into contiguous slices, rank(p) = floor(p * world / n_pairs):
 * the reference's par_iter balances any list (src/locohd.rs:545-557), so must this.
 * lchd_shard_plan_dev computes it (one kernel on a side stream of the context + a wait for that kernel only: the pair list
 * must be complete in device memory when it is called) and returns the pair count of every rank;
 * lchd_shard_select_dev compacts THIS rank's pairs (d_sel_anchors [counts[rank]][2], d_sel_index [counts[rank]] = their
 * positions in the full list; enqueued on the context's stream, no wait);
 * lchd_unshard_scores_dev, on the gathering rank, puts score k of rank r at its pair's original position:
 * d_gathered is [world][2][stride] doubles -- rank r's scores, then its d_sel_index reinterpreted as doubles. */
int lchd_shard_plan_dev(lchd_ctx *ctx, const int64_t *d_anchors, int64_t n_pairs, int64_t n_atoms_a, int64_t n_atoms_b,
                        int32_t world, int64_t *counts_out);
int lchd_shard_select_dev(lchd_ctx *ctx, const int64_t *d_anchors, int64_t n_pairs, int64_t n_atoms_a, int64_t n_atoms_b,
                          int32_t rank, int64_t *d_sel_anchors, int64_t *d_sel_index);
int lchd_unshard_scores_dev(lchd_ctx *ctx, const double *d_gathered, const int64_t *counts, int32_t world, int64_t stride,
                            double *d_out, int64_t n_pairs);

/* Per-kernel timing of the most recent *_dev / driver call, measured with hipEvents on the context's stream.
 * names: "cells" (cell lists + anchor de-duplication: one phase), "anchors" (always ~0, kept for callers of the first
 * version), "env", "sweep"; returns milliseconds, <0 if unknown name / timing disabled. */
int lchd_ctx_enable_timing(lchd_ctx *ctx, int32_t on);
double lchd_ctx_last_ms(lchd_ctx *ctx, const char *phase);
/* Environment statistics of the most recent call: sum over anchor pairs of (n_A + n_B) (points incl. anchors). */
int64_t lchd_ctx_last_env_points(lchd_ctx *ctx);
/* The uniform grid a thresholded pass buckets one side's atoms into, as a pure function (no context, no device): cells are at
 * least (1 + 1e-9) thr / reach wide (reach 1: the one-environment-per-workgroup kernels, reach 2: the grouped kernel), at most 1024
 * per axis, and the largest axis is halved until n_struct * dims[0] * dims[1] * dims[2] <= 2^23.  cell_out: the cell edges
 * (1.0 on an axis of extent 0); *n_cells_out: cells of all structures together.  Returns LCHD_OK or LCHD_EVALUE. */
int lchd_plan_grid(const double bbmin[3], const double bbmax[3], int32_t n_struct, double thr, int32_t reach,
                   int32_t dims_out[3], double cell_out[3], int64_t *n_cells_out);
/* Grid and cell-list build of side `side` (0: A, 1: B) of the most recent thresholded pass.  *build_out: 0 no list built for this
 * side (one object on both sides: shared with side A), 1 fused prologue, 2 one workgroup per structure, 3 general build with the
 * one-workgroup scan, 4 general build with the multi-block scan.  Any output pointer may be null.  Returns 0, or -1 under the
 * conditions under which lchd_ctx_last_env_points returns -1 (and for a side other than 0 / 1). */
int lchd_ctx_last_grid(lchd_ctx *ctx, int32_t side, int32_t dims_out[3], int64_t *n_cells_out, int32_t *build_out);
/* The anchor de-duplication of side `side` (0: A, 1: B) of the same pass: which atoms are anchors, which environment slot each gets.
 * *mode_out: 0 with side A's anchors (one object on both sides: both columns share side A's slots), 1 fused prologue (one workgroup per
 * side, the flags as a bit set in LDS: single structures of at most 4096 atoms and 4096 cells, at most 65 536 pairs), 2 byte flags and
 * the one-workgroup scan (at most 2^18 atoms per side), 3 byte flags and one workgroup per chunk of 2^18 atoms (either side larger),
 * 4 none: every PAIR gets a slot of its own (side B only: its anchors were (almost) all used once in the last regular pass, or
 * LCHD_PER_PAIR=1).  *n_unique_out: the environments the pass built for the side, as the device counted them -- the distinct anchors of
 * the side's column (mode 0: 0, and side A's count covers both columns; mode 4: the number of pairs).  *n_repeated_out: -1, or in
 * mode 4 the pairs whose side-B anchor an earlier pair of the list had used (exact up to 2^17 pairs; longer lists count every 16th
 * pair and report 16 times that).  Any output pointer may be null.  Returns 0, or -1 where lchd_ctx_last_grid returns -1. */
int lchd_ctx_last_anchors(lchd_ctx *ctx, int32_t side, int64_t *n_unique_out, int32_t *mode_out, int64_t *n_repeated_out);
/* The sweep kernel families of a from_primitives pass, one bit each (lchd_sweep_plan::families). */
typedef enum {
    LCHD_SWEEP_INLINE = 1,    /* one launch for a small call: the sweep works out the pair records itself */
    LCHD_SWEEP_TEAM240 = 2,   /* four pairs of at most 240 merged events per wavefront (rule 0) */
    LCHD_SWEEP_TEAM480 = 4,   /* two pairs per wavefront: both environments <= 255 points, at most 480 merged events (rule 2) */
    LCHD_SWEEP_C8 = 8,        /* one pair per wavefront, 8-bit counts: both environments <= 255 points (rule 1) */
    LCHD_SWEEP_INDIRECT = 16, /* the companion: the usable pairs the rule in force leaves over */
    LCHD_SWEEP_PLAIN = 32,    /* one pair per wavefront, every size and distance */
    LCHD_SWEEP_INC = 64,      /* Kullback-Leibler / Renyi in O(1) per event */
    LCHD_SWEEP_WIDE = 128     /* more than 32 category slots, environments beyond 65535 points */
} lchd_sweep_family;
/* The test hooks (LCHD_* environment variables, deterministic mode) the choice depends on, one bit each (lchd_sweep_query::hooks). */
typedef enum {
    LCHD_HOOK_NO_DUO = 1, LCHD_HOOK_NO_COUNT8 = 2, LCHD_HOOK_NO_C8_TEAM = 4, LCHD_HOOK_NO_INLINE_META = 8, LCHD_HOOK_FORCE_WIDE = 16,
    LCHD_HOOK_FORCE_GENERIC = 32, LCHD_HOOK_FORCE_BIGENV = 64, LCHD_HOOK_NO_SWEEP_HINT = 128
} lchd_sweep_hook;
/* Everything the choice of sweep kernels depends on. */
typedef struct lchd_sweep_query {
    int64_t n_pairs;
    int32_t n_categories;
    int32_t force_cmax;        /* LCHD_FORCE_CMAX: at least this many category slots (0: none) */
    int32_t hellinger2;        /* the distance is Hellinger with exponent 2 */
    int32_t unit_weights;      /* every category weight is 1 */
    int32_t wf_pow;            /* a weight function needs pow() (matters only without CDF keys) */
    int32_t sd_fast;           /* 0, 1 Kullback-Leibler / 2 Renyi with parameters the O(1) sweep takes, 3 Kolmogorov-Smirnov */
    int32_t has_wf_index;      /* the call names a weight function per pair */
    int32_t has_left_list;     /* the pass has leftover-list buffers (not in deterministic mode) */
    int64_t stride_a, stride_b; /* points per environment slot */
    int32_t cdf_keys_a, cdf_keys_b; /* key sets of F values in the stores (0: distance keys) */
    int32_t pre_rows;          /* both stores carry prefix-count rows of the width this slot count reads */
    int32_t hint_bits;         /* 0 unknown, else 4 | 1 (pairs of <= 240 events were the previous pass's majority) | 2 (pairs of the
                                  8-bit-count rule were) | 8 (EVERY pair had <= 240 events) | 16 (... was of the 8-bit-count rule) */
    uint32_t hooks;            /* lchd_sweep_hook bits */
} lchd_sweep_query;
/* What a pass launches.  Without a hint (forced == 0) every candidate family is launched and the kernels decide on the device which
 * rule is in force: small_rule if 2 * (pairs of small_rule) >= n_pairs, else second_rule (when not 0) if 2 * (pairs of rule 2) >=
 * n_pairs, else none (-1: the plain family takes every pair).  With a hint (forced == 1) small_rule is in force.  A pair with an
 * unusable anchor or environment (its score is NaN) belongs to the team / 8-bit family of the rule in force, to the plain / incremental
 * family under rule -1. */
typedef struct lchd_sweep_plan {
    uint32_t families;         /* lchd_sweep_family bits: exactly what is launched */
    int32_t slots;             /* category-slot instantiation: 8 / 12 / 16 / 20 / 24 / 28 / 32 (8 / 12 / 16 / 24 / 32 for the incremental
                                  family), 0 for the wide family */
    int32_t pre;               /* the team kernels read prefix-count rows (PRE instantiations) */
    int32_t small_rule;        /* 0: a + b - 2 <= 240; 1: max(a, b) <= 255; 2: max(a, b) <= 255 and a + b - 2 <= 480 (a, b: points of
                                  the two environments); without a team / 8-bit family in `families` it is only what n_small counts */
    int32_t second_rule;       /* 0, or 2: the second team kernel of a pass without a hint */
    int32_t c8_rule;           /* the rule (1 or 2) the pass's n_c8 is counted under */
    int32_t forced;            /* the host picked the kernels: no decision on the device */
    int32_t left_listing;      /* the record pass lists the leftover pairs for the companion */
    int32_t companion_left_out; /* the previous pass had no pair for the companion: it is not launched, and the caller repeats the
                                  pass if this one has such a pair after all */
    int32_t team_mode;         /* team / companion form: 0 Hellinger-2 with unit weights, 1 with category weights, 2 Kolmogorov-Smirnov */
    int32_t plain_mode;        /* plain / wide form: 0 Hellinger-2 unit weights, 1 Hellinger-2 category weights, 2 generic distance */
    int32_t ldstab;            /* the plain family keeps its square-root tables in LDS (environments of at most 512 points) */
    int32_t fmode;             /* 0 the keys are F values, 1 inline CDFs only, 2 any CDF */
    int32_t wide_long;         /* wide family: a stride beyond 65535 points asks for its 64-bit-count form */
    /* How the team families were launched (0 where the family is not in `families`, and from lchd_plan_sweep, which knows no launch):
       consecutive pairs a wavefront takes at a time and co-schedules by chunk length, and workgroups of the launch. */
    int32_t team_batch240, team_grid240;   /* the four-team form (pairs of at most 240 events) */
    int32_t team_batch480, team_grid480;   /* the two-team form (at most 480 events) */
} lchd_sweep_plan;
/* Which sweep kernels a from_primitives pass launches, as a pure function (no context, no device).  Returns LCHD_OK, or LCHD_EVALUE
 * (null argument, n_pairs < 1, n_categories < 1).  The planner checks its own answer: a launch set that would not give every pair
 * exactly one kernel is LCHD_EDEVICE (an internal error; no input is known to produce it). */
int lchd_plan_sweep(const lchd_sweep_query *query, lchd_sweep_plan *plan_out);
/* What the sweep of the most recent from_primitives call did, for its last pass (the one whose scores stand).  *plan_out: what
 * lchd_plan_sweep answered for it.  stats_out[0 .. 3]: pairs of at most 240 merged events (unusable pairs included), pairs of c8_rule
 * (likewise), the largest environment (points) -- as the record pass published them -- and the usable pairs the rule in force leaves
 * to the companion (n_pairs minus the count of that rule; -1 without a rule in force); all -1 where no record pass ran (the inline
 * family).  *rule_out: the rule in force (-1, 0, 1, 2) worked out from those counts by the inequalities the kernels evaluate; -1 where
 * the plan has no team / 8-bit family.  *repeated_out: 1 if the pass repeated one whose companion had been left out.  Any output
 * pointer may be null.  Returns 0, or -1 where lchd_ctx_last_grid returns -1: before the first call, while an asynchronous pass is pending,
 * after a from_primitives call that failed or re-scored overflowed environments in a second pass, after a call of another entry point
 * (from_coords, from_dmxs, from_anchors, the ensembles).  One difference: the record is host data, so a host-pointer
 * lchd_from_primitives / lchd_group_from_primitives call (after which the grid is no longer reported) keeps it. */
int lchd_ctx_last_sweep(lchd_ctx *ctx, lchd_sweep_plan *plan_out, int64_t stats_out[4], int32_t *rule_out, int32_t *repeated_out);
/* ---- which kernels sort the dense rows of from_coords / from_dmxs / the dense ensembles ----
 * One of three paths takes a call: the fused sort + sweep kernel (k_dense_fused: nothing but the scores is written), the register-resident
 * row sort of both sides in one launch (k_env_rows2) followed by the sweep, or the three-pass row sort (k_env_rows), one launch per side,
 * followed by the sweep.  Which one, and which instantiation of it, is a pure function of the query below. */
typedef enum { LCHD_DENSE_NONE = 0, LCHD_DENSE_FUSED = 1, LCHD_DENSE_ROWS2 = 2, LCHD_DENSE_ROWS = 3 } lchd_dense_path;
/* The tuning hooks the choice depends on (lchd_dense_query::hooks): LCHD_OLD_ROWS, LCHD_NO_DENSE_FUSED (deterministic mode sets the latter). */
typedef enum { LCHD_DENSE_HOOK_OLD_ROWS = 1, LCHD_DENSE_HOOK_NO_FUSED = 2 } lchd_dense_hook;
typedef struct lchd_dense_query {
    int64_t cols_a, cols_b;    /* points per row of either side (ragged rows: of the longest row) */
    int32_t n_categories;
    int32_t hellinger2;        /* the distance is Hellinger with exponent 2 */
    int32_t unit_weights;      /* every category weight is 1 */
    int32_t cat16;             /* 16-bit category ids in the environment store (the library: more than 255 categories) */
    int32_t given_rows;        /* the rows are given (from_dmxs, minimum-image rows), not computed from coordinates inside the kernel */
    int32_t ragged;            /* every row carries its own length (lchd_from_dmxs_ragged) */
    uint32_t hooks;            /* lchd_dense_hook bits */
    int32_t attempt;           /* 0, or 1: the repeat of a call in which a row defeated the fused kernel or the segmented sort */
    int32_t single_attempt;    /* the caller cannot repeat (the dense ensembles): no kernel that may give up on a row */
    int32_t reserved;          /* 0 */
} lchd_dense_query;
/* One side of the LCHD_DENSE_ROWS path: k_env_rows<nt, globalkv, 8- or 16-bit ids>. */
typedef struct lchd_dense_rows_side {
    int32_t nt;                /* threads per row: 64, 256 or 1024 */
    int32_t globalkv;          /* keys sorted in place in the environment store (only the bucket histogram in LDS) */
    int32_t cat_bytes;         /* 1 or 2 bytes per category id */
    int32_t buckets;           /* distance buckets of the sort: 2048, 16384 or 32768 */
    int32_t cap;               /* points per environment slot (a power of two >= the row) */
} lchd_dense_rows_side;
typedef struct lchd_dense_plan {
    int32_t path;              /* lchd_dense_path; LCHD_DENSE_NONE with unsupported == 1 */
    int32_t unsupported;       /* no kernel takes such rows (LCHD_EUNSUPPORTED / LCHD_EPANIC from the scoring calls) */
    /* LCHD_DENSE_FUSED: k_dense_fused<fused_slots, fused_dmx>, scr_segs distance segments of scratch per workgroup; else 0 */
    int32_t fused_slots;       /* 8, 12 or 16 category slots */
    int32_t fused_dmx;         /* the given-rows form */
    int32_t scr_segs;
    /* LCHD_DENSE_ROWS2: k_env_rows2<nt, ept, seg>, key array of n2 points; else 0 */
    int32_t nt, ept, seg, n2;
    /* LCHD_DENSE_ROWS: per side; else 0 */
    lchd_dense_rows_side rows[2];
} lchd_dense_plan;
/* The plan of a dense call, as a pure function (no context, no device); the launchers take their instantiation from it and decide
 * nothing themselves.  Returns LCHD_OK (also for an unsupported query: see lchd_dense_plan::unsupported), or LCHD_EVALUE (null
 * argument, n_categories < 1, attempt outside 0 .. 1, unknown hook bits). */
int lchd_plan_dense(const lchd_dense_query *query, lchd_dense_plan *plan_out);
/* What the most recent from_coords / from_dmxs / dense-ensemble call of the context ran. */
typedef struct lchd_dense_record {
    lchd_dense_plan plan;      /* the plan of the attempt whose scores stand */
    int32_t attempts;          /* 1, or 2: a row defeated the first attempt's kernel (ST_ROW_RETRY) and the call was repeated */
    int32_t canon;             /* the tie-canonicalisation kernel ran behind the row sort (deterministic mode) */
    int64_t n_bitonic;         /* rows of that attempt whose sort met a bucket of more than 64 points and took the bitonic network
                                  (counted on the device, one atomic per such row; an ensemble: over all its row-sort launches) */
} lchd_dense_record;
/* Returns 0, or -1 (null argument; no dense call yet; the most recent dense call failed).  Calls of other entry points leave the
 * record alone. */
int lchd_ctx_last_dense(lchd_ctx *ctx, lchd_dense_record *record_out);
/* 1 if the most recent from_coords / from_dmxs call of the context ran the fused sort + sweep kernel (one launch per
 * call, nothing but the scores written: Hellinger-2, unit category weights, at most 16 categories, rows of 1 025 .. 20 480
 * points), 0 if it ran the row sort followed by the sweep (src/locohd.rs:410-476 either way).  Reads the record of
 * lchd_ctx_last_dense: plan.path == LCHD_DENSE_FUSED. */
int32_t lchd_ctx_last_dense_fused(lchd_ctx *ctx);
/* Determinism switch.  The reference is ONE code path (src/locohd.rs:61-226): the same anchor pair gives the same bits whatever
 * else the call holds.  By default this library picks among several sweep kernels per call -- from the call's size, from what the
 * majority of its pairs look like and from the statistics of the context's previous pass -- and they sum a pair's intervals in
 * different per-lane orders: the same pair can differ by <= 1e-13 between calls of different shape or history.
 * on != 0 pins ONE sweep family (one pair per wavefront, global-memory tables; dense rows through the row sort + that sweep) and
 * switches every history-dependent choice off: a pair's score is then a function of the pair and the configuration alone --
 * bitwise equal across batch composition, call order, sharding and second passes -- at roughly half the default throughput.
 * Ties: with on != 0 the categories inside every run of EXACTLY equal keys of an environment are put in ascending order, so an
 * environment's stored (distance, category) sequence depends on the multiset of (distance, category) of its points alone (the
 * first point included: several points at distance 0 are ordered like any other tie).  Scores are then invariant under any permutation of the
 * points (from_primitives: with the anchor pairs renumbered; from_coords: out[k] follows point k; from_dmxs: rows and columns
 * permuted together), on lattices, duplicated coordinates, extra zeros and +inf entries of distance matrices included
 * (tests/test_gpu_deterministic.py).  With on == 0 points of DIFFERENT categories at exactly the same distance enter an environment in
 * the order the cell lists' and row sorts' atomics produced, which may differ from run to run; they span zero-width intervals, so only
 * the rounding of the running sums differs: a few 1e-16 in a handful of pairs.  Inputs without such ties are bit-reproducible in
 * both modes.  The one exception to the one-family rule: environments of more than 65 535 points take the 64-bit-count sweep in
 * both modes (their scores are still a function of the pair and the configuration).
 * on == 0 returns to the default selection.  Not allowed while an asynchronous call is pending. */
int lchd_ctx_set_deterministic(lchd_ctx *ctx, int32_t on);
int32_t lchd_ctx_get_deterministic(lchd_ctx *ctx);
/* from_primitives passes the context has enqueued since it was created.  A call is one pass in the steady state; a pass is
 * repeated when an environment overflowed the capacity tried (src/locohd.rs:514-542 has no capacity) or when the sweep launch
 * set picked from the previous call's pair statistics did not cover this call's pairs. */
int64_t lchd_ctx_pass_count(lchd_ctx *ctx);
/* Regular passes so far whose side B was NOT de-duplicated: environment slot p belongs to anchor pair p and its anchor record is
 * written straight from the pair list -- taken when the previous regular pass of the context found (almost) every side-B anchor
 * used once (trajectory frames, (i, i) lists, a rank's partners under strong scaling).  The reference builds an environment per
 * pair and side as well (src/locohd.rs:514-554). */
int64_t lchd_ctx_per_pair_pass_count(lchd_ctx *ctx);
/* Second passes run so far.  Environments live in fixed-stride slots (512 points by default); the reference's environments have no
 * capacity (src/locohd.rs:514-542: a Vec per anchor).  When a FEW environments of a call do not fit their slots, only the pairs
 * that touch them are scored again -- a pass of their own with larger slots, its scores scattered over the first pass's --
 * instead of giving every environment of the call the larger slot. */
int64_t lchd_ctx_subset_pass_count(lchd_ctx *ctx);
/* Environment-store bytes (keys + categories, both sides) carved by the passes of the most recent from_primitives call, summed. */
int64_t lchd_ctx_last_store_bytes(lchd_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* LOCO_HD_HIP_H */
