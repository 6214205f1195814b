// lchd_device.h -- internal interface between the C-ABI host layer (lchd_capi.hip) and the gfx950
// kernels (lchd_*.hip, one kernel family per translation unit).  Plain-old-data argument blocks + launcher prototypes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <iterator>
#include <type_traits>

#include "lchd_cell_reduce.h"  // host only: kMinImageRecord, the cell of the dense minimum-image calls
#include "lchd_pass_plan.h"  // the host-only part: Tuning, HostStatus, the ST_* status bits, the pass planner
#include "lchd_dense_plan.h"  // host only: the dense-row planner and every limit of its three kernels

struct lchd_sweep_query;  // include/loco_hd_hip.h
struct lchd_sweep_plan;

namespace lchd {

// (kMaxCategories = 255, lchd_pass_plan.h: categories travel as u8 on the device ...)
constexpr int kHugeCategories = 65534;  // ... beyond kWideCategories: the same 16-bit ids (0xFFFF = not in the map), the sweep's per-category state in global memory
// scratch of one workgroup of k_sweep_wide<.., HUGE>: [C][64] u32 count columns | [C] u32 carry row | 2 x [64][C] f64 normalised vectors
inline size_t wide_scratch_bytes_per_wave(int C) { return (((size_t)C * 65 * 4 + 15) & ~(size_t)15) + (size_t)C * 64 * 16; }
constexpr int kWideCategories = 512;  // ... or, for 256 .. 512 categories, as u16 (CloudView::cat_hi, EnvStore::cat16): from_primitives and
                                      // from_anchors only, through k_env_cells<.., uint16_t> and k_sweep_wide<.., CAT16> (its per-lane
                                      // category counts, 256 bytes per category, must fit the LDS)
constexpr int kSweepEPL = 6;  // merged events per lane per tile in the sweep kernel (16-bit counts, LDS tables, <= 16 category slots; the generic distances)
constexpr int kSweepTile = 64 * kSweepEPL;
constexpr int kMetaPartials = 4096;   // most workgroups of k_pair_meta
// Category slots the register-resident sweeps are instantiated for.  A configuration runs the smallest entry that holds its categories
// (the last one beyond it); the launchers and plan_sweep (lchd_sweep_plan::slots) both go through with_slots.
inline constexpr int kSweepSlots[] = {8, 12, 16, 20, 24, 28, 32};  // k_sweep, k_sweep_duo
inline constexpr int kIncSlots[] = {8, 12, 16, 24, 32};            // k_sweep_inc
// f(std::integral_constant<int, S>) for the entry S of TAB that `cmax` categories round up to
template <const auto& TAB, size_t I = 0, class F>
inline void with_slots(int cmax, F&& f) {
    if (cmax <= TAB[I] || I + 1 == std::size(TAB)) f(std::integral_constant<int, TAB[I]>{});
    else if constexpr (I + 1 < std::size(TAB)) with_slots<TAB, I + 1>(cmax, f);
}
constexpr uint64_t kPadKey = ~0ull;   // sorts after every valid (non-negative, non-NaN) f64 bit pattern

// Device-resident status of a pass.  Invariant between passes: flags == max_env == 0 -- the last workgroup of
// k_pair_meta copies the words the host needs into the host-mapped HostStatus and resets them, so a pass needs neither a
// memset in front of it nor a device-to-host copy behind it.  n_unique / n_small are plain-stored by every pass.
struct DeviceStatus {
    uint32_t flags;
    uint32_t max_env;        // largest environment seen (for the overflow retry)
    uint32_t n_unique[2];    // unique anchors per side
    uint32_t n_overflow[2];  // environments per side that did not fit their slot (entries of EnvSide::ovf_list); reset with the flags
    unsigned long long n_small;     // pairs under the pass's first-choice small rule (k_pair_meta): who sweeps them is decided on the device
    unsigned long long n_c8;        // pairs under SweepArgs::c8_rule (the second choice of a pass without a hint)
    uint32_t max_bound;      // k_env_group: most CANDIDATES of an anchor whose candidate table overflowed (an upper bound of its environment; max_env
                             //  then only says "more than the capacity"); reset with the flags
    uint32_t n_dup_b;        // a pass without de-duplication of side B (k_pair_anchor_recs): pairs whose side-B anchor another pair of the list had
                             //  marked before (a bit set in the side's flag region, one returning atomic per pair); reset with the flags
    uint32_t n_bitonic;      // dense rows whose sort met a bucket beyond kRowBucketLimit points and took the bitonic network (k_env_rows, k_env_rows2:
                             //  one atomic per such row); reset with the flags
    uint32_t pad;
};


struct WfEntry {
    int32_t kind, n_params, offset, pad;
};

// Device-resident LoCoHD configuration (src/locohd.rs:42-55).
struct DevConfig {
    int32_t n_categories;
    int32_t n_wf;
    int32_t sd_kind;
    int32_t tag_mode, tag_accept_same, tag_accepted_pairs, tag_ordered;
    int32_t n_tag_pairs;
    double sd_p0, sd_p1;
    const double* cat_w;        // [n_categories]
    const WfEntry* wf;          // [n_wf]
    const double* wf_params;    // concatenated
    const double* wf_finf;      // [n_wf] F(+inf) per weight function (host-evaluated; 1.0 except for degenerate dagum)
    const double* wf_inv;       // [n_wf] 1 / (the CDF's constant divisor): 1 / sum a_i (hyper_exp), 1 / (x_max - x_min) (uniform, kumaraswamy)
    const uint64_t* tag_pairs;  // sorted, (anchor_tag << 32) | neighbour_tag
    const double* pow_tab;      // Hellinger with exponent e != 2: [2][65536] k^(1/e), k^(-1/e) (context-owned, filled by set_config); else null
};

// SoA structure in HBM.
struct CloudView {
    const double *x, *y, *z;
    const uint8_t* cat;       // low byte of the category id
    const uint8_t* cat_hi;    // high byte (nullptr: every id fits a byte; 255 = not in the category map, with cat_hi: 0xFFFF)
    const int32_t* tag;
    int32_t n;
    const int32_t* sid;   // structure id per atom for a batch of structures (nullptr = one structure)
    int32_t n_struct;     // >= 1
    int32_t struct_size;  // > 0: every structure is exactly this many CONSECUTIVE atoms (frames buffers, regular batches)
};

struct __attribute__((aligned(16))) CellRec {
    double x, y, z;
    uint32_t tag;   // interned tag
    uint32_t cat;   // category id (255 = not in the category map)
};
static_assert(sizeof(CellRec) == 32, "CellRec is read as two 16-byte words");

// One unique anchor, written by k_compact_anchors so that the environment kernel starts from ONE record instead of the
// chain slot -> atom -> coordinates / tag / position.
struct __attribute__((aligned(8))) AnchorRec {
    double x, y, z;
    uint32_t tag;    // interned tag of the anchor
    uint32_t apos;   // its position in cell order
    int32_t sid;     // structure of a batch (0 otherwise)
    uint32_t atom;   // index in the cloud
};

// Uniform grid over one cloud (replaces KdTree::build_by_ordered_float, src/locohd.rs:504-510).
struct GridView {
    double min[3], inv[3];   // cell index = clamp(floor((p - min) * inv), 0, dim-1)
    double cell[3];          // 1 / inv: the cell edge (only used to skip neighbour cells that lie wholly outside the radius)
    int32_t dim[3];          // per structure; cell = ((sid * dim[2] + cz) * dim[1] + cy) * dim[0] + cx
    int32_t n_cells;         // n_struct * dim[0] * dim[1] * dim[2]
    const uint32_t* cell_start;  // [n_cells + 1]
    // points permuted into cell order, one 32-byte record each (two 16-byte loads fetch everything the radius search,
    // the tag filter and the environment need: no dependent second round of loads for the survivors)
    const CellRec* rec;
    const uint32_t* pos_of;      // atom -> its position in cell order (an anchor recognises itself by position)
};

// Sorted environments: env e occupies [e*stride, e*stride + len[e]).
struct EnvStore {
    uint64_t* key;   // f64 distance bit patterns, ascending
    uint8_t* cat;
    int32_t* len;
    int64_t stride;
    int32_t cdf_keys;  // k >= 1: the store holds k SETS of keys, set w = bits of F_w(distance) for weight function w of the configuration (the
                       // sweep needs no CDF evaluation: a pair reads the set of its weight function); 0: keys are the distances
    int32_t cat16;     // 1: `cat` holds 16-bit category ids (more than 255 categories): two bytes per point
    int64_t set_stride;  // elements between two key sets (slots x stride); categories and lengths exist once
    uint64_t* pre;       // prefix-count rows, or null: row j of environment e = pre[(e * stride / kPreStep + j) * pre_words ...] = the category
                         // counts of the environment's first kPreStep * j + 1 sorted points (one row per kPreStep points) as 8-bit fields
                         // (slot c in byte c % 8 of word c / 8), written by k_env_group for configurations of at most 16 categories: the
                         // team sweeps read a chunk's start counts from them -- the row below the chunk's start plus the one-hot fields of
                         // at most kPreStep - 1 category bytes -- instead of building a histogram and a scan per tile (lchd_team_tile.h, PRE)
    int32_t pre_words;   // u64 words per row (1: up to 8 category slots, 2: up to 16, 3: up to 24, 4: up to 32)
    int32_t pad_pre;
    uint8_t* cat0;       // [slots] category of every environment's first (sorted) point, or null: what k_pair_meta puts into the pair records -- one
                         // gather into a small array instead of one into the store itself (k_env_group writes it; the other environment kernels do not)
};
constexpr int kPreStep = 4;  // points per prefix-count row (round 6: every row of round 5's store cost the sweeps one 128-byte line per lane)

// One structure (or batch of structures) of a from_primitives pass as the prologue sees it: the inputs, and the arrays the
// prologue fills (cell list, anchor slots, anchor records).
struct PrepSide {
    CloudView c;
    GridView g;              // geometry; g.cell_start / g.rec / g.pos_of alias the three output arrays below
    uint32_t* cell_start;    // [n_cells + 1]
    CellRec* rec;            // [n] atoms permuted into cell order
    uint32_t* pos_of;        // [n] atom -> position in cell order
    uint32_t *cell_of, *cell_count;  // scratch of the general cell-list build (cell_count [n_cells + 1] inside the zero region)
    uint32_t* scan_tmp;      // (n_cells / 4096 + 4) u32 of scratch for the multi-block scan
    uint8_t* flag8;          // [n rounded up to 32, + 32] one byte per atom: "is an anchor" (inside the zero region, 16-byte aligned)
    uint32_t* bits;          // [(n + 31) / 32 + 1] the same as a bit set (k_prep_scan / k_flags_to_bits)
    uint32_t* wpre;          // [(n + 31) / 32 + 2] anchors before each bit-set word (inside its chunk of 2^18 atoms)
    uint32_t* chunk_base;    // [(n >> 18) + 2] anchors before each chunk
    uint32_t* slot;          // [n + 1] atom -> environment slot (anchors only)
    AnchorRec* uniq;         // [max_envs]
    int32_t no_anchors;      // 1: this side's anchors are neither flagged nor de-duplicated (side B without de-duplication: k_pair_anchor_recs writes an anchor record per PAIR): cell list only
};
// Cell lists of both sides + anchor de-duplication (see lchd_prologue.hip).  [zero_base, zero_base + zero_bytes) is the
// contiguous region holding cell_count of both sides followed by flag8_a, flag8_b (in this order, flag8_b last): the prologue
// zeroes what its launch tier needs with at most one operation.  Returns the number of stream operations enqueued.
// `same`: both sides are one device object -- side B's cell list and slots are not built, the anchors of both columns are
// de-duplicated together into side A's flags / slots / records and n_unique[1] = 0.
// builds_out (optional, two entries): which cell-list build each side took -- 0 none (side B of `same`), 1 fused prologue, 2 one
// workgroup per structure, 3 general build with the one-workgroup scan, 4 general build with the multi-block scan.
// dedup_out (optional, two entries): how each side's anchors get their environment slots -- 0 with side A's (side B of `same`),
// 1 fused prologue (LDS bit set), 2 byte flags + the one-workgroup scan, 3 byte flags + one workgroup per chunk of 2^18 atoms,
// 4 not at all (PrepSide::no_anchors: launch_pair_anchor_recs gives every PAIR a slot).
int launch_prologue(hipStream_t s, const Tuning& t, const int64_t* anchors, int64_t n_pairs, const PrepSide& a, const PrepSide& b,
                    void* zero_base, size_t zero_bytes, DeviceStatus* st, bool same = false, int* builds_out = nullptr,
                    int* dedup_out = nullptr);
// Anchor records of a side without de-duplication (PrepSide::no_anchors), one per PAIR: record p = the side-B anchor of pair p; sets
// DeviceStatus::n_unique[1] = n_pairs.  Behind launch_prologue (reads the side's atom -> position map).
void launch_pair_anchor_recs(hipStream_t s, const int64_t* anchors, int64_t n_pairs, const PrepSide& b, DeviceStatus* st);
// Per-device function attributes (dynamic LDS above 64 KB): called by lchd_ctx_create with the context's device current.
void init_device_kernels();

// returns false if `cap` is not an available variant
// one side of an environment-build launch (both structures are built by ONE launch: workgroups [0, a.max_envs) side A, the rest B)
struct EnvSide {
    CloudView c;
    GridView g;
    const AnchorRec* uniq;
    EnvStore env;
    int64_t max_envs;   // upper bound of the side's unique anchors (the kernel stops at DeviceStatus::n_unique[side])
    double* raw_key;    // environments of more than 16384 points only: [max_envs][cap] unsorted distances ...
    uint8_t* raw_cat;   // ... and categories (k_env_collect -> k_env_rows)
    // Environments that do not fit their slot (k_env_group / k_env_cells): the slot receives the anchor alone (a valid one-point
    // environment, so the sweeps of this pass run cleanly over it) and the slot index is appended here
    // (DeviceStatus::n_overflow[side] counts); the host scores the pairs of these anchors again with larger slots.
    uint32_t* ovf_list;
};
struct EnvSides {
    EnvSide s[2];
};
bool launch_env_cells(hipStream_t s, int cap, const DevConfig* cfg, bool tag_list, const EnvSide& a, const EnvSide& b, double thr,
                      DeviceStatus* st);   // (EnvStore::cat16 of the sides picks the 16-bit-category instantiation: cap <= 16384)
// The default capacity (environments of at most kEnvGroupCap points), several environments per wavefront (lchd_env_group.hip).
// Needs a grid whose cells are at least thr / 2 wide (the search walks the 5 x 5 x 5 neighbourhood), record arrays padded by
// kEnvGroupRecPad records, fewer than 2^29 records per side and environment slots of at least kEnvGroupCap points.
// small_cap: the instantiation for environments of at most kEnvGroupCapSmall points (less LDS, one more wavefront per SIMD).
// (kEnvGroupCap, kEnvGroupCapSmall, kEnvGroupSmallUpTo, kEnvGroupRecPad: lchd_pass_plan.h)
bool launch_env_group(hipStream_t s, const DevConfig* cfg, bool tag_list, bool small_cap, const EnvSide& a, const EnvSide& b, double thr,
                      int anchors_per_wave, DeviceStatus* st);

// dense rows: either distances from coordinates (dmx == nullptr) or given rows (dmx != nullptr, leading dim ld)
struct RowExtras {            // all null for from_coords / from_dmxs
    const uint8_t* row_cat;   // [n_rows][ld] categories of the row's own points (instead of the structure's)
    const int32_t* row_lens;  // [n_rows] points of each row (<= 0: skip the row)
    const uint32_t* n_unique; // rows at or beyond *n_unique do not exist
};
// side: the instantiation (plan_dense_rows_side / lchd_dense_plan::rows, lchd_dense_plan.h); false: it names none, nothing launched
bool launch_env_rows(hipStream_t s, const lchd_dense_rows_side& side, const DevConfig* cfg, const CloudView& c, const double* dmx, int64_t ld,
                     int64_t n_rows, int64_t row_len, double image_bound /* coords: >= largest squared distance, or 0 */, EnvStore env,
                     DeviceStatus* st, const RowExtras& ex = RowExtras{nullptr, nullptr, nullptr});

// The cell of a dense minimum-image call as the kernels take it (by value: it is wave-uniform).
struct MinImageCell { double v[kMinImageRecord]; };  // lchd_cell_reduce.h: reduced cell, inverse, 1.0 if diagonal

// "last workgroup" detection + hand-over through memory-side atomics (lchd_sweep_common.h: last_workgroup_done)
struct DoneState {
    uint32_t ctr[65 * 32];
    uint32_t acc_max[64 * 32];
    unsigned long long acc_sum[64 * 16];
};
// one side of a dense-row launch (lchd_env_rows.hip: k_env_rows2 builds both structures' rows in one launch)
struct RowSide {
    CloudView c;           // categories (and coordinates when dmx == nullptr)
    const double* dmx;     // given distance rows [n_rows][ld], or nullptr: distances from the coordinates of c
    int64_t ld, row_len;
    double image_bound;    // coordinates: >= largest squared distance (bounding-box diagonal^2); ignored for given rows
    EnvStore env;
    const int32_t* row_lens;  // ragged given rows: [n_rows] points of each row (1 .. row_len); nullptr: every row has row_len
};
struct RowSides {
    RowSide s[2];
    int64_t n_rows;
};
// both sides in one launch of the plan's k_env_rows2<nt, ept, seg> (path LCHD_DENSE_ROWS2); false: the plan names no instantiation
bool launch_env_rows2(hipStream_t s, const lchd_dense_plan& plan, const DevConfig* cfg, const RowSide& a, const RowSide& b, int64_t n_rows,
                      DeviceStatus* st);

// Dense rows, sort and sweep fused (lchd_dense_fused.hip): one workgroup per row pair, only the score is written.
// Applies to Hellinger-2 with unit category weights, at most 16 categories and rows of kDenseFusedMinRow < n <= kDenseFusedMaxRow points
// (lchd_dense_plan.h: plan_dense decides, launch_dense_fused follows lchd_dense_plan::fused_slots / fused_dmx).
struct DenseSide {
    CloudView c;              // categories (and coordinates when dmx == nullptr)
    const double* dmx;        // given distance rows [n_rows][ld], or nullptr
    int64_t ld;
    int32_t row_len;          // points per row
    const int32_t* row_lens;  // ragged given rows: [n_rows] points of each row (1 .. row_len), or nullptr
};
struct DenseArgs {
    const DevConfig* cfg;
    DenseSide s[2];
    int64_t n_rows;
    double image_bound;       // coordinates: >= the largest squared distance of either structure; ignored for given rows
    const int32_t* wf_index;  // [n_rows] or nullptr => 0
    double* out;
    DeviceStatus* st;
    const double* sqrt_tab;   // [65536] sqrt(k), context-owned
    // scratch of the distance pass: workgroup w keeps the (key, value) pairs of distance segment s of its CURRENT row pair at
    // [(w * scr_segs + s) * dense_fused_seg_cap() ...); dense_fused_scratch() sizes both arrays and sets scr_segs / scr_grid
    uint64_t* scr_key;
    uint8_t* scr_val;
    int32_t scr_segs, scr_grid;
    unsigned long long* ticket;  // context-owned: rows handed out beyond the first one of every workgroup (zero between launches)
};
// workgroups of a launch of n_rows row pairs with the plan's scr_segs segments per workgroup; returns the ENTRIES of either scratch array
size_t dense_fused_scratch(int64_t n_rows, int32_t scr_segs, int32_t* grid_out);
// returns false (nothing launched) when the plan or the arguments are not the kernel's; otherwise the kernel and the status hand-over are enqueued
bool launch_dense_fused(hipStream_t s, const lchd_dense_plan& plan, const DenseArgs& a, HostStatus* hst, uint32_t seq);
void init_dense_fused_kernels();  // per device (dynamic LDS above 64 KB), called by lchd_ctx_create

struct SweepArgs {
    const DevConfig* cfg;
    EnvStore env_a, env_b;
    const int64_t* anchors;   // [P][2] or nullptr => pair p uses env (p, p)
    const uint32_t* slot_a;   // anchor index -> env slot (nullptr with anchors == nullptr)
    const uint32_t* slot_b;   // (nullptr with anchors != nullptr: side B's slot of pair p is p -- side B without de-duplication)
    int64_t n_slot_a, n_slot_b;  // atoms per side (bounds for the anchor indices)
    const int32_t* wf_index;  // [P] or nullptr => 0
    int64_t n_pairs;
    double* out;
    DeviceStatus* st;
    const double* sqrt_tab;   // [65536] sqrt(k), context-owned
    const double* rsqrt_tab;  // [65536] 1/sqrt(k)
    int4* meta;               // [P] workspace: per-pair records written by k_pair_meta, read by the sweep kernels
    DoneState* done;          // context-owned, zero between kernels: "last workgroup" counters and accumulators
    unsigned char* wide_scratch;      // more than kWideCategories categories (k_sweep_wide<.., HUGE>): context-owned global-memory block,
    int64_t wide_scratch_per_wave;    //   bytes per workgroup (wide_scratch_bytes_per_wave(C)),
    int32_t wide_scratch_waves;       //   workgroups it serves (= the grid of that launch)
    HostStatus* hst;          // host-mapped mirror (snapshot by k_pair_meta, error words by the sweep kernels)
    uint32_t seq;             // pass counter echoed into HostStatus::snapshot_seq
    int32_t duo_enabled;      // set by launch_sweep: k_sweep_duo was launched too and sweeps the small pairs when they are the majority
    int32_t small_rule;       // set by launch_sweep: which pairs count as "small" (0: <= kDuoTile merged events, k_sweep_duo; 1: both
                              // environments <= 255 points, the 8-bit-count k_sweep; 2: ... and at most 480 merged events, its
                              // two-pairs-per-wavefront form); the indirect k_sweep takes the others
    int32_t c8_rule;          // set by launch_sweep: the rule (1 or 2) HostStatus::n_c8 is counted under
    int32_t second_rule;      // set by launch_sweep: 0, or the rule of the second small-pair kernel a pass without a hint launched
    int32_t gen_tab;          // set by launch_sweep: MODE_GEN may use power tables (Hellinger with a general exponent, unit category weights)
    int32_t forced;           // set by launch_sweep: the host picked the sweep kernels (hint from the previous pass): no device-side decision
    int32_t sd_fast;          // the configuration qualifies for k_sweep_inc (lchd_sweep_inc.hip): 0 no, 1 Kullback-Leibler form, 2 Renyi form
    // Leftover list (round 6): in a pass whose sweep kernels the host picked (forced: the rule is known at launch) k_pair_meta appends
    // the pairs the team kernel's rule leaves over to left_list (wave-aggregated, a handful of atomics per launch) and the INDIRECT
    // companion walks that list instead of scanning every pair record for them (C2a: 223 of 10^6 pairs; 16.6 -> ~3 us per pass).
    // Two counter slots take turns: the pass that appends to one zeroes the other for the next pass -- no memset, no reset kernel.
    uint32_t* left_list;      // [P] workspace (nullptr: no list, the companion scans the records)
    uint32_t* left_count;     // this pass's counter slot (zero when the pass starts)
    uint32_t* left_zero;      // the other slot: zeroed by k_pair_meta of this pass
    int32_t left_listing;     // set by launch_sweep: k_pair_meta appends and the companion reads the list
    int64_t left_expected;    // pairs the previous pass of the context left over (sizes the companion's grid; any grid is correct)
};
// sweep_hint: SweepHintBits (lchd_pass_plan.h), what k_pair_meta counted in the previous pass of this configuration.  Returns what the
// caller's bookkeeping needs (SweepLaunched); !ok: nothing was launched.
// plan_sweep is the decision alone (lchd_plan_sweep); launch_sweep launches what it returns and, if asked, hands the plan back.
bool plan_sweep(const lchd_sweep_query& q, lchd_sweep_plan& p);  // false: the set would not give every pair exactly one kernel (unreachable); launch_sweep then launches nothing
SweepLaunched launch_sweep(hipStream_t s, const Tuning& t, int n_categories, bool hellinger2, bool unit_weights, bool wf_pow, int sweep_hint,
                           const SweepArgs& a, lchd_sweep_plan* plan_out = nullptr);
// Kullback-Leibler / Renyi in O(1) per event (lchd_sweep_inc.hip): unit weights, CDF-keyed environments of at most 512 points, tiny eps;
// reads the pair records of k_pair_meta.  kind: SweepArgs::sd_fast.
void launch_sweep_inc(hipStream_t s, int kind, int cmax, const SweepArgs& a);
// trajectory frames: replicate the template's labels / unpack [frames][atoms][3] into SoA + bounding box keys
void launch_frames_labels(hipStream_t s, const uint8_t* tcat, const int32_t* ttag, int64_t n_tmpl, int32_t n_frames, uint8_t* cat,
                          int32_t* tag, int32_t* sid);
void launch_frames_unpack(hipStream_t s, const double* raw, int64_t n_atoms, double* x, double* y, double* z,
                          unsigned long long* bbox7);
// primitive atoms of every frame = float32 centroids of their source atoms (CSR src_start / src_idx), widened to f64
// tiles: [n_tiles][4] = {first primitive, end primitive, first source atom, end source atom} with a span of at most
// centroid_tile_span() source atoms, or {p0, p1, -1, -1} for a primitive range that is gathered from global memory
void launch_frames_centroids(hipStream_t s, const float* raw, int64_t n_src, const int32_t* src_start, const int32_t* src_idx,
                             const int32_t* tiles, int n_tiles, int64_t n_prim, int32_t n_frames, double* x, double* y, double* z,
                             unsigned long long* bbox7, unsigned long long* bbox_part /* [bbox_parts_capacity()][7] */);
int centroid_tile_span();
int bbox_parts_capacity();
// Periodic images of a cloud as a cloud (lchd_images.hip): the wrapped originals in slots 0 .. n - 1, their ghosts behind them.
constexpr int kImgScanSpan = 256;  // atoms per workgroup of the three steps = items one workgroup of the scan covers
constexpr int kImgCellRecord = 21;  // doubles per triclinic cell on the device: cell, inverse, widths
struct ImageArgs {
    CloudView src;              // the source (cat: the low bytes, cat_hi: the high bytes or null)
    const uint8_t* src_narrow;  // with cat_hi: the source's one-byte view
    const double* boxes;        // DEVICE [n_boxes][3] box edges; n_boxes == 1: one box for every structure, else box[sid]
    int32_t n_boxes;
    const double* cells;        // triclinic cells instead of boxes: DEVICE [n_boxes][kImgCellRecord] = cell (9, row-major, row 0 = a),
                                // its inverse (9), the perpendicular widths (3); indexed like `boxes`.  Null: an orthorhombic box, `boxes` is set
    double reach;               // an image within `reach` of the box is materialised (threshold <= reach <= smallest edge / width)
    double *x, *y, *z;          // the image cloud's arrays, `capacity` atoms each
    uint8_t *cat, *cat_hi, *cat_narrow;
    int32_t *tag, *sid;         // (sid null: one structure)
    int64_t capacity;
    uint32_t* count;            // [n] ghosts per atom
    uint32_t* offset;           // [n] ghosts of the atom's span in front of the atom
    unsigned long long* span_sum;  // [spans] ghosts in front of each span of kImgScanSpan atoms, or null: n <= kImgScanSpan
    unsigned long long* bbox;   // [8]: the seven bounding-box words of a frames buffer (ordered keys, non-finite flag), then the ghost total
};
// (count and emit pick the triclinic kernels when a.cells is set)
void launch_img_count(hipStream_t s, const ImageArgs& a);  // wrapped originals, counts, bounding box (of originals and ghosts)
void launch_img_scan(hipStream_t s, const ImageArgs& a);   // offsets, span sums, total
void launch_img_emit(hipStream_t s, const ImageArgs& a);   // the ghosts
// The way back from a slot of a built image cloud to its source atom (k_img_origin): origin[o] = the source atom (origin[i] = i for the
// wrapped originals), code[o] = its image code (0: an original).  Reads only what the build left in the image cloud: `a` as the build
// filled it, with src.n = the source atoms and src.sid = the image cloud's own structure ids; capacity bounds origin / code.
void launch_img_origin(hipStream_t s, const ImageArgs& a, int32_t* origin, int8_t* code);
void launch_fill_sqrt_tables(hipStream_t s, double* sqrt_tab, double* rsqrt_tab);  // 65536 entries each
void launch_fill_pow_tables(hipStream_t s, double* tab /* [2][65536] */, double exponent);  // k^(1/e), k^(-1/e)

// Multi-GPU sharding of an anchor-pair list by anchor bins (see lchd_kernels.hip).  ShardState lives in device memory,
// zero-initialised once; hist / hist_b / cursor / done are zero again after every plan.
constexpr int kShardBins = 1024, kShardMaxWorld = 64;
struct ShardState {
    uint32_t hist[kShardBins], hist_b[kShardBins];
    uint16_t rank_of_bin[kShardBins];
    int32_t mode, pad;   // key side of the last plan: 0 side-A anchor, 1 side-B anchor, 2 pair index
    int64_t counts[kShardMaxWorld];
    unsigned long long cursor;
    DoneState done;
};
struct ShardCounts {
    int64_t n[kShardMaxWorld];
};
void launch_shard_plan(hipStream_t s, const int64_t* anchors, int64_t n_pairs, int64_t n_atoms_a, int64_t n_atoms_b /* <= 0: unknown */,
                       int world, ShardState* st, int64_t* counts_host /* host-mapped [kShardMaxWorld + 1]: counts, then the key side */);
void launch_shard_select(hipStream_t s, const int64_t* anchors, int64_t n_pairs, int64_t n_atoms_a, int64_t n_atoms_b, int rank, int world,
                         ShardState* st, int64_t* sel_anchors, int64_t* sel_index);
// The pairs of a finished pass that touch an overflowed environment (EnvSide::ovf_list), in list order: lchd_ctx_finish scores
// them again with larger slots.  wave_count: kOverflowWaves words of scratch.
constexpr int kOverflowWaves = 4096;
struct OverflowSelect {
    const int64_t* anchors;
    int64_t n_pairs;
    const uint32_t *slot_a, *slot_b;   // atom -> environment slot of the finished pass
    const uint32_t *bits_a, *bits_b;   // bit sets over the slots (launch_mark_overflow)
    const int32_t* wf;                 // per-pair weight-function index or null
    unsigned long long* wave_count;
    int64_t *sel_index, *sel_anchors;  // [n], [n][2]
    int32_t* sel_wf;
};
void launch_env_key_sets(hipStream_t s, const DevConfig* cfg, const EnvStore& ea, const EnvStore& eb, int n_sets, int64_t max_envs, const DeviceStatus* st);
// deterministic mode: the categories of every run of equal keys in ascending order, one wavefront per environment;
// st != nullptr (from_primitives): the environments in use are DeviceStatus::n_unique (n_a / n_b bound the launch), otherwise exactly
// n_a / n_b; position 0 takes part (EnvStore::cat0, where there is one, follows it)
void launch_env_canon(hipStream_t s, const EnvStore& ea, const EnvStore& eb, int64_t n_a, int64_t n_b, const DeviceStatus* st);
// Local composition profiles (lchd_profile.hip): one row of n_categories doubles per entry, from a store whose keys are F values.
constexpr int kProfMaxPoints = 65536;  // points of an environment the profile kernel takes (its chunk carries live in LDS)
struct ProfileArgs {
    const DevConfig* cfg;
    EnvStore env;              // cdf_keys >= 1: entry p reads key set wf_index[p]
    const int64_t* anchors;    // [n] atom indices, or nullptr: entry p is environment p (dense rows)
    const uint32_t* slot;      // atom -> environment slot (with anchors)
    int64_t n_atoms;           // bound of the atom indices
    const int32_t* wf_index;   // [n] or nullptr => 0
    const int64_t* out_row;    // [n] output row of entry p, or nullptr: row p
    int64_t n;
    double* out;               // [rows][n_categories]
    int32_t n_categories;      // DevConfig::n_categories (the launcher sizes the LDS with it)
    HostStatus* hst;           // host-mapped mirror: ST_BAD_WF is reported there
};
void launch_profile(hipStream_t s, const ProfileArgs& a);
void launch_profile_pairs(hipStream_t s, const int64_t* anchors, int64_t n, int64_t* pairs);  // pairs[p] = (anchors[p], anchors[p])
void launch_profile_rows(hipStream_t s, DeviceStatus* st, int64_t n_rows);  // DeviceStatus::n_unique = (n_rows, 0)
// the end of a pass that has no record pass: status words into the host-mapped mirror, device status reset (publish_status)
void launch_profile_publish(hipStream_t s, DeviceStatus* st, HostStatus* hst, uint32_t seq);
// Radial score profiles (lchd_radial.hip): a pair's integrand resolved over distance bins, one row of n_bins doubles per pair, from
// stores whose keys are F values.  The pair list, the stores, the records and the status words travel in a SweepArgs, as for a sweep.
constexpr int kRadialMaxPoints = 65535;  // points of an environment or row (the 16-bit count fields; the 16-bit-category pair record)
struct RadialEdges {                     // the caller's edges e_0 < ... < e_K, by value (lchd_radial_bins.h: kRadialMaxBins + 1 of them at most)
    double e[65];
    int32_t n;
};
struct RadialArgs {
    SweepArgs sw;         // cfg, env_a / env_b (cdf_keys >= 1), anchors / slots, wf_index, n_pairs, meta, sqrt tables, st / hst / seq / done; out unused
    const double* bounds; // [n_wf][n_bins + 1] E_k = F_w(e_k), written by launch_radial_bounds
    int32_t n_bins;
    int32_t n_categories; // DevConfig::n_categories (the launcher sizes the LDS with it)
    double* out;          // [n_pairs][n_bins]
};
void launch_pair_meta(hipStream_t s, const SweepArgs& a);  // k_pair_meta alone (lchd_kernels.hip): the records, the counts, the status hand-over
void launch_radial_bounds(hipStream_t s, const DevConfig* cfg, int n_wf, const RadialEdges& edges, double* bounds);
bool launch_radial(hipStream_t s, bool hellinger2_unit, const RadialArgs& a);  // false: nothing launched (more than kWideCategories categories)
void init_radial_kernels();  // per device (dynamic LDS above 64 KB), called by init_device_kernels
// Score attribution by category (lchd_attribution.hip): a pair's score split over the categories (Hellinger distances only), one row of
// n_categories doubles per pair, from the stores and records a radial call reads.
constexpr int kAttributionMaxCategories = 64;  // (the per-lane accumulator columns, 512 bytes per category and wavefront, live in LDS)
struct AttributionArgs {
    SweepArgs sw;          // as RadialArgs::sw
    int32_t n_categories;  // DevConfig::n_categories (the launcher sizes the LDS with it)
    double* out;           // [n_pairs][n_categories]
};
// false: nothing launched (more than kAttributionMaxCategories categories, 16-bit category stores)
bool launch_attribution(hipStream_t s, bool exponent2, bool unit_weights, const AttributionArgs& a);
void init_attribution_kernels();  // per device, as init_radial_kernels
// Category-weight gradients (lchd_category_gradient.hip): dS/dw_c of a pair's score (Hellinger and Kullback-Leibler distances), one row
// of n_categories doubles per pair, from the stores and records an attribution call reads; at most kAttributionMaxCategories categories.
struct CategoryGradientArgs {
    SweepArgs sw;          // as RadialArgs::sw
    int32_t n_categories;  // DevConfig::n_categories (the launcher sizes the LDS with it)
    double* out;           // [n_pairs][n_categories]
};
// false: nothing launched (another distance, more than kAttributionMaxCategories categories, 16-bit category stores)
bool launch_category_gradient(hipStream_t s, int sd_kind, bool exponent2, const CategoryGradientArgs& a);
void init_category_gradient_kernels();  // per device, as init_radial_kernels
// Neighbour sensitivities (lchd_sensitivity.hip): dS/dd of every member of a pair's two environments, and the score, from INDEXED
// environment lists -- (distance, atom index, category) per point, ascending by (distance bits, atom index), the anchor first -- built
// next to the scoring stores of the pass from the same cell lists and anchor records.
constexpr int kSensitivityMaxCategories = 64;  // (tested up to here; the count columns of a wavefront, 260 bytes per category, live in LDS)
struct IndexedStore {
    double* dist;      // [slots][stride]
    uint32_t* idx;     // [slots][stride] atom index in the cloud
    uint8_t* cat;      // [slots][stride] category (255: not in the map)
    int32_t* len;      // [slots] points incl. the anchor; 1 (the anchor alone) for a list that did not fit, 0 for an empty one
    int64_t stride;    // a power of two, at most kRadialMaxPoints + 1
};
struct IndexedSide {
    GridView g;              // the pass's cell list of the side
    const AnchorRec* uniq;   // its anchor records
    int64_t max_envs;        // slots (0: side B of a pass whose two sides are one object)
    int32_t n;               // atoms
    uint32_t* atom_of;       // [n] workspace: cell-order position -> atom (written by the launch)
    IndexedStore env;
};
struct IndexedArgs {
    const DevConfig* cfg;
    IndexedSide s[2];
    double thr;
    int32_t reach;           // PassPlan::reach: the cell neighbourhood walked
    int32_t tag_list;        // PassPlan::tag_list
    const DeviceStatus* st;  // n_unique: the slots in use
};
bool launch_env_indexed(hipStream_t s, const IndexedArgs& a);  // false: nothing launched (a stride that is no power of two)
// The indexed lists of DENSE rows (k_rows_indexed): slot r of a side = row r of its distance matrix (given rows, or distances from the
// side's coordinates in the expression of k_env_rows), every column a member, sorted ascending by (distance bits, column index) -- the
// reference's stable co-sort of a row with seq (utils.rs:25-39).  No forced anchor: slot 0 is the first of that order.  The row checks
// are k_env_rows' (ST_BAD_DISTANCE, ST_FIRST_NOT_ZERO, ST_BAD_CATEGORY into DeviceStatus::flags: launch it in front of the record pass).
// Rows of at most kRowsIdxLdsPoints (padded) points are sorted in LDS, 12 bytes per point -- only (key, column) pairs travel through
// the sort, the category is gathered from the column behind it -- longer ones, up to kRadialMaxPoints, in place in the list block.  The
// in-place path is a correctness path: every compare-exchange of the network goes through L2.  Measured on the MI355X (512 rows a side):
// 0.127 ns per point at the capacity, 0.498 ns one point over it -- 3.9x, of which 2.3x is the network of the next power of two -- and
// 0.352 ns at 16 384 points: well inside an order of magnitude ("Dense sensitivities").
constexpr int kRowsIdxLdsPoints = LCHD_SENSITIVITY_ROWS_LDS_POINTS;  // 8192: 96 KB of the 160 KB of a CU (the public header exports it)
struct RowsIndexedSide {
    CloudView c;          // categories (and coordinates when dmx == nullptr)
    const double* dmx;    // DEVICE rows [rows][ld], or nullptr: distances from the coordinates of c (row r seen from atom r)
    int64_t ld;
    int32_t cols;         // points of every row, 1 .. kRadialMaxPoints
    IndexedStore env;     // [rows] slots of `stride` points, stride a power of two >= cols
};
struct RowsIndexedArgs {
    const DevConfig* cfg;
    RowsIndexedSide s[2];
    int64_t rows;         // of each side: workgroups [0, rows) build side A, the rest side B
    DeviceStatus* st;
};
bool launch_rows_indexed(hipStream_t s, const RowsIndexedArgs& a);  // false: nothing launched (a stride that is no power of two or below cols)
struct SensitivityOut {      // all DEVICE; K = SensitivityArgs::width
    double* scores;          // [P]
    int32_t *count_a, *count_b;        // [P] members incl. the anchor (0: an unusable pair)
    int32_t *idx_a, *idx_b;            // [P][K], padded with -1
    double *dist_a, *dist_b, *g_a, *g_b;  // [P][K], padded with 0
    // launch_sens_resolve (both) and launch_sens_min_image_disp (disp alone), null otherwise: the image code of every member and its
    // displacement from the anchor / the row's atom
    double *disp_a, *disp_b;           // [P][K][3], padded with 0
    int8_t *image_a, *image_b;         // [P][K], padded with 0
};
struct SensitivityArgs {
    SweepArgs sw;            // as RadialArgs::sw; the stores only through the pair records
    IndexedStore env_a, env_b;
    int32_t n_categories;    // DevConfig::n_categories (the launcher sizes the LDS with it)
    int32_t width;           // K
    SensitivityOut out;
};
bool launch_sensitivity(hipStream_t s, const SensitivityArgs& a);  // false: nothing launched (more than kSensitivityMaxCategories categories)
void init_sensitivity_kernels();  // per device, as init_radial_kernels
// Weight-function gradients (lchd_weight_gradient.hip): dS/dtheta_k for every parameter of the pair's weight function, and the score, from
// the indexed lists and pair records a sensitivity call reads.  Row p of grad holds the derivatives in the function's parameter order;
// the columns behind its n_params are exact zeros.
constexpr int kWeightGradientMaxParams = 16;  // (per-lane register accumulators: hyper_exp up to 8 components, and every other family)
struct WeightGradientArgs {
    SweepArgs sw;            // as SensitivityArgs::sw
    IndexedStore env_a, env_b;
    int32_t n_categories;    // DevConfig::n_categories (the launcher sizes the LDS with it)
    int32_t width;           // NP: columns of a row, the most parameters of any function of the dictionary, 1 .. kWeightGradientMaxParams
    double* scores;          // [P]
    double* grad;            // [P][NP]
};
// false: nothing launched (more than kSensitivityMaxCategories categories, a width outside 1 .. kWeightGradientMaxParams)
bool launch_weight_gradient(hipStream_t s, const WeightGradientArgs& a);
void init_weight_gradient_kernels();  // per device, as init_radial_kernels
// Behind launch_sensitivity on lists that index image clouds (k_sens_resolve_images): per member slot the displacement from the anchor in
// the cloud the list indexes, the image code, and -- in place -- the source atom instead of the cloud index.
struct SensResolveSide {
    const double *x, *y, *z;   // the cloud the side's lists index (an image cloud: wrapped originals, then ghosts)
    int64_t n;                 // its atoms
    const int32_t* origin;     // [n] launch_img_origin's map, or null: not an image cloud (idx stays, image = 0)
    const int8_t* code;        // [n] with origin
    int32_t* idx;              // [P][K] in: cloud indices (-1: padding), out: source atoms
    int8_t* image;             // [P][K] out
    double* disp;              // [P][K][3] out
};
struct SensResolveArgs {
    SensResolveSide s[2];
    const int64_t* anchors;    // [P][2] the pair list of the pass
    int64_t n_pairs;
    int32_t width;             // K
};
bool launch_sens_resolve(hipStream_t s, const SensResolveArgs& a);  // false: nothing launched (more slots than a grid covers)
// Behind launch_sensitivity on the lists of dense rows from coordinates (k_sens_min_image_disp): per member slot of row r the
// displacement from atom r to the member -- in a periodic cell to the member's nearest image, the vector behind the row's minimum-image
// distance (lchd_min_image.h), on an open side x[member] - x[r] -- so that sqrt((dx dx + dy dy) + dz dz) of it is dist bit for bit.
struct SensDispSide {
    const double *x, *y, *z;   // the side's coordinates
    int64_t n;                 // its atoms (rows and members are checked against it)
    const int32_t* idx;        // [rows][K] members (-1: padding)
    double* disp;              // [rows][K][3] out
    MinImageCell cell;         // kind != 0: the reduced cell of the side
    int32_t kind;              // 0 open, 1 a diagonal cell (the per-axis form), 2 any other cell (the 27 shifts)
};
struct SensDispArgs {
    SensDispSide s[2];
    int64_t rows;
    int32_t width;             // K
};
bool launch_sens_min_image_disp(hipStream_t s, const SensDispArgs& a);  // false: nothing launched (more slots than a grid covers)
// Cross-scoring (lchd_cross.hip): the pair records of one row tile -- anchors_a[row0 .. row0 + rows) against all n_b anchors of B, pair
// p = i * n_b + j -- written on the device in the [P][2] int64 form the thresholded pass reads, with the constant wf index when wf >= 0
// (wf_out is not touched otherwise); and the reduction of a tile's [rows][n_b] scores to the k smallest (score, column) per row, ascending.
// rows * n_b <= 2^31 - 1; 1 <= k <= min(n_b, kNearestMaxK).
void launch_cross_pairs(hipStream_t s, const int64_t* anchors_a, const int64_t* anchors_b, int64_t row0, int64_t rows, int64_t n_b, int32_t wf,
                        int64_t* pairs, int32_t* wf_out);
void launch_nearest_rows(hipStream_t s, const double* scores, int64_t rows, int64_t n_b, int32_t k, double* out_scores, int32_t* out_cols);
// Native coordinate gradients (lchd_gradient.hip): the sensitivity lists of one tile of pairs, in the layouts k_sensitivity writes, added
// into exact fixed-point accumulators (lchd_exact_sum.h: LCHD_GRAD_LIMBS int64 limbs per atom and component), and their rounding to doubles.
struct GradSide {
    const int32_t* idx;        // [P][K] members (-1: padding)
    const double *dist, *g;    // [P][K]
    const double* disp;        // [P][K][3] the members' displacements, or null: x[member] - x[anchor] from the coordinates below
    const double *x, *y, *z;   // the side's coordinates (not read with disp)
    int64_t n;                 // its atoms (anchors and members are checked against it)
    int64_t* acc;              // [n][3][LCHD_GRAD_LIMBS]
};
struct GradAccumArgs {
    GradSide s[2];
    const double* weights;     // [P] pair weights of the tile, or null: 1.0
    int64_t n_pairs;           // P
    int32_t width;             // K
    int32_t dense;             // 0: the anchor of pair p is idx[p][0]; 1: dense rows, the anchor of row p is atom p
    uint32_t* flag;            // LCHD_XS_OUT_OF_RANGE is ORed into it
};
bool launch_grad_accumulate(hipStream_t s, const GradAccumArgs& a);  // false: nothing launched (a null array, a side shorter than its rows)
bool launch_grad_finish(hipStream_t s, int64_t* acc, int64_t n_atoms, double* grad);  // grad [n_atoms][3]; zeroes acc
// The strain derivative of the same lists (k_strain_accumulate; every side needs `disp`): six exact sums per side, acc [2][6][LCHD_GRAD_LIMBS]
// with side A first.  The grid does not grow with the pair count: at most kStrainMaxBlocks workgroups of four wavefronts, each wavefront
// on one side, so at most 2 kStrainMaxBlocks wavefronts per side add their 48 limb totals once.
constexpr int kStrainMaxBlocks = 512;
bool launch_strain_accumulate(hipStream_t s, const GradAccumArgs& a, int64_t* acc);  // false: nothing launched (a null array, no disp)
bool launch_strain_finish(hipStream_t s, int64_t* acc, double* strain_a, double* strain_b);  // strain [9] row-major each; zeroes acc
// Reduced parameter gradients (lchd_param_sum.hip): the rows of one tile of a per-pair parameter-gradient call times the pair weights,
// added into exact accumulators acc [n_buckets][width][LCHD_GRAD_LIMBS].  The grid does not grow with the pair count: at most
// kParamSumMaxBlocks workgroups of four wavefronts (max_blocks > 0: at most that many, the LCHD_PARAM_SUM_BLOCKS hook).
constexpr int kParamSumMaxBlocks = 512;
constexpr int kParamSumMaxWidth = 64;  // columns of a row: the categories of a category gradient, the parameters of a weight gradient
struct ParamSumArgs {
    const double* rows;        // [P][ld], the first `width` columns of a row are summed; a NaN in column 0: the pair adds nothing
    const double* weights;     // [P] pair weights of the tile, or null: 1.0
    const int32_t* bucket;     // [P] the pair's bucket (its weight-function index), or null: every pair adds to bucket 0
    const double* scores_in;   // [P] the tile's scores, copied to scores_out [P]; both or neither
    double* scores_out;
    int64_t* acc;
    uint32_t* flag;            // LCHD_XS_OUT_OF_RANGE is ORed into it
    int64_t n_pairs, ld;       // P, the leading dimension of rows
    int32_t width, n_buckets;
    int32_t width_pow2;        // (set by the launcher)
};
bool launch_param_accumulate(hipStream_t s, const ParamSumArgs& a, int max_blocks);  // false: nothing launched (a null array, a bad shape)
bool launch_param_finish(hipStream_t s, int64_t* acc, int64_t n, double* out);       // out [n]; zeroes acc
void launch_mark_overflow(hipStream_t s, const uint32_t* list_a, uint32_t na, const uint32_t* list_b, uint32_t nb, uint32_t* bits_a, uint32_t* bits_b);
void launch_count_overflow(hipStream_t s, const OverflowSelect& a, unsigned long long* total);
void launch_write_overflow(hipStream_t s, const OverflowSelect& a);
void launch_scatter_scores(hipStream_t s, const double* scores, const int64_t* index, int64_t n, double* out);
void launch_unshard_scores(hipStream_t s, const double* gathered, const ShardCounts& counts, int world, int64_t stride, double* out,
                           int64_t n_pairs, uint32_t* bad);
void launch_env_points(hipStream_t s, const SweepArgs& a, unsigned long long* out);
// Dense ensemble call (lchd_ensemble.hip).  Distance rows [n_rows][n] of the consecutive n-atom structures that start at atom
// atom0 of c (row k * n + r: atom r of structure k), the excluded entries (CSR over the n rows of a structure, or null) +inf.
void launch_ens_dist(hipStream_t s, const CloudView& c, int64_t atom0, int32_t n, int64_t n_rows, const int32_t* excl_start,
                     const int32_t* excl_idx, double* dmx);
// The same rows in a periodic cell (minimum image).  `one`: the cell of every structure, or d_recs: DEVICE [structures][kMinImageRecord],
// indexed by atom0 / n + the structure's position in the launch.  all_diagonal: every cell is diagonal (the orthorhombic kernel).
void launch_min_image_rows(hipStream_t s, const CloudView& c, int64_t atom0, int32_t n, int64_t n_rows, const MinImageCell& one,
                           const double* d_recs, bool all_diagonal, const int32_t* excl_start, const int32_t* excl_idx, double* dmx);
void launch_ens_iota(hipStream_t s, uint32_t* slot, int64_t n);
// plan[k] = {slot of structure i, slot of structure j, output pair, 0}: record k * n + r = (slot_i * n + r, slot_j * n + r),
// weight function wf[r] (wf / wf_rec null: all 0); the scatter puts score k * n + r at out[plan[k].z * n + r]
void launch_ens_records(hipStream_t s, const int4* plan, int64_t n_plan, int32_t n, const int32_t* wf, int64_t* anchors, int32_t* wf_rec);
void launch_ens_scatter(hipStream_t s, const double* scores, const int4* plan, int64_t n_plan, int32_t n, double* out);
// from_anchors on lists whose distances do not ascend: the reference's loop walked literally by one lane (lchd_sweep.hip)
void launch_anchors_literal(hipStream_t s, const DevConfig* cfg, int n_categories, const EnvStore& ea, const EnvStore& eb, int nA, int nB, int wfi,
                            double* out);

}  // namespace lchd
