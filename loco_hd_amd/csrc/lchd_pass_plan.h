// lchd_pass_plan.h -- the decisions of one thresholded from_primitives pass as pure host functions: what a pass will look like
// (plan_pass), what to do once it has finished (pass_verdict) and what the context remembers for the next one (hints_after_pass,
// hints_for_repeat).  No context, no device, no pointer into device memory, no HIP header: plain structs in, plain structs out
// (tests/test_pass_plan.py compiles this file with the host compiler alone).  lchd_device.h includes it; lchd_capi.hip joins the
// decisions to the arena and the launches (prims_enqueue, finish_passes).
#pragma once
#include <stdint.h>

#include <algorithm>

namespace lchd {

constexpr int kMaxCategories = 255;   // categories travel as u8 on the device ...
// The default capacity (environments of at most kEnvGroupCap points), several environments per wavefront (lchd_env_group.hip).
// small_cap: the instantiation for environments of at most kEnvGroupCapSmall points (less LDS, one more wavefront per SIMD).
constexpr int kEnvGroupCap = 512, kEnvGroupCapSmall = 320, kEnvGroupSmallUpTo = 288, kEnvGroupRecPad = 8;
constexpr int kMaxKeySets = 4;  // weight-function dictionaries of up to 4 entries get one key set each (k_env_group); larger ones keep distance keys
// u64 words of a prefix-count row that the team sweep of `cmax` category slots reads: TeamTile<CM>::NW of the instantiation launch_team
// picks (8, 12 / 16 slots); 0: no instantiation reads rows (k_env_group's writer handles up to four words)
inline int team_pre_words(int cmax) { return cmax <= 8 ? 1 : (cmax <= 16 ? 2 : 0); }

// status word written by kernels (device memory, zeroed per call)
enum : uint32_t {
    ST_BAD_ANCHOR = 1u << 0,      // anchor index outside the cloud            (reference: panic, :521)
    ST_EMPTY_ENV = 1u << 1,       // environment without any point              (reference: panic, :74)
    ST_FIRST_NOT_ZERO = 1u << 2,  // sorted dists[0] != 0                       (reference: ValueError, :74-77)
    ST_BAD_CATEGORY = 1u << 3,    // category id outside [0, C)                 (reference: ValueError, pmf.rs:38-42)
    ST_ENV_OVERFLOW = 1u << 4,    // environment larger than the kernel variant's LDS capacity (retry bigger)
    ST_ZERO_NORM = 1u << 5,       // PMF norm 0                                 (reference: ValueError, pmf.rs:70-76)
    ST_BAD_DISTANCE = 1u << 6,    // negative / NaN distance in a matrix row    (reference: ValueError / panic)
    ST_BAD_WF = 1u << 7,          // weight-function index outside the table
    ST_ROW_RETRY = 1u << 8,       // a dense row of more than 16384 points defeated the segmented sort: repeat the call with k_env_rows
};
// Host-mapped (pinned, device-visible) mirror of DeviceStatus (lchd_device.h): written with plain stores only -- the snapshot by one
// thread of k_pair_meta, the error words by whichever sweep wavefront meets the (rare) condition; every writer of a word stores the
// same value.
struct HostStatus {
    uint32_t flags;          // DeviceStatus::flags at the end of the record pass (everything the kernels before the sweep reported)
    uint32_t max_env;
    uint32_t n_unique[2];
    unsigned long long n_small;
    uint32_t sweep_flags[8]; // word k != 0 <=> a sweep kernel reported status bit k (ST_* above)
    uint32_t snapshot_seq;   // pass counter written with the snapshot (the host checks that the pass it waited for got this far)
    uint32_t pad;
    unsigned long long n_duo, n_c8;  // pairs of at most kDuoTile merged events / with both environments <= 255 points (both always counted)
    uint32_t n_overflow[2];  // DeviceStatus::n_overflow at the end of the record pass
    uint32_t max_bound;      // DeviceStatus::max_bound
    uint32_t n_dup_b;        // DeviceStatus::n_dup_b
    uint32_t n_bitonic;      // DeviceStatus::n_bitonic
    uint32_t pad2;
};

// Test / tuning hooks.  Read from the environment ONCE, when a context is created (lchd_ctx_create), and handed to the
// launchers by value: nothing in the launch path calls getenv().
struct Tuning {
    bool no_struct_cells = false;   // LCHD_NO_STRUCT_CELLS: always the generic (multi-pass, global atomics) cell list
    bool no_share = false;          // LCHD_NO_SHARED_ENVS: build both sides even when they are the same device object
    bool no_key_sets = false;       // LCHD_NO_KEY_SETS: weight-function dictionaries keep distance keys (the CDF is evaluated by the sweep, per event)
    bool no_cdf_keys = false;       // LCHD_NO_CDF_KEYS: environments keep distance keys even with a single weight function
    bool no_duo = false;            // LCHD_NO_DUO: never two pairs per wavefront
    bool force_wide = false;        // LCHD_FORCE_WIDE: k_sweep_wide for any category count
    bool force_generic = false;     // LCHD_FORCE_GENERIC: MODE_GEN even for Hellinger-2
    bool force_bigenv = false;      // LCHD_FORCE_BIGENV: the !LDSTAB sweep instantiations
    bool no_sweep_hint = false;     // (deterministic mode only) always launch all three sweep kernels and let the device decide
    bool no_inline_meta = false;    // LCHD_NO_INLINE_META: small calls also run k_pair_meta + the regular sweep kernels
    bool old_rows = false;          // LCHD_OLD_ROWS: dense rows through k_env_rows (three distance passes) for every length
    bool no_dense_fused = false;    // LCHD_NO_DENSE_FUSED: dense rows always through the two-kernel path (row sort, then sweep)
    bool no_count8 = false;         // LCHD_NO_COUNT8: never the 8-bit-count sweep
    bool no_c8_team = false;        // LCHD_NO_C8_TEAM: the 8-bit-count sweep always one pair per wavefront (k_sweep<.., CNT8>)
    bool no_overflow_subset = false;  // LCHD_NO_OVERFLOW_SUBSET: an overflowing environment repeats the WHOLE pass with larger slots (never only its pairs)
    bool no_env_group = false;      // LCHD_NO_ENV_GROUP: environments of the default capacity through k_env_cells (one per wavefront) too
    bool no_sd_inc = false;         // LCHD_NO_SD_INC: Kullback-Leibler / Renyi through the generic sweep even where k_sweep_inc applies
    int env_apw = 0;                // LCHD_ENV_APW: anchors per wavefront of k_env_group (0: chosen from the number of anchors)
    int force_cmax = 0;             // LCHD_FORCE_CMAX: at least this many category slots
    int per_pair = 0;               // LCHD_PER_PAIR: -1 never a side B without de-duplication, 1 whenever it applies, 0: from the previous pass (side-B anchors (almost) all unique)
    int pre_rows = 0;               // LCHD_PRE_ROWS: -1 never prefix-count rows next to the environments (the team sweeps build their chunk-start counts per tile), 1 also for small calls, 0: by the rule of plan_pass
    int team_batch = 0;             // LCHD_TEAM_BATCH: pairs per wavefront and batch of the team sweeps (0: team_batch() of lchd_kernels.hip; else rounded to a multiple of the teams, at most 64)
    int team_grid = 0;              // LCHD_TEAM_GRID: at most this many workgroups per team-sweep launch (0: the measured caps of launch_sweep)
    int ensemble_block = 0;         // LCHD_ENSEMBLE_BLOCK: at most this many structures resident in the dense ensemble call's environment store (0: as many as the free HBM holds)
    int param_sum_blocks = 0;       // LCHD_PARAM_SUM_BLOCKS: at most this many workgroups of k_param_accumulate (0: kParamSumMaxBlocks)
};

inline int next_pow2_host(int64_t n) {
    int p = 64;
    while (p < n) p <<= 1;
    return p;
}

// ------------------------------------------------------------------------------------------------
// the sweep hint and what a sweep launch reports back
// ------------------------------------------------------------------------------------------------
// Bits of the sweep hint (PassHints::sweep_hint, lchd_sweep_query::hint_bits -- the values are public through that field): 0 = nothing
// known (launch every candidate kernel, the device decides from the pair records), otherwise what k_pair_meta counted in the previous
// pass of this configuration.  Any choice is correct for any input; the hint only picks the launch set (plan_sweep).
enum SweepHintBits : int {
    HINT_DUO_MAJOR = 1,   // pairs of at most 240 merged events were the majority: k_sweep_duo + the indirect k_sweep
    HINT_C8_MAJOR = 2,    // pairs with both environments <= 255 points were: the 8-bit-count k_sweep + the indirect one
    HINT_KNOWN = 4,       // a pass of this configuration has been counted (neither majority: the plain k_sweep only)
    HINT_ALL_DUO = 8,     // EVERY pair of the previous pass had at most 240 events ...
    HINT_ALL_C8 = 16,     // ... both environments <= 255 points: the companion launch for the larger pairs is left out
    HINT_ALL = HINT_ALL_DUO | HINT_ALL_C8,
};
// The hint from the counts of a pass.  with_all: also the "every pair" bits -- left out where the counts are those of a pass whose
// overflowed environments' pairs were scored again (the first pass counted those environments as one point each, so "every pair was
// small" says nothing about them).
inline int sweep_hint_from_counts(unsigned long long n_duo, unsigned long long n_c8, int64_t n_pairs, bool with_all) {
    const unsigned long long P = (unsigned long long)n_pairs;
    int hint = HINT_KNOWN | (2 * n_duo >= P ? HINT_DUO_MAJOR : 0) | (2 * n_c8 >= P ? HINT_C8_MAJOR : 0);
    if (with_all) hint |= (n_duo == P ? HINT_ALL_DUO : 0) | (n_c8 == P ? HINT_ALL_C8 : 0);
    return hint;
}

// What launch_sweep (lchd_kernels.hip) did, as far as the host's bookkeeping needs to know.
struct SweepLaunched {
    bool ok = true;                   // false: the planned set would not give every pair exactly one kernel (unreachable); nothing launched
    bool small_is_c8 = false;         // the "small" rule of this pass was the 8-bit-count one (HostStatus::n_c8 counts its pairs, else n_duo)
    bool companion_left_out = false;  // the companion launch was left out: the caller must check this pass's counts against the number of pairs
    bool left_counters_used = false;  // k_pair_meta ran with the leftover-list counters: the caller swaps the two counter slots for the next pass
};
// pairs the small rule of the pass took (the others went to the companion, if there was one)
inline unsigned long long pairs_taken(const HostStatus& h, const SweepLaunched& sl) { return sl.small_is_c8 ? h.n_c8 : h.n_duo; }

// ------------------------------------------------------------------------------------------------
// what a context remembers from one pass for the next
// ------------------------------------------------------------------------------------------------
// The hints describe the caller's workload: a second pass over the pairs of overflowed environments leaves no trace in them
// (rescore_overflow_pairs saves and restores the block as a whole).
struct PassHints {
    int cap_hint = 512;        // environment slot size the next call starts with
    int shrink_votes = 0;      // consecutive passes whose largest environment would fit half of cap_hint
    int sweep_hint = 0;        // SweepHintBits
    bool group_small = false;  // the last pass had no environment beyond kEnvGroupSmallUpTo points: k_env_group's small instantiation
    int64_t last_biggest = 0;  // largest environment of the last pass (0: unknown): anchors per wavefront of k_env_group
    int64_t last_left = 0;     // pairs the last pass left to the INDIRECT companion
    // side B without de-duplication (one environment slot per PAIR) for side-B environments that are used once: taken when the last
    // REGULAR pass of the configuration found (almost) every side-B anchor unique; every 64th pass is a regular one again
    // (such a pass does not count side B's unique anchors, so it cannot see the anchors becoming shared)
    bool b_use_once = false;        // the last regular pass: n_unique[1] >= 0.8 n_pairs
    int64_t use_once_pairs = 0, use_once_nb = 0;  // ... its pair count and the size of its side B (the hint holds for lists like it)
    int per_pair_streak = 0;        // passes without side-B de-duplication since the last regular one
};

// ------------------------------------------------------------------------------------------------
// the plan of one pass
// ------------------------------------------------------------------------------------------------
struct PassQuery {
    // sizes
    int64_t n_a = 0, n_b = 0, n_pairs = 0;
    bool same_object = false;   // both sides are the same device object
    bool has_wf_index = false;  // the caller gave a weight-function index per pair
    // the pass
    int cap = kEnvGroupCap;     // environment slot size
    bool subset = false;        // the pass IS a second pass over the pairs of overflowed environments
    // configuration facts
    int n_categories = 1, n_wf = 1;
    bool hellinger2 = false;
    int sd_fast = 0;
    bool unit_weights = false, finf_differ = false, deterministic = false;
    int tag_mode = 0;
    // hooks and hints
    Tuning tune{};
    PassHints hints{};
};
struct PassPlan {
    bool same = false;       // one cell list and one environment store for both columns of the pair list
    bool cat16 = false;      // 16-bit category ids in the environment store
    int64_t max_env_a = 0, max_env_b = 0;  // environment slots per side
    bool group = false;      // k_env_group builds the environments (else k_env_cells)
    bool group_small = false;  // ... its small instantiation
    bool per_pair = false;   // side B is not de-duplicated (slot p = pair p)
    int reach = 1;           // neighbourhood reach of the environment kernel: cells are at least thr / reach wide
    bool dict_sets = false;  // weight-function dictionary: k_env_key_sets fills one key set per function
    int key_sets = 0;        // key sets of the store (0: distance keys)
    int pre_words = 0;       // u64 words per prefix-count row (0: no rows)
    int apw = 0;             // anchors per wavefront of k_env_group
    bool tag_list = false;
};

inline PassPlan plan_pass(const PassQuery& q) {
    PassPlan p;
    const Tuning& t = q.tune;
    const PassHints& h = q.hints;
    const int64_t n_pairs = q.n_pairs;
    // environments of the default capacity: several per wavefront on a grid of half-threshold cells (lchd_env_group.hip)
    // more than 255 categories: 16-bit ids in the environment store, k_env_cells<.., uint16_t> + k_sweep_wide<.., CAT16>
    p.cat16 = q.n_categories > kMaxCategories;
    // Both sides the SAME device object (all-vs-all over one batch of structures, a structure against itself): an anchor's
    // environment does not depend on the side it is used on (src/locohd.rs:514-542 is one closure for both), so the cell
    // list and every environment are built once -- the anchors of both columns share side A's flags, slots and store.
    p.same = q.same_object && !t.no_share;
    p.max_env_a = p.same ? std::min<int64_t>(q.n_a, 2 * n_pairs) : std::min<int64_t>(q.n_a, n_pairs);
    p.max_env_b = p.same ? 0 : std::min<int64_t>(q.n_b, n_pairs);  // (side B without de-duplication: one slot per PAIR, below)
    // (the grouped kernel addresses environment slots and records with 32-bit offsets: the limits of launch_env_group; larger
    //  calls take k_env_cells, which has none)
    p.group = q.cap == kEnvGroupCap && !t.no_env_group && q.n_a < ((int64_t)1 << 27) && q.n_b < ((int64_t)1 << 27) &&
              p.max_env_a < ((int64_t)1 << 22) && p.max_env_b < ((int64_t)1 << 22) && !p.cat16;
    p.group_small = p.group && h.group_small;
    p.reach = p.group ? 2 : 1;
    // Side B used once -- (almost) every side-B anchor of the last regular pass of this context was unique: the frames of a trajectory,
    // (i, i) lists, a rank's partners under strong scaling.  Such a side is not de-duplicated: environment slot p belongs to pair p
    // and its anchor record comes straight from the pair list (launch_pair_anchor_recs) -- no flags, bit set, scan and scatter over
    // the side's atoms.  Any choice is correct for any input: an anchor that occurs in several pairs is built once per pair, as the
    // reference does (src/locohd.rs:514-554).  Every 64th pass is a regular one again (this mode does not count unique anchors).
    const bool per_pair_ok = p.group && !p.same && !q.subset && !q.deterministic && t.per_pair >= 0 && n_pairs < ((int64_t)1 << 22) && n_pairs > 0;
    // (history alone is not enough: the hint must have come from a list of this size on a structure of this size, and a list with more
    //  pairs than the side has atoms repeats anchors by counting -- C2a: 10^6 pairs over 10^4 atoms right after a list of (i, i) pairs)
    const bool like_hinted = n_pairs <= q.n_b && q.n_b == h.use_once_nb && 2 * n_pairs >= h.use_once_pairs && n_pairs <= 2 * h.use_once_pairs;
    p.per_pair = per_pair_ok && (t.per_pair > 0 || (h.b_use_once && like_hinted && n_pairs > 4096 && h.per_pair_streak < 64));
    if (p.per_pair) p.max_env_b = n_pairs;  // (one slot per PAIR)
    // Keys of the store: F(distance) whenever the sweep can use them without evaluating a CDF -- one weight function, or a
    // dictionary of up to kMaxKeySets (src/locohd.rs:230-283: every pair names its function): k_env_group writes one key set per
    // function (the sort is shared, the store's key part grows k-fold) and a pair reads the set of its function.
    // (dictionary: set 0 keeps the distances k_env_group writes, k_env_key_sets fills sets 1 .. n_wf; the sweeps' view starts at set 1)
    p.dict_sets = q.n_wf > 1 && p.group && q.n_wf <= kMaxKeySets && q.has_wf_index && !t.no_key_sets && !t.no_cdf_keys && !q.finf_differ;
    p.key_sets = t.no_cdf_keys ? 0 : (q.n_wf == 1 ? 1 : (p.dict_sets ? q.n_wf + 1 : 0));
    // Prefix-count rows next to the environments (EnvStore::pre, 8 or 16 bytes per point): the team sweeps of up to 16 category slots
    // read a chunk's start counts from them instead of building a histogram and a scan per tile.  Worth their write when environments
    // are swept more than once: not for a side without de-duplication (one pair per environment), not for small calls (one pair per
    // wavefront: the one-launch sweep), only where the team sweeps exist (Hellinger-2 / Kolmogorov-Smirnov on unit weights).
    {
        const int cm = std::max(q.n_categories, t.force_cmax);
        const bool team_cfg = (q.hellinger2 || q.sd_fast == 3) && q.unit_weights && p.key_sets >= 1 && !t.no_duo && !t.no_count8 &&
                              !t.no_c8_team && !t.force_generic && !t.force_wide && !t.force_bigenv;
        // (17 .. 28 slots -- three / four count words, the LDS-byte form of the team sweep -- were built and measured in round 6: C5's
        //  k_sweep_duo<28, 32, 480> 1.690 ms with rows against 1.679 without, k_env_group 0.93 against 0.77 ms: no rows there)
        if (p.group && team_cfg && cm <= 16 && !p.per_pair && !q.deterministic && t.pre_rows >= 0 && (n_pairs > 4096 || t.no_inline_meta || t.pre_rows > 0))
            p.pre_words = team_pre_words(cm);
    }
    if (p.group) {
        // anchors per wavefront: as many as fit ONE group of the kernel's LDS buffer (measured, env phase in ms for 1 / 2 / 4 / 8 /
        // 16 anchors: C4, ~96-point environments 3.87 / 2.88 / 2.68 / 2.69 / 2.96; C5, ~200 points 0.81 / 0.75 / 0.75 / 0.78 / 0.81 --
        // more anchors per wavefront only lengthen the tail of the launch)
        // A call with few anchors is bound by the latency of one wavefront's chain, not by throughput: one anchor per wavefront
        // until there are enough of them to fill the chip twice (3000-atom structure pair: 19.9 -> 11.7 us).
        const int by_size = h.last_biggest > 0 && h.last_biggest <= 140 ? 4 : (h.last_biggest > kEnvGroupSmallUpTo ? 1 : 2);
        p.apw = t.env_apw > 0 ? t.env_apw : (int)std::max<int64_t>(1, std::min<int64_t>(by_size, (p.max_env_a + p.max_env_b) / 8192));
    }
    p.tag_list = q.tag_mode != 0;
    return p;
}

// ------------------------------------------------------------------------------------------------
// after a pass
// ------------------------------------------------------------------------------------------------
enum class PassVerdict {
    STANDS,          // the scores and status words of the pass are the call's
    BAD_ANCHOR,      // ... and so are these: an anchor index outside its cloud (nothing else of the pass is looked at)
    UNSUPPORTED,     // an environment beyond 65535 points with more categories or points than the 64-bit-count sweep handles
    REPEAT_REGULAR,  // the small instantiation of k_env_group overflowed: the same capacity with the regular one
    REPEAT_FULL_SET, // the companion sweep had been left out and this pass had pairs for it: again with the full launch set
    OVERFLOW,        // an environment did not fit its slot: its pairs again with larger slots, else the whole pass with grown_cap
};
struct PassOutcome {
    PassVerdict verdict = PassVerdict::STANDS;
    int64_t biggest = 0;  // largest environment of the pass (k_pair_meta), or what overflowed
    bool overflowed = false;  // ST_ENV_OVERFLOW was set
    int grown_cap = 0;    // OVERFLOW: the slot size of a repeat of the whole pass
};
inline PassOutcome pass_verdict(uint32_t flags, const HostStatus& h, const PassPlan& plan, const SweepLaunched& sl, int n_categories,
                                int64_t n_pairs, int cap, bool subset) {
    PassOutcome o;
    o.biggest = h.max_env;
    if (flags & ST_BAD_ANCHOR) { o.verdict = PassVerdict::BAD_ANCHOR; return o; }
    const bool overflow = o.overflowed = (flags & ST_ENV_OVERFLOW) != 0;
    if (overflow) {
        if (o.biggest > 65535 && (n_categories > kMaxCategories || o.biggest > (1 << 23))) { o.verdict = PassVerdict::UNSUPPORTED; return o; }
        if (plan.group && plan.group_small && o.biggest <= kEnvGroupCap) { o.verdict = PassVerdict::REPEAT_REGULAR; return o; }
    }
    // The companion sweep for the larger pairs was left out (the previous pass of this context had none): if this pass has
    // some, their scores were never written.  After an overflow too: the whole pass again with the full launch set BEFORE the second
    // pass over the overflowed environments' pairs keeps the first pass's scores of everything else.
    // (n_small == ~0: no record pass, the inline sweep counts nothing)
    if (sl.companion_left_out && h.n_small != ~0ull && pairs_taken(h, sl) < (unsigned long long)n_pairs) { o.verdict = PassVerdict::REPEAT_FULL_SET; return o; }
    if (overflow) {
        // (candidate-table overflows reported an upper bound -- candidates, ~2.4 environments' worth on a uniform cloud --: the whole
        //  pass tries the slot size that would fit a typical share of them first; a subset's few slots take the bound itself)
        const int64_t bound = h.max_bound;
        o.grown_cap = next_pow2_host(std::max<int64_t>(std::max<int64_t>(o.biggest, subset ? bound : bound / 3), cap + 1));
        o.verdict = PassVerdict::OVERFLOW;
    }
    return o;
}

// The capacity hint decays: a single dense environment should not make every later call of this context pay for
// its slot size (slots are fixed-stride).  Eight passes in a row that would have fitted half the capacity halve it.
inline void vote_on_capacity(PassHints& n, int64_t biggest) {
    if (n.cap_hint > 512 && biggest > 0 && 2 * next_pow2_host(biggest) <= n.cap_hint) {
        if (++n.shrink_votes >= 8) { n.cap_hint = std::max(512, n.cap_hint / 2); n.shrink_votes = 0; }
    } else {
        n.shrink_votes = 0;
    }
}

// The hints after a pass that stands.  A second pass over the pairs of overflowed environments (subset) touches group_small,
// last_biggest and sweep_hint alone -- what its own repeats read; its caller restores the block afterwards.
inline PassHints hints_after_pass(const PassHints& hints, const HostStatus& h, const PassPlan& plan, const SweepLaunched& sl, int64_t n_pairs,
                                  int64_t n_b, bool subset) {
    PassHints n = hints;
    const int64_t biggest = h.max_env;
    const unsigned long long P = (unsigned long long)n_pairs;
    const bool counted = h.n_small != ~0ull;  // (no record pass: the inline sweep counts nothing)
    if (biggest > 0) { n.group_small = biggest <= kEnvGroupSmallUpTo; n.last_biggest = biggest; }
    if (counted) n.sweep_hint = sweep_hint_from_counts(h.n_duo, h.n_c8, n_pairs, true);  // what the pairs looked like this time picks the sweep kernels of the next pass of this configuration
    if (subset) return n;
    vote_on_capacity(n, biggest);
    if (plan.per_pair) {
        ++n.per_pair_streak;
        // (this pass did not count side B's unique anchors; its bit set counts the repeated ones: a list that shares
        //  more than a fifth of them goes back to the regular pipeline with the next pass)
        if ((unsigned long long)h.n_dup_b * 5ull > P) n.b_use_once = false;
    } else {  // (almost) every side-B anchor unique: the next passes of this context on such lists do not de-duplicate side B
        n.b_use_once = !plan.same && (unsigned long long)h.n_unique[1] * 5ull >= P * 4ull;
        n.use_once_pairs = n_pairs;
        n.use_once_nb = n_b;
        n.per_pair_streak = 0;
    }
    if (counted)  // (sizes the next pass's companion launch when it walks the leftover list)
        n.last_left = n_pairs - (int64_t)std::min<unsigned long long>(pairs_taken(h, sl), P);
    return n;
}

// The hints a repeat of the pass is planned with (o.verdict one of the REPEAT_* or OVERFLOW -- the latter once the second pass over
// the overflowed environments' pairs has turned out not to apply: the whole pass with o.grown_cap).
inline PassHints hints_for_repeat(const PassHints& hints, const PassOutcome& o, bool subset) {
    PassHints n = hints;
    switch (o.verdict) {
        case PassVerdict::REPEAT_REGULAR:
            n.group_small = false;
            n.last_biggest = std::max<int64_t>(o.biggest, kEnvGroupCapSmall + 1);
            break;
        case PassVerdict::REPEAT_FULL_SET:
            // (a pass that fitted its slots casts its capacity vote before it is repeated, and the repeat casts another)
            if (!o.overflowed && !subset) vote_on_capacity(n, o.biggest);
            n.sweep_hint &= ~HINT_ALL;
            break;
        case PassVerdict::OVERFLOW:
            if (!subset) { n.cap_hint = o.grown_cap; n.shrink_votes = 0; }
            break;
        default: break;
    }
    return n;
}

}  // namespace lchd
