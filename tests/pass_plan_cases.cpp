// Table of cases for the pure functions of loco_hd_amd/csrc/lchd_pass_plan.h (tests/test_pass_plan.py builds and runs this with the
// host compiler; the expected values live there, written out by hand).  Prints one line per case: "<name>: key=value ...".
#include <cstdio>

#include "lchd_pass_plan.h"

using namespace lchd;

static void show(const char* name, const PassPlan& p) {
    printf("%s: same=%d cat16=%d max_env_a=%lld max_env_b=%lld group=%d group_small=%d per_pair=%d reach=%d dict_sets=%d key_sets=%d pre_words=%d apw=%d tag_list=%d\n",
           name, p.same, p.cat16, (long long)p.max_env_a, (long long)p.max_env_b, p.group, p.group_small, p.per_pair, p.reach, p.dict_sets,
           p.key_sets, p.pre_words, p.apw, p.tag_list);
}
static void show(const char* name, const PassHints& h) {
    printf("%s: cap_hint=%d shrink_votes=%d sweep_hint=%d group_small=%d last_biggest=%lld last_left=%lld b_use_once=%d use_once_pairs=%lld use_once_nb=%lld per_pair_streak=%d\n",
           name, h.cap_hint, h.shrink_votes, h.sweep_hint, h.group_small, (long long)h.last_biggest, (long long)h.last_left, h.b_use_once,
           (long long)h.use_once_pairs, (long long)h.use_once_nb, h.per_pair_streak);
}
static void show(const char* name, const PassOutcome& o) {
    static const char* names[] = {"STANDS", "BAD_ANCHOR", "UNSUPPORTED", "REPEAT_REGULAR", "REPEAT_FULL_SET", "OVERFLOW"};
    printf("%s: verdict=%s biggest=%lld overflowed=%d grown_cap=%d\n", name, names[(int)o.verdict], (long long)o.biggest, o.overflowed, o.grown_cap);
}

// the default configuration on two structures of 10 000 atoms, 5 000 pairs: grouped kernel, one key set, prefix rows
static PassQuery base() {
    PassQuery q;
    q.n_a = q.n_b = 10000;
    q.n_pairs = 5000;
    q.cap = kEnvGroupCap;
    q.n_categories = 5;
    q.n_wf = 1;
    q.hellinger2 = q.unit_weights = true;
    return q;
}
// ... whose previous regular pass found side B's anchors unique on a list like this one: side B is not de-duplicated
static PassQuery hinted() {
    PassQuery q = base();
    q.hints.b_use_once = true;
    q.hints.use_once_nb = q.n_b;
    q.hints.use_once_pairs = q.n_pairs;
    return q;
}
template <class F>
static void plan_case(const char* name, PassQuery q, F&& change) {
    change(q);
    show(name, plan_pass(q));
}

static void plan_cases() {
    const int64_t M27 = (int64_t)1 << 27, M22 = (int64_t)1 << 22;
    printf("constants: kEnvGroupCap=%d kEnvGroupCapSmall=%d kEnvGroupSmallUpTo=%d kMaxCategories=%d kMaxKeySets=%d\n", kEnvGroupCap,
           kEnvGroupCapSmall, kEnvGroupSmallUpTo, kMaxCategories, kMaxKeySets);
    plan_case("base", base(), [](PassQuery&) {});
    // group
    plan_case("group_cap_next", base(), [](PassQuery& q) { q.cap = 2 * kEnvGroupCap; });
    plan_case("group_na_below", base(), [&](PassQuery& q) { q.n_a = M27 - 1; });
    plan_case("group_na_at", base(), [&](PassQuery& q) { q.n_a = M27; });
    plan_case("group_nb_at", base(), [&](PassQuery& q) { q.n_b = M27; });
    plan_case("group_env_below", base(), [&](PassQuery& q) { q.n_a = q.n_b = 2 * M22; q.n_pairs = M22 - 1; });
    plan_case("group_env_at", base(), [&](PassQuery& q) { q.n_a = q.n_b = 2 * M22; q.n_pairs = M22; });
    plan_case("group_cat_at", base(), [](PassQuery& q) { q.n_categories = kMaxCategories; });
    plan_case("group_cat_above", base(), [](PassQuery& q) { q.n_categories = kMaxCategories + 1; });
    plan_case("group_hook", base(), [](PassQuery& q) { q.tune.no_env_group = true; });
    plan_case("group_small_hint", base(), [](PassQuery& q) { q.hints.group_small = true; });
    plan_case("group_small_hint_not_group", base(), [](PassQuery& q) { q.hints.group_small = true; q.cap = 2 * kEnvGroupCap; });
    plan_case("tag_list", base(), [](PassQuery& q) { q.tag_mode = 2; });
    // max_env
    plan_case("same_few_pairs", base(), [](PassQuery& q) { q.same_object = true; q.n_pairs = 3000; });
    plan_case("same_many_pairs", base(), [](PassQuery& q) { q.same_object = true; q.n_pairs = 6000; });
    plan_case("same_no_share", base(), [](PassQuery& q) { q.same_object = true; q.n_pairs = 3000; q.tune.no_share = true; });
    plan_case("per_pair_slots", base(), [](PassQuery& q) { q.n_b = 3000; q.tune.per_pair = 1; });
    plan_case("regular_slots", base(), [](PassQuery& q) { q.n_b = 3000; });
    // per_pair
    plan_case("pp_hinted", hinted(), [](PassQuery&) {});
    plan_case("pp_4096", hinted(), [](PassQuery& q) { q.n_pairs = q.hints.use_once_pairs = 4096; });
    plan_case("pp_4097", hinted(), [](PassQuery& q) { q.n_pairs = q.hints.use_once_pairs = 4097; });
    plan_case("pp_streak_63", hinted(), [](PassQuery& q) { q.hints.per_pair_streak = 63; });
    plan_case("pp_streak_64", hinted(), [](PassQuery& q) { q.hints.per_pair_streak = 64; });
    plan_case("pp_pairs_eq_nb", hinted(), [](PassQuery& q) { q.n_b = q.hints.use_once_nb = 5000; });
    plan_case("pp_pairs_eq_nb_plus_1", hinted(), [](PassQuery& q) { q.n_b = q.hints.use_once_nb = 5000; q.n_pairs = q.hints.use_once_pairs = 5001; });
    plan_case("pp_other_nb", hinted(), [](PassQuery& q) { q.hints.use_once_nb = 9999; });
    plan_case("pp_2p_eq_hint", hinted(), [](PassQuery& q) { q.hints.use_once_pairs = 10000; });
    plan_case("pp_2p_eq_hint_minus_1", hinted(), [](PassQuery& q) { q.hints.use_once_pairs = 10001; });
    plan_case("pp_p_eq_2hint", hinted(), [](PassQuery& q) { q.hints.use_once_pairs = 2500; });
    plan_case("pp_p_eq_2hint_plus_1", hinted(), [](PassQuery& q) { q.hints.use_once_pairs = 2500; q.n_pairs = 5001; });
    plan_case("pp_not_hinted", hinted(), [](PassQuery& q) { q.hints.b_use_once = false; });
    plan_case("pp_tune_never", hinted(), [](PassQuery& q) { q.tune.per_pair = -1; });
    plan_case("pp_tune_always", base(), [](PassQuery& q) { q.tune.per_pair = 1; q.n_pairs = 100; });
    plan_case("pp_deterministic", base(), [](PassQuery& q) { q.tune.per_pair = 1; q.deterministic = true; });
    plan_case("pp_same", base(), [](PassQuery& q) { q.tune.per_pair = 1; q.same_object = true; });
    plan_case("pp_subset", base(), [](PassQuery& q) { q.tune.per_pair = 1; q.subset = true; });
    plan_case("pp_not_group", base(), [](PassQuery& q) { q.tune.per_pair = 1; q.cap = 2 * kEnvGroupCap; });
    plan_case("pp_pairs_below_2_22", base(), [&](PassQuery& q) { q.tune.per_pair = 1; q.n_pairs = M22 - 1; });
    plan_case("pp_pairs_at_2_22", base(), [&](PassQuery& q) { q.tune.per_pair = 1; q.n_pairs = M22; });
    // key_sets and dict_sets
    for (int n_wf = 2; n_wf <= kMaxKeySets + 1; ++n_wf) {
        char name[32];
        snprintf(name, sizeof name, "keys_dict_%d%s", n_wf, n_wf > kMaxKeySets ? "_too_many" : "");
        plan_case(name, base(), [&](PassQuery& q) { q.n_wf = n_wf; q.has_wf_index = true; });
    }
    plan_case("keys_no_index", base(), [](PassQuery& q) { q.n_wf = 2; });
    plan_case("keys_finf_differ", base(), [](PassQuery& q) { q.n_wf = 2; q.has_wf_index = true; q.finf_differ = true; });
    plan_case("keys_no_key_sets", base(), [](PassQuery& q) { q.n_wf = 2; q.has_wf_index = true; q.tune.no_key_sets = true; });
    plan_case("keys_not_group", base(), [](PassQuery& q) { q.n_wf = 2; q.has_wf_index = true; q.cap = 2 * kEnvGroupCap; });
    plan_case("keys_no_cdf_keys", base(), [](PassQuery& q) { q.tune.no_cdf_keys = true; });
    plan_case("keys_no_cdf_keys_dict", base(), [](PassQuery& q) { q.n_wf = 2; q.has_wf_index = true; q.tune.no_cdf_keys = true; });
    // pre_words
    plan_case("pre_slots_8", base(), [](PassQuery& q) { q.n_categories = 8; });
    plan_case("pre_slots_9", base(), [](PassQuery& q) { q.n_categories = 9; });
    plan_case("pre_slots_16", base(), [](PassQuery& q) { q.n_categories = 16; });
    plan_case("pre_slots_17", base(), [](PassQuery& q) { q.n_categories = 17; });
    plan_case("pre_force_cmax_9", base(), [](PassQuery& q) { q.tune.force_cmax = 9; });
    plan_case("pre_force_cmax_17", base(), [](PassQuery& q) { q.tune.force_cmax = 17; });
    plan_case("pre_pairs_4096", base(), [](PassQuery& q) { q.n_pairs = 4096; });
    plan_case("pre_pairs_4097", base(), [](PassQuery& q) { q.n_pairs = 4097; });
    plan_case("pre_rows_on_4096", base(), [](PassQuery& q) { q.n_pairs = 4096; q.tune.pre_rows = 1; });
    plan_case("pre_no_inline_meta_4096", base(), [](PassQuery& q) { q.n_pairs = 4096; q.tune.no_inline_meta = true; });
    plan_case("pre_rows_off", base(), [](PassQuery& q) { q.tune.pre_rows = -1; });
    plan_case("pre_per_pair", base(), [](PassQuery& q) { q.tune.per_pair = 1; });
    plan_case("pre_deterministic", base(), [](PassQuery& q) { q.deterministic = true; });
    plan_case("pre_not_group", base(), [](PassQuery& q) { q.cap = 2 * kEnvGroupCap; });
    plan_case("pre_other_distance", base(), [](PassQuery& q) { q.hellinger2 = false; });
    plan_case("pre_kolmogorov_smirnov", base(), [](PassQuery& q) { q.hellinger2 = false; q.sd_fast = 3; });
    plan_case("pre_weights", base(), [](PassQuery& q) { q.unit_weights = false; });
    plan_case("pre_no_cdf_keys", base(), [](PassQuery& q) { q.tune.no_cdf_keys = true; });
    plan_case("pre_no_duo", base(), [](PassQuery& q) { q.tune.no_duo = true; });
    plan_case("pre_no_count8", base(), [](PassQuery& q) { q.tune.no_count8 = true; });
    plan_case("pre_no_c8_team", base(), [](PassQuery& q) { q.tune.no_c8_team = true; });
    plan_case("pre_force_generic", base(), [](PassQuery& q) { q.tune.force_generic = true; });
    plan_case("pre_force_wide", base(), [](PassQuery& q) { q.tune.force_wide = true; });
    plan_case("pre_force_bigenv", base(), [](PassQuery& q) { q.tune.force_bigenv = true; });
    // apw: 20 000 + 20 000 environment slots leave the size rule alone (40 000 / 8192 = 4)
    auto big = [](int64_t last_biggest) { PassQuery q = base(); q.n_a = q.n_b = q.n_pairs = 20000; q.hints.last_biggest = last_biggest; return q; };
    plan_case("apw_unknown", big(0), [](PassQuery&) {});
    plan_case("apw_140", big(140), [](PassQuery&) {});
    plan_case("apw_141", big(141), [](PassQuery&) {});
    plan_case("apw_small_up_to", big(kEnvGroupSmallUpTo), [](PassQuery&) {});
    plan_case("apw_small_up_to_plus_1", big(kEnvGroupSmallUpTo + 1), [](PassQuery&) {});
    auto total = [](int64_t n_a, int64_t n_b) { PassQuery q = base(); q.n_a = n_a; q.n_b = n_b; q.n_pairs = 100000; q.hints.last_biggest = 100; return q; };
    plan_case("apw_total_8191", total(4000, 4191), [](PassQuery&) {});
    plan_case("apw_total_8192", total(4000, 4192), [](PassQuery&) {});
    plan_case("apw_total_16383", total(8000, 8383), [](PassQuery&) {});
    plan_case("apw_total_16384", total(8000, 8384), [](PassQuery&) {});
    plan_case("apw_total_32767", total(16000, 16767), [](PassQuery&) {});
    plan_case("apw_total_32768", total(16000, 16768), [](PassQuery&) {});
    plan_case("apw_override", big(0), [](PassQuery& q) { q.tune.env_apw = 7; });
    plan_case("apw_not_group", big(0), [](PassQuery& q) { q.cap = 2 * kEnvGroupCap; });
}

struct Finished {
    uint32_t flags = 0;
    HostStatus h{};
    PassPlan plan;
    SweepLaunched sl;
    int n_categories = 5;
    int64_t n_pairs = 5000, n_b = 10000;
    int cap = kEnvGroupCap;
    bool subset = false;
    PassOutcome verdict() const { return pass_verdict(flags, h, plan, sl, n_categories, n_pairs, cap, subset); }
    PassHints hints(const PassHints& in) const { return hints_after_pass(in, h, plan, sl, n_pairs, n_b, subset); }
};
// a grouped pass of 5 000 pairs whose record pass counted 3 000 pairs under either rule; largest environment 200 points
static Finished finished() {
    Finished f;
    f.plan.group = true;
    f.h.max_env = 200;
    f.h.n_small = f.h.n_duo = f.h.n_c8 = 3000;
    return f;
}
template <class F>
static void verdict_case(const char* name, F&& change) {
    Finished f = finished();
    change(f);
    show(name, f.verdict());
}
template <class F>
static void repeat_case(const char* name, PassHints in, F&& change) {
    Finished f = finished();
    change(f);
    show(name, hints_for_repeat(in, f.verdict(), f.subset));
}

static void verdict_cases() {
    verdict_case("v_stands", [](Finished&) {});
    verdict_case("v_bad_anchor", [](Finished& f) { f.flags = ST_BAD_ANCHOR | ST_ENV_OVERFLOW; f.sl.companion_left_out = true; });
    verdict_case("v_other_flags_stand", [](Finished& f) { f.flags = ST_ZERO_NORM | ST_EMPTY_ENV; });
    // the small instantiation of the grouped kernel overflowed
    verdict_case("v_small_group_at_cap", [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.plan.group_small = true; f.h.max_env = kEnvGroupCap; });
    verdict_case("v_small_group_above_cap", [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.plan.group_small = true; f.h.max_env = kEnvGroupCap + 1; });
    verdict_case("v_regular_group_at_cap", [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.h.max_env = kEnvGroupCap; });
    // the companion sweep was left out
    verdict_case("v_left_out_one_pair_missing", [](Finished& f) { f.sl.companion_left_out = true; f.h.n_duo = 4999; f.h.n_c8 = 5000; });
    verdict_case("v_left_out_all_taken", [](Finished& f) { f.sl.companion_left_out = true; f.h.n_duo = 5000; f.h.n_c8 = 0; });
    verdict_case("v_left_out_c8_one_missing", [](Finished& f) { f.sl.companion_left_out = f.sl.small_is_c8 = true; f.h.n_duo = 5000; f.h.n_c8 = 4999; });
    verdict_case("v_left_out_c8_all_taken", [](Finished& f) { f.sl.companion_left_out = f.sl.small_is_c8 = true; f.h.n_duo = 0; f.h.n_c8 = 5000; });
    verdict_case("v_companion_ran", [](Finished& f) { f.h.n_duo = 0; });
    verdict_case("v_left_out_not_counted", [](Finished& f) { f.sl.companion_left_out = true; f.h.n_small = ~0ull; f.h.n_duo = f.h.n_c8 = 0; });
    verdict_case("v_overflow_left_out_one_missing", [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.h.max_env = 700; f.sl.companion_left_out = true; f.h.n_duo = 4999; });
    verdict_case("v_overflow_left_out_all_taken", [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.h.max_env = 700; f.sl.companion_left_out = true; f.h.n_duo = 5000; });
    verdict_case("v_overflow_left_out_not_counted", [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.h.max_env = 700; f.sl.companion_left_out = true; f.h.n_small = ~0ull; f.h.n_duo = 0; });
    verdict_case("v_small_group_before_full_set", [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.plan.group_small = true; f.h.max_env = 400; f.sl.companion_left_out = true; f.h.n_duo = 0; });
    // unsupported sizes
    verdict_case("v_wide_65535", [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.plan.group = false; f.n_categories = kMaxCategories + 1; f.h.max_env = 65535; f.cap = 8192; });
    verdict_case("v_wide_65536", [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.plan.group = false; f.n_categories = kMaxCategories + 1; f.h.max_env = 65536; f.cap = 8192; });
    verdict_case("v_long_2_23", [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.n_categories = kMaxCategories; f.h.max_env = 1u << 23; });
    verdict_case("v_long_2_23_plus_1", [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.n_categories = kMaxCategories; f.h.max_env = (1u << 23) + 1; });
    verdict_case("v_long_not_overflowed", [](Finished& f) { f.n_categories = kMaxCategories + 1; f.h.max_env = 70000; });
    // the grown capacity
    verdict_case("v_grow_third_of_bound", [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.h.max_env = 700; f.h.max_bound = 6000; });
    verdict_case("v_grow_subset_whole_bound", [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.h.max_env = 700; f.h.max_bound = 6000; f.subset = true; });
    verdict_case("v_grow_biggest", [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.h.max_env = 5000; f.h.max_bound = 9000; });
    verdict_case("v_grow_cap_plus_1", [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.h.max_env = 600; f.h.max_bound = 0; f.cap = 1024; f.plan.group = false; });
    verdict_case("v_grow_exact_power", [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.h.max_env = 1024; f.h.max_bound = 3072; });

    PassHints in;
    in.cap_hint = 1024; in.shrink_votes = 5; in.sweep_hint = 31; in.group_small = true; in.last_biggest = 100; in.last_left = 9;
    in.b_use_once = true; in.use_once_pairs = 77; in.use_once_nb = 88; in.per_pair_streak = 3;
    show("r_input", in);
    repeat_case("r_regular_at_cap", in, [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.plan.group_small = true; f.h.max_env = kEnvGroupCap; });
    repeat_case("r_regular_small_biggest", in, [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.plan.group_small = true; f.h.max_env = 300; });
    repeat_case("r_full_set_after_overflow", in, [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.h.max_env = 700; f.sl.companion_left_out = true; f.h.n_duo = 0; });
    repeat_case("r_full_set_fitted", in, [](Finished& f) { f.sl.companion_left_out = true; f.h.n_duo = 0; });       // (200 points fit half of 1024: a vote)
    repeat_case("r_full_set_fitted_subset", in, [](Finished& f) { f.sl.companion_left_out = true; f.h.n_duo = 0; f.subset = true; });
    repeat_case("r_grow", in, [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.h.max_env = 700; f.h.max_bound = 6000; });
    repeat_case("r_grow_subset", in, [](Finished& f) { f.flags = ST_ENV_OVERFLOW; f.h.max_env = 700; f.h.max_bound = 6000; f.subset = true; });
}

template <class F>
static void hints_case(const char* name, PassHints in, F&& change) {
    Finished f = finished();
    f.n_pairs = 1000;
    f.h.n_small = f.h.n_duo = f.h.n_c8 = 0;
    change(f);
    show(name, f.hints(in));
}

static void hints_cases() {
    auto cap = [](int cap_hint, int votes) { PassHints h; h.cap_hint = cap_hint; h.shrink_votes = votes; return h; };
    // capacity decay: 500 points round up to 512 and fit half of 2048 (and of 1024)
    hints_case("h_vote_7", cap(2048, 6), [](Finished& f) { f.h.max_env = 500; });
    hints_case("h_vote_8", cap(2048, 7), [](Finished& f) { f.h.max_env = 500; });
    hints_case("h_vote_8_to_512", cap(1024, 7), [](Finished& f) { f.h.max_env = 200; });
    hints_case("h_vote_floor", cap(768, 7), [](Finished& f) { f.h.max_env = 100; });
    hints_case("h_vote_at_512", cap(512, 7), [](Finished& f) { f.h.max_env = 100; });
    hints_case("h_vote_fits_exactly_half", cap(2048, 3), [](Finished& f) { f.h.max_env = 1024; });
    hints_case("h_vote_reset", cap(2048, 5), [](Finished& f) { f.h.max_env = 1025; });
    hints_case("h_vote_reset_unknown", cap(2048, 5), [](Finished& f) { f.h.max_env = 0; });
    // sweep hint (1 000 pairs)
    PassHints none;
    hints_case("h_duo_half", none, [](Finished& f) { f.h.n_duo = 500; });
    hints_case("h_duo_below_half", none, [](Finished& f) { f.h.n_duo = 499; });
    hints_case("h_duo_all", none, [](Finished& f) { f.h.n_duo = 1000; });
    hints_case("h_duo_all_but_one", none, [](Finished& f) { f.h.n_duo = 999; });
    hints_case("h_c8_half", none, [](Finished& f) { f.h.n_c8 = 500; });
    hints_case("h_c8_below_half", none, [](Finished& f) { f.h.n_c8 = 499; });
    hints_case("h_c8_all", none, [](Finished& f) { f.h.n_c8 = 1000; });
    hints_case("h_c8_all_but_one", none, [](Finished& f) { f.h.n_c8 = 999; });
    hints_case("h_both_all", none, [](Finished& f) { f.h.n_duo = f.h.n_c8 = 1000; });
    PassHints known;
    known.sweep_hint = 13; known.last_left = 42;
    hints_case("h_not_counted", known, [](Finished& f) { f.h.n_small = ~0ull; f.h.n_duo = f.h.n_c8 = 1000; });
    printf("hint_formula: half_with_all=%d all_with_all=%d all_without_all=%d c8_all_without_all=%d\n", sweep_hint_from_counts(500, 0, 1000, true),
           sweep_hint_from_counts(1000, 0, 1000, true), sweep_hint_from_counts(1000, 0, 1000, false), sweep_hint_from_counts(0, 1000, 1000, false));
    // side B used once
    hints_case("h_use_once_at_four_fifths", none, [](Finished& f) { f.h.n_unique[1] = 800; f.n_b = 1234; });
    hints_case("h_use_once_below", none, [](Finished& f) { f.h.n_unique[1] = 799; f.n_b = 1234; });
    hints_case("h_use_once_same", none, [](Finished& f) { f.h.n_unique[1] = 1000; f.plan.same = true; });
    PassHints streak;
    streak.b_use_once = true; streak.use_once_pairs = 1000; streak.use_once_nb = 1234; streak.per_pair_streak = 5;
    hints_case("h_regular_pass_ends_streak", streak, [](Finished& f) { f.h.n_unique[1] = 1000; f.n_b = 4321; });
    hints_case("h_per_pair_fifth_repeated", streak, [](Finished& f) { f.plan.per_pair = true; f.h.n_dup_b = 200; });
    hints_case("h_per_pair_over_a_fifth", streak, [](Finished& f) { f.plan.per_pair = true; f.n_pairs = 1004; f.h.n_dup_b = 201; });
    hints_case("h_per_pair_1004_at_200", streak, [](Finished& f) { f.plan.per_pair = true; f.n_pairs = 1004; f.h.n_dup_b = 200; });
    // last_left
    hints_case("h_left_100", none, [](Finished& f) { f.h.n_duo = 900; f.h.n_c8 = 1000; });
    hints_case("h_left_c8_rule", none, [](Finished& f) { f.sl.small_is_c8 = true; f.h.n_duo = 900; f.h.n_c8 = 1000; });
    hints_case("h_left_clamped", none, [](Finished& f) { f.h.n_duo = 1500; });
    // group_small / last_biggest
    hints_case("h_biggest_small_up_to", none, [](Finished& f) { f.h.max_env = kEnvGroupSmallUpTo; });
    hints_case("h_biggest_small_up_to_plus_1", none, [](Finished& f) { f.h.max_env = kEnvGroupSmallUpTo + 1; });
    PassHints in;
    in.cap_hint = 2048; in.shrink_votes = 7; in.sweep_hint = 31; in.group_small = true; in.last_biggest = 100; in.last_left = 9;
    in.b_use_once = true; in.use_once_pairs = 77; in.use_once_nb = 88; in.per_pair_streak = 3;
    hints_case("h_biggest_unknown", in, [](Finished& f) { f.h.max_env = 0; f.h.n_small = ~0ull; f.plan.per_pair = true; });
    // a second pass over overflowed environments' pairs
    hints_case("h_subset", in, [](Finished& f) { f.subset = true; f.h.max_env = 400; f.h.n_duo = 600; f.h.n_unique[1] = 0; });
    hints_case("h_whole_pass_same_counts", in, [](Finished& f) { f.h.max_env = 400; f.h.n_duo = 600; f.h.n_unique[1] = 0; });
}

int main() {
    plan_cases();
    verdict_cases();
    hints_cases();
    return 0;
}
