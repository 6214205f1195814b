"""The decisions of a thresholded pass are pure host functions (loco_hd_amd/csrc/lchd_pass_plan.h: plan_pass, pass_verdict,
hints_after_pass, hints_for_repeat).  tests/pass_plan_cases.cpp runs them over a table of cases at every limit of every rule and
prints what they return; the expected values below are written out by hand from the rules, never taken from the functions.  No GPU, no
HIP: the header is compiled with the host compiler alone, which is itself part of what is tested."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
M22 = 1 << 22


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("a host C++ compiler is needed to build tests/pass_plan_cases.cpp")
    exe = tmp_path_factory.mktemp("pass_plan") / "pass_plan_cases"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "loco_hd_amd" / "csrc"),
                           str(ROOT / "tests" / "pass_plan_cases.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = {}
    for line in out.stdout.splitlines():
        name, _, rest = line.partition(": ")
        assert name not in got, f"case {name} printed twice"
        got[name] = dict(tok.split("=") for tok in rest.split())
    return got


def compare(cases, expected):
    wrong = []
    for name, want in expected.items():
        assert name in cases, f"the program printed no case {name}"
        for key, value in want.items():
            if cases[name][key] != str(value):
                wrong.append(f"{name}: {key} = {cases[name][key]}, expected {value}")
    assert not wrong, "\n".join(wrong)


def test_the_header_has_no_hip_include():
    text = (ROOT / "loco_hd_amd" / "csrc" / "lchd_pass_plan.h").read_text()
    assert "hip/" not in text and "__device__" not in text and "__global__" not in text


def test_constants(cases):
    """The limits the cases below are built from, as the headers have them today (a changed constant moves the cases with it; the
    numbers written out in the expectations below assume these)."""
    compare(cases, {"constants": dict(kEnvGroupCap=512, kEnvGroupCapSmall=320, kEnvGroupSmallUpTo=288, kMaxCategories=255, kMaxKeySets=4)})


def test_plan_group_and_slots(cases):
    compare(cases, {
        # two structures of 10 000 atoms, 5 000 pairs, 5 categories, Hellinger-2 on unit weights, capacity kEnvGroupCap
        "base": dict(same=0, cat16=0, max_env_a=5000, max_env_b=5000, group=1, group_small=0, per_pair=0, reach=2, dict_sets=0, key_sets=1,
                     pre_words=1, apw=1, tag_list=0),
        "group_cap_next": dict(group=0, reach=1, group_small=0, pre_words=0, apw=0),
        "group_na_below": dict(group=1, reach=2, max_env_a=5000),
        "group_na_at": dict(group=0, reach=1),
        "group_nb_at": dict(group=0, reach=1),
        "group_env_below": dict(group=1, max_env_a=M22 - 1, max_env_b=M22 - 1),
        "group_env_at": dict(group=0, max_env_a=M22, max_env_b=M22),
        "group_cat_at": dict(group=1, cat16=0),
        "group_cat_above": dict(group=0, cat16=1, reach=1),
        "group_hook": dict(group=0, reach=1),
        "group_small_hint": dict(group=1, group_small=1),
        "group_small_hint_not_group": dict(group=0, group_small=0),
        "tag_list": dict(tag_list=1),
        # max_env
        "same_few_pairs": dict(same=1, max_env_a=6000, max_env_b=0, group=1),     # min(n, 2 P)
        "same_many_pairs": dict(same=1, max_env_a=10000, max_env_b=0, group=1),
        "same_no_share": dict(same=0, max_env_a=3000, max_env_b=3000),
        "per_pair_slots": dict(per_pair=1, max_env_a=5000, max_env_b=5000),       # one slot per PAIR on a side of 3 000 atoms
        "regular_slots": dict(per_pair=0, max_env_a=5000, max_env_b=3000),
    })


def test_plan_per_pair(cases):
    compare(cases, {
        "pp_hinted": dict(per_pair=1, max_env_b=5000, pre_words=0),
        "pp_4096": dict(per_pair=0),
        "pp_4097": dict(per_pair=1, max_env_b=4097),
        "pp_streak_63": dict(per_pair=1),
        "pp_streak_64": dict(per_pair=0),
        "pp_pairs_eq_nb": dict(per_pair=1),
        "pp_pairs_eq_nb_plus_1": dict(per_pair=0),
        "pp_other_nb": dict(per_pair=0),
        "pp_2p_eq_hint": dict(per_pair=1),
        "pp_2p_eq_hint_minus_1": dict(per_pair=0),
        "pp_p_eq_2hint": dict(per_pair=1),
        "pp_p_eq_2hint_plus_1": dict(per_pair=0),
        "pp_not_hinted": dict(per_pair=0),
        "pp_tune_never": dict(per_pair=0),
        "pp_tune_always": dict(per_pair=1, max_env_a=100, max_env_b=100),
        "pp_deterministic": dict(per_pair=0),
        "pp_same": dict(per_pair=0, same=1),
        "pp_subset": dict(per_pair=0),
        "pp_not_group": dict(per_pair=0, group=0),
        "pp_pairs_below_2_22": dict(per_pair=1, group=1, max_env_a=10000, max_env_b=M22 - 1),
        "pp_pairs_at_2_22": dict(per_pair=0, group=1, max_env_a=10000, max_env_b=10000),
    })


def test_plan_key_sets(cases):
    k = int(cases["constants"]["kMaxKeySets"])
    expected = {f"keys_dict_{n}": dict(dict_sets=1, key_sets=n + 1) for n in range(2, k + 1)}
    expected[f"keys_dict_{k + 1}_too_many"] = dict(dict_sets=0, key_sets=0)
    expected.update({
        "base": dict(dict_sets=0, key_sets=1),
        "keys_no_index": dict(dict_sets=0, key_sets=0),
        "keys_finf_differ": dict(dict_sets=0, key_sets=0),
        "keys_no_key_sets": dict(dict_sets=0, key_sets=0),
        "keys_not_group": dict(dict_sets=0, key_sets=0),
        "keys_no_cdf_keys": dict(dict_sets=0, key_sets=0),
        "keys_no_cdf_keys_dict": dict(dict_sets=0, key_sets=0),
    })
    compare(cases, expected)


def test_plan_prefix_rows(cases):
    none = dict(pre_words=0)
    compare(cases, {
        "pre_slots_8": dict(pre_words=1), "pre_slots_9": dict(pre_words=2), "pre_slots_16": dict(pre_words=2), "pre_slots_17": none,
        "pre_force_cmax_9": dict(pre_words=2), "pre_force_cmax_17": none,
        "pre_pairs_4096": none, "pre_pairs_4097": dict(pre_words=1),
        "pre_rows_on_4096": dict(pre_words=1), "pre_no_inline_meta_4096": dict(pre_words=1), "pre_rows_off": none,
        "pre_per_pair": dict(pre_words=0, per_pair=1), "pre_deterministic": none, "pre_not_group": none,
        "pre_other_distance": none, "pre_kolmogorov_smirnov": dict(pre_words=1), "pre_weights": none, "pre_no_cdf_keys": none,
        "pre_no_duo": none, "pre_no_count8": none, "pre_no_c8_team": none, "pre_force_generic": none, "pre_force_wide": none,
        "pre_force_bigenv": none,
    })


def test_plan_anchors_per_wavefront(cases):
    compare(cases, {
        # 40 000 slots: the size rule alone
        "apw_unknown": dict(apw=2), "apw_140": dict(apw=4), "apw_141": dict(apw=2), "apw_small_up_to": dict(apw=2),
        "apw_small_up_to_plus_1": dict(apw=1),
        # environments of 100 points (four per wavefront), clamped to slots / 8192, at least 1
        "apw_total_8191": dict(apw=1), "apw_total_8192": dict(apw=1), "apw_total_16383": dict(apw=1), "apw_total_16384": dict(apw=2),
        "apw_total_32767": dict(apw=3), "apw_total_32768": dict(apw=4),
        "apw_override": dict(apw=7), "apw_not_group": dict(apw=0),
    })


def test_verdict(cases):
    compare(cases, {
        "v_stands": dict(verdict="STANDS", biggest=200, overflowed=0, grown_cap=0),
        "v_bad_anchor": dict(verdict="BAD_ANCHOR"),
        "v_other_flags_stand": dict(verdict="STANDS"),
        "v_small_group_at_cap": dict(verdict="REPEAT_REGULAR", biggest=512, overflowed=1),
        "v_small_group_above_cap": dict(verdict="OVERFLOW", grown_cap=1024),
        "v_regular_group_at_cap": dict(verdict="OVERFLOW", grown_cap=1024),       # max(512, 0, 512 + 1)
        "v_left_out_one_pair_missing": dict(verdict="REPEAT_FULL_SET", overflowed=0),
        "v_left_out_all_taken": dict(verdict="STANDS"),
        "v_left_out_c8_one_missing": dict(verdict="REPEAT_FULL_SET"),
        "v_left_out_c8_all_taken": dict(verdict="STANDS"),
        "v_companion_ran": dict(verdict="STANDS"),
        "v_left_out_not_counted": dict(verdict="STANDS"),
        "v_overflow_left_out_one_missing": dict(verdict="REPEAT_FULL_SET", overflowed=1),   # before any second pass over the overflowed pairs
        "v_overflow_left_out_all_taken": dict(verdict="OVERFLOW", grown_cap=1024),
        "v_overflow_left_out_not_counted": dict(verdict="OVERFLOW", grown_cap=1024),
        "v_small_group_before_full_set": dict(verdict="REPEAT_REGULAR"),
        "v_wide_65535": dict(verdict="OVERFLOW", grown_cap=65536),
        "v_wide_65536": dict(verdict="UNSUPPORTED", biggest=65536),
        "v_long_2_23": dict(verdict="OVERFLOW", grown_cap=1 << 23),
        "v_long_2_23_plus_1": dict(verdict="UNSUPPORTED", biggest=(1 << 23) + 1),
        "v_long_not_overflowed": dict(verdict="STANDS", biggest=70000),
        "v_grow_third_of_bound": dict(verdict="OVERFLOW", grown_cap=2048),        # max(700, 6000 / 3, 513)
        "v_grow_subset_whole_bound": dict(verdict="OVERFLOW", grown_cap=8192),    # max(700, 6000, 513)
        "v_grow_biggest": dict(verdict="OVERFLOW", grown_cap=8192),               # max(5000, 3000, 513)
        "v_grow_cap_plus_1": dict(verdict="OVERFLOW", grown_cap=2048),            # max(600, 0, 1025)
        "v_grow_exact_power": dict(verdict="OVERFLOW", grown_cap=1024),           # max(1024, 1024, 513)
    })


R_INPUT = dict(cap_hint=1024, shrink_votes=5, sweep_hint=31, group_small=1, last_biggest=100, last_left=9, b_use_once=1, use_once_pairs=77,
               use_once_nb=88, per_pair_streak=3)


def test_hints_for_a_repeat(cases):
    compare(cases, {
        "r_input": R_INPUT,
        "r_regular_at_cap": dict(R_INPUT, group_small=0, last_biggest=512),
        "r_regular_small_biggest": dict(R_INPUT, group_small=0, last_biggest=321),          # at least kEnvGroupCapSmall + 1
        "r_full_set_after_overflow": dict(R_INPUT, sweep_hint=7),
        "r_full_set_fitted": dict(R_INPUT, sweep_hint=7, shrink_votes=6),
        "r_full_set_fitted_subset": dict(R_INPUT, sweep_hint=7),
        "r_grow": dict(R_INPUT, cap_hint=2048, shrink_votes=0),
        "r_grow_subset": R_INPUT,
    })


# 1 000 pairs on a side B of 10 000 atoms, largest environment 200 points, a record pass that counted no small pair and no unique
# side-B anchor, starting from default hints
H_PLAIN = dict(cap_hint=512, shrink_votes=0, sweep_hint=4, group_small=1, last_biggest=200, last_left=1000, b_use_once=0,
               use_once_pairs=1000, use_once_nb=10000, per_pair_streak=0)
H_INPUT = dict(cap_hint=2048, shrink_votes=7, sweep_hint=31, group_small=1, last_biggest=100, last_left=9, b_use_once=1, use_once_pairs=77,
               use_once_nb=88, per_pair_streak=3)


def test_hints_after_a_pass(cases):
    compare(cases, {
        "h_vote_7": dict(H_PLAIN, cap_hint=2048, shrink_votes=7, group_small=0, last_biggest=500),
        "h_vote_8": dict(cap_hint=1024, shrink_votes=0),
        "h_vote_8_to_512": dict(cap_hint=512, shrink_votes=0),
        "h_vote_floor": dict(cap_hint=512, shrink_votes=0),
        "h_vote_at_512": dict(cap_hint=512, shrink_votes=0),
        "h_vote_fits_exactly_half": dict(cap_hint=2048, shrink_votes=4),
        "h_vote_reset": dict(cap_hint=2048, shrink_votes=0),
        "h_vote_reset_unknown": dict(cap_hint=2048, shrink_votes=0, group_small=0, last_biggest=0),
        "h_duo_half": dict(H_PLAIN, sweep_hint=4 | 1, last_left=500),
        "h_duo_below_half": dict(H_PLAIN, sweep_hint=4, last_left=501),
        "h_duo_all": dict(H_PLAIN, sweep_hint=4 | 1 | 8, last_left=0),
        "h_duo_all_but_one": dict(H_PLAIN, sweep_hint=4 | 1, last_left=1),
        "h_c8_half": dict(H_PLAIN, sweep_hint=4 | 2),
        "h_c8_below_half": dict(H_PLAIN, sweep_hint=4),
        "h_c8_all": dict(H_PLAIN, sweep_hint=4 | 2 | 16),
        "h_c8_all_but_one": dict(H_PLAIN, sweep_hint=4 | 2),
        "h_both_all": dict(H_PLAIN, sweep_hint=31, last_left=0),
        "h_not_counted": dict(H_PLAIN, sweep_hint=13, last_left=42),
        "hint_formula": dict(half_with_all=5, all_with_all=13, all_without_all=5, c8_all_without_all=6),
        "h_use_once_at_four_fifths": dict(H_PLAIN, b_use_once=1, use_once_nb=1234),
        "h_use_once_below": dict(H_PLAIN, b_use_once=0, use_once_nb=1234),
        "h_use_once_same": dict(H_PLAIN, b_use_once=0),
        "h_regular_pass_ends_streak": dict(H_PLAIN, b_use_once=1, use_once_pairs=1000, use_once_nb=4321, per_pair_streak=0),
        "h_per_pair_fifth_repeated": dict(H_PLAIN, b_use_once=1, use_once_pairs=1000, use_once_nb=1234, per_pair_streak=6),
        "h_per_pair_over_a_fifth": dict(H_PLAIN, b_use_once=0, use_once_pairs=1000, use_once_nb=1234, per_pair_streak=6, last_left=1004),
        "h_per_pair_1004_at_200": dict(H_PLAIN, b_use_once=1, use_once_pairs=1000, use_once_nb=1234, per_pair_streak=6, last_left=1004),
        "h_left_100": dict(H_PLAIN, sweep_hint=4 | 1 | 2 | 16, last_left=100),
        "h_left_c8_rule": dict(H_PLAIN, sweep_hint=4 | 1 | 2 | 16, last_left=0),
        "h_left_clamped": dict(last_left=0),
        "h_biggest_small_up_to": dict(H_PLAIN, group_small=1, last_biggest=288),
        "h_biggest_small_up_to_plus_1": dict(H_PLAIN, group_small=0, last_biggest=289),
        "h_biggest_unknown": dict(H_INPUT, shrink_votes=0, per_pair_streak=4),
        # a second pass over overflowed environments' pairs: group_small, last_biggest and sweep_hint alone
        "h_subset": dict(H_INPUT, group_small=0, last_biggest=400, sweep_hint=4 | 1),
        "h_whole_pass_same_counts": dict(cap_hint=1024, shrink_votes=0, sweep_hint=4 | 1, group_small=0, last_biggest=400, last_left=400,
                                         b_use_once=0, use_once_pairs=1000, use_once_nb=10000, per_pair_streak=0),
    })
