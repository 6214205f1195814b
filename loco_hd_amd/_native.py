"""ctypes binding of libloco_hd_hip.so (the C ABI in include/loco_hd_hip.h).

This is the stub a maintainer of the reference would write instead of the PyO3 module
`loco_hd.loco_hd` (/root/reference/src/lib.rs:9-17).  The library is built in-tree by
`make -C loco_hd_amd/csrc` (or `__graft_entry__.build()`); if it is missing, importing any scoring
entry point fails loudly -- there is no Python/CPU fallback for the scoring path.
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os
import sys
from pathlib import Path

_PKG = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ["LCHD_LIB"]) if os.environ.get("LCHD_LIB") else _PKG / "libloco_hd_hip.so"  # LCHD_LIB: tuning builds

OK, EVALUE, EPANIC, EDEVICE, EUNSUPPORTED = 0, 1, 2, 3, 4


class PanicException(RuntimeError):
    """Raised where the reference's Rust core would panic (pyo3_runtime.PanicException)."""


class DeviceError(RuntimeError):
    """HIP failure or no usable MI355X: the scoring path has no CPU fallback."""


class WeightFunctionC(C.Structure):
    _fields_ = [("kind", C.c_int32), ("n_params", C.c_int32), ("params", C.POINTER(C.c_double))]


class ConfigC(C.Structure):
    _fields_ = [
        ("n_categories", C.c_int32),
        ("category_weights", C.POINTER(C.c_double)),
        ("n_weight_functions", C.c_int32),
        ("weight_functions", C.POINTER(WeightFunctionC)),
        ("sd_kind", C.c_int32),
        ("sd_n_params", C.c_int32),
        ("sd_params", C.c_double * 2),
        ("tag_mode", C.c_int32),
        ("tag_accept_same", C.c_int32),
        ("tag_accepted_pairs", C.c_int32),
        ("tag_ordered", C.c_int32),
        ("tag_pairs", C.POINTER(C.c_int32)),
        ("n_tag_pairs", C.c_int64),
    ]


class SweepQueryC(C.Structure):
    """lchd_sweep_query: what the choice of sweep kernels depends on (include/loco_hd_hip.h)."""
    _fields_ = [("n_pairs", C.c_int64), ("n_categories", C.c_int32), ("force_cmax", C.c_int32), ("hellinger2", C.c_int32),
                ("unit_weights", C.c_int32), ("wf_pow", C.c_int32), ("sd_fast", C.c_int32), ("has_wf_index", C.c_int32),
                ("has_left_list", C.c_int32), ("stride_a", C.c_int64), ("stride_b", C.c_int64), ("cdf_keys_a", C.c_int32),
                ("cdf_keys_b", C.c_int32), ("pre_rows", C.c_int32), ("hint_bits", C.c_int32), ("hooks", C.c_uint32)]


class SweepPlanC(C.Structure):
    """lchd_sweep_plan: what a pass launches."""
    _fields_ = [("families", C.c_uint32), ("slots", C.c_int32), ("pre", C.c_int32), ("small_rule", C.c_int32), ("second_rule", C.c_int32),
                ("c8_rule", C.c_int32), ("forced", C.c_int32), ("left_listing", C.c_int32), ("companion_left_out", C.c_int32),
                ("team_mode", C.c_int32), ("plain_mode", C.c_int32), ("ldstab", C.c_int32), ("fmode", C.c_int32), ("wide_long", C.c_int32),
                ("team_batch240", C.c_int32), ("team_grid240", C.c_int32), ("team_batch480", C.c_int32), ("team_grid480", C.c_int32)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class DenseQueryC(C.Structure):
    """lchd_dense_query: what the choice of the dense-row kernels depends on (include/loco_hd_hip.h)."""
    _fields_ = [("cols_a", C.c_int64), ("cols_b", C.c_int64), ("n_categories", C.c_int32), ("hellinger2", C.c_int32),
                ("unit_weights", C.c_int32), ("cat16", C.c_int32), ("given_rows", C.c_int32), ("ragged", C.c_int32), ("hooks", C.c_uint32),
                ("attempt", C.c_int32), ("single_attempt", C.c_int32), ("reserved", C.c_int32)]


class DenseRowsSideC(C.Structure):
    """lchd_dense_rows_side: one side of the k_env_rows path."""
    _fields_ = [("nt", C.c_int32), ("globalkv", C.c_int32), ("cat_bytes", C.c_int32), ("buckets", C.c_int32), ("cap", C.c_int32)]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class DensePlanC(C.Structure):
    """lchd_dense_plan: the path of a dense call and the instantiation of its kernels."""
    _fields_ = [("path", C.c_int32), ("unsupported", C.c_int32), ("fused_slots", C.c_int32), ("fused_dmx", C.c_int32), ("scr_segs", C.c_int32),
                ("nt", C.c_int32), ("ept", C.c_int32), ("seg", C.c_int32), ("n2", C.c_int32), ("rows", DenseRowsSideC * 2)]

    def as_dict(self) -> dict:
        rec = {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "rows"}
        rec["rows"] = [self.rows[0].as_dict(), self.rows[1].as_dict()]
        return rec


class DenseRecordC(C.Structure):
    """lchd_dense_record: what the most recent dense call ran."""
    _fields_ = [("plan", DensePlanC), ("attempts", C.c_int32), ("canon", C.c_int32), ("n_bitonic", C.c_int64)]


# lchd_dense_path / lchd_dense_hook
DENSE_NONE, DENSE_FUSED, DENSE_ROWS2, DENSE_ROWS = 0, 1, 2, 3
DENSE_HOOK_OLD_ROWS, DENSE_HOOK_NO_FUSED = 1, 2

# LCHD_SENSITIVITY_ROWS_LDS_POINTS: the longest (padded) dense row whose indexed list is sorted in LDS; longer ones are sorted in place
SENSITIVITY_ROWS_LDS_POINTS = 8192

# LCHD_GRAD_LIMBS / LCHD_GRAD_QUANTUM_LOG2 / LCHD_GRAD_LIMIT_LOG2: the exact accumulator of the native gradient calls
GRAD_LIMBS, GRAD_QUANTUM_LOG2, GRAD_LIMIT_LOG2 = 8, -192, 63

# lchd_sweep_family / lchd_sweep_hook bits
SWEEP_INLINE, SWEEP_TEAM240, SWEEP_TEAM480, SWEEP_C8, SWEEP_INDIRECT, SWEEP_PLAIN, SWEEP_INC, SWEEP_WIDE = (1 << k for k in range(8))
HOOK_NO_DUO, HOOK_NO_COUNT8, HOOK_NO_C8_TEAM, HOOK_NO_INLINE_META, HOOK_FORCE_WIDE, HOOK_FORCE_GENERIC, HOOK_FORCE_BIGENV, HOOK_NO_SWEEP_HINT = (
    1 << k for k in range(8))

_DP, _IP, _LP, _VP = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_void_p
_i32, _i64, _f64 = C.c_int32, C.c_int64, C.c_double

_PROTOS = {
    "lchd_last_error": (C.c_char_p, []),
    "lchd_version": (C.c_char_p, []),
    "lchd_wf_validate": (C.c_int, [_i32, _DP, _i32]),
    "lchd_wf_cdf": (C.c_int, [_i32, _DP, _i32, _DP, _i64, _DP]),
    "lchd_wf_pdf": (C.c_int, [_i32, _DP, _i32, _DP, _i64, _DP]),
    "lchd_wf_cdf_grad": (C.c_int, [_i32, _DP, _i32, _DP, _i64, _DP]),
    "lchd_sd_validate": (C.c_int, [_i32, _i32]),
    "lchd_sd_run": (C.c_int, [_i32, _DP, _DP, _DP, _i32, _DP]),
    "lchd_config_validate": (C.c_int, [_i64, _i64, _DP, _i64]),
    "lchd_ctx_create": (C.c_int, [_i32, C.POINTER(_VP)]),
    "lchd_ctx_destroy": (None, [_VP]),
    "lchd_ctx_set_stream": (C.c_int, [_VP, _VP]),
    "lchd_ctx_set_config": (C.c_int, [_VP, C.POINTER(ConfigC)]),
    "lchd_from_anchors": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _DP, _i64, _IP, _i64, _DP, _i64, _i32, _DP]),
    "lchd_from_dmxs": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _IP, _i64, _DP, _i64, _i64, _DP, _i64, _i64, _IP, _DP]),
    "lchd_from_dmxs_ragged": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _IP, _i64, _DP, _i64, _i64, _IP, _DP, _i64, _i64, _IP, _IP, _DP]),
    "lchd_from_coords": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _IP, _i64, _DP, _i64, _DP, _i64, _IP, _DP]),
    "lchd_from_primitives": (C.c_int, [_VP, C.POINTER(ConfigC), _DP, _IP, _IP, _i64, _DP, _IP, _IP, _i64, _LP, _IP, _i64, _f64, _DP]),
    "lchd_from_primitives_periodic": (C.c_int, [_VP, C.POINTER(ConfigC), _DP, _IP, _IP, _i64, _DP, _IP, _IP, _i64, _LP, _IP, _i64, _f64, _DP, _DP, _DP]),
    "lchd_box_validate": (C.c_int, [_DP, _i32, _f64]),
    "lchd_cloud_create_images": (C.c_int, [_VP, _VP, _DP, _i32, _f64, C.POINTER(_VP)]),
    "lchd_cloud_update_images": (C.c_int, [_VP, _VP, _VP, _DP, _i32]),
    "lchd_images_scan_span": (_i32, []),
    "lchd_cell_validate": (C.c_int, [_DP, _i32, _f64]),
    "lchd_cloud_create_images_cell": (C.c_int, [_VP, _VP, _DP, _i32, _f64, C.POINTER(_VP)]),
    "lchd_cloud_update_images_cell": (C.c_int, [_VP, _VP, _VP, _DP, _i32]),
    "lchd_from_primitives_periodic_cell": (C.c_int, [_VP, C.POINTER(ConfigC), _DP, _IP, _IP, _i64, _DP, _IP, _IP, _i64, _LP, _IP, _i64, _f64, _DP, _DP, _DP]),
    "lchd_cell_reduce": (C.c_int, [_DP, _DP, _DP]),
    "lchd_from_coords_periodic": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _IP, _i64, _DP, _i64, _DP, _i64, _IP, _DP, _DP, _DP]),
    "lchd_from_coords_periodic_dev": (C.c_int, [_VP, _VP, _VP, _VP, _DP, _DP, _VP]),
    "lchd_ensemble_from_coords_periodic": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _DP, _i64, _IP, _i64, _IP, _IP, _IP, _DP, _i32, _DP]),
    "lchd_ensemble_from_coords_periodic_dev": (C.c_int, [_VP, _VP, _VP, _i64, _VP, _VP, _VP, _DP, _i32, _VP]),
    "lchd_composition_primitives_dev": (C.c_int, [_VP, _VP, _VP, _VP, _i64, _f64, _VP]),
    "lchd_composition_primitives": (C.c_int, [_VP, C.POINTER(ConfigC), _DP, _IP, _IP, _i64, _LP, _IP, _i64, _f64, _DP]),
    "lchd_composition_primitives_periodic": (C.c_int, [_VP, C.POINTER(ConfigC), _DP, _IP, _IP, _i64, _LP, _IP, _i64, _f64, _DP, _DP, _DP]),
    "lchd_composition_coords_dev": (C.c_int, [_VP, _VP, _VP, _DP, _VP]),
    "lchd_composition_coords": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _DP, _i64, _IP, _DP, _DP]),
    "lchd_composition_dmx": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _DP, _i64, _i64, _IP, _DP]),
    "lchd_radial_validate": (C.c_int, [_DP, _i32]),
    "lchd_radial_primitives_dev": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _i64, _f64, _DP, _i32, _VP]),
    "lchd_radial_primitives": (C.c_int, [_VP, C.POINTER(ConfigC), _DP, _IP, _IP, _i64, _DP, _IP, _IP, _i64, _LP, _IP, _i64, _f64, _DP, _DP, _DP,
                                         _DP, _DP, _i32, _DP]),
    "lchd_radial_coords_dev": (C.c_int, [_VP, _VP, _VP, _VP, _DP, _DP, _DP, _i32, _VP]),
    "lchd_radial_coords": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _IP, _i64, _DP, _i64, _DP, _i64, _IP, _DP, _DP, _DP, _i32, _DP]),
    "lchd_radial_dmxs": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _IP, _i64, _DP, _DP, _i64, _i64, _i64, _IP, _DP, _i32, _DP]),
    "lchd_attribution_primitives_dev": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _i64, _f64, _VP]),
    "lchd_attribution_primitives": (C.c_int, [_VP, C.POINTER(ConfigC), _DP, _IP, _IP, _i64, _DP, _IP, _IP, _i64, _LP, _IP, _i64, _f64, _DP, _DP,
                                              _DP, _DP, _DP]),
    "lchd_attribution_coords_dev": (C.c_int, [_VP, _VP, _VP, _VP, _DP, _DP, _VP]),
    "lchd_attribution_coords": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _IP, _i64, _DP, _i64, _DP, _i64, _IP, _DP, _DP, _DP]),
    "lchd_attribution_dmxs": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _IP, _i64, _DP, _DP, _i64, _i64, _i64, _IP, _DP]),
    "lchd_category_gradient_primitives_dev": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _i64, _f64, _VP]),
    "lchd_category_gradient_primitives": (C.c_int, [_VP, C.POINTER(ConfigC), _DP, _IP, _IP, _i64, _DP, _IP, _IP, _i64, _LP, _IP, _i64, _f64, _DP,
                                                    _DP, _DP, _DP, _DP]),
    "lchd_category_gradient_coords_dev": (C.c_int, [_VP, _VP, _VP, _VP, _DP, _DP, _VP]),
    "lchd_category_gradient_coords": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _IP, _i64, _DP, _i64, _DP, _i64, _IP, _DP, _DP, _DP]),
    "lchd_category_gradient_dmxs": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _IP, _i64, _DP, _DP, _i64, _i64, _i64, _IP, _DP]),
    "lchd_weight_gradient_width": (_i32, [_VP]),
    "lchd_weight_gradient_primitives_dev": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _i64, _f64, _VP]),
    "lchd_weight_gradient_primitives": (C.c_int, [_VP, C.POINTER(ConfigC), _DP, _IP, _IP, _i64, _DP, _IP, _IP, _i64, _LP, _IP, _i64, _f64, _DP]),
    "lchd_weight_gradient_coords_dev": (C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    "lchd_weight_gradient_coords": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _IP, _i64, _DP, _DP, _i64, _IP, _DP]),
    "lchd_weight_gradient_dmxs": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _IP, _i64, _DP, _DP, _i64, _i64, _i64, _IP, _DP]),
    "lchd_sensitivity_primitives_dev": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _i64, _f64, _i32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lchd_sensitivity_primitives": (C.c_int, [_VP, C.POINTER(ConfigC), _DP, _IP, _IP, _i64, _DP, _IP, _IP, _i64, _LP, _IP, _i64, _f64, _i32,
                                              _DP, _IP, _IP, _DP, _DP, _IP, _IP, _DP, _DP]),
    "lchd_sensitivity_needed_width": (C.c_int64, [_VP]),
    "lchd_sensitivity_images_dev": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _i64, _f64, _i32, _VP] + [_VP] * 12),
    "lchd_sensitivity_primitives_periodic": (C.c_int, [_VP, C.POINTER(ConfigC), _DP, _IP, _IP, _i64, _DP, _IP, _IP, _i64, _LP, _IP, _i64, _f64,
                                                       _i32, _DP, _DP, _DP, _DP, _DP, _IP, _IP, _VP, _DP, _DP, _DP, _IP, _IP, _VP, _DP, _DP,
                                                       _DP]),
    "lchd_cloud_image_origin": (C.c_int, [_VP, _VP, _IP, _VP, _i64]),
    "lchd_cloud_home_size": (C.c_int64, [_VP]),
    "lchd_sensitivity_coords_dev": (C.c_int, [_VP, _VP, _VP, _VP, _i32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lchd_sensitivity_coords": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _IP, _i64, _DP, _DP, _i64, _IP, _i32,
                                          _DP, _IP, _IP, _DP, _DP, _IP, _IP, _DP, _DP]),
    "lchd_sensitivity_dmxs": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _IP, _i64, _DP, _DP, _i64, _i64, _i64, _IP, _i32,
                                        _DP, _IP, _IP, _DP, _DP, _IP, _IP, _DP, _DP]),
    "lchd_sensitivity_coords_periodic_dev": (C.c_int, [_VP, _VP, _VP, _VP, _DP, _DP, _i32] + [_VP] * 11),
    "lchd_sensitivity_coords_periodic": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _IP, _i64, _DP, _DP, _i64, _IP, _DP, _DP, _i32,
                                                   _DP, _IP, _IP, _DP, _DP, _IP, _IP, _DP, _DP, _DP, _DP]),
    "lchd_gradient_plan": (C.c_int, [_i64, _i32, _i64, _LP]),
    "lchd_gradient_primitives_dev": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _i64, _f64, _VP, _i64, _VP, _VP, _VP]),
    "lchd_gradient_primitives": (C.c_int, [_VP, C.POINTER(ConfigC), _DP, _IP, _IP, _i64, _DP, _IP, _IP, _i64, _LP, _IP, _i64, _f64, _DP, _i64,
                                           _DP, _DP, _DP]),
    "lchd_gradient_coords_dev": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lchd_gradient_coords": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _IP, _i64, _DP, _DP, _i64, _IP, _DP, _DP, _DP, _DP]),
    "lchd_gradient_plan_periodic": (C.c_int, [_i64, _i32, _i32, _i64, _LP]),
    "lchd_gradient_strain_waves": (C.c_int64, []),
    "lchd_gradient_images_dev": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _i64, _f64, _VP, _i64, _VP, _VP, _VP, _VP, _VP]),
    "lchd_gradient_primitives_periodic": (C.c_int, [_VP, C.POINTER(ConfigC), _DP, _IP, _IP, _i64, _DP, _IP, _IP, _i64, _LP, _IP, _i64, _f64,
                                                    _DP, _DP, _DP, _DP, _DP, _i64, _DP, _DP, _DP, _DP, _DP]),
    "lchd_gradient_coords_periodic_dev": (C.c_int, [_VP, _VP, _VP, _VP, _DP, _DP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lchd_gradient_coords_periodic": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _IP, _i64, _DP, _DP, _i64, _IP, _DP, _DP, _DP, _DP, _DP,
                                                _DP, _DP, _DP]),
    "lchd_param_sum_plan": (C.c_int, [_i64, _i32, _i64, _LP]),
    "lchd_category_gradient_sum_primitives_dev": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _i64, _f64, _VP, _i64, _VP]),
    "lchd_category_gradient_sum_primitives": (C.c_int, [_VP, C.POINTER(ConfigC), _DP, _IP, _IP, _i64, _DP, _IP, _IP, _i64, _LP, _IP, _i64, _f64,
                                                        _DP, _DP, _DP, _DP, _DP, _i64, _DP]),
    "lchd_category_gradient_sum_coords_dev": (C.c_int, [_VP, _VP, _VP, _VP, _DP, _DP, _VP, _VP]),
    "lchd_category_gradient_sum_coords": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _IP, _i64, _DP, _i64, _DP, _i64, _IP, _DP, _DP, _DP, _DP]),
    "lchd_weight_gradient_sum_primitives_dev": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _i64, _f64, _VP, _i64, _VP, _VP]),
    "lchd_weight_gradient_sum_primitives": (C.c_int, [_VP, C.POINTER(ConfigC), _DP, _IP, _IP, _i64, _DP, _IP, _IP, _i64, _LP, _IP, _i64, _f64,
                                                      _DP, _i64, _DP, _DP]),
    "lchd_weight_gradient_sum_coords_dev": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "lchd_weight_gradient_sum_coords": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _IP, _i64, _DP, _DP, _i64, _IP, _DP, _DP, _DP]),
    "lchd_cross_plan": (C.c_int, [_i64, _i64, _i64, _LP]),
    "lchd_cross_primitives_dev": (C.c_int, [_VP, _VP, _VP, _VP, _i64, _VP, _i64, _i32, _f64, _i64, _VP]),
    "lchd_nearest_primitives_dev": (C.c_int, [_VP, _VP, _VP, _VP, _i64, _VP, _i64, _i32, _f64, _i64, _i32, _VP, _VP]),
    "lchd_cross_primitives": (C.c_int, [_VP, C.POINTER(ConfigC), _DP, _IP, _IP, _i64, _DP, _IP, _IP, _i64, _LP, _i64, _LP, _i64, _i32, _f64, _i64,
                                        _DP]),
    "lchd_nearest_primitives": (C.c_int, [_VP, C.POINTER(ConfigC), _DP, _IP, _IP, _i64, _DP, _IP, _IP, _i64, _LP, _i64, _LP, _i64, _i32, _f64, _i64,
                                          _i32, _DP, _IP]),
    "lchd_cloud_create": (C.c_int, [_VP, _DP, _IP, _IP, _i64, C.POINTER(_VP)]),
    "lchd_cloud_create_batch": (C.c_int, [_VP, _DP, _IP, _IP, _IP, _i64, _i32, C.POINTER(_VP)]),
    "lchd_cloud_size": (C.c_int64, [_VP]),
    "lchd_cloud_structures": (_i32, [_VP]),
    "lchd_cloud_set_coords": (C.c_int, [_VP, _VP, _DP]),
    "lchd_cloud_destroy": (None, [_VP, _VP]),
    "lchd_from_primitives_dev": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _i64, _f64, _VP]),
    "lchd_from_primitives_dev_async": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _i64, _f64, _VP]),
    "lchd_ctx_finish": (C.c_int, [_VP]),
    "lchd_from_coords_dev": (C.c_int, [_VP, _VP, _VP, _VP, _VP]),
    "lchd_ensemble_from_coords_dev": (C.c_int, [_VP, _VP, _VP, _i64, _VP, _VP, _VP, _VP]),
    "lchd_ensemble_from_coords": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _DP, _i64, _IP, _i64, _IP, _IP, _IP, _DP]),
    "lchd_ensemble_from_dmxs": (C.c_int, [_VP, C.POINTER(ConfigC), _IP, _i64, _DP, _i64, _IP, _i64, _IP, _DP]),
    "lchd_frames_create": (C.c_int, [_VP, _VP, _i32, C.POINTER(_VP)]),
    "lchd_frames_load": (C.c_int, [_VP, _VP, _DP, _i32, _VP]),
    "lchd_frames_set_sources": (C.c_int, [_VP, _VP, _IP, _IP, _i64]),
    "lchd_frames_load_atoms": (C.c_int, [_VP, _VP, C.POINTER(C.c_float), _i32, _VP]),
    "lchd_frames_load_atoms_dev": (C.c_int, [_VP, _VP, _VP, _i32, _VP]),
    "lchd_frames_last_convert_ms": (C.c_double, [_VP, _VP]),
    "lchd_cloud_get_coords": (C.c_int, [_VP, _VP, _DP, _i64]),
    "lchd_group_create": (C.c_int, [_IP, _i32, C.POINTER(_VP)]),
    "lchd_group_destroy": (None, [_VP]),
    "lchd_group_size": (_i32, [_VP]),
    "lchd_group_from_primitives": (C.c_int, [_VP, C.POINTER(ConfigC), _DP, _IP, _IP, _i64, _DP, _IP, _IP, _i64, _LP, _IP, _i64, _f64, _DP]),
    "lchd_group_last_counts": (C.c_int, [_VP, _LP]),
    "lchd_shard_plan_dev": (C.c_int, [_VP, _VP, _i64, _i64, _i64, _i32, _LP]),
    "lchd_shard_select_dev": (C.c_int, [_VP, _VP, _i64, _i64, _i64, _i32, _VP, _VP]),
    "lchd_unshard_scores_dev": (C.c_int, [_VP, _VP, _LP, _i32, _i64, _VP, _i64]),
    "lchd_ctx_enable_timing": (C.c_int, [_VP, _i32]),
    "lchd_ctx_last_ms": (C.c_double, [_VP, C.c_char_p]),
    "lchd_ctx_last_env_points": (C.c_int64, [_VP]),
    "lchd_plan_grid": (C.c_int, [_DP, _DP, _i32, _f64, _i32, _IP, _DP, _LP]),
    "lchd_ctx_last_grid": (C.c_int, [_VP, _i32, _IP, _LP, _IP]),
    "lchd_ctx_last_anchors": (C.c_int, [_VP, _i32, _LP, _IP, _LP]),
    "lchd_plan_sweep": (C.c_int, [C.POINTER(SweepQueryC), C.POINTER(SweepPlanC)]),
    "lchd_ctx_last_sweep": (C.c_int, [_VP, C.POINTER(SweepPlanC), _LP, _IP, _IP]),
    "lchd_plan_dense": (C.c_int, [C.POINTER(DenseQueryC), C.POINTER(DensePlanC)]),
    "lchd_ctx_last_dense": (C.c_int, [_VP, C.POINTER(DenseRecordC)]),
    "lchd_ctx_last_dense_fused": (C.c_int32, [_VP]),
    "lchd_ctx_set_deterministic": (C.c_int, [_VP, _i32]),
    "lchd_ctx_get_deterministic": (C.c_int32, [_VP]),
    "lchd_ctx_pass_count": (C.c_int64, [_VP]),
    "lchd_ctx_subset_pass_count": (C.c_int64, [_VP]),
    "lchd_ctx_per_pair_pass_count": (C.c_int64, [_VP]),
    "lchd_ctx_last_store_bytes": (C.c_int64, [_VP]),
}

_lib = None


def _preload_torch_hip_runtime() -> None:
    """PyTorch-ROCm wheels bundle their own libamdhip64.so with the same soname as /opt/rocm's.  A process can only
    hold one of them: if ours pulled in the system runtime first, a later `import torch` would find no GPU.  So when
    torch is installed but not imported yet, map its bundled runtime first; our library then binds to it (exactly what
    happens when torch is imported first)."""
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    cand = Path(spec.origin).parent / "lib" / "libamdhip64.so"
    if cand.exists():
        try:
            C.CDLL(str(cand), mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """Load the HIP core.  Raises ImportError if it has not been built -- never falls back."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `make -C {_PKG / 'csrc'}` (hipcc --offload-arch=gfx950). "
                "loco_hd_amd has no CPU fallback for the scoring path."
            )
        _preload_torch_hip_runtime()
        handle = C.CDLL(str(LIB_PATH))
        for name, (res, args) in _PROTOS.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(rc: int) -> None:
    if rc == OK:
        return
    msg = lib().lchd_last_error().decode(errors="replace")
    if rc == EVALUE:
        raise ValueError(msg)
    if rc == EPANIC:
        raise PanicException(msg)
    if rc == EUNSUPPORTED:
        raise NotImplementedError(msg)
    raise DeviceError(msg)


def dp(a):
    return None if a is None else a.ctypes.data_as(_DP)


def ip(a):
    return None if a is None else a.ctypes.data_as(_IP)


def lp(a):
    return a.ctypes.data_as(_LP)
