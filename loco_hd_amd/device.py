"""Device-resident scoring session (additive API; what bench.py, the multi-GPU sharding and batch callers use).

The reference API is one structure pair per call with everything copied in and out
(/root/reference/src/locohd.rs:479-567).  A `DeviceSession` keeps the two structures in HBM as SoA arrays,
takes anchor pairs / scores as torch CUDA tensors (torch is only the allocator and the stream provider
here) and runs the same kernels through `lchd_from_primitives_dev`.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _native as N
from .api import _CATEGORY_GRADIENT, LoCoHD, MinImageSensitivity, NativeGradient, Nearest, PeriodicSensitivity, Sensitivity, WeightGradient, WeightGradientSum, dense_cells, periodic_boxes, periodic_cells


def last_sweep_of(ctx):
    """lchd_ctx_last_sweep of a context handle as a dict (DeviceSession.last_sweep), or None."""
    plan, stats, rule, repeated = N.SweepPlanC(), (C.c_int64 * 4)(), C.c_int32(), C.c_int32()
    if N.lib().lchd_ctx_last_sweep(ctx, C.byref(plan), stats, C.byref(rule), C.byref(repeated)) != 0:
        return None
    rec = plan.as_dict()
    rec.update(n_duo=int(stats[0]), n_c8=int(stats[1]), max_env=int(stats[2]), left=int(stats[3]), rule=int(rule.value),
               repeated=bool(repeated.value))
    return rec


def last_dense_of(ctx):
    """lchd_ctx_last_dense of a context handle as a dict (DeviceSession.last_dense), or None."""
    rec = N.DenseRecordC()
    if N.lib().lchd_ctx_last_dense(ctx, C.byref(rec)) != 0:
        return None
    out = rec.plan.as_dict()
    out.update(attempts=int(rec.attempts), canon=bool(rec.canon), n_bitonic=int(rec.n_bitonic))
    return out


def last_anchors_of(ctx):
    """lchd_ctx_last_anchors of a context handle as a list of two dicts (DeviceSession.last_anchors), or None."""
    sides = []
    for side in (0, 1):
        n_unique, mode, n_repeated = C.c_int64(), C.c_int32(), C.c_int64()
        if N.lib().lchd_ctx_last_anchors(ctx, side, C.byref(n_unique), C.byref(mode), C.byref(n_repeated)) != 0:
            return None
        sides.append({"mode": int(mode.value), "n_unique": int(n_unique.value), "n_repeated": int(n_repeated.value)})
    return sides


class DeviceSession:
    def __init__(self, lchd: LoCoHD, device: Optional[int] = None, interner: Optional[dict] = None):
        import torch

        self.torch = torch
        if not torch.cuda.is_available():
            raise N.DeviceError("no usable HIP device: loco_hd_amd has no CPU fallback for the scoring path")
        self.device = torch.cuda.current_device() if device is None else int(device)
        torch.cuda.set_device(self.device)
        self.lchd = lchd
        self._ctx = C.c_void_p()
        N.check(N.lib().lchd_ctx_create(self.device, C.byref(self._ctx)))
        self._cfg, self._keep = lchd._config(interner)
        N.check(N.lib().lchd_ctx_set_config(self._ctx, C.byref(self._cfg)))
        if getattr(lchd, "_deterministic", False):
            self.set_deterministic(True)
        self.use_current_stream()
        self._clouds = []

    def use_current_stream(self):
        """Move the session to torch's current stream on its device (lchd_ctx_set_stream; non-blocking side streams are fine).

        The call first waits for everything the session has queued on the stream it leaves, and raises ValueError while an
        asynchronous pass is pending (the pass stays intact).  Afterwards every CUDA tensor handed to a scoring call (anchors,
        wf_index, pairs, out) is read and written in the order of THAT stream: torch kernels queued on it before the call may
        still be filling them, and no synchronise is needed in between.  from_primitives / from_coords / from_coords_ensemble /
        finish return with `out` complete (the host has waited), so it may be read from any stream; from_primitives_async only
        queues the pass.  Host arrays (upload, set_coords, load_frames, load_atom_frames) are read before the call returns.  A
        frames load runs on the `stream=` it is given, behind what that stream holds (the producer of a load_atom_frames_dev
        tensor included) and behind the last pass that read the buffer; whatever reads the buffer later waits for the load.
        The one input that must be complete when it is passed is the pair list of the sharding plan (dist.select_shard /
        score_sharded).  tests/test_gpu_streams.py enforces this with delayed producers (include/loco_hd_hip.h, "Streams", names the two
        internal stream waits that the host-side waits make unobservable)."""
        s = self.torch.cuda.current_stream(self.device).cuda_stream
        N.check(N.lib().lchd_ctx_set_stream(self._ctx, C.c_void_p(s)))

    def set_deterministic(self, on: bool = True):
        """Pin one sweep kernel family (lchd_ctx_set_deterministic): a pair's score then depends on the pair and the configuration
        only, bit for bit, whatever the batch, the call history or the sharding -- at about half the default throughput."""
        N.check(N.lib().lchd_ctx_set_deterministic(self._ctx, int(bool(on))))

    def enable_timing(self, on: bool = True):
        N.lib().lchd_ctx_enable_timing(self._ctx, int(on))

    def last_ms(self) -> dict:
        return {k: N.lib().lchd_ctx_last_ms(self._ctx, k.encode()) for k in ("cells", "anchors", "env", "sweep")}

    def last_env_points(self) -> int:
        return int(N.lib().lchd_ctx_last_env_points(self._ctx))

    def last_grid(self):
        """Grid and cell-list build of both sides of the most recent thresholded pass (lchd_ctx_last_grid): a list of two dicts
        {"dims": (d0, d1, d2), "n_cells": int, "build": 0 .. 4}, or None where last_env_points() would return -1."""
        sides = []
        for side in (0, 1):
            dims, n_cells, build = (C.c_int32 * 3)(), C.c_int64(), C.c_int32()
            if N.lib().lchd_ctx_last_grid(self._ctx, side, dims, C.byref(n_cells), C.byref(build)) != 0:
                return None
            sides.append({"dims": tuple(dims), "n_cells": int(n_cells.value), "build": int(build.value)})
        return sides

    def last_anchors(self):
        """Anchor de-duplication of both sides of the same pass (lchd_ctx_last_anchors): a list of two dicts {"mode": 0 shared with
        side A / 1 fused / 2 one-workgroup scan / 3 chunked / 4 per pair, "n_unique": environments built for the side as the device
        counted them, "n_repeated": -1, or in mode 4 the pairs whose side-B anchor an earlier pair had used}; None where last_grid()
        returns None."""
        return last_anchors_of(self._ctx)

    def last_sweep(self):
        """Sweep kernels of the most recent from_primitives call's last pass (lchd_ctx_last_sweep): the fields of lchd_sweep_plan
        ("families" is a mask of the _native.SWEEP_* bits) plus "n_duo", "n_c8", "max_env", "left" (what the record pass counted; -1
        where none ran), "rule" (the rule in force: -1, 0, 1, 2) and "repeated" (the pass repeated one whose companion sweep had been
        left out); None where last_grid() returns None."""
        return last_sweep_of(self._ctx)

    def last_dense(self):
        """What the most recent from_coords / from_coords_ensemble call ran (lchd_ctx_last_dense): the fields of lchd_dense_plan for the
        attempt whose scores stand ("path" is one of the _native.DENSE_* values, "rows" a list of two dicts) plus "attempts" (1, or 2: a
        row defeated the first kernel and the call was repeated), "canon" (the tie-canonicalisation kernel ran) and "n_bitonic" (rows
        whose sort took the bitonic network); None before the first dense call and after one that failed."""
        return last_dense_of(self._ctx)

    def last_dense_fused(self) -> bool:
        """True if the most recent from_coords call ran the fused sort + sweep kernel (lchd_ctx_last_dense_fused)."""
        return bool(N.lib().lchd_ctx_last_dense_fused(self._ctx))

    def pass_counts(self) -> dict:
        """Passes the context has run: all of them, and the second passes over the pairs of overflowed environments
        (lchd_ctx_pass_count, lchd_ctx_subset_pass_count); store_bytes: environment-store bytes of the last call's passes."""
        lib = N.lib()
        return {"passes": int(lib.lchd_ctx_pass_count(self._ctx)), "subset_passes": int(lib.lchd_ctx_subset_pass_count(self._ctx)),
                "per_pair_passes": int(lib.lchd_ctx_per_pair_pass_count(self._ctx)),
                "store_bytes": int(lib.lchd_ctx_last_store_bytes(self._ctx))}

    def upload(self, xyz: np.ndarray, cat: np.ndarray, tag: Optional[np.ndarray] = None):
        """Put one structure (xyz [n][3] f64, category ids, interned tags) into HBM; returns an opaque handle."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        cat = np.ascontiguousarray(cat, dtype=np.int32)
        tag = np.zeros(len(cat), dtype=np.int32) if tag is None else np.ascontiguousarray(tag, dtype=np.int32)
        h = C.c_void_p()
        N.check(N.lib().lchd_cloud_create(self._ctx, N.dp(xyz), N.ip(cat), N.ip(tag), len(xyz), C.byref(h)))
        self._clouds.append(h)
        return h

    def upload_batch(self, structures):
        """Put MANY structures into HBM as one object.  `structures` = sequence of (xyz [n_k][3], cat [n_k], tag [n_k] or
        None).  Returns (handle, offsets): atom j of structure k is global atom offsets[k] + j -- the index to use in the
        anchor tensor; environments never mix atoms of different structures."""
        xs, cs, ts, ss, offs = [], [], [], [], [0]
        for k, st in enumerate(structures):
            xyz = np.ascontiguousarray(st[0], dtype=np.float64).reshape(-1, 3)
            cat = np.ascontiguousarray(st[1], dtype=np.int32)
            tag = np.zeros(len(cat), dtype=np.int32) if len(st) < 3 or st[2] is None else np.ascontiguousarray(st[2], dtype=np.int32)
            xs.append(xyz); cs.append(cat); ts.append(tag); ss.append(np.full(len(cat), k, dtype=np.int32))
            offs.append(offs[-1] + len(cat))
        xyz, cat, tag, sid = np.concatenate(xs), np.concatenate(cs), np.concatenate(ts), np.concatenate(ss)
        h = C.c_void_p()
        N.check(N.lib().lchd_cloud_create_batch(self._ctx, N.dp(xyz), N.ip(cat), N.ip(tag), N.ip(sid), len(xyz), len(structures),
                                                C.byref(h)))
        self._clouds.append(h)
        return h, np.asarray(offs, dtype=np.int64)

    def set_coords(self, cloud, xyz: np.ndarray):
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        N.check(N.lib().lchd_cloud_set_coords(self._ctx, cloud, N.dp(xyz)))

    def periodic_images(self, cloud, box=None, reach: float = None, *, cell=None):
        """The periodic images of an uploaded structure / batch / frames buffer as a cloud of its own (lchd_cloud_create_images):
        the wrapped atoms at their indices, then every image within `reach` of the orthorhombic `box` (Lx, Ly, Lz; one, or one
        per structure).  Use it in place of `cloud` in from_primitives with threshold_distance <= reach <= the smallest edge;
        the session owns it like any other cloud.

        `cell` (keyword-only) in place of `box`: a triclinic cell, 3 x 3 with the lattice vectors as rows (one, or one per structure;
        lchd_cloud_create_images_cell); reach <= its smallest perpendicular width."""
        if (box is None) == (cell is None):
            raise ValueError("periodic_images takes a box or a cell" + (", not both" if box is not None else "; neither was given"))
        if reach is None:
            raise ValueError("periodic_images needs the reach of the images (the largest threshold_distance to be used)")
        h = C.c_void_p()
        if cell is not None:
            arr = periodic_cells(cell, self._n_structures(cloud), reach)
            N.check(N.lib().lchd_cloud_create_images_cell(self._ctx, cloud, N.dp(arr), len(arr), float(reach), C.byref(h)))
        else:
            arr = periodic_boxes(box, self._n_structures(cloud), reach)
            N.check(N.lib().lchd_cloud_create_images(self._ctx, cloud, N.dp(arr), len(arr), float(reach), C.byref(h)))
        self._clouds.append(h)
        return h

    def update_images(self, images, cloud, box=None, *, cell=None):
        """Rebuild an image cloud in place from the current coordinates of `cloud` (lchd_cloud_update_images); its reach stays.
        A cloud made with `cell=` is updated with `cell=` (lchd_cloud_update_images_cell), one made with a box with `box`."""
        if (box is None) == (cell is None):
            raise ValueError("update_images takes a box or a cell" + (", not both" if box is not None else "; neither was given"))
        if cell is not None:
            arr = np.ascontiguousarray(cell, dtype=np.float64)
            arr = arr.reshape(1, 3, 3) if arr.shape == (3, 3) else arr
            if arr.ndim != 3 or arr.shape[1:] != (3, 3):
                raise ValueError(f"cell must be a 3 x 3 matrix of lattice vectors (rows a, b, c), got an array of shape {arr.shape}")
            N.check(N.lib().lchd_cloud_update_images_cell(self._ctx, images, cloud, N.dp(arr), len(arr)))
            return
        arr = np.ascontiguousarray(box, dtype=np.float64)
        arr = arr.reshape(1, 3) if arr.shape == (3,) else arr
        if arr.ndim != 2 or arr.shape[1] != 3:
            raise ValueError(f"box must be three edge lengths (Lx, Ly, Lz), got an array of shape {arr.shape}")
        N.check(N.lib().lchd_cloud_update_images(self._ctx, images, cloud, N.dp(arr), len(arr)))

    def from_primitives(self, cloud_a, cloud_b, anchors, threshold_distance: float, out=None, wf_index=None):
        """anchors: torch int64 CUDA tensor [P][2]; returns (or fills) a torch float64 CUDA tensor [P]."""
        torch = self.torch
        assert anchors.is_cuda and anchors.dtype == torch.int64 and anchors.is_contiguous()
        p = anchors.shape[0]
        if out is None:
            out = torch.empty(p, dtype=torch.float64, device=anchors.device)
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= p
        wf_ptr = None
        if wf_index is not None:
            assert wf_index.is_cuda and wf_index.dtype == torch.int32 and wf_index.is_contiguous()
            wf_ptr = C.c_void_p(wf_index.data_ptr())
        N.check(N.lib().lchd_from_primitives_dev(self._ctx, cloud_a, cloud_b, C.c_void_p(anchors.data_ptr()), wf_ptr, p,
                                                 float(threshold_distance), C.c_void_p(out.data_ptr())))
        return out

    def from_coords(self, cloud_a, cloud_b, out=None, wf_index=None, *, box_a=None, box_b=None, cell_a=None, cell_b=None):
        """LoCoHD.from_coords on two uploaded structures of equal size: pair r = (atom r, atom r), environments = the whole
        structures.  Returns (or fills) a torch float64 CUDA tensor [n].

        `box_a` / `box_b` / `cell_a` / `cell_b` (keyword-only, host arrays): the periodic box (Lx, Ly, Lz) or cell (3 x 3) of a side;
        its rows then follow the minimum-image convention (LoCoHD.from_coords; lchd_from_coords_periodic_dev)."""
        for side, box, cell in (("a", box_a, cell_a), ("b", box_b, cell_b)):
            if box is not None and cell is not None:
                raise ValueError(f"box_{side} and cell_{side} were both given: a structure has one periodic box or one periodic cell")
        pc_a = dense_cells(box_a, cell_a, 1, "box_a", "cell_a")
        pc_b = dense_cells(box_b, cell_b, 1, "box_b", "cell_b")
        torch = self.torch
        n = int(N.lib().lchd_cloud_size(cloud_a))
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=torch.device("cuda", self.device))
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= n
        wf_ptr = None
        if wf_index is not None:
            assert wf_index.is_cuda and wf_index.dtype == torch.int32 and wf_index.is_contiguous() and wf_index.numel() >= n
            wf_ptr = C.c_void_p(wf_index.data_ptr())
        if pc_a is not None or pc_b is not None:
            N.check(N.lib().lchd_from_coords_periodic_dev(self._ctx, cloud_a, cloud_b, wf_ptr, N.dp(pc_a), N.dp(pc_b), C.c_void_p(out.data_ptr())))
            return out
        N.check(N.lib().lchd_from_coords_dev(self._ctx, cloud_a, cloud_b, wf_ptr, C.c_void_p(out.data_ptr())))
        return out

    def composition(self, cloud, anchors, threshold_distance: float, out=None, wf_index=None):
        """Composition profiles (LoCoHD.composition_from_primitives) of anchors of an uploaded structure, batch, frames buffer or
        image cloud.  anchors: torch int64 CUDA tensor [P] of global atom indices (repeats allowed); wf_index: torch int32 CUDA tensor
        [P] or None; returns (or fills) a torch float64 CUDA tensor [P][C] (lchd_composition_primitives_dev)."""
        torch = self.torch
        assert anchors.is_cuda and anchors.dtype == torch.int64 and anchors.is_contiguous() and anchors.dim() == 1
        p, n_cat = anchors.shape[0], int(self._cfg.n_categories)
        if out is None:
            out = torch.empty((p, n_cat), dtype=torch.float64, device=anchors.device)
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= p * n_cat
        wf_ptr = None
        if wf_index is not None:
            assert wf_index.is_cuda and wf_index.dtype == torch.int32 and wf_index.is_contiguous() and wf_index.numel() >= p
            wf_ptr = C.c_void_p(wf_index.data_ptr())
        N.check(N.lib().lchd_composition_primitives_dev(self._ctx, cloud, C.c_void_p(anchors.data_ptr()), wf_ptr, p,
                                                        float(threshold_distance), C.c_void_p(out.data_ptr())))
        return out

    def composition_coords(self, cloud, out=None, wf_index=None, *, box=None, cell=None):
        """Composition profiles of the dense rows of an uploaded structure (LoCoHD.composition_from_coords): returns (or fills) a torch
        float64 CUDA tensor [n][C].  `box` / `cell` (keyword-only, host arrays): minimum-image rows (lchd_composition_coords_dev)."""
        if box is not None and cell is not None:
            raise ValueError("box and cell were both given: a structure has one periodic box or one periodic cell")
        pc = dense_cells(box, cell, 1, "box", "cell")
        torch = self.torch
        n, n_cat = int(N.lib().lchd_cloud_size(cloud)), int(self._cfg.n_categories)
        if out is None:
            out = torch.empty((n, n_cat), dtype=torch.float64, device=torch.device("cuda", self.device))
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= n * n_cat
        wf_ptr = None
        if wf_index is not None:
            assert wf_index.is_cuda and wf_index.dtype == torch.int32 and wf_index.is_contiguous() and wf_index.numel() >= n
            wf_ptr = C.c_void_p(wf_index.data_ptr())
        N.check(N.lib().lchd_composition_coords_dev(self._ctx, cloud, wf_ptr, N.dp(pc), C.c_void_p(out.data_ptr())))
        return out

    @staticmethod
    def _radial_edges(edges) -> np.ndarray:
        ed = np.ascontiguousarray(np.asarray(edges, dtype=np.float64).reshape(-1))
        N.check(N.lib().lchd_radial_validate(N.dp(ed), len(ed)))
        return ed

    # `ed`: the checked edges of a radial call (rows of len(ed) - 1 bins), None: an attribution, or _CATEGORY_GRADIENT: a category-weight
    # gradient (rows of C categories)
    def _pair_rows(self, ed, cloud_a, cloud_b, anchors, threshold_distance, out, wf_index):
        torch = self.torch
        assert anchors.is_cuda and anchors.dtype == torch.int64 and anchors.is_contiguous()
        p, k = anchors.shape[0], int(self._cfg.n_categories) if ed is None or ed is _CATEGORY_GRADIENT else len(ed) - 1
        if out is None:
            out = torch.empty((p, k), dtype=torch.float64, device=anchors.device)
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= p * k
        wf_ptr = None
        if wf_index is not None:
            assert wf_index.is_cuda and wf_index.dtype == torch.int32 and wf_index.is_contiguous() and wf_index.numel() >= p
            wf_ptr = C.c_void_p(wf_index.data_ptr())
        head = (self._ctx, cloud_a, cloud_b, C.c_void_p(anchors.data_ptr()), wf_ptr, p, float(threshold_distance))
        if ed is _CATEGORY_GRADIENT:
            N.check(N.lib().lchd_category_gradient_primitives_dev(*head, C.c_void_p(out.data_ptr())))
        elif ed is None:
            N.check(N.lib().lchd_attribution_primitives_dev(*head, C.c_void_p(out.data_ptr())))
        else:
            N.check(N.lib().lchd_radial_primitives_dev(*head, N.dp(ed), len(ed), C.c_void_p(out.data_ptr())))
        return out

    def _pair_rows_coords(self, ed, cloud_a, cloud_b, out, wf_index, box_a, box_b, cell_a, cell_b):
        for side, box, cell in (("a", box_a, cell_a), ("b", box_b, cell_b)):
            if box is not None and cell is not None:
                raise ValueError(f"box_{side} and cell_{side} were both given: a structure has one periodic box or one periodic cell")
        pc_a = dense_cells(box_a, cell_a, 1, "box_a", "cell_a")
        pc_b = dense_cells(box_b, cell_b, 1, "box_b", "cell_b")
        torch = self.torch
        n, k = int(N.lib().lchd_cloud_size(cloud_a)), int(self._cfg.n_categories) if ed is None or ed is _CATEGORY_GRADIENT else len(ed) - 1
        if out is None:
            out = torch.empty((n, k), dtype=torch.float64, device=torch.device("cuda", self.device))
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= n * k
        wf_ptr = None
        if wf_index is not None:
            assert wf_index.is_cuda and wf_index.dtype == torch.int32 and wf_index.is_contiguous() and wf_index.numel() >= n
            wf_ptr = C.c_void_p(wf_index.data_ptr())
        head = (self._ctx, cloud_a, cloud_b, wf_ptr, N.dp(pc_a), N.dp(pc_b))
        if ed is _CATEGORY_GRADIENT:
            N.check(N.lib().lchd_category_gradient_coords_dev(*head, C.c_void_p(out.data_ptr())))
        elif ed is None:
            N.check(N.lib().lchd_attribution_coords_dev(*head, C.c_void_p(out.data_ptr())))
        else:
            N.check(N.lib().lchd_radial_coords_dev(*head, N.dp(ed), len(ed), C.c_void_p(out.data_ptr())))
        return out

    def radial(self, cloud_a, cloud_b, anchors, threshold_distance: float, edges, out=None, wf_index=None):
        """Radial profiles (LoCoHD.radial_from_primitives) of anchor pairs of two uploaded clouds of any kind (structures, batches,
        frames buffers, image clouds).  anchors: torch int64 CUDA tensor [P][2]; edges: host array of K + 1 ascending distances;
        wf_index: torch int32 CUDA tensor [P] or None; returns (or fills) a torch float64 CUDA tensor [P][K]
        (lchd_radial_primitives_dev)."""
        return self._pair_rows(self._radial_edges(edges), cloud_a, cloud_b, anchors, threshold_distance, out, wf_index)

    def radial_coords(self, cloud_a, cloud_b, edges, out=None, wf_index=None, *, box_a=None, box_b=None, cell_a=None, cell_b=None):
        """Radial profiles of the dense row pairs of two uploaded structures of equal size (LoCoHD.radial_from_coords): returns (or
        fills) a torch float64 CUDA tensor [n][K].  `box_a` / `box_b` / `cell_a` / `cell_b` (keyword-only, host arrays): minimum-image
        rows (lchd_radial_coords_dev)."""
        return self._pair_rows_coords(self._radial_edges(edges), cloud_a, cloud_b, out, wf_index, box_a, box_b, cell_a, cell_b)

    def attribution(self, cloud_a, cloud_b, anchors, threshold_distance: float, out=None, wf_index=None):
        """Score attribution by category (LoCoHD.attribution_from_primitives) of anchor pairs of two uploaded clouds of any kind.
        anchors: torch int64 CUDA tensor [P][2]; wf_index: torch int32 CUDA tensor [P] or None; returns (or fills) a torch float64
        CUDA tensor [P][C] (lchd_attribution_primitives_dev)."""
        return self._pair_rows(None, cloud_a, cloud_b, anchors, threshold_distance, out, wf_index)

    def category_gradient(self, cloud_a, cloud_b, anchors, threshold_distance: float, out=None, wf_index=None):
        """Category-weight gradients dS/dw_c (LoCoHD.category_gradient_from_primitives) of anchor pairs of two uploaded clouds of any
        kind, at the session's current category weights (set_category_weights).  anchors: torch int64 CUDA tensor [P][2]; wf_index: torch
        int32 CUDA tensor [P] or None; returns (or fills) a torch float64 CUDA tensor [P][C] (lchd_category_gradient_primitives_dev)."""
        return self._pair_rows(_CATEGORY_GRADIENT, cloud_a, cloud_b, anchors, threshold_distance, out, wf_index)

    def category_gradient_coords(self, cloud_a, cloud_b, out=None, wf_index=None, *, box_a=None, box_b=None, cell_a=None, cell_b=None):
        """Category-weight gradients of the dense row pairs of two uploaded structures of equal size
        (LoCoHD.category_gradient_from_coords): returns (or fills) a torch float64 CUDA tensor [n][C]
        (lchd_category_gradient_coords_dev)."""
        return self._pair_rows_coords(_CATEGORY_GRADIENT, cloud_a, cloud_b, out, wf_index, box_a, box_b, cell_a, cell_b)

    def set_category_weights(self, weights):
        """Replace the category weights of the session's configuration (lchd_ctx_set_config with everything else unchanged): every later
        call of the session scores and differentiates with them, until they are set again.  `weights`: C positive values (a sequence, an
        array or a torch tensor), validated as the LoCoHD constructor validates them (ValueError); also ValueError while an asynchronous
        pass is pending.  Uploaded clouds stay valid: they hold no weights.  The LoCoHD object the session was made from keeps its own."""
        if hasattr(weights, "detach"):
            weights = weights.detach().cpu().numpy()
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
        n_cat = int(self._cfg.n_categories)
        N.check(N.lib().lchd_config_validate(n_cat, n_cat, N.dp(w), w.size))
        cfg = N.ConfigC.from_buffer_copy(self._cfg)  # (its other pointers stay alive in self._keep)
        cfg.category_weights = N.dp(w)
        N.check(N.lib().lchd_ctx_set_config(self._ctx, C.byref(cfg)))
        self._cfg, self._weights = cfg, w

    def _weight_gradient_out(self, p, out, device):
        """(WeightGradient of views into one block of p * (1 + NP) doubles, the block): the layout the C call writes."""
        torch = self.torch
        k = int(N.lib().lchd_weight_gradient_width(self._ctx))
        if out is None:
            out = torch.empty(p * (1 + k), dtype=torch.float64, device=device)
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= p * (1 + k)
        flat = out.view(-1)
        return WeightGradient(flat[:p], flat[p:p * (1 + k)].view(p, k)), flat

    def weight_gradient(self, cloud_a, cloud_b, anchors, threshold_distance: float, out=None, wf_index=None):
        """Weight-function gradients dS/dtheta_k (LoCoHD.weight_gradient_from_primitives) of anchor pairs of two uploaded structures or
        batches (no image clouds), at the session's current parameters (set_weight_function).  anchors: torch int64 CUDA tensor [P][2];
        wf_index: torch int32 CUDA tensor [P] or None; out: a float64 CUDA tensor of at least P * (1 + NP) elements or None.  Returns
        `WeightGradient(scores [P], grad [P][NP])`, views into one block scores | grad (lchd_weight_gradient_primitives_dev)."""
        torch = self.torch
        assert anchors.is_cuda and anchors.dtype == torch.int64 and anchors.is_contiguous()
        p = anchors.shape[0]
        res, flat = self._weight_gradient_out(p, out, anchors.device)
        wf_ptr = None
        if wf_index is not None:
            assert wf_index.is_cuda and wf_index.dtype == torch.int32 and wf_index.is_contiguous() and wf_index.numel() >= p
            wf_ptr = C.c_void_p(wf_index.data_ptr())
        N.check(N.lib().lchd_weight_gradient_primitives_dev(self._ctx, cloud_a, cloud_b, C.c_void_p(anchors.data_ptr()), wf_ptr, p,
                                                            float(threshold_distance), C.c_void_p(flat.data_ptr())))
        return res

    def weight_gradient_coords(self, cloud_a, cloud_b, out=None, wf_index=None):
        """Weight-function gradients of the dense row pairs of two uploaded structures of equal size n
        (LoCoHD.weight_gradient_from_coords): `WeightGradient(scores [n], grad [n][NP])` (lchd_weight_gradient_coords_dev)."""
        torch = self.torch
        n = int(N.lib().lchd_cloud_size(cloud_a))
        res, flat = self._weight_gradient_out(n, out, torch.device("cuda", self.device))
        wf_ptr = None
        if wf_index is not None:
            assert wf_index.is_cuda and wf_index.dtype == torch.int32 and wf_index.is_contiguous() and wf_index.numel() >= n
            wf_ptr = C.c_void_p(wf_index.data_ptr())
        N.check(N.lib().lchd_weight_gradient_coords_dev(self._ctx, cloud_a, cloud_b, wf_ptr, C.c_void_p(flat.data_ptr())))
        return res

    # ---- reduced parameter gradients: sum_p v_p dS_p/dw_c and sum_p v_p dS_p/dtheta in one native call ----
    def _param_sum_args(self, p, pair_weights, wf_index, tile_pairs):
        """Checked arguments of the four reduced calls: (weights tensor or None, its pointer, wf pointer, tile_pairs)."""
        torch = self.torch
        if int(tile_pairs) < 0:
            raise ValueError(f"tile_pairs = {int(tile_pairs)} is negative (0: planned from the free device memory)")
        w = wf_ptr = None
        if pair_weights is not None:
            if not (pair_weights.dtype.is_floating_point or pair_weights.dtype in (torch.int32, torch.int64)):
                raise ValueError(f"pair_weights must be real numbers (got dtype {pair_weights.dtype})")
            if pair_weights.numel() != p:
                raise ValueError(f"pair_weights has {pair_weights.numel()} entries for {p} pairs")
            w = pair_weights.detach().to(device=torch.device("cuda", self.device), dtype=torch.float64).reshape(-1).contiguous()
        if wf_index is not None:
            assert wf_index.is_cuda and wf_index.dtype == torch.int32 and wf_index.is_contiguous() and wf_index.numel() >= p
            wf_ptr = C.c_void_p(wf_index.data_ptr())
        # (`w` lives until the call, which returns with its outputs complete, is over)
        return w, (None if w is None else C.c_void_p(w.data_ptr())), wf_ptr, int(tile_pairs)

    def _category_sum_out(self, out):
        torch = self.torch
        n_cat = int(self._cfg.n_categories)
        if out is None:
            out = torch.empty(n_cat, dtype=torch.float64, device=torch.device("cuda", self.device))
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and tuple(out.shape) == (n_cat,)
        return out

    def _weight_sum_out(self, p, out):
        torch = self.torch
        dev = torch.device("cuda", self.device)
        shapes = ((p,), (int(self._cfg.n_weight_functions), int(N.lib().lchd_weight_gradient_width(self._ctx))))
        if out is None:
            out = tuple(torch.empty(shape, dtype=torch.float64, device=dev) for shape in shapes)
        for t, shape in zip(out, shapes):
            assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape
        return WeightGradientSum(*out)

    def category_gradient_sum(self, cloud_a, cloud_b, anchors, threshold_distance: float, pair_weights=None, wf_index=None, *, tile_pairs=0,
                              out=None):
        """sum_p v_p dS_p/dw_c (LoCoHD.category_gradient_sum_from_primitives) over the anchor pairs of two uploaded clouds of any kind, as
        a torch float64 CUDA tensor [C], in ONE native call (lchd_category_gradient_sum_primitives_dev): the rows of `category_gradient`
        are reduced on the device, tile by tile, into exact fixed-point accumulators and never reach torch.  anchors: torch int64 CUDA
        tensor [P][2]; pair_weights: v, a tensor [P] (default: ones); wf_index: torch int32 CUDA tensor [P] or None; tile_pairs: pairs per
        pass, 0 = planned from the free device memory; out: a float64 CUDA tensor [C], filled and returned.  The bits are a function of
        the rows and weights alone: the same for every tile size, mode and run.  ValueError if a term is not finite or reaches 2^63."""
        torch = self.torch
        assert anchors.is_cuda and anchors.dtype == torch.int64 and anchors.is_contiguous()
        p = anchors.shape[0]
        w, w_ptr, wf_ptr, tile = self._param_sum_args(p, pair_weights, wf_index, tile_pairs)
        out = self._category_sum_out(out)
        N.check(N.lib().lchd_category_gradient_sum_primitives_dev(self._ctx, cloud_a, cloud_b, C.c_void_p(anchors.data_ptr()), wf_ptr, p,
                                                                  float(threshold_distance), w_ptr, tile, C.c_void_p(out.data_ptr())))
        return out

    def category_gradient_sum_coords(self, cloud_a, cloud_b, pair_weights=None, wf_index=None, *, tile_pairs=0, out=None, box_a=None,
                                     box_b=None, cell_a=None, cell_b=None):
        """`category_gradient_sum` for the dense row pairs of two uploaded structures of equal size n
        (LoCoHD.category_gradient_sum_from_coords): pair_weights / wf_index [n] or None; one tile, whatever `tile_pairs` (>= 0) says
        (lchd_category_gradient_sum_coords_dev)."""
        for side, box, cell in (("a", box_a, cell_a), ("b", box_b, cell_b)):
            if box is not None and cell is not None:
                raise ValueError(f"box_{side} and cell_{side} were both given: a structure has one periodic box or one periodic cell")
        pc_a = dense_cells(box_a, cell_a, 1, "box_a", "cell_a")
        pc_b = dense_cells(box_b, cell_b, 1, "box_b", "cell_b")
        n = int(N.lib().lchd_cloud_size(cloud_a))
        w, w_ptr, wf_ptr, _ = self._param_sum_args(n, pair_weights, wf_index, tile_pairs)
        out = self._category_sum_out(out)
        N.check(N.lib().lchd_category_gradient_sum_coords_dev(self._ctx, cloud_a, cloud_b, wf_ptr, N.dp(pc_a), N.dp(pc_b), w_ptr,
                                                              C.c_void_p(out.data_ptr())))
        return out

    def weight_gradient_sum(self, cloud_a, cloud_b, anchors, threshold_distance: float, pair_weights=None, wf_index=None, *, tile_pairs=0,
                            out=None):
        """`WeightGradientSum(scores [P], grad [n_wf][NP])` (LoCoHD.weight_gradient_sum_from_primitives) of the anchor pairs of two
        uploaded structures or batches (no image clouds) in ONE native call (lchd_weight_gradient_sum_primitives_dev): the scores of
        `weight_gradient`, bit for bit, and per weight function f the exact sum of v_p dS_p/dtheta over the pairs with wf_index[p] = f
        (all pairs without an index), rounded once, zeros behind f's parameters.  Arguments as `category_gradient_sum`; out: two float64
        CUDA tensors [P] and [n_wf][NP].  ValueError if a term is not finite or reaches 2^63 (the scores in `out` are then valid)."""
        torch = self.torch
        assert anchors.is_cuda and anchors.dtype == torch.int64 and anchors.is_contiguous()
        p = anchors.shape[0]
        w, w_ptr, wf_ptr, tile = self._param_sum_args(p, pair_weights, wf_index, tile_pairs)
        res = self._weight_sum_out(p, out)
        N.check(N.lib().lchd_weight_gradient_sum_primitives_dev(self._ctx, cloud_a, cloud_b, C.c_void_p(anchors.data_ptr()), wf_ptr, p,
                                                                float(threshold_distance), w_ptr, tile, C.c_void_p(res.scores.data_ptr()),
                                                                C.c_void_p(res.grad.data_ptr())))
        return res

    def weight_gradient_sum_coords(self, cloud_a, cloud_b, pair_weights=None, wf_index=None, *, tile_pairs=0, out=None):
        """`weight_gradient_sum` for the dense row pairs of two uploaded structures of equal size n
        (LoCoHD.weight_gradient_sum_from_coords): one tile (lchd_weight_gradient_sum_coords_dev)."""
        n = int(N.lib().lchd_cloud_size(cloud_a))
        w, w_ptr, wf_ptr, _ = self._param_sum_args(n, pair_weights, wf_index, tile_pairs)
        res = self._weight_sum_out(n, out)
        N.check(N.lib().lchd_weight_gradient_sum_coords_dev(self._ctx, cloud_a, cloud_b, wf_ptr, w_ptr, C.c_void_p(res.scores.data_ptr()),
                                                            C.c_void_p(res.grad.data_ptr())))
        return res

    def set_weight_function(self, params):
        """Replace the parameters of the session's single weight function (lchd_ctx_set_config with everything else unchanged): every
        later call of the session scores and differentiates with them, until they are set again.  The family and the parameter count stay;
        `params` (a sequence, an array or a torch tensor) is validated as the WeightFunction constructor validates it (ValueError).  Also
        ValueError for a session with a dictionary of weight functions and while an asynchronous pass is pending.  Uploaded clouds stay
        valid: they hold no weight function.  The LoCoHD object the session was made from keeps its own."""
        if int(self._cfg.n_weight_functions) != 1:
            raise ValueError("set_weight_function applies to a session with a single weight function, not a dictionary")
        if hasattr(params, "detach"):
            params = params.detach().cpu().numpy()
        prm = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1))
        old = self._cfg.weight_functions[0]
        if prm.size != int(old.n_params):
            raise ValueError(f"set_weight_function keeps the parameter count: {int(old.n_params)} expected, got {prm.size}")
        N.check(N.lib().lchd_wf_validate(int(old.kind), N.dp(prm), prm.size))
        arr = (N.WeightFunctionC * 1)(N.WeightFunctionC(int(old.kind), prm.size, N.dp(prm)))
        cfg = N.ConfigC.from_buffer_copy(self._cfg)  # (its other pointers stay alive in self._keep)
        cfg.weight_functions = arr
        N.check(N.lib().lchd_ctx_set_config(self._ctx, C.byref(cfg)))
        self._cfg, self._wf = cfg, (arr, prm)

    def sensitivity(self, cloud_a, cloud_b, anchors, threshold_distance: float, out=None, wf_index=None, *, width=None):
        """Neighbour sensitivities (LoCoHD.sensitivity_from_primitives) of anchor pairs of two uploaded structures or batches (no image
        clouds).  anchors: torch int64 CUDA tensor [P][2]; wf_index: torch int32 CUDA tensor [P] or None.  Returns a `Sensitivity` of
        torch CUDA tensors: scores [P] f64, count_a / count_b [P] i32, idx_a / idx_b [P][K] i32 (padded with -1; for a batch the global
        atom indices of `upload_batch`, as the anchors are), dist_a / dist_b /
        g_a / g_b [P][K] f64 (padded with 0).  K: `width`, or the width of `out` (a `Sensitivity` of such tensors, filled and
        returned; ValueError if an environment is longer), or -- with neither -- the longest environment, found by repeating a call
        whose first guess of 128 was too narrow (lchd_sensitivity_primitives_dev).  The derivative ignores points entering or leaving at
        the threshold and is one-sided at ties."""
        torch = self.torch
        assert anchors.is_cuda and anchors.dtype == torch.int64 and anchors.is_contiguous()
        p = anchors.shape[0]
        wf_ptr = None
        if wf_index is not None:
            assert wf_index.is_cuda and wf_index.dtype == torch.int32 and wf_index.is_contiguous() and wf_index.numel() >= p
            wf_ptr = C.c_void_p(wf_index.data_ptr())
        fixed = out is not None or width is not None
        k = int(out.idx_a.shape[1]) if out is not None else (128 if width is None else int(width))
        while True:
            if out is None:
                dev = anchors.device
                f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)  # noqa: E731
                i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)  # noqa: E731
                res = Sensitivity(f64(p), i32(p), i32(p, k), f64(p, k), f64(p, k), i32(p), i32(p, k), f64(p, k), f64(p, k))
            else:
                res = out
                for name, t in zip(Sensitivity._fields, res):
                    want = torch.int32 if name.startswith(("count", "idx")) else torch.float64
                    rows = (p,) if name in ("scores", "count_a", "count_b") else (p, k)
                    assert t.is_cuda and t.dtype == want and t.is_contiguous() and tuple(t.shape) == rows, name
            if p == 0:
                return res
            rc = N.lib().lchd_sensitivity_primitives_dev(self._ctx, cloud_a, cloud_b, C.c_void_p(anchors.data_ptr()), wf_ptr, p,
                                                         float(threshold_distance), k, *[C.c_void_p(t.data_ptr()) for t in res])
            need = int(N.lib().lchd_sensitivity_needed_width(self._ctx))
            if rc == N.EVALUE and not fixed and need > k:
                k = need
                continue
            N.check(rc)
            if not fixed and 0 < need < k:  # rows as wide as the longest environment, as the host call returns them
                res = Sensitivity(*[t[:, :need].contiguous() if t.dim() == 2 else t for t in res])
            return res

    def image_origin(self, images):
        """The way back from every slot of an image cloud (periodic_images) to its source: `(origin, code)` as NumPy arrays, int32 source
        atom (origin[i] = i for the wrapped atoms themselves) and int8 image code (0: no shift) per slot (lchd_cloud_image_origin)."""
        n = int(N.lib().lchd_cloud_size(images))
        origin, code = np.empty(max(n, 0), dtype=np.int32), np.empty(max(n, 0), dtype=np.int8)
        N.check(N.lib().lchd_cloud_image_origin(self._ctx, images, N.ip(origin), C.c_void_p(code.ctypes.data), n))
        return origin, code

    def sensitivity_images(self, cloud_a, cloud_b, anchors, threshold_distance: float, out=None, wf_index=None, *, width=None):
        """`sensitivity` for clouds of which any may be an image cloud (periodic_images), every member resolved to its source atom
        (LoCoHD.sensitivity_from_primitives_periodic).  Returns a `PeriodicSensitivity` of torch CUDA tensors: next to the fields of
        `sensitivity`, idx names source atoms (global indices for a batch), image_a / image_b [P][K] int8 are the image codes and
        disp_a / disp_b [P][K][3] f64 the members' displacements from their anchors.  K, `out` (a `PeriodicSensitivity` of such tensors)
        and `width` as in `sensitivity`; ValueError naming the width the pairs take if K is too small (lchd_sensitivity_images_dev)."""
        torch = self.torch
        assert anchors.is_cuda and anchors.dtype == torch.int64 and anchors.is_contiguous()
        p = anchors.shape[0]
        wf_ptr = None
        if wf_index is not None:
            assert wf_index.is_cuda and wf_index.dtype == torch.int32 and wf_index.is_contiguous() and wf_index.numel() >= p
            wf_ptr = C.c_void_p(wf_index.data_ptr())
        fixed = out is not None or width is not None
        k = int(out.idx_a.shape[1]) if out is not None else (128 if width is None else int(width))
        kinds = {"scores": torch.float64, "count": torch.int32, "idx": torch.int32, "image": torch.int8, "dist": torch.float64, "g": torch.float64,
                 "disp": torch.float64}
        while True:
            shapes = {"scores": (p,), "count": (p,), "disp": (p, k, 3)}
            if out is None:
                res = PeriodicSensitivity(*[torch.empty(shapes.get(f.split("_")[0], (p, k)), dtype=kinds[f.split("_")[0]], device=anchors.device)
                                            for f in PeriodicSensitivity._fields])
            else:
                res = out
                for name, t in zip(PeriodicSensitivity._fields, res):
                    kind = name.split("_")[0]
                    assert t.is_cuda and t.dtype == kinds[kind] and t.is_contiguous() and tuple(t.shape) == shapes.get(kind, (p, k)), name
            if p == 0:
                return res
            rc = N.lib().lchd_sensitivity_images_dev(self._ctx, cloud_a, cloud_b, C.c_void_p(anchors.data_ptr()), wf_ptr, p,
                                                     float(threshold_distance), k, *[C.c_void_p(t.data_ptr()) for t in res])
            need = int(N.lib().lchd_sensitivity_needed_width(self._ctx))
            if rc == N.EVALUE and not fixed and need > k:
                k = need
                continue
            N.check(rc)
            if not fixed and 0 < need < k:  # rows as wide as the longest environment, as the host call returns them
                res = PeriodicSensitivity(*[t[:, :need].contiguous() if t.dim() >= 2 else t for t in res])
            return res

    def gradient_images(self, cloud_a, cloud_b, anchors, threshold_distance: float, pair_weights=None, wf_index=None):
        """`(scores, grad_a, grad_b)` with grad = sum_p v_p dS_p/dx (LoCoHD.gradient_from_primitives_periodic) as torch CUDA tensors, for
        clouds of which any may be an image cloud.  grad_a / grad_b have one row per SOURCE atom (lchd_cloud_home_size): a ghost's term
        goes to the atom it is an image of.  pair_weights: v, a tensor [P] (default: ones).  Assembled from `sensitivity_images` with
        torch.Tensor.index_add_: its summation order, and so the last bits, follow torch's determinism setting."""
        sens = self.sensitivity_images(cloud_a, cloud_b, anchors, threshold_distance, wf_index=wf_index)
        na, nb = (int(N.lib().lchd_cloud_home_size(cl)) for cl in (cloud_a, cloud_b))
        return (sens.scores, self.side_gradient_images(sens.scores, sens.idx_a, sens.dist_a, sens.g_a, sens.disp_a, na, pair_weights),
                self.side_gradient_images(sens.scores, sens.idx_b, sens.dist_b, sens.g_b, sens.disp_b, nb, pair_weights))

    def side_gradient_images(self, scores, idx, dist, g, disp, n_atoms: int, pair_weights=None):
        """One side of gradient_images: [n_atoms][3] f64, `side_gradient` with the displacements given instead of coordinates."""
        torch = self.torch
        v = torch.ones_like(scores) if pair_weights is None else pair_weights.to(scores.dtype).reshape(-1)
        grad = torch.zeros((n_atoms, 3), dtype=torch.float64, device=scores.device)
        use = (idx >= 0) & (dist > 0.0) & torch.isfinite(g)
        use[:, 0] = False
        member = idx.clamp(min=0).long()
        anchor = member[:, :1].expand_as(member)
        coef = torch.where(use, v[:, None] * g / torch.where(use, dist, torch.ones_like(dist)), torch.zeros_like(g))
        step = coef[..., None] * disp  # [P][K][3]; zero rows where `use` is false
        grad.index_add_(0, member.reshape(-1), step.reshape(-1, 3))
        grad.index_add_(0, anchor.reshape(-1), -step.reshape(-1, 3))
        return grad

    def _cross_head(self, cloud_a, cloud_b, anchors_a, anchors_b, threshold_distance, wf_index, tile_rows):
        torch = self.torch
        for t in (anchors_a, anchors_b):
            assert t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.dim() == 1
        if int(tile_rows) < 0:
            raise ValueError(f"tile_rows = {int(tile_rows)} is negative (0: planned from the free device memory)")
        return (self._ctx, cloud_a, cloud_b, C.c_void_p(anchors_a.data_ptr()), anchors_a.shape[0], C.c_void_p(anchors_b.data_ptr()),
                anchors_b.shape[0], -1 if wf_index is None else int(wf_index), float(threshold_distance), int(tile_rows))

    def cross(self, cloud_a, cloud_b, anchors_a, anchors_b, threshold_distance: float, out=None, wf_index=None, *, tile_rows=0):
        """Cross-scoring (LoCoHD.cross_from_primitives) of two uploaded clouds of any kind (structures, batches, frames buffers, image
        clouds): every anchor of anchors_a against every anchor of anchors_b, torch int64 CUDA tensors [Na] and [Nb] of global atom
        indices (repeats allowed).  wf_index: ONE weight-function index for the whole call (an int) or None.  Returns (or fills) a torch
        float64 CUDA tensor [Na][Nb]; no pair list is built (lchd_cross_primitives_dev).  tile_rows: rows of A per pass, 0 = planned
        from the free device memory."""
        torch = self.torch
        head = self._cross_head(cloud_a, cloud_b, anchors_a, anchors_b, threshold_distance, wf_index, tile_rows)
        na, nb = anchors_a.shape[0], anchors_b.shape[0]
        if out is None:
            out = torch.empty((na, nb), dtype=torch.float64, device=anchors_a.device)
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= na * nb
        N.check(N.lib().lchd_cross_primitives_dev(*head, C.c_void_p(out.data_ptr())))
        return out

    def nearest(self, cloud_a, cloud_b, anchors_a, anchors_b, threshold_distance: float, k: int, out=None, wf_index=None, *, tile_rows=0):
        """The k best matches of every anchor of anchors_a among anchors_b (LoCoHD.nearest_from_primitives): a `Nearest` of torch CUDA
        tensors, scores [Na][k] f64 and cols [Na][k] i32 (positions in anchors_b), each row ascending in (score, j); `out`: such a
        pair of tensors, filled and returned.  With a batch as cloud_b this searches a set of structures in one call
        (lchd_nearest_primitives_dev).  Other arguments as `cross`."""
        torch = self.torch
        head = self._cross_head(cloud_a, cloud_b, anchors_a, anchors_b, threshold_distance, wf_index, tile_rows)
        na, nb, k = anchors_a.shape[0], anchors_b.shape[0], int(k)
        if not 1 <= k <= min(nb, 64):
            raise ValueError(f"k = {k} is outside 1 .. min(Nb, 64) with Nb = {nb}")
        if out is None:
            out = Nearest(torch.empty((na, k), dtype=torch.float64, device=anchors_a.device),
                          torch.empty((na, k), dtype=torch.int32, device=anchors_a.device))
        scores, cols = out
        assert scores.is_cuda and scores.dtype == torch.float64 and scores.is_contiguous() and tuple(scores.shape) == (na, k)
        assert cols.is_cuda and cols.dtype == torch.int32 and cols.is_contiguous() and tuple(cols.shape) == (na, k)
        N.check(N.lib().lchd_nearest_primitives_dev(*head, k, C.c_void_p(scores.data_ptr()), C.c_void_p(cols.data_ptr())))
        return Nearest(scores, cols)

    def gradient(self, cloud_a, cloud_b, anchors, threshold_distance: float, xyz_a, xyz_b, pair_weights=None, wf_index=None):
        """`(scores, grad_a[Na, 3], grad_b[Nb, 3])` with grad = sum_p v_p dS_p/dx (LoCoHD.gradient_from_primitives) as torch CUDA tensors.
        xyz_a / xyz_b: the coordinates of the two clouds as torch float64 CUDA tensors [N][3]; pair_weights: v, a tensor [P] (default:
        ones).  Assembled from `sensitivity` with torch.Tensor.index_add_: its summation order, and so the last bits, follow torch's
        determinism setting."""
        sens = self.sensitivity(cloud_a, cloud_b, anchors, threshold_distance, wf_index=wf_index)
        return (sens.scores,) + self.assemble_gradient(sens, xyz_a, xyz_b, pair_weights)

    def assemble_gradient(self, sens, xyz_a, xyz_b, pair_weights=None):
        """The two coordinate gradients of sum_p v_p S_p from a `Sensitivity` of tensors: member += v g (x_m - x_anchor) / d, anchor -= the
        same; members at distance 0 and the padding are skipped."""
        return (self.side_gradient(sens.scores, sens.idx_a, sens.dist_a, sens.g_a, xyz_a, pair_weights),
                self.side_gradient(sens.scores, sens.idx_b, sens.dist_b, sens.g_b, xyz_b, pair_weights))

    def side_gradient(self, scores, idx, dist, g, xyz, pair_weights=None):
        """One side of assemble_gradient: [N][3] f64."""
        torch = self.torch
        v = torch.ones_like(scores) if pair_weights is None else pair_weights.to(scores.dtype).reshape(-1)
        grad = torch.zeros(xyz.shape, dtype=torch.float64, device=xyz.device)
        use = (idx >= 0) & (dist > 0.0) & torch.isfinite(g)
        use[:, 0] = False
        member = idx.clamp(min=0).long()
        anchor = member[:, :1].expand_as(member)
        coef = torch.where(use, v[:, None] * g / torch.where(use, dist, torch.ones_like(dist)), torch.zeros_like(g))
        step = coef[..., None] * (xyz[member] - xyz[anchor])  # [P][K][3]; zero rows where `use` is false
        grad.index_add_(0, member.reshape(-1), step.reshape(-1, 3))
        grad.index_add_(0, anchor.reshape(-1), -step.reshape(-1, 3))
        return grad

    def _native_gradient_buffers(self, cloud_a, cloud_b, p, pair_weights, wf_index, out):
        """Checked arguments of the two native gradient calls: (weights tensor or None, wf pointer, (scores, grad_a, grad_b))."""
        torch = self.torch
        na, nb = (int(N.lib().lchd_cloud_size(cl)) for cl in (cloud_a, cloud_b))
        dev = torch.device("cuda", self.device)
        w = wf_ptr = None
        if pair_weights is not None:
            if pair_weights.numel() != p:
                raise ValueError(f"pair_weights has {pair_weights.numel()} entries for {p} pairs")
            w = pair_weights.detach().to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
        if wf_index is not None:
            assert wf_index.is_cuda and wf_index.dtype == torch.int32 and wf_index.is_contiguous() and wf_index.numel() >= p
            wf_ptr = C.c_void_p(wf_index.data_ptr())
        if out is None:
            out = (torch.empty(p, dtype=torch.float64, device=dev), torch.empty((na, 3), dtype=torch.float64, device=dev),
                   torch.empty((nb, 3), dtype=torch.float64, device=dev))
        for t, shape in zip(out, ((p,), (na, 3), (nb, 3))):
            assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape
        return w, wf_ptr, tuple(out)

    def native_gradient(self, cloud_a, cloud_b, anchors, threshold_distance: float, pair_weights=None, wf_index=None, *, tile_pairs=0,
                        out=None):
        """`(scores, grad_a[Na, 3], grad_b[Nb, 3])` with grad = sum_p v_p dS_p/dx (LoCoHD.native_gradient_from_primitives) in ONE native
        call (lchd_gradient_primitives_dev): the sensitivity lists are reduced on the device, tile by tile, into exact fixed-point
        accumulators and never reach torch.  Coordinates are the clouds' own.  anchors: torch int64 CUDA tensor [P][2]; pair_weights: v, a
        tensor [P] (default: ones); wf_index: torch int32 CUDA tensor [P] or None; tile_pairs: pairs per pass, 0 = planned from the free
        device memory; out: three float64 CUDA tensors [P], [Na][3], [Nb][3], filled and returned.  The bits of the result are a
        function of the inputs alone: the same for every tile size, mode and run.  ValueError if a contribution is not finite or reaches
        2^63 (the scores in `out` are then valid)."""
        torch = self.torch
        assert anchors.is_cuda and anchors.dtype == torch.int64 and anchors.is_contiguous()
        if int(tile_pairs) < 0:
            raise ValueError(f"tile_pairs = {int(tile_pairs)} is negative (0: planned from the free device memory)")
        p = anchors.shape[0]
        w, wf_ptr, out = self._native_gradient_buffers(cloud_a, cloud_b, p, pair_weights, wf_index, out)
        w_ptr = None if w is None else C.c_void_p(w.data_ptr())  # (`w` lives until the call, which returns with its outputs complete, is over)
        N.check(N.lib().lchd_gradient_primitives_dev(self._ctx, cloud_a, cloud_b, C.c_void_p(anchors.data_ptr()), wf_ptr, p,
                                                     float(threshold_distance), w_ptr, int(tile_pairs), *[C.c_void_p(t.data_ptr()) for t in out]))
        return out

    def native_gradient_coords(self, cloud_a, cloud_b, pair_weights=None, wf_index=None, *, out=None):
        """`native_gradient` for the dense rows of two uploaded structures of equal size (LoCoHD.native_gradient_from_coords): row r is
        anchored at atom r itself; pair_weights / wf_index: [n] or None (lchd_gradient_coords_dev)."""
        n = int(N.lib().lchd_cloud_size(cloud_a))
        w, wf_ptr, out = self._native_gradient_buffers(cloud_a, cloud_b, n, pair_weights, wf_index, out)
        w_ptr = None if w is None else C.c_void_p(w.data_ptr())
        N.check(N.lib().lchd_gradient_coords_dev(self._ctx, cloud_a, cloud_b, wf_ptr, w_ptr, *[C.c_void_p(t.data_ptr()) for t in out]))
        return out

    def _native_periodic_buffers(self, cloud_a, cloud_b, p, pair_weights, wf_index, out, strain):
        """`_native_gradient_buffers` with one gradient row per SOURCE atom and, with `strain`, the two [3][3] tensors behind them."""
        torch = self.torch
        na, nb = (int(N.lib().lchd_cloud_home_size(cl)) for cl in (cloud_a, cloud_b))
        dev = torch.device("cuda", self.device)
        w = wf_ptr = None
        if pair_weights is not None:
            if pair_weights.numel() != p:
                raise ValueError(f"pair_weights has {pair_weights.numel()} entries for {p} pairs")
            w = pair_weights.detach().to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
        if wf_index is not None:
            assert wf_index.is_cuda and wf_index.dtype == torch.int32 and wf_index.is_contiguous() and wf_index.numel() >= p
            wf_ptr = C.c_void_p(wf_index.data_ptr())
        shapes = ((p,), (na, 3), (nb, 3)) + (((3, 3), (3, 3)) if strain else ())
        if out is None:
            out = tuple(torch.empty(shape, dtype=torch.float64, device=dev) for shape in shapes)
        if len(out) != len(shapes):
            raise ValueError(f"out holds {len(out)} tensors; this call fills {len(shapes)}")
        for t, shape in zip(out, shapes):
            assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == shape
        return w, wf_ptr, tuple(out)

    def native_gradient_images(self, cloud_a, cloud_b, anchors, threshold_distance: float, pair_weights=None, wf_index=None, *,
                               tile_pairs=0, strain=False, out=None):
        """`native_gradient` for clouds of which any may be an image cloud (periodic_images): `(scores, grad_a, grad_b)` with one gradient
        row per SOURCE atom (lchd_cloud_home_size), the terms `gradient_images` sums with index_add_ reduced exactly on the device
        (lchd_gradient_images_dev).  strain=True: a `NativeGradient` whose strain_a / strain_b [3][3] are the strain derivatives of
        sum_p v_p S_p per side (LoCoHD.native_gradient_from_primitives_periodic); NotImplementedError with a batch cloud.  out: the three
        (with strain: five) float64 CUDA tensors, filled and returned.  Other arguments and the bit guarantee as `native_gradient`."""
        torch = self.torch
        assert anchors.is_cuda and anchors.dtype == torch.int64 and anchors.is_contiguous()
        if int(tile_pairs) < 0:
            raise ValueError(f"tile_pairs = {int(tile_pairs)} is negative (0: planned from the free device memory)")
        p = anchors.shape[0]
        w, wf_ptr, out = self._native_periodic_buffers(cloud_a, cloud_b, p, pair_weights, wf_index, out, strain)
        w_ptr = None if w is None else C.c_void_p(w.data_ptr())
        ptrs = [C.c_void_p(t.data_ptr()) for t in out] + ([] if strain else [None, None])
        N.check(N.lib().lchd_gradient_images_dev(self._ctx, cloud_a, cloud_b, C.c_void_p(anchors.data_ptr()), wf_ptr, p,
                                                 float(threshold_distance), w_ptr, int(tile_pairs), *ptrs))
        return NativeGradient(*out) if strain else out

    def native_gradient_coords_periodic(self, cloud_a, cloud_b, pair_weights=None, wf_index=None, *, box_a=None, box_b=None, cell_a=None,
                                        cell_b=None, strain=False, out=None):
        """`native_gradient_coords` on minimum-image rows (LoCoHD.native_gradient_from_coords_periodic): boxes and cells (keyword-only,
        host arrays) as `sensitivity_coords_periodic` takes them, a side with neither is open; strain and out as in
        `native_gradient_images` (lchd_gradient_coords_periodic_dev)."""
        for side, box, cell in (("a", box_a, cell_a), ("b", box_b, cell_b)):
            if box is not None and cell is not None:
                raise ValueError(f"box_{side} and cell_{side} were both given: a structure has one periodic box or one periodic cell")
        pc_a = dense_cells(box_a, cell_a, 1, "box_a", "cell_a")
        pc_b = dense_cells(box_b, cell_b, 1, "box_b", "cell_b")
        n = int(N.lib().lchd_cloud_size(cloud_a))
        w, wf_ptr, out = self._native_periodic_buffers(cloud_a, cloud_b, n, pair_weights, wf_index, out, strain)
        w_ptr = None if w is None else C.c_void_p(w.data_ptr())
        ptrs = [C.c_void_p(t.data_ptr()) for t in out] + ([] if strain else [None, None])
        N.check(N.lib().lchd_gradient_coords_periodic_dev(self._ctx, cloud_a, cloud_b, wf_ptr, N.dp(pc_a), N.dp(pc_b), w_ptr, *ptrs))
        return NativeGradient(*out) if strain else out

    def sensitivity_coords(self, cloud_a, cloud_b, out=None, wf_index=None, *, width=None):
        """Neighbour sensitivities of the dense row pairs of two uploaded structures of equal size (LoCoHD.sensitivity_from_coords; no
        batches, no image clouds).  wf_index: torch int32 CUDA tensor [n] or None.  Returns a `Sensitivity` of torch CUDA tensors as
        `sensitivity` does, row r the whole structure seen from atom r sorted by (distance, atom index): K = `width`, or the width of
        `out` (a `Sensitivity` of such tensors, filled and returned), or n; ValueError if K < n (lchd_sensitivity_coords_dev)."""
        torch = self.torch
        n = int(N.lib().lchd_cloud_size(cloud_a))
        wf_ptr = None
        if wf_index is not None:
            assert wf_index.is_cuda and wf_index.dtype == torch.int32 and wf_index.is_contiguous() and wf_index.numel() >= n
            wf_ptr = C.c_void_p(wf_index.data_ptr())
        if width is not None and int(width) < 1:
            raise ValueError(f"width = {width}: a row holds at least one member")
        k = int(out.idx_a.shape[1]) if out is not None else (n if width is None else int(width))
        if out is None:
            dev = torch.device("cuda", self.device)
            f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)  # noqa: E731
            i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)  # noqa: E731
            out = Sensitivity(f64(n), i32(n), i32(n, k), f64(n, k), f64(n, k), i32(n), i32(n, k), f64(n, k), f64(n, k))
        else:
            for name, t in zip(Sensitivity._fields, out):
                want = torch.int32 if name.startswith(("count", "idx")) else torch.float64
                rows = (n,) if name in ("scores", "count_a", "count_b") else (n, k)
                assert t.is_cuda and t.dtype == want and t.is_contiguous() and tuple(t.shape) == rows, name
        if n:
            N.check(N.lib().lchd_sensitivity_coords_dev(self._ctx, cloud_a, cloud_b, wf_ptr, k, *[C.c_void_p(t.data_ptr()) for t in out]))
        return out

    def gradient_coords(self, cloud_a, cloud_b, xyz_a, xyz_b, pair_weights=None, wf_index=None):
        """`(scores, grad_a[n, 3], grad_b[n, 3])` with grad = sum_r v_r dS_r/dx over the dense rows (LoCoHD.gradient_from_coords) as
        torch CUDA tensors: exact (a dense row has no threshold), one-sided at ties.  xyz_a / xyz_b: the coordinates of the two clouds
        as torch float64 CUDA tensors [n][3]; pair_weights: v, a tensor [n] (default: ones).  Assembled from `sensitivity_coords` as one
        dense product (`dense_side_gradient`): no index_add_, so the bits do not depend on torch's determinism setting."""
        sens = self.sensitivity_coords(cloud_a, cloud_b, wf_index=wf_index)
        return (sens.scores, self.dense_side_gradient(sens.idx_a, sens.dist_a, sens.g_a, xyz_a, pair_weights),
                self.dense_side_gradient(sens.idx_b, sens.dist_b, sens.g_b, xyz_b, pair_weights))

    def dense_side_gradient(self, idx, dist, g, xyz, pair_weights=None):
        """One side of gradient_coords, [n][3] f64: W = v g / d scattered into atom order (every atom occurs once per row: one writer
        per element; 0 in slot 0, where d == 0 and where g is not finite), M = W + W^T, grad = rowsum(M) x - M x."""
        torch = self.torch
        n = xyz.shape[0]
        idx, dist, g = idx[:, :n], dist[:, :n], g[:, :n]  # (a wider row: the padding goes)
        x = xyz.to(torch.float64)
        v = torch.ones(n, dtype=torch.float64, device=x.device) if pair_weights is None else pair_weights.to(torch.float64).reshape(-1)
        use = (idx >= 0) & (dist > 0.0) & torch.isfinite(g)
        use[:, 0] = False
        coef = torch.where(use, v[:, None] * g / torch.where(use, dist, torch.ones_like(dist)), torch.zeros_like(g))
        w = torch.zeros((n, n), dtype=torch.float64, device=x.device).scatter_(1, idx.long(), coef)
        m = w + w.t()
        return m.sum(dim=1)[:, None] * x - m @ x

    def sensitivity_coords_periodic(self, cloud_a, cloud_b, out=None, wf_index=None, *, width=None, box_a=None, box_b=None, cell_a=None,
                                    cell_b=None):
        """`sensitivity_coords` on minimum-image rows (LoCoHD.sensitivity_from_coords_periodic): `box_a` / `box_b` / `cell_a` / `cell_b`
        (keyword-only, host arrays) as `from_coords` takes them, a side with neither is open.  Returns a `MinImageSensitivity` of torch
        CUDA tensors: the fields of `sensitivity_coords` and disp_a / disp_b [n][K][3] f64, the displacement from row atom r to the
        nearest image of member idx[r][k] (dist = |disp| bit for bit).  K, `out` (a `MinImageSensitivity` of such tensors) and `width`
        as in `sensitivity_coords` (lchd_sensitivity_coords_periodic_dev)."""
        for side, box, cell in (("a", box_a, cell_a), ("b", box_b, cell_b)):
            if box is not None and cell is not None:
                raise ValueError(f"box_{side} and cell_{side} were both given: a structure has one periodic box or one periodic cell")
        pc_a = dense_cells(box_a, cell_a, 1, "box_a", "cell_a")
        pc_b = dense_cells(box_b, cell_b, 1, "box_b", "cell_b")
        torch = self.torch
        n = int(N.lib().lchd_cloud_size(cloud_a))
        wf_ptr = None
        if wf_index is not None:
            assert wf_index.is_cuda and wf_index.dtype == torch.int32 and wf_index.is_contiguous() and wf_index.numel() >= n
            wf_ptr = C.c_void_p(wf_index.data_ptr())
        if width is not None and int(width) < 1:
            raise ValueError(f"width = {width}: a row holds at least one member")
        k = int(out.idx_a.shape[1]) if out is not None else (n if width is None else int(width))
        shapes = {"scores": (n,), "count": (n,), "disp": (n, k, 3)}
        if out is None:
            dev = torch.device("cuda", self.device)
            out = MinImageSensitivity(*[torch.empty(shapes.get(f.split("_")[0], (n, k)), device=dev,
                                                    dtype=torch.int32 if f.startswith(("count", "idx")) else torch.float64)
                                        for f in MinImageSensitivity._fields])
        else:
            for name, t in zip(MinImageSensitivity._fields, out):
                want = torch.int32 if name.startswith(("count", "idx")) else torch.float64
                assert t.is_cuda and t.dtype == want and t.is_contiguous() and tuple(t.shape) == shapes.get(name.split("_")[0], (n, k)), name
        if n:
            nine = [t for name, t in zip(MinImageSensitivity._fields, out) if not name.startswith("disp")]
            N.check(N.lib().lchd_sensitivity_coords_periodic_dev(self._ctx, cloud_a, cloud_b, wf_ptr, N.dp(pc_a), N.dp(pc_b), k,
                                                                 *[C.c_void_p(t.data_ptr()) for t in nine],
                                                                 C.c_void_p(out.disp_a.data_ptr()), C.c_void_p(out.disp_b.data_ptr())))
        return out

    def gradient_coords_periodic(self, cloud_a, cloud_b, pair_weights=None, wf_index=None, *, box_a=None, box_b=None, cell_a=None, cell_b=None):
        """`(scores, grad_a[n, 3], grad_b[n, 3])` with grad = sum_r v_r dS_r/dx over the minimum-image rows
        (LoCoHD.gradient_from_coords_periodic) as torch CUDA tensors.  No coordinates are passed: disp carries the geometry.
        pair_weights: v, a tensor [n] (default: ones).  Assembled from `sensitivity_coords_periodic` by `dense_side_gradient_disp`."""
        sens = self.sensitivity_coords_periodic(cloud_a, cloud_b, wf_index=wf_index, box_a=box_a, box_b=box_b, cell_a=cell_a, cell_b=cell_b)
        return (sens.scores, self.dense_side_gradient_disp(sens.idx_a, sens.dist_a, sens.g_a, sens.disp_a, pair_weights),
                self.dense_side_gradient_disp(sens.idx_b, sens.dist_b, sens.g_b, sens.disp_b, pair_weights))

    def dense_side_gradient_disp(self, idx, dist, g, disp, pair_weights=None):
        """One side of gradient_coords_periodic, [n][3] f64: c = v g / d (0 in slot 0, where d == 0 and where g is not finite), T = c disp
        scattered into atom order by three [n][n] scatter_ passes (every atom occurs once per row and the padding has a column of its own: one
        writer per element), grad =
        T.sum(0) - T.sum(1): the atom as a member minus the atom as the row's own.  No index_add_, so the bits do not depend on torch's
        determinism setting."""
        torch = self.torch
        n = idx.shape[0]
        v = torch.ones(n, dtype=torch.float64, device=g.device) if pair_weights is None else pair_weights.to(torch.float64).reshape(-1)
        use = (idx >= 0) & (dist > 0.0) & torch.isfinite(g)
        use[:, 0] = False
        coef = torch.where(use, v[:, None] * g / torch.where(use, dist, torch.ones_like(dist)), torch.zeros_like(g))
        cols = torch.where(idx >= 0, idx, torch.full_like(idx, n)).long()  # (the padding goes to a spare column that is dropped)
        grad = torch.empty((n, 3), dtype=torch.float64, device=g.device)
        for d in range(3):
            t = torch.zeros((n, n + 1), dtype=torch.float64, device=g.device).scatter_(1, cols, coef * disp[..., d])[:, :n]
            grad[:, d] = t.sum(dim=0) - t.sum(dim=1)
        return grad

    def attribution_coords(self, cloud_a, cloud_b, out=None, wf_index=None, *, box_a=None, box_b=None, cell_a=None, cell_b=None):
        """Score attribution by category of the dense row pairs of two uploaded structures of equal size
        (LoCoHD.attribution_from_coords): returns (or fills) a torch float64 CUDA tensor [n][C] (lchd_attribution_coords_dev)."""
        return self._pair_rows_coords(None, cloud_a, cloud_b, out, wf_index, box_a, box_b, cell_a, cell_b)

    def from_coords_ensemble(self, batch, pairs=None, out=None, wf_index=None, excluded=None, *, boxes=None, cells=None):
        """LoCoHD.from_coords_ensemble on a batch from `upload_batch` (structures of equal size) or a frames buffer: row r of
        structure pair p = from_coords(seq, seq, X[i_p], X[j_p])[r].  pairs: torch int32 CUDA tensor [P][2] or None (every
        i < j); wf_index: torch int32 CUDA tensor [n] or None; excluded: iterable of (r, c) atom pairs counted as +inf.
        Returns (or fills) a torch float64 CUDA tensor [P][n].

        `boxes` / `cells` (keyword-only, host arrays): one periodic box (Lx, Ly, Lz) or cell (3 x 3) for all structures, or one per
        structure; the rows then follow the minimum-image convention (lchd_ensemble_from_coords_periodic_dev)."""
        if boxes is not None and cells is not None:
            raise ValueError("boxes and cells were both given: a batch is periodic in boxes or in cells")
        torch = self.torch
        dev = torch.device("cuda", self.device)
        total = int(N.lib().lchd_cloud_size(batch))
        m = self._n_structures(batch)
        pc = dense_cells(boxes, cells, m, "boxes", "cells")
        n = total // m if m else 0
        pairs_ptr, p = None, m * (m - 1) // 2
        if pairs is not None:
            assert pairs.is_cuda and pairs.dtype == torch.int32 and pairs.is_contiguous() and pairs.dim() == 2 and pairs.shape[1] == 2
            pairs_ptr, p = C.c_void_p(pairs.data_ptr()), pairs.shape[0]
        if out is None:
            out = torch.empty((p, n), dtype=torch.float64, device=dev)
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= p * n
        wf_ptr = None
        if wf_index is not None:
            assert wf_index.is_cuda and wf_index.dtype == torch.int32 and wf_index.is_contiguous() and wf_index.numel() >= n
            wf_ptr = C.c_void_p(wf_index.data_ptr())
        xs_ptr = xi_ptr = None
        keep = []
        if excluded is not None:
            xs, xi = LoCoHD._exclusion_csr(excluded, n)
            xs_t, xi_t = torch.from_numpy(xs).to(dev), torch.from_numpy(xi if len(xi) else np.zeros(1, dtype=np.int32)).to(dev)
            keep += [xs_t, xi_t]
            xs_ptr, xi_ptr = C.c_void_p(xs_t.data_ptr()), C.c_void_p(xi_t.data_ptr())
        if pc is not None:
            N.check(N.lib().lchd_ensemble_from_coords_periodic_dev(self._ctx, batch, pairs_ptr, p, xs_ptr, xi_ptr, wf_ptr, N.dp(pc), len(pc),
                                                                   C.c_void_p(out.data_ptr())))
            return out
        N.check(N.lib().lchd_ensemble_from_coords_dev(self._ctx, batch, pairs_ptr, p, xs_ptr, xi_ptr, wf_ptr, C.c_void_p(out.data_ptr())))
        return out

    def _n_structures(self, cloud) -> int:
        """Structures a cloud / batch / frames buffer currently holds (lchd_cloud_structures)."""
        return int(N.lib().lchd_cloud_structures(cloud))

    # ---- asynchronous form + trajectory streaming ----------------------------------------------------------------
    def from_primitives_async(self, cloud_a, cloud_b, anchors, threshold_distance: float, out, wf_index=None):
        """Enqueue one pass and return immediately; `finish()` waits for it and raises on errors."""
        torch = self.torch
        assert anchors.is_cuda and anchors.dtype == torch.int64 and anchors.is_contiguous()
        assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= anchors.shape[0]
        wf_ptr = None if wf_index is None else C.c_void_p(wf_index.data_ptr())
        N.check(N.lib().lchd_from_primitives_dev_async(self._ctx, cloud_a, cloud_b, C.c_void_p(anchors.data_ptr()), wf_ptr,
                                                       anchors.shape[0], float(threshold_distance), C.c_void_p(out.data_ptr())))

    def finish(self):
        N.check(N.lib().lchd_ctx_finish(self._ctx))

    def frames_buffer(self, template_cloud, capacity_frames: int):
        """Device buffer for `capacity_frames` frames of the template structure (same atoms, new coordinates)."""
        h = C.c_void_p()
        N.check(N.lib().lchd_frames_create(self._ctx, template_cloud, int(capacity_frames), C.byref(h)))
        self._clouds.append(h)
        return h

    def load_frames(self, buf, xyz: np.ndarray, stream=None):
        """Stage xyz [n_frames][n_atoms][3] (host) into a frames buffer; the copy runs on `stream` (a torch.cuda.Stream)
        without waiting, so it overlaps a pass that is running on the session's own stream."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        assert xyz.ndim == 3 and xyz.shape[2] == 3
        sp = None if stream is None else C.c_void_p(stream.cuda_stream)
        N.check(N.lib().lchd_frames_load(self._ctx, buf, N.dp(xyz), xyz.shape[0], sp))

    def set_frame_sources(self, buf, topology):
        """Tell a frames buffer how its primitive atoms are made from SOURCE atoms (a `PrimitiveTopology` from
        PrimitiveAssigner.compile_topology): afterwards `load_atom_frames` takes raw float32 atom coordinates and the
        centroids are evaluated on the device."""
        ss = np.ascontiguousarray(topology.src_start, dtype=np.int32)
        si = np.ascontiguousarray(topology.src_idx, dtype=np.int32)
        N.check(N.lib().lchd_frames_set_sources(self._ctx, buf, N.ip(ss), N.ip(si), int(topology.n_atoms)))

    def load_atom_frames(self, buf, atom_xyz: np.ndarray, stream=None):
        """Stage float32 SOURCE-atom coordinates [n_frames][n_src_atoms][3] (host); H2D copy and the centroid kernel run on
        `stream` without waiting (same overlap rules as load_frames)."""
        atom_xyz = np.ascontiguousarray(atom_xyz, dtype=np.float32)
        assert atom_xyz.ndim == 3 and atom_xyz.shape[2] == 3
        sp = None if stream is None else C.c_void_p(stream.cuda_stream)
        N.check(N.lib().lchd_frames_load_atoms(self._ctx, buf, atom_xyz.ctypes.data_as(C.POINTER(C.c_float)), atom_xyz.shape[0], sp))

    def load_atom_frames_dev(self, buf, atom_xyz, stream=None):
        """As load_atom_frames with the float32 source atoms already on the device: a torch CUDA tensor [n_frames][n_src][3]."""
        assert atom_xyz.is_cuda and atom_xyz.dtype == self.torch.float32 and atom_xyz.is_contiguous() and atom_xyz.dim() == 3
        sp = None if stream is None else C.c_void_p(stream.cuda_stream)
        N.check(N.lib().lchd_frames_load_atoms_dev(self._ctx, buf, C.c_void_p(atom_xyz.data_ptr()), atom_xyz.shape[0], sp))

    def last_convert_ms(self, buf) -> float:
        return float(N.lib().lchd_frames_last_convert_ms(self._ctx, buf))

    def coords_of(self, cloud, n: int) -> np.ndarray:
        """Primitive-atom coordinates currently held by a cloud / frames buffer, as float64 [n][3] on the host."""
        out = np.empty((int(n), 3), dtype=np.float64)
        N.check(N.lib().lchd_cloud_get_coords(self._ctx, cloud, N.dp(out), int(n)))
        return out

    def score_trajectory(self, ref_cloud, frames_xyz: np.ndarray, local_pairs, threshold_distance: float, chunk: int = 1024,
                         topology=None, ref_box=None, boxes=None, ref_cell=None, cells=None):
        """MD-trajectory mode (python_codes/trajectory_analyzer.py:97-119): score every frame of `frames_xyz`
        [n_frames][n_atoms][3] against the reference structure for the anchor pairs `local_pairs` [(atom in reference,
        atom in frame)].  Frames are streamed in chunks: while chunk k is scored, chunk k+1 is copied on a second
        stream into the other of two buffers.  Returns a float64 array [n_frames][len(local_pairs)].

        With `topology` (PrimitiveAssigner.compile_topology of the trajectory's structure) `frames_xyz` holds the float32
        coordinates of the SOURCE atoms, [n_frames][topology.n_atoms][3], and the per-frame structure -> primitive-atom
        conversion (trajectory_analyzer.py:37-74) runs on the device as well.

        `ref_box` / `boxes` (additive): orthorhombic periodic boxes (Lx, Ly, Lz) of the reference structure and of the frames
        ([n_frames][3], or [3] for a constant box); environments then hold the periodic images within `threshold_distance`.
        The reference's image cloud is built once, a chunk's is rebuilt on the scoring stream behind the chunk's upload.

        `ref_cell` / `cells` (additive): triclinic cells (3 x 3, rows = lattice vectors) in place of `ref_box` / `boxes`:
        [n_frames][3][3] (a cell per frame, NPT) or [3][3] for a constant cell."""
        if ref_box is not None and ref_cell is not None:
            raise ValueError("ref_box and ref_cell were both given: the reference has one periodic box or one periodic cell")
        if boxes is not None and cells is not None:
            raise ValueError("boxes and cells were both given: the frames are periodic in boxes or in cells")
        torch = self.torch
        if topology is not None:
            frames_xyz = np.ascontiguousarray(frames_xyz, dtype=np.float32)
            if frames_xyz.ndim != 3 or frames_xyz.shape[1:] != (topology.n_atoms, 3):
                raise ValueError(f"expected [n_frames][{topology.n_atoms}][3] source-atom coordinates, got {frames_xyz.shape}")
            n_frames, n_atoms = frames_xyz.shape[0], len(topology)
            load = self.load_atom_frames
        else:
            frames_xyz = np.ascontiguousarray(frames_xyz, dtype=np.float64)
            n_frames, n_atoms = frames_xyz.shape[0], frames_xyz.shape[1]
            load = self.load_frames
        thr = float(threshold_distance)
        if boxes is not None:
            boxes = periodic_boxes(boxes, n_frames, thr, "boxes")
        if cells is not None:
            cells = periodic_cells(cells, n_frames, thr, "cells")
        if ref_cell is not None:
            ref_side = self.periodic_images(ref_cloud, reach=thr, cell=ref_cell)
        else:
            ref_side = ref_cloud if ref_box is None else self.periodic_images(ref_cloud, ref_box, thr)
        lp = np.ascontiguousarray(local_pairs, dtype=np.int64).reshape(-1, 2)
        chunk = max(1, min(int(chunk), n_frames))
        dev = torch.device("cuda", self.device)
        offs = torch.arange(chunk, dtype=torch.int64, device=dev).repeat_interleave(len(lp)) * n_atoms
        anchors = torch.from_numpy(np.tile(lp, (chunk, 1))).to(dev)
        anchors[:, 1] += offs
        anchors = anchors.contiguous()
        out = torch.empty(n_frames * len(lp), dtype=torch.float64, device=dev)
        bufs = [self.frames_buffer(ref_cloud, chunk), self.frames_buffer(ref_cloud, chunk)]
        images = [None, None]  # one image cloud per buffer, made by the first chunk that uses the buffer
        if topology is not None:
            for b in bufs:
                self.set_frame_sources(b, topology)
        try:
            copy_stream = torch.cuda.Stream(device=dev)
            starts = list(range(0, n_frames, chunk))
            load(bufs[0], frames_xyz[starts[0]:starts[0] + chunk], copy_stream)
            for k, f0 in enumerate(starts):
                nf = min(chunk, n_frames - f0)
                side_b = bufs[k % 2]
                if boxes is not None:
                    bx = boxes if len(boxes) == 1 else boxes[f0:f0 + nf]
                    if images[k % 2] is None:
                        images[k % 2] = self.periodic_images(side_b, bx, thr)
                    else:
                        self.update_images(images[k % 2], side_b, bx)
                    side_b = images[k % 2]
                if cells is not None:
                    cx = cells if len(cells) == 1 else cells[f0:f0 + nf]
                    if images[k % 2] is None:
                        images[k % 2] = self.periodic_images(side_b, reach=thr, cell=cx)
                    else:
                        self.update_images(images[k % 2], side_b, cell=cx)
                    side_b = images[k % 2]
                self.from_primitives_async(ref_side, side_b, anchors[: nf * len(lp)], threshold_distance,
                                           out[f0 * len(lp):(f0 + nf) * len(lp)])
                if k + 1 < len(starts):
                    f1 = starts[k + 1]
                    load(bufs[(k + 1) % 2], frames_xyz[f1:f1 + chunk], copy_stream)
                self.finish()
            return out.cpu().numpy().reshape(n_frames, len(lp))
        finally:  # the two frames buffers go away on every path out (a failed load or finish included)
            try:
                self.finish()
            except Exception:
                pass
            for b in bufs + [h for h in images if h is not None] + ([ref_side] if ref_side is not ref_cloud else []):
                N.lib().lchd_cloud_destroy(self._ctx, b)
                self._clouds.remove(b)

    def close(self):
        if self._ctx:
            from .dist import clear_shard_cache

            clear_shard_cache(self)  # remembered partitions made with this session pin device tensors
            for h in self._clouds:
                N.lib().lchd_cloud_destroy(self._ctx, h)
            self._clouds = []
            N.lib().lchd_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
