"""LoCoHD scores as a differentiable torch function (additive): a movable structure against a fixed uploaded reference.

    scores = locohd_scores(session, cloud_b_ref, xyz_a, cat_a, tag_a, anchors, threshold_distance)
    scores.sum().backward()          # xyz_a.grad = d sum(scores) / d xyz_a

Forward is DeviceSession.sensitivity, backward is DeviceSession.assemble_gradient with grad_output as the pair weights.  The derivative
ignores points entering or leaving at the threshold (exact when the weight function's support ends at or inside it: the default, uniform
[3, 10] with threshold 10) and is one-sided at ties.  The movable structure is uploaded from the host on every forward call.

    scores = locohd_scores_dense(session, cloud_b_ref, xyz_a, cat_a)     # the dense rows of from_coords: no threshold, an exact derivative

Forward is DeviceSession.sensitivity_coords, backward is side A of DeviceSession.gradient_coords (dense_side_gradient).

Both take `native=True`: backward is then one DeviceSession.native_gradient / native_gradient_coords call with grad_output as the pair
weights -- the gradient reduced on the device into exact accumulators, its bits a function of the inputs alone.

    scores = locohd_scores_dense_periodic(session, cloud_b_ref, xyz_a, cat_a, box=(Lx, Ly, Lz))   # ... on minimum-image rows

Forward is DeviceSession.sensitivity_coords_periodic, backward is side A of DeviceSession.gradient_coords_periodic
(dense_side_gradient_disp): the displacements of the chosen images carry the geometry.

    scores = locohd_scores_periodic(session, cloud_b_ref, xyz_a, cat_a, tag_a, anchors, threshold_distance, box=(Lx, Ly, Lz))

The movable structure in a periodic box or cell: forward is DeviceSession.sensitivity_images on its image cloud, backward is side A of
DeviceSession.gradient_images (side_gradient_images).

    scores = locohd_scores_weighted(session, cloud_a, cloud_b, anchors, threshold_distance, category_weights)

Two fixed uploaded clouds, differentiable with respect to the category weights: forward is DeviceSession.set_category_weights and
DeviceSession.from_primitives, backward one DeviceSession.category_gradient call.  The session keeps the last weights set.

    scores = locohd_scores_wf(session, cloud_a, cloud_b, anchors, threshold_distance, wf_params)

Two fixed uploaded clouds, differentiable with respect to the parameters of the session's single weight function: forward is
DeviceSession.set_weight_function and DeviceSession.from_primitives, backward one DeviceSession.weight_gradient call.  The session keeps
the last parameters set.

Both take `native=True`: backward is then one DeviceSession.category_gradient_sum / weight_gradient_sum call with grad_output as the pair
weights, the exact sum of the terms rounded once, with no per-pair block in torch.

The two periodic forms take `native=True` as well: forward and backward are then one DeviceSession.native_gradient_images /
native_gradient_coords_periodic call each, backward with grad_output as the pair weights.  Boxes and cells stay non-differentiable.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N


class _LoCoHDScores(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz_a, session, cloud_b_ref, cat_a, tag_a, anchors, threshold_distance):
        x = xyz_a.detach()
        cloud_a = session.upload(x.cpu().numpy(), np.asarray(cat_a, dtype=np.int32), None if tag_a is None else np.asarray(tag_a, dtype=np.int32))
        try:
            sens = session.sensitivity(cloud_a, cloud_b_ref, anchors, threshold_distance)
        finally:
            session._clouds.remove(cloud_a)
            N.lib().lchd_cloud_destroy(session._ctx, cloud_a)
        ctx.session = session
        ctx.sens = sens
        ctx.save_for_backward(x)
        return sens.scores

    @staticmethod
    def backward(ctx, grad_output):
        (x,) = ctx.saved_tensors
        s = ctx.sens
        grad_a = ctx.session.side_gradient(s.scores, s.idx_a, s.dist_a, s.g_a, x.to(torch.float64), grad_output)  # side A alone moves
        return grad_a.to(x.dtype), None, None, None, None, None, None


class _LoCoHDScoresNative(torch.autograd.Function):
    """locohd_scores(native=True): forward and backward are one DeviceSession.native_gradient call each, no list is kept between them."""

    @staticmethod
    def forward(ctx, xyz_a, session, cloud_b_ref, cat_a, tag_a, anchors, threshold_distance):
        x = xyz_a.detach()
        ctx.session, ctx.cloud_b, ctx.anchors, ctx.thr = session, cloud_b_ref, anchors, threshold_distance
        ctx.cat = np.asarray(cat_a, dtype=np.int32)
        ctx.tag = None if tag_a is None else np.asarray(tag_a, dtype=np.int32)
        ctx.save_for_backward(x)
        return _native_call(ctx, x, None)[0]

    @staticmethod
    def backward(ctx, grad_output):
        (x,) = ctx.saved_tensors
        return _native_call(ctx, x, grad_output)[1].to(x.dtype), None, None, None, None, None, None  # side A alone moves


def _native_call(ctx, x, weights):
    """The movable structure uploaded, one native gradient call (thresholded with ctx.anchors, dense without), the structure dropped."""
    session = ctx.session
    cloud_a = session.upload(x.cpu().numpy(), ctx.cat, ctx.tag)
    try:
        if ctx.anchors is None:
            return session.native_gradient_coords(cloud_a, ctx.cloud_b, pair_weights=weights, wf_index=ctx.wf_index)
        return session.native_gradient(cloud_a, ctx.cloud_b, ctx.anchors, ctx.thr, pair_weights=weights)
    finally:
        session._clouds.remove(cloud_a)
        N.lib().lchd_cloud_destroy(session._ctx, cloud_a)


class _LoCoHDScoresDenseNative(torch.autograd.Function):
    """locohd_scores_dense(native=True): as _LoCoHDScoresNative, on DeviceSession.native_gradient_coords."""

    @staticmethod
    def forward(ctx, xyz_a, session, cloud_b_ref, cat_a, wf_index):
        x = xyz_a.detach()
        ctx.session, ctx.cloud_b, ctx.anchors, ctx.wf_index = session, cloud_b_ref, None, wf_index
        ctx.cat, ctx.tag = np.asarray(cat_a, dtype=np.int32), None
        ctx.save_for_backward(x)
        return _native_call(ctx, x, None)[0]

    @staticmethod
    def backward(ctx, grad_output):
        (x,) = ctx.saved_tensors
        return _native_call(ctx, x, grad_output)[1].to(x.dtype), None, None, None, None


class _LoCoHDScoresPeriodic(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz_a, session, cloud_b_ref, cat_a, tag_a, anchors, threshold_distance, box, cell):
        x = xyz_a.detach()
        mine = []  # the structure and its image cloud: both leave the session again
        try:
            mine.append(session.upload(x.cpu().numpy(), np.asarray(cat_a, dtype=np.int32), None if tag_a is None else np.asarray(tag_a, dtype=np.int32)))
            mine.append(session.periodic_images(mine[0], box, threshold_distance, cell=cell))
            sens = session.sensitivity_images(mine[1], cloud_b_ref, anchors, threshold_distance)
        finally:
            for cl in reversed(mine):
                session._clouds.remove(cl)
                N.lib().lchd_cloud_destroy(session._ctx, cl)
        ctx.session = session
        ctx.sens = sens
        ctx.n_atoms, ctx.dtype = x.shape[0], x.dtype
        return sens.scores

    @staticmethod
    def backward(ctx, grad_output):
        s = ctx.sens
        grad_a = ctx.session.side_gradient_images(s.scores, s.idx_a, s.dist_a, s.g_a, s.disp_a, ctx.n_atoms, grad_output)  # side A alone moves
        return grad_a.to(ctx.dtype), None, None, None, None, None, None, None, None


def _native_periodic_call(ctx, x, weights):
    """The movable structure uploaded (thresholded: with its image cloud), one native periodic gradient call, both dropped again."""
    session = ctx.session
    mine = []
    try:
        mine.append(session.upload(x.cpu().numpy(), ctx.cat, ctx.tag))
        if ctx.anchors is None:
            return session.native_gradient_coords_periodic(mine[0], ctx.cloud_b, pair_weights=weights, wf_index=ctx.wf_index, box_a=ctx.box,
                                                           cell_a=ctx.cell, box_b=ctx.ref_box, cell_b=ctx.ref_cell)
        mine.append(session.periodic_images(mine[0], ctx.box, ctx.thr, cell=ctx.cell))
        return session.native_gradient_images(mine[1], ctx.cloud_b, ctx.anchors, ctx.thr, pair_weights=weights)
    finally:
        for cl in reversed(mine):
            session._clouds.remove(cl)
            N.lib().lchd_cloud_destroy(session._ctx, cl)


class _LoCoHDScoresPeriodicNative(torch.autograd.Function):
    """locohd_scores_periodic(native=True): as _LoCoHDScoresNative, on DeviceSession.native_gradient_images."""

    @staticmethod
    def forward(ctx, xyz_a, session, cloud_b_ref, cat_a, tag_a, anchors, threshold_distance, box, cell):
        x = xyz_a.detach()
        ctx.session, ctx.cloud_b, ctx.anchors, ctx.thr, ctx.box, ctx.cell = session, cloud_b_ref, anchors, threshold_distance, box, cell
        ctx.cat = np.asarray(cat_a, dtype=np.int32)
        ctx.tag = None if tag_a is None else np.asarray(tag_a, dtype=np.int32)
        ctx.save_for_backward(x)
        return _native_periodic_call(ctx, x, None)[0]

    @staticmethod
    def backward(ctx, grad_output):
        (x,) = ctx.saved_tensors
        return (_native_periodic_call(ctx, x, grad_output)[1].to(x.dtype),) + (None,) * 8  # side A alone moves


class _LoCoHDScoresDensePeriodicNative(torch.autograd.Function):
    """locohd_scores_dense_periodic(native=True): as _LoCoHDScoresDenseNative, on DeviceSession.native_gradient_coords_periodic."""

    @staticmethod
    def forward(ctx, xyz_a, session, cloud_b_ref, cat_a, wf_index, box, cell, ref_box, ref_cell):
        x = xyz_a.detach()
        ctx.session, ctx.cloud_b, ctx.anchors, ctx.wf_index = session, cloud_b_ref, None, wf_index
        ctx.box, ctx.cell, ctx.ref_box, ctx.ref_cell = box, cell, ref_box, ref_cell
        ctx.cat, ctx.tag = np.asarray(cat_a, dtype=np.int32), None
        ctx.save_for_backward(x)
        return _native_periodic_call(ctx, x, None)[0]

    @staticmethod
    def backward(ctx, grad_output):
        (x,) = ctx.saved_tensors
        return (_native_periodic_call(ctx, x, grad_output)[1].to(x.dtype),) + (None,) * 8


class _LoCoHDScoresDense(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz_a, session, cloud_b_ref, cat_a, wf_index):
        x = xyz_a.detach()
        cloud_a = session.upload(x.cpu().numpy(), np.asarray(cat_a, dtype=np.int32))
        try:
            sens = session.sensitivity_coords(cloud_a, cloud_b_ref, wf_index=wf_index)
        finally:
            session._clouds.remove(cloud_a)
            N.lib().lchd_cloud_destroy(session._ctx, cloud_a)
        ctx.session = session
        ctx.sens = sens
        ctx.save_for_backward(x)
        return sens.scores

    @staticmethod
    def backward(ctx, grad_output):
        (x,) = ctx.saved_tensors
        s = ctx.sens
        grad_a = ctx.session.dense_side_gradient(s.idx_a, s.dist_a, s.g_a, x, grad_output)  # side A alone moves
        return grad_a.to(x.dtype), None, None, None, None


class _LoCoHDScoresDensePeriodic(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz_a, session, cloud_b_ref, cat_a, wf_index, box, cell, ref_box, ref_cell):
        x = xyz_a.detach()
        cloud_a = session.upload(x.cpu().numpy(), np.asarray(cat_a, dtype=np.int32))
        try:
            sens = session.sensitivity_coords_periodic(cloud_a, cloud_b_ref, wf_index=wf_index, box_a=box, cell_a=cell, box_b=ref_box,
                                                       cell_b=ref_cell)
        finally:
            session._clouds.remove(cloud_a)
            N.lib().lchd_cloud_destroy(session._ctx, cloud_a)
        ctx.session = session
        ctx.sens = sens
        ctx.dtype = x.dtype
        return sens.scores

    @staticmethod
    def backward(ctx, grad_output):
        s = ctx.sens
        grad_a = ctx.session.dense_side_gradient_disp(s.idx_a, s.dist_a, s.g_a, s.disp_a, grad_output)  # side A alone moves
        return grad_a.to(ctx.dtype), None, None, None, None, None, None, None, None


def locohd_scores_dense_periodic(session, cloud_b_ref, xyz_a, cat_a, wf_index=None, *, box=None, cell=None, ref_box=None, ref_cell=None,
                                 native=False):
    """`locohd_scores_dense` under minimum-image periodic boundaries (DeviceSession.sensitivity_coords_periodic): `box` / `cell` is the
    periodic box (Lx, Ly, Lz) or cell (3 x 3) of the movable structure, `ref_box` / `ref_cell` that of the reference; a structure with
    neither is open.  Backward is side A of DeviceSession.gradient_coords_periodic with grad_output as the row weights; xyz_a need not be
    wrapped: the gradient is the one with respect to xyz_a as given.  native=True: forward and backward are one
    DeviceSession.native_gradient_coords_periodic call each (its bits); boxes and cells are not differentiable either way."""
    if native:
        return _LoCoHDScoresDensePeriodicNative.apply(xyz_a, session, cloud_b_ref, cat_a, wf_index, box, cell, ref_box, ref_cell)
    return _LoCoHDScoresDensePeriodic.apply(xyz_a, session, cloud_b_ref, cat_a, wf_index, box, cell, ref_box, ref_cell)


def locohd_scores_dense(session, cloud_b_ref, xyz_a, cat_a, wf_index=None, native=False):
    """The scores of the dense rows (DeviceSession.sensitivity_coords: row r = both structures seen from their atoms r) of a movable
    structure -- xyz_a: torch float64 CUDA tensor [n][3], cat_a: its category ids (host array) -- against `cloud_b_ref`, a structure of
    the same size uploaded to `session`; differentiable with respect to xyz_a.  Backward is side A of DeviceSession.gradient_coords with
    grad_output as the row weights: exact (no threshold), one-sided at ties.  native=True: backward is one
    DeviceSession.native_gradient_coords call with grad_output as the pair weights (its bits; forward is such a call too, so no list is
    kept between the two)."""
    if native:
        return _LoCoHDScoresDenseNative.apply(xyz_a, session, cloud_b_ref, cat_a, wf_index)
    return _LoCoHDScoresDense.apply(xyz_a, session, cloud_b_ref, cat_a, wf_index)


def locohd_scores(session, cloud_b_ref, xyz_a, cat_a, tag_a, anchors, threshold_distance, native=False):
    """The scores of the anchor pairs (torch int64 CUDA tensor [P][2]: atom of the movable structure, atom of the reference) of a
    movable structure -- xyz_a: torch float64 CUDA tensor [Na][3], cat_a / tag_a: its category ids and interned tags (host arrays) --
    against `cloud_b_ref`, a cloud uploaded to `session`; differentiable with respect to xyz_a.  native=True: backward is one
    DeviceSession.native_gradient call with grad_output as the pair weights (its bits; forward is such a call too, so no list is kept
    between the two); the default leaves the assembly in torch."""
    if native:
        return _LoCoHDScoresNative.apply(xyz_a, session, cloud_b_ref, cat_a, tag_a, anchors, float(threshold_distance))
    return _LoCoHDScores.apply(xyz_a, session, cloud_b_ref, cat_a, tag_a, anchors, float(threshold_distance))


def locohd_scores_periodic(session, cloud_b_ref, xyz_a, cat_a, tag_a, anchors, threshold_distance, *, box=None, cell=None, native=False):
    """`locohd_scores` for a movable structure in a periodic box (Lx, Ly, Lz) or triclinic cell (3 x 3, lattice vectors as rows): the
    structure is uploaded, its image cloud is built with reach = threshold_distance, and both leave the session again.  `cloud_b_ref` is
    any cloud of `session`, an image cloud (DeviceSession.periodic_images) included.  xyz_a need not be wrapped: a wrap is a translation
    by a lattice vector, so the gradient is the one with respect to xyz_a as given.  native=True: forward and backward are one
    DeviceSession.native_gradient_images call each (its bits); the box or cell is not differentiable either way."""
    if native:
        return _LoCoHDScoresPeriodicNative.apply(xyz_a, session, cloud_b_ref, cat_a, tag_a, anchors, float(threshold_distance), box, cell)
    return _LoCoHDScoresPeriodic.apply(xyz_a, session, cloud_b_ref, cat_a, tag_a, anchors, float(threshold_distance), box, cell)


class _LoCoHDScoresWeighted(torch.autograd.Function):
    @staticmethod
    def forward(ctx, category_weights, session, cloud_a, cloud_b, anchors, threshold_distance, wf_index, native):
        w = category_weights.detach()
        session.set_category_weights(w)
        ctx.session, ctx.clouds, ctx.anchors, ctx.thr, ctx.wf_index = session, (cloud_a, cloud_b), anchors, threshold_distance, wf_index
        ctx.native = bool(native)
        ctx.save_for_backward(w)
        return session.from_primitives(cloud_a, cloud_b, anchors, threshold_distance, wf_index=wf_index)

    @staticmethod
    def backward(ctx, grad_output):
        (w,) = ctx.saved_tensors
        session = ctx.session
        session.set_category_weights(w)  # (a no-op unless the session's weights were set again since forward)
        if ctx.native:  # (one call, grad_output as the pair weights: the rows never reach torch)
            grad_w = session.category_gradient_sum(ctx.clouds[0], ctx.clouds[1], ctx.anchors, ctx.thr, grad_output, wf_index=ctx.wf_index)
        else:
            g = session.category_gradient(ctx.clouds[0], ctx.clouds[1], ctx.anchors, ctx.thr, wf_index=ctx.wf_index)
            grad_w = (g * grad_output.to(g.dtype)[:, None]).sum(0)
        return grad_w.to(device=w.device, dtype=w.dtype), None, None, None, None, None, None, None


def locohd_scores_weighted(session, cloud_a, cloud_b, anchors, threshold_distance, category_weights, wf_index=None, native=False):
    """The scores of the anchor pairs (torch int64 CUDA tensor [P][2]) of two clouds uploaded to `session`, differentiable with respect
    to `category_weights`, a float64 tensor [C] of positive values (on any device) that may require grad.  Forward sets the session's
    weights (DeviceSession.set_category_weights) and scores (DeviceSession.from_primitives); backward is one
    DeviceSession.category_gradient call, returning (G * grad_output[:, None]).sum(0).  Hellinger and Kullback-Leibler distances.
    Coordinates are not differentiated here.  The session keeps the last weights set: later calls of the session score with them, and a
    backward call puts the weights of its forward call back first.  native=True: backward is one DeviceSession.category_gradient_sum call
    with grad_output as the pair weights -- no (P, C) block, every column the correctly rounded exact sum (its bits); forward is the same
    either way."""
    return _LoCoHDScoresWeighted.apply(category_weights, session, cloud_a, cloud_b, anchors, float(threshold_distance), wf_index, native)


class _LoCoHDScoresWf(torch.autograd.Function):
    @staticmethod
    def forward(ctx, wf_params, session, cloud_a, cloud_b, anchors, threshold_distance, native):
        prm = wf_params.detach()
        session.set_weight_function(prm)
        ctx.session, ctx.clouds, ctx.anchors, ctx.thr = session, (cloud_a, cloud_b), anchors, threshold_distance
        ctx.native = bool(native)
        ctx.save_for_backward(prm)
        return session.from_primitives(cloud_a, cloud_b, anchors, threshold_distance)

    @staticmethod
    def backward(ctx, grad_output):
        (prm,) = ctx.saved_tensors
        session = ctx.session
        session.set_weight_function(prm)  # (a no-op unless the session's parameters were set again since forward)
        if ctx.native:  # (one call, grad_output as the pair weights; a single function: row 0 of [1][NP])
            grad_prm = session.weight_gradient_sum(ctx.clouds[0], ctx.clouds[1], ctx.anchors, ctx.thr, grad_output).grad[0]
        else:
            grad = session.weight_gradient(ctx.clouds[0], ctx.clouds[1], ctx.anchors, ctx.thr).grad
            grad_prm = (grad * grad_output.to(grad.dtype)[:, None]).sum(0)
        return grad_prm.to(device=prm.device, dtype=prm.dtype), None, None, None, None, None, None


def locohd_scores_wf(session, cloud_a, cloud_b, anchors, threshold_distance, wf_params, native=False):
    """The scores of the anchor pairs (torch int64 CUDA tensor [P][2]) of two clouds uploaded to `session`, differentiable with respect
    to `wf_params`, a float64 tensor of the parameters of the session's single weight function (on any device) that may require grad.
    Forward sets the parameters (DeviceSession.set_weight_function) and scores (DeviceSession.from_primitives); backward is one
    DeviceSession.weight_gradient call, returning (grad * grad_output[:, None]).sum(0).  Every statistical distance; a single weight
    function only (a dictionary is a ValueError).  Coordinates and category weights are not differentiated here.  The session keeps the
    last parameters set: later calls of the session score with them, and a backward call puts the parameters of its forward call back
    first.  native=True: backward is one DeviceSession.weight_gradient_sum call with grad_output as the pair weights (its bits); forward is
    the same either way."""
    return _LoCoHDScoresWf.apply(wf_params, session, cloud_a, cloud_b, anchors, float(threshold_distance), native)
