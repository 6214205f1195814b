"""The reference's Python surface (loco_hd/loco_hd.pyi) over the MI355X-native core.

Five classes with the reference's names, argument meaning and error behaviour:

    WeightFunction        /root/reference/src/locohd/weight_function.rs:6-120
    PrimitiveAtom         /root/reference/src/locohd/primitive_atom.rs:4-25
    TagPairingRule        /root/reference/src/locohd/tag_pairing_rule.rs:5-75
    StatisticalDistance   /root/reference/src/locohd/pmf/statistical_distances.rs:87-142
    LoCoHD                /root/reference/src/locohd.rs:42-55, 286-568

This module only validates, interns strings (categories -> the index the reference's HashMap gives
them, tags -> integers) and packs contiguous NumPy buffers; all scoring happens in
libloco_hd_hip.so on the GPU.  There is no CPU fallback: without a usable MI355X the four from_*
methods raise DeviceError.
"""
from __future__ import annotations

import ctypes as C
import threading
from collections import namedtuple
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _native as N

# what LoCoHD.sensitivity_from_primitives returns (DeviceSession.sensitivity: the same fields as torch tensors)
Sensitivity = namedtuple("Sensitivity", "scores count_a idx_a dist_a g_a count_b idx_b dist_b g_b")
# what LoCoHD.sensitivity_from_primitives_periodic returns (DeviceSession.sensitivity_images: the same fields as torch tensors)
PeriodicSensitivity = namedtuple("PeriodicSensitivity", "scores count_a idx_a image_a dist_a g_a disp_a count_b idx_b image_b dist_b g_b disp_b")
# what LoCoHD.sensitivity_from_coords_periodic returns (DeviceSession.sensitivity_coords_periodic: the same fields as torch tensors): a
# Sensitivity of dense minimum-image rows plus, per side, disp[n, K, 3], the displacement from row atom r to the nearest image of member
# idx[r, k] (dist = |disp| bit for bit); every atom occurs once, so there are no image codes
MinImageSensitivity = namedtuple("MinImageSensitivity", "scores count_a idx_a dist_a g_a disp_a count_b idx_b dist_b g_b disp_b")
# what the native periodic gradient calls return with strain=True (DeviceSession: the same fields as torch tensors): strain_a / strain_b are
# the (3, 3) strain derivatives of the weighted score sum, one per side (include/loco_hd_hip.h, "the strain derivative")
NativeGradient = namedtuple("NativeGradient", "scores grad_a grad_b strain_a strain_b")
# what the weight-function gradient calls return (DeviceSession.weight_gradient: the same fields as torch tensors): scores (P,) and
# grad (P, NP), row p the derivatives of pair p's score with respect to the parameters of its weight function, zero-padded to NP columns
WeightGradient = namedtuple("WeightGradient", "scores grad")
# what the reduced weight-function gradient calls return (DeviceSession.weight_gradient_sum: the same fields as torch tensors): scores (P,)
# and grad (n_wf, NP), row f the exact sum of v_p dS_p/dtheta over the pairs scored with function f, zero-padded to NP columns
WeightGradientSum = namedtuple("WeightGradientSum", "scores grad")
# what LoCoHD.nearest_from_primitives returns (DeviceSession.nearest: the same fields as torch tensors)
Nearest = namedtuple("Nearest", "scores cols")

try:  # built by `make -C loco_hd_amd/csrc`; argument conversion only -- without it the same conversion runs as a Python loop
    from . import _fastpack
except ImportError:  # pragma: no cover
    _fastpack = None

WF_KINDS = {"hyper_exp": 0, "dagum": 1, "uniform": 2, "kumaraswamy": 3}
SD_KINDS = {"Hellinger": 0, "Kolmogorov-Smirnov": 1, "Kullback-Leibler": 2, "Renyi": 3}
_CATEGORY_GRADIENT = "category gradient"  # the third selector of the _pair_rows_from_* helpers, next to None and an edge array


def _f64(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float64)


def periodic_boxes(box, n_structures: int, reach: float, what: str = "box") -> np.ndarray:
    """An orthorhombic box (Lx, Ly, Lz), or one per structure, as a float64 array [n_boxes][3] (n_boxes is 1 or `n_structures`).
    ValueError for another shape and for what lchd_box_validate rejects (an edge or `reach` that is not finite and > 0, `reach`
    beyond the smallest edge).  No device is touched."""
    try:
        arr = _f64(box)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be three edge lengths (Lx, Ly, Lz)") from None
    if arr.shape == (3,):
        arr = arr.reshape(1, 3)
    elif arr.ndim != 2 or arr.shape[1] != 3:
        raise ValueError(f"{what} must be three edge lengths (Lx, Ly, Lz), got an array of shape {arr.shape}")
    if len(arr) not in (1, int(n_structures)):
        raise ValueError(f"{what}: {len(arr)} boxes given for {n_structures} structures (pass one box, or one per structure)")
    N.check(N.lib().lchd_box_validate(N.dp(arr), len(arr), float(reach)))
    return arr


def periodic_cells(cell, n_structures: int, reach: float, what: str = "cell") -> np.ndarray:
    """A triclinic cell (3 x 3, rows = the lattice vectors a, b, c), or one per structure, as a float64 array [n_cells][3][3] (n_cells
    is 1 or `n_structures`).  ValueError for another shape and for what lchd_cell_validate rejects (a non-finite entry, a singular
    cell, a `reach` that is not finite and > 0 or lies beyond the smallest perpendicular width).  No device is touched."""
    try:
        arr = _f64(cell)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a 3 x 3 matrix of lattice vectors (rows a, b, c)") from None
    if arr.shape == (3, 3):
        arr = arr.reshape(1, 3, 3)
    elif arr.ndim != 3 or arr.shape[1:] != (3, 3):
        raise ValueError(f"{what} must be a 3 x 3 matrix of lattice vectors (rows a, b, c), got an array of shape {arr.shape}")
    if len(arr) not in (1, int(n_structures)):
        raise ValueError(f"{what}: {len(arr)} cells given for {n_structures} structures (pass one cell, or one per structure)")
    N.check(N.lib().lchd_cell_validate(N.dp(arr), len(arr), float(reach)))
    return arr


def dense_cells(box, cell, n_structures: int, what_box: str = "box", what_cell: str = "cell") -> Optional[np.ndarray]:
    """The periodic cells of a dense (minimum-image) call as a float64 array [n_cells][3][3] (n_cells is 1 or `n_structures`), or None
    when neither is given: a box (Lx, Ly, Lz) becomes its diagonal cell.  The shape checks of `periodic_boxes` / `periodic_cells`
    without a reach (a dense row has no threshold); ValueError for an edge that is not finite and > 0 and for what lchd_cell_reduce
    rejects (a non-finite entry, a singular cell).  No device is touched."""
    if box is None and cell is None:
        return None
    if box is not None:
        try:
            arr = _f64(box)
        except (TypeError, ValueError):
            raise ValueError(f"{what_box} must be three edge lengths (Lx, Ly, Lz)") from None
        if arr.shape == (3,):
            arr = arr.reshape(1, 3)
        elif arr.ndim != 2 or arr.shape[1] != 3:
            raise ValueError(f"{what_box} must be three edge lengths (Lx, Ly, Lz), got an array of shape {arr.shape}")
        if len(arr) not in (1, int(n_structures)):
            raise ValueError(f"{what_box}: {len(arr)} boxes given for {n_structures} structures (pass one box, or one per structure)")
        if not (np.isfinite(arr).all() and (arr > 0.0).all()):
            raise ValueError(f"{what_box}: every edge must be finite and > 0")
        cells = np.zeros((len(arr), 3, 3))
        for k in range(3):
            cells[:, k, k] = arr[:, k]
    else:
        try:
            cells = _f64(cell)
        except (TypeError, ValueError):
            raise ValueError(f"{what_cell} must be a 3 x 3 matrix of lattice vectors (rows a, b, c)") from None
        if cells.shape == (3, 3):
            cells = cells.reshape(1, 3, 3)
        elif cells.ndim != 3 or cells.shape[1:] != (3, 3):
            raise ValueError(f"{what_cell} must be a 3 x 3 matrix of lattice vectors (rows a, b, c), got an array of shape {cells.shape}")
        if len(cells) not in (1, int(n_structures)):
            raise ValueError(f"{what_cell}: {len(cells)} cells given for {n_structures} structures (pass one cell, or one per structure)")
    cells = np.ascontiguousarray(cells, dtype=np.float64)
    reduced, inverse = np.empty(9), np.empty(9)
    for c in cells:
        N.check(N.lib().lchd_cell_reduce(N.dp(np.ascontiguousarray(c)), N.dp(reduced), N.dp(inverse)))
    return cells


def cell_reduce(cell) -> Tuple[np.ndarray, np.ndarray]:
    """lchd_cell_reduce: the Minkowski-reduced form of a 3 x 3 cell (same lattice) and the inverse of the reduced cell, the two
    matrices the minimum-image rows of the dense periodic calls are computed with.  A diagonal cell comes back unchanged."""
    c = _f64(cell)
    if c.shape != (3, 3):
        raise ValueError(f"cell must be a 3 x 3 matrix of lattice vectors (rows a, b, c), got an array of shape {c.shape}")
    reduced, inverse = np.empty((3, 3)), np.empty((3, 3))
    N.check(N.lib().lchd_cell_reduce(N.dp(c), N.dp(reduced), N.dp(inverse)))
    return reduced, inverse


def cell_gradient(strain, cell) -> np.ndarray:
    """dL/dh at fixed fractional coordinates from a strain derivative W (`NativeGradient.strain_a` / `strain_b`): inv(h).T @ W for the
    cell h (3 x 3, rows = the lattice vectors); a box (Lx, Ly, Lz) is taken as diag(Lx, Ly, Lz), the derivative with respect to Lx is
    then element [0, 0].  Host arithmetic in float64; ValueError for another shape or a singular cell."""
    w, h = _f64(strain), _f64(cell)
    if w.shape != (3, 3):
        raise ValueError(f"strain must be a 3 x 3 matrix, got an array of shape {w.shape}")
    if h.shape == (3,):
        h = np.diag(h)
    if h.shape != (3, 3):
        raise ValueError(f"cell must be a 3 x 3 matrix of lattice vectors (rows a, b, c) or three edge lengths, got an array of shape {h.shape}")
    if not np.isfinite(h).all() or np.linalg.matrix_rank(h) < 3:
        raise ValueError("cell is singular or not finite")
    return np.linalg.solve(h.T, w)  # inv(h).T @ w


def cell_from_lengths_angles(a: float, b: float, c: float, alpha: float, beta: float, gamma: float) -> np.ndarray:
    """The 3 x 3 cell (rows = lattice vectors) of the lengths a, b, c and the angles alpha = (b, c), beta = (a, c), gamma = (a, b) in
    degrees, in the orientation of PDB / GROMACS / MDAnalysis: a along x, b in the xy plane.  An angle of exactly 90 gives exact
    zeros, so (L, L, L, 90, 90, 90) is diag(L)."""
    a, b, c = float(a), float(b), float(c)

    def cos_sin(deg):
        deg = float(deg)
        if deg == 90.0:
            return 0.0, 1.0
        rad = np.deg2rad(deg)
        return float(np.cos(rad)), float(np.sin(rad))
    (ca, _), (cb, _), (cg, sg) = cos_sin(alpha), cos_sin(beta), cos_sin(gamma)
    if not (a > 0.0 and b > 0.0 and c > 0.0 and sg > 0.0):
        raise ValueError(f"no cell has the lengths ({a}, {b}, {c}) and the angle gamma = {gamma}")
    cy = (ca - cb * cg) / sg
    cz2 = 1.0 - cb * cb - cy * cy
    if not cz2 > 0.0:
        raise ValueError(f"no cell has the angles ({alpha}, {beta}, {gamma})")
    return np.array([[a, 0.0, 0.0], [b * cg, b * sg, 0.0], [c * cb, c * cy, c * float(np.sqrt(cz2))]])


class WeightFunction:
    """weight_function.rs:6-120.  ``parameters`` and ``function_name`` are read-only like the pyo3 getters."""

    __slots__ = ("_name", "_params", "_kind", "_p")

    def __init__(self, function_name: str, parameters: Sequence[float]) -> None:
        name = str(function_name)
        self._params = [float(x) for x in parameters]
        self._p = _f64(self._params)
        if name not in WF_KINDS:  # weight_function.rs:85-89
            raise ValueError(f'No function implemented with name "{name}"!')
        self._name, self._kind = name, WF_KINDS[name]
        N.check(N.lib().lchd_wf_validate(self._kind, N.dp(self._p), len(self._p)))

    @property
    def parameters(self) -> List[float]:
        return list(self._params)

    @property
    def function_name(self) -> str:
        return self._name

    def integral_vec(self, points: Sequence[float]) -> List[float]:
        x = _f64(points).reshape(-1)
        out = np.empty_like(x)
        N.check(N.lib().lchd_wf_cdf(self._kind, N.dp(self._p), len(self._p), N.dp(x), x.size, N.dp(out)))
        return out.tolist()

    def density_vec(self, points: Sequence[float]) -> List[float]:
        """Additive: the density w = F' of the weight function at every point (0 below 0 and outside a bounded support)."""
        x = _f64(points).reshape(-1)
        out = np.empty_like(x)
        N.check(N.lib().lchd_wf_pdf(self._kind, N.dp(self._p), len(self._p), N.dp(x), x.size, N.dp(out)))
        return out.tolist()

    def cdf_param_grad_vec(self, points: Sequence[float]) -> np.ndarray:
        """Additive: the derivatives of the CDF with respect to the parameters, dF/dtheta_k at every point, as an (n, n_params) array
        with columns in `parameters` order (0 at +inf; finite everywhere: include/loco_hd_hip.h, "weight-function gradients")."""
        x = _f64(points).reshape(-1)
        out = np.empty((x.size, len(self._p)))
        N.check(N.lib().lchd_wf_cdf_grad(self._kind, N.dp(self._p), len(self._p), N.dp(x), x.size, N.dp(out)))
        return out

    def density_point(self, point: float) -> float:
        return self.density_vec([float(point)])[0]

    def integral_point(self, point: float) -> float:
        return self.integral_vec([float(point)])[0]

    def integral_range(self, point_from: float, point_to: float) -> float:
        hi = self.integral_point(point_to)  # weight_function.rs:118-120 evaluates the upper bound first
        return hi - self.integral_point(point_from)

    def _c(self) -> N.WeightFunctionC:
        return N.WeightFunctionC(self._kind, len(self._p), N.dp(self._p))

    def __repr__(self) -> str:
        return f"WeightFunction({self._name!r}, {self._params!r})"


def weight_gradient_width(w_funcs: Sequence[WeightFunction]) -> int:
    """NP of a weight-function gradient over these functions -- the most parameters of any of them -- after the refusals of the call that
    need no device: more than 16 parameters (NotImplementedError), a function whose F(inf) is not 1 (a degenerate dagum: ValueError)."""
    np_max = max(len(w._p) for w in w_funcs)
    if np_max > 16:
        raise NotImplementedError(f"a weight-function gradient takes weight functions of at most 16 parameters (got {np_max})")
    for w in w_funcs:
        if w.integral_point(float("inf")) != 1.0:
            raise ValueError(f"a weight-function gradient needs F(+inf) = 1 whatever the parameters: {w!r} is degenerate")
    return np_max


# Bumped by every PrimitiveAtom SETTER (not by construction): LoCoHD caches the packed form of the lists it is given and a
# cached list is only valid while none of its atoms has been changed (see LoCoHD._packed_lists).  A setter bumps it AFTER it has
# changed the atom, and a pack reads it BEFORE it reads the atoms: a pack that overlaps a setter is then stored under an older stamp.
_ATOM_MUTATIONS = [0]


# Process-wide string tables of PrimitiveAtom: every atom interns its two strings ONCE, when it is constructed or changed, and carries
# the ids (slots _pid / _tid) -- packing a list for a from_primitives call is then a gather of three doubles and two integers per
# atom in native code (_fastpack.pack_atoms), whatever list object the atoms arrive in.  The reference's PyO3 extraction clones
# both Strings of every atom on every call instead (primitive_atom.rs:4-16, src/locohd.rs:479-485).  Ids are never re-used; the
# tables grow with the number of DISTINCT strings the process has seen (residue tags, primitive type names).
# New entries (and the mutation stamp) are written under _INTERN_LOCK: two threads interning new names at once would otherwise
# read the same next id.  A name is entered in _TYPE_NAMES before its id is published in _TYPE_IDS.  (Re-entrant: hashing a str
# subclass runs Python code, which may pack a list while the lock is held.)
_TYPE_IDS: Dict[Any, int] = {}
_TYPE_NAMES: List[Any] = []
_TAG_IDS: Dict[Any, int] = {}
_INTERN_LOCK = threading.RLock()


def _type_id(value) -> int:
    try:
        i = _TYPE_IDS.get(value)
        if i is None:
            with _INTERN_LOCK:
                i = _TYPE_IDS.get(value)
                if i is None:
                    i = len(_TYPE_NAMES)
                    _TYPE_NAMES.append(value)
                    _TYPE_IDS[value] = i
    except TypeError:  # unhashable: no id (the general packing path looks str(value) up)
        return -1
    return i


def _tag_id(value) -> int:
    try:
        i = _TAG_IDS.get(value)
        if i is None:
            with _INTERN_LOCK:
                i = _TAG_IDS.setdefault(value, len(_TAG_IDS))
    except TypeError:
        return -1
    return i


def _bump_mutations() -> None:
    with _INTERN_LOCK:
        _ATOM_MUTATIONS[0] += 1


class PrimitiveAtom:
    """primitive_atom.rs:4-25: a record with get+set attributes."""

    __slots__ = ("_primitive_type", "_tag", "_coordinates", "_pid", "_tid")

    def __init__(self, primitive_type: str, tag: str, coordinates: Sequence[float]) -> None:
        self._primitive_type = primitive_type
        self._tag = tag
        v = [float(x) for x in coordinates]
        if len(v) != 3:
            raise ValueError(f"expected a sequence of length 3 (got {len(v)})")
        self._coordinates = v
        self._pid = _type_id(primitive_type)
        self._tid = _tag_id(tag)

    @property
    def primitive_type(self) -> str:
        return self._primitive_type

    @primitive_type.setter
    def primitive_type(self, value: str) -> None:
        self._primitive_type = value
        self._pid = _type_id(value)
        _bump_mutations()

    @property
    def tag(self) -> str:
        return self._tag

    @tag.setter
    def tag(self, value: str) -> None:
        self._tag = value
        self._tid = _tag_id(value)
        _bump_mutations()

    @property
    def coordinates(self) -> List[float]:
        return list(self._coordinates)

    @coordinates.setter
    def coordinates(self, value: Sequence[float]) -> None:
        v = [float(x) for x in value]
        if len(v) != 3:
            raise ValueError(f"expected a sequence of length 3 (got {len(v)})")
        self._coordinates = v
        _bump_mutations()

    def __getstate__(self):
        return (self._primitive_type, self._tag, self._coordinates)

    def __setstate__(self, state):
        self._primitive_type, self._tag, self._coordinates = state
        self._pid, self._tid = _type_id(self._primitive_type), _tag_id(self._tag)

    def __repr__(self) -> str:
        return f"PrimitiveAtom({self._primitive_type!r}, {self._tag!r}, {self._coordinates!r})"


class TagPairingRule:
    """tag_pairing_rule.rs:5-75.  The dict is tried as {"accept_same"} first, then as
    {"tag_pairs", "accepted_pairs", "ordered"} (derive(FromPyObject) order)."""

    def __init__(self, variant: Dict[str, Any]) -> None:
        if not hasattr(variant, "__getitem__"):
            raise TypeError("TagPairingRule expects a dict")
        if "accept_same" in variant:
            self._mode, self._accept_same = 0, bool(variant["accept_same"])
            self._pairs, self._accepted_pairs, self._ordered = frozenset(), True, True
        elif all(k in variant for k in ("tag_pairs", "accepted_pairs", "ordered")):
            self._mode, self._accept_same = 1, True
            self._pairs = frozenset((str(a), str(b)) for a, b in variant["tag_pairs"])
            self._accepted_pairs, self._ordered = bool(variant["accepted_pairs"]), bool(variant["ordered"])
        else:
            raise TypeError("failed to extract enum TagPairingRuleVariants ('WithoutList | WithList')")

    def pair_accepted(self, pair: Tuple[str, str]) -> bool:
        t0, t1 = pair
        if self._mode == 0:  # :53-61
            accepted = t0 == t1
            return accepted if self._accept_same else not accepted
        accepted = (t0, t1) in self._pairs  # :63-74
        if not self._ordered:
            accepted = accepted or (t1, t0) in self._pairs
        return accepted if self._accepted_pairs else not accepted

    def get_dbg_str(self) -> str:
        if self._mode == 0:
            return f"TagPairingRule {{\n    variant: WithoutList {{\n        accept_same: {str(self._accept_same).lower()},\n    }},\n}}"
        pairs = "".join(f'            (\n                "{a}",\n                "{b}",\n            ),\n' for a, b in sorted(self._pairs))
        return ("TagPairingRule {\n    variant: WithList {\n        tag_pairs: {\n" + pairs + "        },\n"
                f"        accepted_pairs: {str(self._accepted_pairs).lower()},\n        ordered: {str(self._ordered).lower()},\n    }},\n}}")


class StatisticalDistance:
    """statistical_distances.rs:87-142."""

    def __init__(self, distance_name: str, parameters: Sequence[float]) -> None:
        name = str(distance_name)
        self._params = [float(x) for x in parameters]
        if name not in SD_KINDS:  # :112-115
            raise ValueError(f"Invalid statistical distance name {name}!")
        self._name, self._kind = name, SD_KINDS[name]
        N.check(N.lib().lchd_sd_validate(self._kind, len(self._params)))

    def run(self, p1: Sequence[float], p2: Sequence[float]) -> float:
        a, b = _f64(p1).reshape(-1), _f64(p2).reshape(-1)
        n = min(a.size, b.size)  # iter().zip() stops at the shorter one
        prm = np.zeros(2)
        prm[: len(self._params)] = self._params
        out = C.c_double()
        N.check(N.lib().lchd_sd_run(self._kind, N.dp(prm), N.dp(a), N.dp(b), n, C.cast(C.byref(out), N._DP)))
        return out.value

    def __repr__(self) -> str:
        return f"StatisticalDistance({self._name!r}, {self._params!r})"


class _Packed:
    """A structure interned into SoA arrays (xyz [n][3] f64, category i32, tag i32)."""

    __slots__ = ("xyz", "cat", "tag")

    def __init__(self, xyz, cat, tag):
        self.xyz, self.cat, self.tag = xyz, cat, tag


class LoCoHD:
    """src/locohd.rs:42-55, 286-568.

    Same constructor as the reference; ``n_of_threads`` is accepted and ignored (the rayon pool is
    replaced by the GPU).  ``device`` (keyword-only, additive) selects the HIP device; default = current.
    ``devices`` (keyword-only, additive): a list of HIP device ordinals -- the counterpart of the reference's thread pool,
    which is a field of the instance (src/locohd.rs:53,373-383): ``from_primitives`` then spreads the anchor pairs of every
    call over these GPUs inside the C library (lchd_group_from_primitives), results in anchor-pair order as always.
    ``deterministic`` (keyword-only, additive): pin ONE sweep kernel family (lchd_ctx_set_deterministic) -- like the reference's
    single code path (src/locohd.rs:61-226) a pair's score is then bitwise independent of the other pairs of the call and of what
    the instance scored before, at about half the default throughput; the default picks kernels per call (<= 1e-13 apart).
    """

    def __init__(self, categories: Sequence[str], w_func: Union[None, WeightFunction, Dict[str, WeightFunction]] = None,
                 tag_pairing_rule: Optional[TagPairingRule] = None, n_of_threads: Optional[int] = None,
                 category_weights: Optional[Sequence[float]] = None,
                 statistical_distance: Optional[StatisticalDistance] = None, *, device: Optional[int] = None,
                 devices: Optional[Sequence[int]] = None, deterministic: bool = False) -> None:
        names = [str(c) for c in categories]
        cat_map: Dict[str, int] = {}
        for i, nm in enumerate(names):  # :312-316 HashMap collect: a repeated name keeps its last index
            cat_map[nm] = i
        w = np.ones(len(cat_map)) if category_weights is None else _f64(list(category_weights)).reshape(-1)
        N.check(N.lib().lchd_config_validate(len(names), len(cat_map), N.dp(w), w.size))  # :305-346
        if n_of_threads is not None and int(n_of_threads) < 0:
            raise OverflowError("can't convert negative int to unsigned")
        self._categories, self._weights = cat_map, w
        if w_func is None:  # :349-354
            w_func = WeightFunction("uniform", [3.0, 10.0])
        elif not isinstance(w_func, WeightFunction):
            if not isinstance(w_func, dict) or not all(isinstance(v, WeightFunction) for v in w_func.values()):
                raise TypeError("w_func must be None, a WeightFunction or a dict of WeightFunctions")
            w_func = {str(k): v for k, v in w_func.items()}
        self._w_func = w_func
        self._tpr = TagPairingRule({"accept_same": True}) if tag_pairing_rule is None else tag_pairing_rule  # :357-362
        self._sd = StatisticalDistance("Hellinger", [2.0]) if statistical_distance is None else statistical_distance  # :365-370
        if not isinstance(self._tpr, TagPairingRule):
            raise TypeError("tag_pairing_rule must be a TagPairingRule")
        if not isinstance(self._sd, StatisticalDistance):
            raise TypeError("statistical_distance must be a StatisticalDistance")
        self._n_threads = n_of_threads
        self._device = -1 if device is None else int(device)
        self._devices = None if devices is None else [int(d) for d in devices]
        if self._devices is not None and not self._devices:
            raise ValueError("devices must name at least one HIP device")
        if self._devices is not None and device is None:
            self._device = self._devices[0]  # the single-device entry points (from_anchors, from_dmxs, from_coords)
        self._deterministic = bool(deterministic)
        if self._deterministic and self._devices is not None and len(self._devices) > 1:
            raise ValueError("deterministic=True applies to one device (the device group picks kernels per share)")
        self._ctx = None
        self._group = None
        self._handle_lock = threading.Lock()  # the context / device group is created once, whichever threads ask first
        self._cache_lock = threading.Lock()   # _pack_cache is reordered and trimmed by every thread that uses the instance
        self._pack_cache: List[Any] = []   # most recent first: (list, its items, mutation stamp, None, packed, interner)
        self._pid_map = np.empty(0, dtype=np.int32)  # PrimitiveAtom type id -> category index (_type_map)
        self._anchor_cache = None
        self._wf_names = list(self._w_func) if isinstance(self._w_func, dict) else None

    # ---- getters (#[pyo3(get)], :45-52) -------------------------------------------------------------
    @property
    def categories(self) -> Dict[str, int]:
        return dict(self._categories)

    @property
    def category_weights(self) -> List[float]:
        return self._weights.tolist()

    @property
    def w_func(self):
        return self._w_func

    @property
    def tag_pairing_rule(self) -> TagPairingRule:
        return self._tpr

    # ---- plumbing -----------------------------------------------------------------------------------
    # Threads may share an instance: the C library serialises the calls on one context / device group (include/loco_hd_hip.h,
    # "Threads"); for parallel throughput give every thread a LoCoHD of its own.
    def _context(self):
        ctx = self._ctx
        if ctx is None:
            with self._handle_lock:
                if self._ctx is None:
                    h = C.c_void_p()
                    N.check(N.lib().lchd_ctx_create(self._device, C.byref(h)))
                    if self._deterministic:
                        rc = N.lib().lchd_ctx_set_deterministic(h, 1)
                        if rc:
                            N.lib().lchd_ctx_destroy(h)
                            N.check(rc)
                    self._ctx = h  # published once it is fully set up
                ctx = self._ctx
        return ctx

    def _device_group(self):
        grp = self._group
        if grp is None:
            with self._handle_lock:
                if self._group is None:
                    h = C.c_void_p()
                    devs = np.asarray(self._devices, dtype=np.int32)
                    N.check(N.lib().lchd_group_create(N.ip(devs), len(devs), C.byref(h)))
                    self._group = h
                grp = self._group
        return grp

    def last_group_counts(self) -> List[int]:
        """Anchor pairs each device of ``devices`` scored in the most recent from_primitives / from_packed call."""
        if self._group is None:
            return []
        out = np.zeros(len(self._devices), dtype=np.int64)
        N.check(N.lib().lchd_group_last_counts(self._group, N.lp(out)))
        return out.tolist()

    def __del__(self):
        ctx, self._ctx = getattr(self, "_ctx", None), None
        grp, self._group = getattr(self, "_group", None), None
        try:
            if ctx is not None:
                N.lib().lchd_ctx_destroy(ctx)
            if grp is not None:
                N.lib().lchd_group_destroy(grp)
        except Exception:
            pass

    def _cats(self, seq) -> np.ndarray:
        if _fastpack is not None and hasattr(_fastpack, "cats_into"):  # the same loop in native code (Vec<String> extraction)
            out = np.empty(len(seq), dtype=np.int32)
            _fastpack.cats_into(seq, self._categories, out)
            return out
        get = self._categories.get
        return np.fromiter((get(str(s), -1) for s in seq), dtype=np.int32, count=len(seq))

    def _config(self, interner: Optional[Dict[str, int]] = None):
        """Build the lchd_config; returns (struct, keep-alive list)."""
        keep: List[Any] = []
        cfg = N.ConfigC()
        cfg.n_categories = len(self._weights)
        cfg.category_weights = N.dp(self._weights)
        wfs = list(self._w_func.values()) if isinstance(self._w_func, dict) else [self._w_func]
        arr = (N.WeightFunctionC * len(wfs))(*[w._c() for w in wfs])
        keep += [arr, wfs]
        cfg.n_weight_functions = len(wfs)
        cfg.weight_functions = arr
        cfg.sd_kind = self._sd._kind
        cfg.sd_n_params = len(self._sd._params)
        for i, v in enumerate(self._sd._params[:2]):
            cfg.sd_params[i] = v
        t = self._tpr
        cfg.tag_mode, cfg.tag_accept_same = t._mode, int(t._accept_same)
        cfg.tag_accepted_pairs, cfg.tag_ordered = int(t._accepted_pairs), int(t._ordered)
        interner = {} if interner is None else interner
        if interner is _TAG_IDS:  # the process-wide table: ids are handed out under its lock
            intern = _tag_id
        else:
            def intern(s):
                return interner.setdefault(s, len(interner))
        pairs = np.asarray([[intern(a), intern(b)] for a, b in sorted(t._pairs)], dtype=np.int32).reshape(-1, 2)
        keep.append(pairs)
        cfg.tag_pairs = N.ip(pairs) if len(pairs) else None
        cfg.n_tag_pairs = len(pairs)
        return cfg, keep

    def _wf_indices(self, keys: Optional[Sequence[str]], target_len: int) -> Optional[np.ndarray]:
        """keys_to_weight_functions, src/locohd.rs:230-283.  None => every pair uses weight function 0."""
        multiple = isinstance(self._w_func, dict)
        if multiple and keys is not None:
            if len(keys) != target_len:
                raise ValueError(f"The w_func_keys vector has an invalid length ({len(keys)} instead of {target_len})!")
            pos = {k: i for i, k in enumerate(self._wf_names)}
            bad = sum(1 for k in keys if k not in pos)
            if bad:
                raise ValueError(f"The vector contains {bad} out of {len(keys)} invalid weight function keys!")
            return np.fromiter((pos[k] for k in keys), dtype=np.int32, count=len(keys))
        if not multiple and keys is None:
            return None
        raise ValueError("Invalid pairing for the LoCoHD instance's w_func option and the method's w_func_keys parameter!")

    # ---- the four drivers -----------------------------------------------------------------------------
    def from_anchors(self, seq_a, seq_b, dists_a, dists_b, w_func_key: Optional[str] = None) -> float:
        """src/locohd.rs:392-406."""
        idx = self._wf_indices(None if w_func_key is None else [str(w_func_key)], 1)
        ca, cb = self._cats(list(seq_a)), self._cats(list(seq_b))
        da, db = _f64(dists_a).reshape(-1), _f64(dists_b).reshape(-1)
        cfg, keep = self._config()
        out = C.c_double()
        N.check(N.lib().lchd_from_anchors(self._context(), C.byref(cfg), N.ip(ca), ca.size, N.dp(da), da.size, N.ip(cb),
                                          cb.size, N.dp(db), db.size, 0 if idx is None else int(idx[0]),
                                          C.cast(C.byref(out), N._DP)))
        return out.value

    def from_dmxs(self, seq_a, seq_b, dmx_a, dmx_b, w_func_keys: Optional[Sequence[str]] = None) -> List[float]:
        """src/locohd.rs:410-458."""
        (ma, la), (mb, lb) = self._matrix(dmx_a), self._matrix(dmx_b)
        if ma.shape[0] != mb.shape[0]:  # :420-428
            raise ValueError(f"Expected matrices with the same length, got lengths {ma.shape[0]} and {mb.shape[0]}!")
        idx = self._wf_indices(None if w_func_keys is None else [str(k) for k in w_func_keys], ma.shape[0])
        ca, cb = self._cats(list(seq_a)), self._cats(list(seq_b))
        cfg, keep = self._config()
        out = np.empty(ma.shape[0])
        if ma.shape[0] == 0:
            return []
        if la is None and lb is None:
            N.check(N.lib().lchd_from_dmxs(self._context(), C.byref(cfg), N.ip(ca), ca.size, N.ip(cb), cb.size, N.dp(ma),
                                           ma.shape[0], ma.shape[1], N.dp(mb), mb.shape[0], mb.shape[1], N.ip(idx), N.dp(out)))
        else:  # ragged rows: every row with its own length (what lies beyond a row is never looked at, as in the reference)
            la = np.full(ma.shape[0], ma.shape[1], dtype=np.int32) if la is None else la
            lb = np.full(mb.shape[0], mb.shape[1], dtype=np.int32) if lb is None else lb
            N.check(N.lib().lchd_from_dmxs_ragged(self._context(), C.byref(cfg), N.ip(ca), ca.size, N.ip(cb), cb.size, N.dp(ma),
                                                  ma.shape[0], ma.shape[1], N.ip(la), N.dp(mb), mb.shape[0], mb.shape[1], N.ip(lb),
                                                  N.ip(idx), N.dp(out)))
        return out.tolist()

    def from_coords(self, seq_a, seq_b, coords_a, coords_b, w_func_keys: Optional[Sequence[str]] = None, *, box_a=None, box_b=None,
                    cell_a=None, cell_b=None) -> List[float]:
        """src/locohd.rs:463-476.

        ``box_a`` / ``box_b`` / ``cell_a`` / ``cell_b`` (keyword-only, additive): an orthorhombic periodic box (Lx, Ly, Lz) or a triclinic
        cell (3 x 3, rows = lattice vectors, any non-singular one) of the structure.  A dense row then follows the MINIMUM-IMAGE
        convention: every atom appears exactly once, at the distance of its nearest periodic image (coordinates need not be wrapped).
        This differs from ``from_primitives(..., box_a=...)``, where an atom beyond half an edge may enter through two images.  A side
        takes a box or a cell, not both; the two sides are independent."""
        periodic = box_a is not None or box_b is not None or cell_a is not None or cell_b is not None
        if periodic:
            for side, box, cell in (("a", box_a, cell_a), ("b", box_b, cell_b)):
                if box is not None and cell is not None:
                    raise ValueError(f"box_{side} and cell_{side} were both given: a structure has one periodic box or one periodic cell")
            self._no_device_group_with_box()
            pc_a = dense_cells(box_a, cell_a, 1, "box_a", "cell_a")
            pc_b = dense_cells(box_b, cell_b, 1, "box_b", "cell_b")
        xa, xb = self._coords(coords_a), self._coords(coords_b)
        if len(xa) != len(xb):
            raise ValueError(f"Expected matrices with the same length, got lengths {len(xa)} and {len(xb)}!")
        idx = self._wf_indices(None if w_func_keys is None else [str(k) for k in w_func_keys], len(xa))
        ca, cb = self._cats(list(seq_a)), self._cats(list(seq_b))
        cfg, keep = self._config()
        out = np.empty(len(xa))
        if len(xa) == 0:
            return []
        if periodic:
            N.check(N.lib().lchd_from_coords_periodic(self._context(), C.byref(cfg), N.ip(ca), ca.size, N.ip(cb), cb.size, N.dp(xa), len(xa),
                                                      N.dp(xb), len(xb), N.ip(idx), N.dp(pc_a), N.dp(pc_b), N.dp(out)))
            return out.tolist()
        N.check(N.lib().lchd_from_coords(self._context(), C.byref(cfg), N.ip(ca), ca.size, N.ip(cb), cb.size, N.dp(xa), len(xa),
                                         N.dp(xb), len(xb), N.ip(idx), N.dp(out)))
        return out.tolist()

    # ---- dense ensembles (additive) ----------------------------------------------------------------------
    def from_coords_ensemble(self, seq, coords, structure_pairs=None, w_func_keys: Optional[Sequence[str]] = None,
                             excluded_pairs=None, *, boxes=None, cells=None) -> np.ndarray:
        """Additive: `from_coords(seq, seq, coords[i], coords[j])` for every structure pair (i, j) of M structures of one
        topology, in one call -- python_codes/ensembles/compare_ensembles.py:277-296, where each structure's dense rows are
        sorted once.  `coords`: (M, n, 3) or a list of (n, 3); `structure_pairs`: (i, j) pairs, default every i < j (i outer);
        `excluded_pairs`: (r, c) atom-index pairs whose distance counts as +inf in every structure (directional: give both
        orders, as the script's homo-residue ban does).  Returns a float64 array (P, n).

        ``boxes`` / ``cells`` (keyword-only, additive): one orthorhombic box (Lx, Ly, Lz) or one triclinic cell (3 x 3) for all
        structures, or one per structure (NPT); the rows then follow the minimum-image convention of ``from_coords(..., box_a=...)``."""
        if boxes is not None and cells is not None:
            raise ValueError("boxes and cells were both given: a batch is periodic in boxes or in cells")
        if boxes is not None or cells is not None:
            self._no_device_group_with_box()
        xs = [self._coords(x) for x in coords]
        n = len(xs[0]) if xs else 0
        for x in xs[1:]:
            if len(x) != n:
                raise ValueError(f"Expected matrices with the same length, got lengths {n} and {len(x)}!")
        xyz = np.ascontiguousarray(np.stack(xs) if xs else np.zeros((0, 0, 3)), dtype=np.float64)
        pairs = self._structure_pairs(structure_pairs, len(xs))
        idx = self._wf_indices(None if w_func_keys is None else [str(k) for k in w_func_keys], n)
        cs = self._cats(list(seq))
        if len(cs) < n:
            raise N.PanicException("index out of bounds: a distance row is longer than its seq")
        xstart, xidx = self._exclusion_csr(excluded_pairs, n)
        cfg, keep = self._config()
        p = len(pairs) if pairs is not None else len(xs) * (len(xs) - 1) // 2
        out = np.empty((p, n))
        pc = dense_cells(boxes, cells, len(xs), "boxes", "cells")
        if pc is not None:
            N.check(N.lib().lchd_ensemble_from_coords_periodic(self._context(), C.byref(cfg), N.ip(cs), n, N.dp(xyz), len(xs),
                                                               N.ip(pairs), p, N.ip(xstart), N.ip(xidx), N.ip(idx), N.dp(pc), len(pc), N.dp(out)))
            return out
        N.check(N.lib().lchd_ensemble_from_coords(self._context(), C.byref(cfg), N.ip(cs), n, N.dp(xyz), len(xs),
                                                  N.ip(pairs), p, N.ip(xstart), N.ip(xidx), N.ip(idx), N.dp(out)))
        return out

    def from_dmxs_ensemble(self, seq, dmxs, structure_pairs=None, w_func_keys: Optional[Sequence[str]] = None) -> np.ndarray:
        """Additive: `from_dmxs(seq, seq, dmxs[i], dmxs[j])` for every structure pair (i, j), in one call (the exact call of
        python_codes/ensembles/compare_ensembles.py:277-296).  `dmxs`: (M, n, n) square matrices, +inf allowed.  Returns a
        float64 array (P, n)."""
        ms = [self._matrix(m)[0] for m in dmxs]
        n = ms[0].shape[0] if ms else 0
        for m in ms:
            if m.shape[0] != n:
                raise ValueError(f"Expected matrices with the same length, got lengths {n} and {m.shape[0]}!")
            if m.shape[1] != m.shape[0]:
                raise ValueError(f"from_dmxs_ensemble takes square distance matrices, got {m.shape[0]} x {m.shape[1]}")
        dmx = np.ascontiguousarray(np.stack(ms) if ms else np.zeros((0, 0, 0)), dtype=np.float64)
        pairs = self._structure_pairs(structure_pairs, len(ms))
        idx = self._wf_indices(None if w_func_keys is None else [str(k) for k in w_func_keys], n)
        cs = self._cats(list(seq))
        if len(cs) < n:
            raise N.PanicException("index out of bounds: a distance row is longer than its seq")
        cfg, keep = self._config()
        p = len(pairs) if pairs is not None else len(ms) * (len(ms) - 1) // 2
        out = np.empty((p, n))
        N.check(N.lib().lchd_ensemble_from_dmxs(self._context(), C.byref(cfg), N.ip(cs), n, N.dp(dmx), len(ms), N.ip(pairs), p,
                                                N.ip(idx), N.dp(out)))
        return out

    @staticmethod
    def _structure_pairs(structure_pairs, m: int) -> Optional[np.ndarray]:
        if structure_pairs is None:
            return None
        pairs = np.ascontiguousarray(np.asarray(list(structure_pairs), dtype=np.int64).reshape(-1, 2))
        if len(pairs) and (pairs.min() < 0 or pairs.max() >= m):
            raise ValueError(f"a structure pair refers to a structure outside [0, {m})")
        return pairs.astype(np.int32)

    @staticmethod
    def _exclusion_csr(excluded_pairs, n: int) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
        """(r, c) pairs -> CSR (row starts [n + 1], columns) of the excluded entries, or (None, None)."""
        if excluded_pairs is None:
            return None, None
        ex = np.asarray(list(excluded_pairs), dtype=np.int64).reshape(-1, 2)
        if len(ex) and (ex.min() < 0 or ex.max() >= n):
            raise ValueError(f"an excluded pair refers to an atom outside [0, {n})")
        ex = ex[np.lexsort((ex[:, 1], ex[:, 0]))]
        start = np.zeros(n + 1, dtype=np.int32)
        np.cumsum(np.bincount(ex[:, 0], minlength=n), out=start[1:])
        return start, np.ascontiguousarray(ex[:, 1], dtype=np.int32)

    def from_primitives(self, prim_a: Sequence[PrimitiveAtom], prim_b: Sequence[PrimitiveAtom], anchor_pairs,
                        threshold_distance: float, *, box_a=None, box_b=None, cell_a=None, cell_b=None) -> List[float]:
        """src/locohd.rs:479-567.

        ``box_a`` / ``box_b`` (keyword-only, additive): an orthorhombic periodic box (Lx, Ly, Lz) of the structure.  Its environments
        then hold every periodic image of every atom closer than ``threshold_distance`` (<= the smallest edge) to the anchor: the
        minimum-image convention up to half an edge, beyond it an atom may enter through two images.

        ``cell_a`` / ``cell_b`` (keyword-only, additive): a triclinic periodic cell instead, a 3 x 3 matrix whose rows are the lattice
        vectors (``cell_from_lengths_angles`` makes one from a CRYST1 record); ``threshold_distance`` <= the smallest perpendicular
        width.  A side takes a box or a cell, not both; the two sides are independent."""
        if box_a is not None or box_b is not None or cell_a is not None or cell_b is not None:
            return self._from_primitives_periodic(prim_a, prim_b, anchor_pairs, threshold_distance, box_a, box_b, cell_a, cell_b)
        pairs, idx = self._anchor_arrays(anchor_pairs)
        pa, pb, interner = self._packed_lists(prim_a, prim_b)
        return self.from_packed(pa, pb, pairs, threshold_distance, wf_index=idx, interner=interner).tolist()

    # ---- local composition profiles (additive) -----------------------------------------------------------
    # P[a][c] = sum_k (F(d_{k+1}) - F(d_k)) * w_c n_c(k) / sum_c' w_c' n_c'(k) over the sorted environment of anchor a: the
    # weight-function-averaged local composition a score is the distance of (include/loco_hd_hip.h, "local composition profiles").
    # Columns follow `categories`; a row sums to F(inf) - F(0).  The environment is the one the scoring call of the same name builds.
    def _no_device_group_for_composition(self) -> None:
        if self._devices is not None:
            raise ValueError("a composition profile applies to one device (a device group has no profile call): drop devices=[...]")

    def composition_from_primitives(self, prims: Sequence[PrimitiveAtom], anchors, threshold_distance: float,
                                    w_func_keys: Optional[Sequence[str]] = None, *, box=None, cell=None) -> np.ndarray:
        """Additive: the composition profile of the environment `from_primitives` would build around every anchor (an index into
        `prims`; repeats allowed), as a float64 array (len(anchors), C).  `w_func_keys`: one key per anchor for a weight-function
        dictionary (the pairing rules of the scoring calls).  `box` / `cell` (keyword-only): the structure's periodic box (Lx, Ly, Lz)
        or triclinic cell (3 x 3), as `from_primitives(..., box_a=...)` / `cell_a=...` take them."""
        if box is not None and cell is not None:
            raise ValueError("box and cell were both given: a structure has one periodic box or one periodic cell")
        self._no_device_group_for_composition()
        thr = float(threshold_distance)
        bx = None if box is None else periodic_boxes(box, 1, thr, "box")
        cl = None if cell is None else periodic_cells(cell, 1, thr, "cell")
        idx_list = [int(a) for a in anchors]
        if any(a < 0 for a in idx_list):
            raise OverflowError("can't convert negative int to unsigned")
        anc = np.asarray(idx_list, dtype=np.int64).reshape(-1)
        idx = self._wf_indices(None if w_func_keys is None else [str(k) for k in w_func_keys], len(anc))
        pk, _, interner = self._packed_lists(prims, prims)
        cfg, keep = self._config(interner)
        out = np.empty((len(anc), len(self._weights)))
        if len(anc) == 0:
            return out
        xyz = _f64(pk.xyz).reshape(-1, 3)
        if len(anc) and anc.max() >= len(xyz):
            raise N.PanicException("index out of bounds: an anchor index is outside its structure (src/locohd.rs:521)")
        N.check(N.lib().lchd_composition_primitives_periodic(self._context(), C.byref(cfg), N.dp(xyz), N.ip(pk.cat), N.ip(pk.tag), len(xyz),
                                                             N.lp(anc), N.ip(idx), len(anc), thr, N.dp(bx), N.dp(cl), N.dp(out)))
        return out

    def composition_from_coords(self, seq, coords, w_func_keys: Optional[Sequence[str]] = None, *, box=None, cell=None) -> np.ndarray:
        """Additive: the composition profile of every dense row `from_coords` would build (row r: the whole structure seen from atom r),
        as a float64 array (n, C).  `box` / `cell` (keyword-only): minimum-image rows, as `from_coords(..., box_a=...)`."""
        if box is not None and cell is not None:
            raise ValueError("box and cell were both given: a structure has one periodic box or one periodic cell")
        self._no_device_group_for_composition()
        pc = dense_cells(box, cell, 1, "box", "cell")
        x = self._coords(coords)
        idx = self._wf_indices(None if w_func_keys is None else [str(k) for k in w_func_keys], len(x))
        cs = self._cats(list(seq))
        cfg, keep = self._config()
        out = np.empty((len(x), len(self._weights)))
        if len(x) == 0:
            return out
        N.check(N.lib().lchd_composition_coords(self._context(), C.byref(cfg), N.ip(cs), cs.size, N.dp(x), len(x), N.ip(idx), N.dp(pc), N.dp(out)))
        return out

    def composition_from_dmx(self, seq, dmx, w_func_keys: Optional[Sequence[str]] = None) -> np.ndarray:
        """Additive: the composition profile of every given distance row (`from_dmxs` semantics: row r sorted together with `seq`, +inf
        entries allowed, every row holds a 0), as a float64 array (rows, C)."""
        self._no_device_group_for_composition()
        m, lens = self._matrix(dmx)
        if lens is not None:
            raise ValueError("composition_from_dmx takes a rectangular distance matrix (rows of equal length)")
        idx = self._wf_indices(None if w_func_keys is None else [str(k) for k in w_func_keys], m.shape[0])
        cs = self._cats(list(seq))
        cfg, keep = self._config()
        out = np.empty((m.shape[0], len(self._weights)))
        if m.shape[0] == 0:
            return out
        N.check(N.lib().lchd_composition_dmx(self._context(), C.byref(cfg), N.ip(cs), cs.size, N.dp(m), m.shape[0], m.shape[1], N.ip(idx), N.dp(out)))
        return out

    # ---- radial score profiles (additive) ----------------------------------------------------------------
    # R[p][k] = sum_j H_j * |[F(u_j), F(u_{j+1})] n [F(e_k), F(e_{k+1})]| over the merged breakpoints u_j of pair p: the integrand of the
    # pair's score resolved over the distance bins `edges` (include/loco_hd_hip.h, "radial score profiles").  With edges[0] = 0 and
    # edges[-1] = inf a row sums to the pair's score.
    @staticmethod
    def _radial_edges(edges) -> np.ndarray:
        """The edges as a float64 array, checked on the host (lchd_radial_validate: ValueError before any device is touched)."""
        ed = np.ascontiguousarray(np.asarray(list(edges) if not isinstance(edges, np.ndarray) else edges, dtype=np.float64).reshape(-1))
        N.check(N.lib().lchd_radial_validate(N.dp(ed), len(ed)))
        return ed

    def _no_device_group_for_pair_rows(self, ed) -> None:
        if ed is _CATEGORY_GRADIENT:  # (and what else its kernel does not take, before any device is touched)
            if self._devices is not None:
                raise NotImplementedError("a category-weight gradient applies to one device (a device group has no such call): drop devices=[...]")
            if self._sd._name not in ("Hellinger", "Kullback-Leibler"):
                raise NotImplementedError("a category-weight gradient is implemented for the Hellinger and Kullback-Leibler distances; not for "
                                          f"the {self._sd._name} distance")
            if len(self._weights) > 64:
                raise NotImplementedError(f"a category-weight gradient takes at most 64 categories (got {len(self._weights)})")
            return
        if self._devices is not None:
            what, call = ("an attribution", "attribution") if ed is None else ("a radial profile", "radial")
            raise ValueError(f"{what} applies to one device (a device group has no {call} call): drop devices=[...]")

    def _pair_rows_width(self, ed) -> int:
        return len(self._weights) if ed is None or ed is _CATEGORY_GRADIENT else len(ed) - 1

    # The three radial methods, the three attribution methods and the three category-gradient methods differ in the kernel their pass
    # ends in and in the row it writes: `ed` is the checked edge array of a radial call (rows of len(ed) - 1 bins), None for an
    # attribution or _CATEGORY_GRADIENT for a category-weight gradient (rows of C categories).
    def _pair_rows_from_primitives(self, ed, prim_a, prim_b, anchor_pairs, threshold_distance, box_a, box_b, cell_a, cell_b) -> np.ndarray:
        for side, box, cell in (("a", box_a, cell_a), ("b", box_b, cell_b)):
            if box is not None and cell is not None:
                raise ValueError(f"box_{side} and cell_{side} were both given: a structure has one periodic box or one periodic cell")
        self._no_device_group_for_pair_rows(ed)
        thr = float(threshold_distance)
        ba = None if box_a is None else periodic_boxes(box_a, 1, thr, "box_a")
        bb = None if box_b is None else periodic_boxes(box_b, 1, thr, "box_b")
        ca = None if cell_a is None else periodic_cells(cell_a, 1, thr, "cell_a")
        cb = None if cell_b is None else periodic_cells(cell_b, 1, thr, "cell_b")
        pairs, idx = self._anchor_arrays(anchor_pairs)
        pa, pb, interner = self._packed_lists(prim_a, prim_b)
        anchors = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        cfg, keep = self._config(interner)
        out = np.empty((len(anchors), self._pair_rows_width(ed)))
        if len(anchors) == 0:
            return out
        xa, xb = _f64(pa.xyz).reshape(-1, 3), _f64(pb.xyz).reshape(-1, 3)
        head = (self._context(), C.byref(cfg), N.dp(xa), N.ip(pa.cat), N.ip(pa.tag), len(xa), N.dp(xb), N.ip(pb.cat), N.ip(pb.tag), len(xb),
                N.lp(anchors), N.ip(idx), len(anchors), thr, N.dp(ba), N.dp(ca), N.dp(bb), N.dp(cb))
        if ed is _CATEGORY_GRADIENT:
            N.check(N.lib().lchd_category_gradient_primitives(*head, N.dp(out)))
        elif ed is None:
            N.check(N.lib().lchd_attribution_primitives(*head, N.dp(out)))
        else:
            N.check(N.lib().lchd_radial_primitives(*head, N.dp(ed), len(ed), N.dp(out)))
        return out

    def _pair_rows_from_coords(self, ed, seq_a, seq_b, coords_a, coords_b, w_func_keys, box_a, box_b, cell_a, cell_b) -> np.ndarray:
        for side, box, cell in (("a", box_a, cell_a), ("b", box_b, cell_b)):
            if box is not None and cell is not None:
                raise ValueError(f"box_{side} and cell_{side} were both given: a structure has one periodic box or one periodic cell")
        self._no_device_group_for_pair_rows(ed)
        pc_a = dense_cells(box_a, cell_a, 1, "box_a", "cell_a")
        pc_b = dense_cells(box_b, cell_b, 1, "box_b", "cell_b")
        xa, xb = self._coords(coords_a), self._coords(coords_b)
        if len(xa) != len(xb):
            raise ValueError(f"Expected matrices with the same length, got lengths {len(xa)} and {len(xb)}!")
        idx = self._wf_indices(None if w_func_keys is None else [str(k) for k in w_func_keys], len(xa))
        ca, cb = self._cats(list(seq_a)), self._cats(list(seq_b))
        cfg, keep = self._config()
        out = np.empty((len(xa), self._pair_rows_width(ed)))
        if len(xa) == 0:
            return out
        head = (self._context(), C.byref(cfg), N.ip(ca), ca.size, N.ip(cb), cb.size, N.dp(xa), len(xa), N.dp(xb), len(xb), N.ip(idx), N.dp(pc_a),
                N.dp(pc_b))
        if ed is _CATEGORY_GRADIENT:
            N.check(N.lib().lchd_category_gradient_coords(*head, N.dp(out)))
        elif ed is None:
            N.check(N.lib().lchd_attribution_coords(*head, N.dp(out)))
        else:
            N.check(N.lib().lchd_radial_coords(*head, N.dp(ed), len(ed), N.dp(out)))
        return out

    def _pair_rows_from_dmxs(self, ed, seq_a, seq_b, dmx_a, dmx_b, w_func_keys) -> np.ndarray:
        self._no_device_group_for_pair_rows(ed)
        (ma, la), (mb, lb) = self._matrix(dmx_a), self._matrix(dmx_b)
        if la is not None or lb is not None:
            name = "category_gradient_from_dmxs" if ed is _CATEGORY_GRADIENT else "attribution_from_dmxs" if ed is None else "radial_from_dmxs"
            raise ValueError(f"{name} takes rectangular distance matrices (rows of equal length)")
        if ma.shape[0] != mb.shape[0]:
            raise ValueError(f"Expected matrices with the same length, got lengths {ma.shape[0]} and {mb.shape[0]}!")
        idx = self._wf_indices(None if w_func_keys is None else [str(k) for k in w_func_keys], ma.shape[0])
        ca, cb = self._cats(list(seq_a)), self._cats(list(seq_b))
        cfg, keep = self._config()
        out = np.empty((ma.shape[0], self._pair_rows_width(ed)))
        if ma.shape[0] == 0:
            return out
        head = (self._context(), C.byref(cfg), N.ip(ca), ca.size, N.ip(cb), cb.size, N.dp(ma), N.dp(mb), ma.shape[0], ma.shape[1], mb.shape[1],
                N.ip(idx))
        if ed is _CATEGORY_GRADIENT:
            N.check(N.lib().lchd_category_gradient_dmxs(*head, N.dp(out)))
        elif ed is None:
            N.check(N.lib().lchd_attribution_dmxs(*head, N.dp(out)))
        else:
            N.check(N.lib().lchd_radial_dmxs(*head, N.dp(ed), len(ed), N.dp(out)))
        return out

    def radial_from_primitives(self, prim_a: Sequence[PrimitiveAtom], prim_b: Sequence[PrimitiveAtom], anchor_pairs,
                               threshold_distance: float, edges, *, box_a=None, box_b=None, cell_a=None, cell_b=None) -> np.ndarray:
        """Additive: the radial profile of every anchor pair `from_primitives` would score, as a float64 array (P, K) for K + 1
        `edges` (ascending distances, the first >= 0, the last may be inf; at most 64 bins).  Bin k holds the part of the pair's score
        that the distances between edges[k] and edges[k + 1] contribute; with edges[0] = 0 and edges[-1] = inf a row sums to the score.
        `anchor_pairs`, `box_a` / `box_b` / `cell_a` / `cell_b`: as `from_primitives` takes them."""
        return self._pair_rows_from_primitives(self._radial_edges(edges), prim_a, prim_b, anchor_pairs, threshold_distance, box_a, box_b, cell_a,
                                               cell_b)

    def radial_from_coords(self, seq_a, seq_b, coords_a, coords_b, edges, w_func_keys: Optional[Sequence[str]] = None, *, box_a=None,
                           box_b=None, cell_a=None, cell_b=None) -> np.ndarray:
        """Additive: the radial profile of every dense row pair `from_coords` would score (pair r: the two structures seen from their
        atoms r), as a float64 array (n, K).  `box_a` / `box_b` / `cell_a` / `cell_b` (keyword-only): minimum-image rows, as
        `from_coords(..., box_a=...)`."""
        return self._pair_rows_from_coords(self._radial_edges(edges), seq_a, seq_b, coords_a, coords_b, w_func_keys, box_a, box_b, cell_a, cell_b)

    def radial_from_dmxs(self, seq_a, seq_b, dmx_a, dmx_b, edges, w_func_keys: Optional[Sequence[str]] = None) -> np.ndarray:
        """Additive: the radial profile of every row pair `from_dmxs` would score (rectangular matrices with the same number of rows,
        +inf entries allowed, every row holds a 0), as a float64 array (rows, K)."""
        return self._pair_rows_from_dmxs(self._radial_edges(edges), seq_a, seq_b, dmx_a, dmx_b, w_func_keys)

    # ---- score attribution by category (additive) ----------------------------------------------------------
    # A[p][c] = sum_j (F(u_{j+1}) - F(u_j)) * H_j * t_{c,j} / T_j with t_c = |a_c^(1/e) - b_c^(1/e)|^e, T = sum_c t_c, H = (T / 2)^(1/e): the
    # part of pair p's score that category c carries (include/loco_hd_hip.h, "score attribution by category").  Columns follow
    # `categories`; a row sums to the pair's score.  Hellinger distances only (NotImplementedError otherwise), at most 64 categories.
    def attribution_from_primitives(self, prim_a: Sequence[PrimitiveAtom], prim_b: Sequence[PrimitiveAtom], anchor_pairs,
                                    threshold_distance: float, *, box_a=None, box_b=None, cell_a=None, cell_b=None) -> np.ndarray:
        """Additive: the score of every anchor pair `from_primitives` would score, split over the categories, as a float64 array
        (P, C) with columns in `categories` order; a row sums to the pair's score.  `anchor_pairs`, `box_a` / `box_b` / `cell_a` /
        `cell_b`: as `from_primitives` takes them."""
        return self._pair_rows_from_primitives(None, prim_a, prim_b, anchor_pairs, threshold_distance, box_a, box_b, cell_a, cell_b)

    def attribution_from_coords(self, seq_a, seq_b, coords_a, coords_b, w_func_keys: Optional[Sequence[str]] = None, *, box_a=None,
                                box_b=None, cell_a=None, cell_b=None) -> np.ndarray:
        """Additive: the score of every dense row pair `from_coords` would score, split over the categories, as a float64 array
        (n, C).  `box_a` / `box_b` / `cell_a` / `cell_b` (keyword-only): minimum-image rows, as `from_coords(..., box_a=...)`."""
        return self._pair_rows_from_coords(None, seq_a, seq_b, coords_a, coords_b, w_func_keys, box_a, box_b, cell_a, cell_b)

    def attribution_from_dmxs(self, seq_a, seq_b, dmx_a, dmx_b, w_func_keys: Optional[Sequence[str]] = None) -> np.ndarray:
        """Additive: the score of every row pair `from_dmxs` would score, split over the categories, as a float64 array (rows, C)."""
        return self._pair_rows_from_dmxs(None, seq_a, seq_b, dmx_a, dmx_b, w_func_keys)

    # ---- category-weight gradients (additive) -------------------------------------------------------------
    # G[p][c] = dS_p / dw_c, the derivative of pair p's score with respect to `category_weights` (include/loco_hd_hip.h, "category-weight
    # gradients"): with p_c = w_c n_c / sum_k w_k n_k per side, w_c dD/dw_c = x_c + y_c - p_c sum_k x_k - q_c sum_k y_k, integrated over
    # the pieces of the pair as the score is.  Columns follow `categories`; sum_c w_c G[p][c] = 0.  Hellinger and Kullback-Leibler
    # distances (NotImplementedError otherwise), at most 64 categories, no device groups.
    def category_gradient_from_primitives(self, prim_a: Sequence[PrimitiveAtom], prim_b: Sequence[PrimitiveAtom], anchor_pairs,
                                          threshold_distance: float, *, box_a=None, box_b=None, cell_a=None, cell_b=None) -> np.ndarray:
        """Additive: the derivative of the score of every anchor pair `from_primitives` would score with respect to every category
        weight, as a float64 array (P, C) with columns in `categories` order.  `anchor_pairs`, `box_a` / `box_b` / `cell_a` / `cell_b`: as
        `attribution_from_primitives` takes them."""
        return self._pair_rows_from_primitives(_CATEGORY_GRADIENT, prim_a, prim_b, anchor_pairs, threshold_distance, box_a, box_b, cell_a, cell_b)

    def category_gradient_from_coords(self, seq_a, seq_b, coords_a, coords_b, w_func_keys: Optional[Sequence[str]] = None, *, box_a=None,
                                      box_b=None, cell_a=None, cell_b=None) -> np.ndarray:
        """Additive: the derivative of the score of every dense row pair `from_coords` would score with respect to every category
        weight, as a float64 array (n, C).  `box_a` / `box_b` / `cell_a` / `cell_b` (keyword-only): minimum-image rows."""
        return self._pair_rows_from_coords(_CATEGORY_GRADIENT, seq_a, seq_b, coords_a, coords_b, w_func_keys, box_a, box_b, cell_a, cell_b)

    def category_gradient_from_dmxs(self, seq_a, seq_b, dmx_a, dmx_b, w_func_keys: Optional[Sequence[str]] = None) -> np.ndarray:
        """Additive: the derivative of the score of every row pair `from_dmxs` would score with respect to every category weight, as a
        float64 array (rows, C)."""
        return self._pair_rows_from_dmxs(_CATEGORY_GRADIENT, seq_a, seq_b, dmx_a, dmx_b, w_func_keys)

    # ---- weight-function gradients (additive) ---------------------------------------------------------------
    # grad[p][k] = dS_p / dtheta_k, the derivative of pair p's score with respect to parameter k of the pair's weight function
    # (include/loco_hd_hip.h, "weight-function gradients"): sum over the members of G_k(d) (H- - H+) minus G_k(0) H_first with
    # G_k = dF/dtheta_k (WeightFunction.cdf_param_grad_vec).  Every statistical distance; open structures, one device.
    def _weight_gradient_width(self, what: str, boxes=()) -> int:
        """NP, the columns of a weight-gradient row, after every refusal that needs no device."""
        if any(b is not None for b in boxes):
            raise NotImplementedError(f"{what} takes open structures: periodic boxes and cells are not supported")
        if self._devices is not None:
            raise NotImplementedError("a weight-function gradient applies to one device (a device group has no such call): drop devices=[...]")
        if len(self._weights) > 64:
            raise NotImplementedError(f"a weight-function gradient takes at most 64 categories (got {len(self._weights)})")
        return weight_gradient_width(list(self._w_func.values()) if isinstance(self._w_func, dict) else [self._w_func])

    def weight_gradient_from_primitives(self, prim_a: Sequence[PrimitiveAtom], prim_b: Sequence[PrimitiveAtom], anchor_pairs,
                                        threshold_distance: float, *, box_a=None, box_b=None, cell_a=None, cell_b=None) -> WeightGradient:
        """Additive: for every anchor pair `from_primitives` would score, the derivative of its score with respect to every parameter of
        its weight function.  Returns `WeightGradient(scores (P,), grad (P, NP))` of float64 arrays: NP is the most parameters of any
        function of `w_func`, row p holds the derivatives in the `parameters` order of pair p's function, and the columns behind its
        parameter count are exact zeros.  This is the exact derivative of the score as computed (no threshold caveat), one-sided only
        for a member exactly on a support bound of uniform / kumaraswamy.  At most 16 parameters (NotImplementedError); a dagum with
        F(inf) != 1 is a ValueError; periodic boxes and cells and device groups are not supported (NotImplementedError)."""
        np_max = self._weight_gradient_width("weight_gradient_from_primitives", (box_a, box_b, cell_a, cell_b))
        thr = float(threshold_distance)
        pairs, idx = self._anchor_arrays(anchor_pairs)
        pa, pb, interner = self._packed_lists(prim_a, prim_b)
        anchors = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        cfg, keep = self._config(interner)
        n = len(anchors)
        out = np.empty(n * (1 + np_max))
        if n:
            xa, xb = _f64(pa.xyz).reshape(-1, 3), _f64(pb.xyz).reshape(-1, 3)
            N.check(N.lib().lchd_weight_gradient_primitives(self._context(), C.byref(cfg), N.dp(xa), N.ip(pa.cat), N.ip(pa.tag), len(xa), N.dp(xb),
                                                            N.ip(pb.cat), N.ip(pb.tag), len(xb), N.lp(anchors), N.ip(idx), n, thr, N.dp(out)))
        return WeightGradient(out[:n].copy(), out[n:].reshape(n, np_max).copy())

    def weight_gradient_from_coords(self, seq_a, seq_b, coords_a, coords_b, w_func_keys: Optional[Sequence[str]] = None, *, box_a=None,
                                    box_b=None, cell_a=None, cell_b=None) -> WeightGradient:
        """Additive: `weight_gradient_from_primitives` for the dense row pairs `from_coords` scores (pair r: the two structures of equal
        size seen from their atoms r): `WeightGradient(scores (n,), grad (n, NP))`.  Open structures only."""
        np_max = self._weight_gradient_width("weight_gradient_from_coords", (box_a, box_b, cell_a, cell_b))
        xa, xb = self._coords(coords_a), self._coords(coords_b)
        if len(xa) != len(xb):
            raise ValueError(f"Expected matrices with the same length, got lengths {len(xa)} and {len(xb)}!")
        n = len(xa)
        idx = self._wf_indices(None if w_func_keys is None else [str(k) for k in w_func_keys], n)
        if n > 65535:
            raise NotImplementedError(f"a weight-function gradient takes dense rows of at most 65535 points (got {n} / {n})")
        ca, cb = self._cats(list(seq_a)), self._cats(list(seq_b))
        cfg, keep = self._config()
        out = np.empty(n * (1 + np_max))
        if n:
            N.check(N.lib().lchd_weight_gradient_coords(self._context(), C.byref(cfg), N.ip(ca), ca.size, N.ip(cb), cb.size, N.dp(xa), N.dp(xb), n,
                                                        N.ip(idx), N.dp(out)))
        return WeightGradient(out[:n].copy(), out[n:].reshape(n, np_max).copy())

    def weight_gradient_from_dmxs(self, seq_a, seq_b, dmx_a, dmx_b, w_func_keys: Optional[Sequence[str]] = None) -> WeightGradient:
        """Additive: `weight_gradient_from_primitives` for the row pairs `from_dmxs` scores (rectangular matrices with the same number
        of rows): `WeightGradient(scores (rows,), grad (rows, NP))`."""
        np_max = self._weight_gradient_width("weight_gradient_from_dmxs")
        (ma, la), (mb, lb) = self._matrix(dmx_a), self._matrix(dmx_b)
        if la is not None or lb is not None:
            raise ValueError("weight_gradient_from_dmxs takes rectangular distance matrices (rows of equal length)")
        if ma.shape[0] != mb.shape[0]:
            raise ValueError(f"Expected matrices with the same length, got lengths {ma.shape[0]} and {mb.shape[0]}!")
        n = ma.shape[0]
        idx = self._wf_indices(None if w_func_keys is None else [str(k) for k in w_func_keys], n)
        if max(ma.shape[1], mb.shape[1]) > 65535:
            raise NotImplementedError(f"a weight-function gradient takes dense rows of at most 65535 points (got {ma.shape[1]} / {mb.shape[1]})")
        ca, cb = self._cats(list(seq_a)), self._cats(list(seq_b))
        cfg, keep = self._config()
        out = np.empty(n * (1 + np_max))
        if n:
            N.check(N.lib().lchd_weight_gradient_dmxs(self._context(), C.byref(cfg), N.ip(ca), ca.size, N.ip(cb), cb.size, N.dp(ma), N.dp(mb), n,
                                                      ma.shape[1], mb.shape[1], N.ip(idx), N.dp(out)))
        return WeightGradient(out[:n].copy(), out[n:].reshape(n, np_max).copy())

    # ---- reduced parameter gradients (additive) --------------------------------------------------------------
    # sum_p v_p dS_p/dw_c and sum_p v_p dS_p/dtheta in ONE native call (include/loco_hd_hip.h, "reduced parameter gradients"): the rows of
    # the two families above never reach the host; every term v_p * row[p][k] is one float64 product, the terms of a column are summed
    # EXACTLY (fixed point, quantum 2^-192) and rounded once.  The bits are the same for every `tile_pairs`, mode and run.
    @staticmethod
    def _param_sum_args(pair_weights, n: int, tile_pairs, what: str):
        """(pair weights as a contiguous float64 array or None, tile_pairs as an int) after the refusals that need no device."""
        if int(tile_pairs) < 0:
            raise ValueError(f"tile_pairs = {int(tile_pairs)} is negative (0: planned from the free device memory)")
        if pair_weights is None:
            return None, int(tile_pairs)
        v = np.asarray(pair_weights)
        if v.dtype.kind not in "fiu":
            raise ValueError(f"pair_weights must be real numbers (got dtype {v.dtype})")
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        if len(v) != n:
            raise ValueError(f"pair_weights has {len(v)} entries for {n} {what}")
        return v, int(tile_pairs)

    def category_gradient_sum_from_primitives(self, prim_a: Sequence[PrimitiveAtom], prim_b: Sequence[PrimitiveAtom], anchor_pairs,
                                              threshold_distance: float, pair_weights=None, *, tile_pairs: int = 0, box_a=None, box_b=None,
                                              cell_a=None, cell_b=None) -> np.ndarray:
        """Additive: sum_p v_p dS_p/dw_c over the anchor pairs, v = `pair_weights` (default: ones), as a float64 array (C,): the rows of
        `category_gradient_from_primitives` reduced on the device (lchd_category_gradient_sum_primitives) in tiles of `tile_pairs` pairs
        (0: planned from the free device memory), every column the correctly rounded exact sum of its terms.  An unusable pair (a NaN row)
        adds nothing.  ValueError if a term is not finite or reaches 2^63.  Boxes and cells as `category_gradient_from_primitives`."""
        for side, box, cell in (("a", box_a, cell_a), ("b", box_b, cell_b)):
            if box is not None and cell is not None:
                raise ValueError(f"box_{side} and cell_{side} were both given: a structure has one periodic box or one periodic cell")
        self._no_device_group_for_pair_rows(_CATEGORY_GRADIENT)
        thr = float(threshold_distance)
        ba = None if box_a is None else periodic_boxes(box_a, 1, thr, "box_a")
        bb = None if box_b is None else periodic_boxes(box_b, 1, thr, "box_b")
        ca = None if cell_a is None else periodic_cells(cell_a, 1, thr, "cell_a")
        cb = None if cell_b is None else periodic_cells(cell_b, 1, thr, "cell_b")
        pairs, idx = self._anchor_arrays(anchor_pairs)
        anchors = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        v, tile = self._param_sum_args(pair_weights, len(anchors), tile_pairs, "anchor pairs")
        pa, pb, interner = self._packed_lists(prim_a, prim_b)
        cfg, keep = self._config(interner)
        out = np.zeros(len(self._weights))
        xa, xb = _f64(pa.xyz).reshape(-1, 3), _f64(pb.xyz).reshape(-1, 3)
        N.check(N.lib().lchd_category_gradient_sum_primitives(self._context(), C.byref(cfg), N.dp(xa), N.ip(pa.cat), N.ip(pa.tag), len(xa),
                                                              N.dp(xb), N.ip(pb.cat), N.ip(pb.tag), len(xb), N.lp(anchors), N.ip(idx),
                                                              len(anchors), thr, N.dp(ba), N.dp(ca), N.dp(bb), N.dp(cb), N.dp(v), tile,
                                                              N.dp(out)))
        return out

    def category_gradient_sum_from_coords(self, seq_a, seq_b, coords_a, coords_b, w_func_keys: Optional[Sequence[str]] = None,
                                          pair_weights=None, *, box_a=None, box_b=None, cell_a=None, cell_b=None) -> np.ndarray:
        """Additive: `category_gradient_sum_from_primitives` for the dense row pairs `from_coords` scores: sum_r v_r dS_r/dw_c as a
        float64 array (C,), one tile (lchd_category_gradient_sum_coords).  `box_a` / `box_b` / `cell_a` / `cell_b`: minimum-image rows."""
        for side, box, cell in (("a", box_a, cell_a), ("b", box_b, cell_b)):
            if box is not None and cell is not None:
                raise ValueError(f"box_{side} and cell_{side} were both given: a structure has one periodic box or one periodic cell")
        self._no_device_group_for_pair_rows(_CATEGORY_GRADIENT)
        pc_a = dense_cells(box_a, cell_a, 1, "box_a", "cell_a")
        pc_b = dense_cells(box_b, cell_b, 1, "box_b", "cell_b")
        xa, xb = self._coords(coords_a), self._coords(coords_b)
        if len(xa) != len(xb):
            raise ValueError(f"Expected matrices with the same length, got lengths {len(xa)} and {len(xb)}!")
        v, _ = self._param_sum_args(pair_weights, len(xa), 0, "rows")
        idx = self._wf_indices(None if w_func_keys is None else [str(k) for k in w_func_keys], len(xa))
        ca, cb = self._cats(list(seq_a)), self._cats(list(seq_b))
        cfg, keep = self._config()
        out = np.zeros(len(self._weights))
        N.check(N.lib().lchd_category_gradient_sum_coords(self._context(), C.byref(cfg), N.ip(ca), ca.size, N.ip(cb), cb.size, N.dp(xa), len(xa),
                                                          N.dp(xb), len(xb), N.ip(idx), N.dp(pc_a), N.dp(pc_b), N.dp(v), N.dp(out)))
        return out

    def _n_weight_functions(self) -> int:
        return len(self._w_func) if isinstance(self._w_func, dict) else 1

    def weight_gradient_sum_from_primitives(self, prim_a: Sequence[PrimitiveAtom], prim_b: Sequence[PrimitiveAtom], anchor_pairs,
                                            threshold_distance: float, pair_weights=None, *, tile_pairs: int = 0, box_a=None, box_b=None,
                                            cell_a=None, cell_b=None) -> WeightGradientSum:
        """Additive: `WeightGradientSum(scores (P,), grad (n_wf, NP))`: the scores of `weight_gradient_from_primitives`, bit for bit, and
        per weight function f of `w_func` (in its order) the exact sum of v_p dS_p/dtheta over the pairs scored with f, rounded once, with
        exact zeros behind f's parameter count (lchd_weight_gradient_sum_primitives).  v = `pair_weights` (default: ones); `tile_pairs`:
        pairs per pass, 0 = planned from the free device memory.  ValueError if a term is not finite or reaches 2^63.  Open structures
        on one device only; at most 16 parameters."""
        np_max = self._weight_gradient_width("weight_gradient_sum_from_primitives", (box_a, box_b, cell_a, cell_b))
        thr = float(threshold_distance)
        pairs, idx = self._anchor_arrays(anchor_pairs)
        anchors = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        n = len(anchors)
        v, tile = self._param_sum_args(pair_weights, n, tile_pairs, "anchor pairs")
        pa, pb, interner = self._packed_lists(prim_a, prim_b)
        cfg, keep = self._config(interner)
        scores, out = np.empty(n), np.zeros((self._n_weight_functions(), np_max))
        xa, xb = _f64(pa.xyz).reshape(-1, 3), _f64(pb.xyz).reshape(-1, 3)
        N.check(N.lib().lchd_weight_gradient_sum_primitives(self._context(), C.byref(cfg), N.dp(xa), N.ip(pa.cat), N.ip(pa.tag), len(xa), N.dp(xb),
                                                            N.ip(pb.cat), N.ip(pb.tag), len(xb), N.lp(anchors), N.ip(idx), n, thr, N.dp(v), tile,
                                                            N.dp(scores), N.dp(out)))
        return WeightGradientSum(scores, out)

    def weight_gradient_sum_from_coords(self, seq_a, seq_b, coords_a, coords_b, w_func_keys: Optional[Sequence[str]] = None, pair_weights=None, *,
                                        box_a=None, box_b=None, cell_a=None, cell_b=None) -> WeightGradientSum:
        """Additive: `weight_gradient_sum_from_primitives` for the dense row pairs `from_coords` scores:
        `WeightGradientSum(scores (n,), grad (n_wf, NP))`, one tile (lchd_weight_gradient_sum_coords).  Open structures only."""
        np_max = self._weight_gradient_width("weight_gradient_sum_from_coords", (box_a, box_b, cell_a, cell_b))
        xa, xb = self._coords(coords_a), self._coords(coords_b)
        if len(xa) != len(xb):
            raise ValueError(f"Expected matrices with the same length, got lengths {len(xa)} and {len(xb)}!")
        n = len(xa)
        v, _ = self._param_sum_args(pair_weights, n, 0, "rows")
        idx = self._wf_indices(None if w_func_keys is None else [str(k) for k in w_func_keys], n)
        if n > 65535:
            raise NotImplementedError(f"a weight-function gradient takes dense rows of at most 65535 points (got {n} / {n})")
        ca, cb = self._cats(list(seq_a)), self._cats(list(seq_b))
        cfg, keep = self._config()
        scores, out = np.empty(n), np.zeros((self._n_weight_functions(), np_max))
        N.check(N.lib().lchd_weight_gradient_sum_coords(self._context(), C.byref(cfg), N.ip(ca), ca.size, N.ip(cb), cb.size, N.dp(xa), N.dp(xb), n,
                                                        N.ip(idx), N.dp(v), N.dp(scores), N.dp(out)))
        return WeightGradientSum(scores, out)

    # ---- neighbour sensitivities and coordinate gradients (additive) ---------------------------------------
    # g = dS/dd = w(d) (H- - H+) for every member of the pair's two environments (include/loco_hd_hip.h, "neighbour sensitivities"): which
    # neighbours carry the score, and -- through dd/dx = (x - x_anchor) / d -- in which direction they would have to move to change it.
    def sensitivity_from_primitives(self, prim_a: Sequence[PrimitiveAtom], prim_b: Sequence[PrimitiveAtom], anchor_pairs,
                                    threshold_distance: float, *, width: Optional[int] = None, box_a=None, box_b=None, cell_a=None,
                                    cell_b=None) -> Sensitivity:
        """Additive: for every anchor pair `from_primitives` would score, the derivative of its score with respect to the distance of
        every member of its two environments.  Returns `Sensitivity(scores, count_a, idx_a, dist_a, g_a, count_b, idx_b, dist_b, g_b)` of
        NumPy arrays: per pair and side the environment as a list sorted by (distance, atom index) with the anchor in slot 0 -- `count`
        members, their atom indices `idx` (padded with -1), distances `dist` and sensitivities `g` (padded with 0; slot 0 is 0) -- and
        the pair's score.  Rows are as wide as the longest environment, or `width` (ValueError if that is too small).

        The derivative ignores points entering or leaving at the threshold: it is exact when the weight function's support ends at or
        inside the threshold (the default, uniform [3, 10] with threshold 10), and it is one-sided at ties.  Every statistical distance
        is supported.  Periodic boxes and cells, the dense calls and device groups are not (NotImplementedError)."""
        if box_a is not None or box_b is not None or cell_a is not None or cell_b is not None:
            raise NotImplementedError("sensitivity_from_primitives takes open structures: periodic boxes and cells are not supported")
        return self._sensitivity_primitives(prim_a, prim_b, anchor_pairs, threshold_distance, width, None)

    def _sensitivity_primitives(self, prim_a, prim_b, anchor_pairs, threshold_distance, width, periodic):
        """The thresholded sensitivity call and its retry on the row width.  periodic: None (lchd_sensitivity_primitives, a `Sensitivity`) or
        the checked (box_a, cell_a, box_b, cell_b) arrays, None for an open side (lchd_sensitivity_primitives_periodic, a
        `PeriodicSensitivity`)."""
        if self._devices is not None:
            raise NotImplementedError("a sensitivity call applies to one device (a device group has no sensitivity call): drop devices=[...]")
        thr = float(threshold_distance)
        pairs, idx = self._anchor_arrays(anchor_pairs)
        pa, pb, interner = self._packed_lists(prim_a, prim_b)
        anchors = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        cfg, keep = self._config(interner)
        n = len(anchors)
        if width is not None and int(width) < 1:
            raise ValueError(f"width = {width}: a row holds at least the anchor")
        xa, xb = _f64(pa.xyz).reshape(-1, 3), _f64(pb.xyz).reshape(-1, 3)
        k = 128 if width is None else int(width)
        while True:
            scores = np.empty(n)
            cnt = [np.empty(n, dtype=np.int32) for _ in range(2)]
            ix = [np.empty((n, k), dtype=np.int32) for _ in range(2)]
            ds = [np.empty((n, k)) for _ in range(2)]
            gs = [np.empty((n, k)) for _ in range(2)]
            im = [np.zeros((n, k), dtype=np.int8) for _ in range(2)] if periodic is not None else None
            dp = [np.zeros((n, k, 3)) for _ in range(2)] if periodic is not None else None
            if n == 0:
                break
            ctx = self._context()
            head = (ctx, C.byref(cfg), N.dp(xa), N.ip(pa.cat), N.ip(pa.tag), len(xa), N.dp(xb), N.ip(pb.cat), N.ip(pb.tag), len(xb),
                    N.lp(anchors), N.ip(idx), n, thr, k)
            if periodic is None:
                rc = N.lib().lchd_sensitivity_primitives(*head, N.dp(scores), N.ip(cnt[0]), N.ip(ix[0]), N.dp(ds[0]), N.dp(gs[0]), N.ip(cnt[1]),
                                                         N.ip(ix[1]), N.dp(ds[1]), N.dp(gs[1]))
            else:
                sides = [(N.ip(cnt[j]), N.ip(ix[j]), C.c_void_p(im[j].ctypes.data), N.dp(ds[j]), N.dp(gs[j]), N.dp(dp[j])) for j in range(2)]
                rc = N.lib().lchd_sensitivity_primitives_periodic(*head, *[N.dp(b) for b in periodic], N.dp(scores), *sides[0], *sides[1])
            need = int(N.lib().lchd_sensitivity_needed_width(ctx))
            if rc == N.EVALUE and width is None and need > k:  # the first guess was too narrow: once more with the width the pairs take
                k = need
                continue
            N.check(rc)
            if width is None and 0 < need < k:
                ix, ds, gs = ([np.ascontiguousarray(a[:, :need]) for a in t] for t in (ix, ds, gs))
                if periodic is not None:
                    im, dp = ([np.ascontiguousarray(a[:, :need]) for a in t] for t in (im, dp))
            break
        if periodic is not None:
            return PeriodicSensitivity(scores, cnt[0], ix[0], im[0], ds[0], gs[0], dp[0], cnt[1], ix[1], im[1], ds[1], gs[1], dp[1])
        return Sensitivity(scores, cnt[0], ix[0], ds[0], gs[0], cnt[1], ix[1], ds[1], gs[1])

    # ---- ... under periodic boundaries (additive) ---------------------------------------------------------
    # The same pass on the periodic image clouds of the structures, every member resolved to the atom it is an image of
    # (include/loco_hd_hip.h, lchd_sensitivity_images_dev).  The two calls above keep refusing boxes and cells.
    def sensitivity_from_primitives_periodic(self, prim_a: Sequence[PrimitiveAtom], prim_b: Sequence[PrimitiveAtom], anchor_pairs,
                                             threshold_distance: float, *, width: Optional[int] = None, box_a=None, box_b=None, cell_a=None,
                                             cell_b=None) -> PeriodicSensitivity:
        """Additive: `sensitivity_from_primitives` for structures in periodic boxes (Lx, Ly, Lz) or triclinic cells (3 x 3, lattice
        vectors as rows), given per side as `from_primitives` takes them; a side with neither is open.  Returns
        `PeriodicSensitivity(scores, count_a, idx_a, image_a, dist_a, g_a, disp_a, count_b, ...)`: `idx` names the SOURCE atom of every
        member -- an atom that enters through two periodic images appears twice --, `image` (int8) its image code (0: the atom itself,
        else c0 + 3 c1 + 9 c2 with c = 0 original, 1 plus, 2 minus per axis) and `disp` (P, K, 3) the member's displacement from the
        anchor as the pass saw it (dist = |disp|).  Among exact ties the list order is: home atoms before images, then source index,
        then image code.  Device groups are not supported (NotImplementedError)."""
        for side, box, cell in (("a", box_a, cell_a), ("b", box_b, cell_b)):
            if box is not None and cell is not None:
                raise ValueError(f"box_{side} and cell_{side} were both given: a structure has one periodic box or one periodic cell")
        if self._devices is not None:
            raise NotImplementedError("a sensitivity call applies to one device (a device group has no sensitivity call): drop devices=[...]")
        thr = float(threshold_distance)
        ba = None if box_a is None else periodic_boxes(box_a, 1, thr, "box_a")
        bb = None if box_b is None else periodic_boxes(box_b, 1, thr, "box_b")
        ca = None if cell_a is None else periodic_cells(cell_a, 1, thr, "cell_a")
        cb = None if cell_b is None else periodic_cells(cell_b, 1, thr, "cell_b")
        return self._sensitivity_primitives(prim_a, prim_b, anchor_pairs, thr, width, (ba, ca, bb, cb))

    @staticmethod
    def _assemble_gradient_periodic(sens: "PeriodicSensitivity", n_a: int, n_b: int, pair_weights=None):
        """grad = sum_p v_p dS_p/dx from a PeriodicSensitivity: source atom += v g disp / d, anchor -= the same; the padding, members at
        d == 0 and non-finite g are skipped; np.add.at in pair order, then slot order.  No coordinates are needed: disp carries them."""
        v = np.ones(len(sens.scores)) if pair_weights is None else _f64(pair_weights).reshape(-1)
        if len(v) != len(sens.scores):
            raise ValueError(f"pair_weights has {len(v)} entries for {len(sens.scores)} anchor pairs")
        grads = []
        for n, idx, dist, g, disp in ((n_a, sens.idx_a, sens.dist_a, sens.g_a, sens.disp_a), (n_b, sens.idx_b, sens.dist_b, sens.g_b, sens.disp_b)):
            grad = np.zeros((n, 3))
            if idx.size:
                use = (idx >= 0) & (dist > 0.0) & np.isfinite(g)
                use[:, 0] = False
                p, k = np.nonzero(use)  # (row-major: pair order, then slot order)
                step = (v[p] * g[p, k] / dist[p, k])[:, None] * disp[p, k]
                np.add.at(grad, idx[p, k], step)
                np.add.at(grad, idx[p, 0], -step)
            grads.append(grad)
        return grads[0], grads[1]

    def gradient_from_primitives_periodic(self, prim_a: Sequence[PrimitiveAtom], prim_b: Sequence[PrimitiveAtom], anchor_pairs,
                                          threshold_distance: float, pair_weights=None, *, box_a=None, box_b=None, cell_a=None, cell_b=None):
        """Additive: `gradient_from_primitives` under periodic boundaries: `(scores, grad_a[Na, 3], grad_b[Nb, 3])` assembled on the host
        from `sensitivity_from_primitives_periodic` in a fixed order.  A wrap is a translation by a lattice vector, so this is the
        gradient with respect to the coordinates as given (wrapped or not); an atom that enters an environment through two images
        contributes both terms.  The derivative with respect to the box or cell is not part of it."""
        if pair_weights is not None:  # (checked in front of the device call: the list length is known from the pairs alone)
            n_pairs, n_w = len(self._anchor_arrays(anchor_pairs)[0]), len(_f64(pair_weights).reshape(-1))
            if n_w != n_pairs:
                raise ValueError(f"pair_weights has {n_w} entries for {n_pairs} anchor pairs")
        sens = self.sensitivity_from_primitives_periodic(prim_a, prim_b, anchor_pairs, threshold_distance, box_a=box_a, box_b=box_b,
                                                         cell_a=cell_a, cell_b=cell_b)
        ga, gb = self._assemble_gradient_periodic(sens, len(prim_a), len(prim_b), pair_weights)
        return sens.scores, ga, gb

    @staticmethod
    def _assemble_gradient(sens: "Sensitivity", xyz_a: np.ndarray, xyz_b: np.ndarray, pair_weights=None):
        """grad = sum_p v_p dS_p/dx from a Sensitivity: member += v g (x_m - x_anchor) / d, anchor -= the same, members at d == 0 skipped;
        np.add.at in pair order, then slot order: one fixed summation order."""
        v = np.ones(len(sens.scores)) if pair_weights is None else _f64(pair_weights).reshape(-1)
        if len(v) != len(sens.scores):
            raise ValueError(f"pair_weights has {len(v)} entries for {len(sens.scores)} anchor pairs")
        grads = []
        for xyz, idx, dist, g in ((xyz_a, sens.idx_a, sens.dist_a, sens.g_a), (xyz_b, sens.idx_b, sens.dist_b, sens.g_b)):
            grad = np.zeros((len(xyz), 3))
            if idx.size:
                use = (idx >= 0) & (dist > 0.0) & np.isfinite(g)
                use[:, 0] = False
                p, k = np.nonzero(use)  # (row-major: pair order, then slot order)
                member, anchor = idx[p, k], idx[p, 0]
                step = (v[p] * g[p, k] / dist[p, k])[:, None] * (xyz[member] - xyz[anchor])
                np.add.at(grad, member, step)
                np.add.at(grad, anchor, -step)
            grads.append(grad)
        return grads[0], grads[1]

    def gradient_from_primitives(self, prim_a: Sequence[PrimitiveAtom], prim_b: Sequence[PrimitiveAtom], anchor_pairs,
                                 threshold_distance: float, pair_weights=None, *, box_a=None, box_b=None, cell_a=None, cell_b=None):
        """Additive: `(scores, grad_a[Na, 3], grad_b[Nb, 3])` with grad = sum_p v_p dS_p/dx over the anchor pairs, v = `pair_weights`
        (default: ones): the coordinate gradient of a weighted sum of scores, assembled on the host from `sensitivity_from_primitives`
        in a fixed order.  The derivative ignores points entering or leaving at the threshold (exact when the weight function's support
        ends at or inside it) and is one-sided at ties; members at distance 0 contribute no direction."""
        sens = self.sensitivity_from_primitives(prim_a, prim_b, anchor_pairs, threshold_distance, box_a=box_a, box_b=box_b, cell_a=cell_a,
                                                cell_b=cell_b)
        pa, pb, _ = self._packed_lists(prim_a, prim_b)
        ga, gb = self._assemble_gradient(sens, _f64(pa.xyz).reshape(-1, 3), _f64(pb.xyz).reshape(-1, 3), pair_weights)
        return sens.scores, ga, gb

    # ---- ... of dense rows (additive) ----------------------------------------------------------------------
    # Row r of both sides, every column a member (include/loco_hd_hip.h, "Dense rows" under "neighbour sensitivities").  A dense row has
    # no threshold: g is the whole derivative of the row's score with respect to the row's entries, for any weight function.
    def _dense_sensitivity(self, name: str, seq_a, seq_b, a, b, w_func_keys, width, pair_weights=None, weighted=False, cells=None):
        """sensitivity_from_coords / sensitivity_from_dmxs (`name`) and the head of the two gradient calls: every check that needs no
        device, then the call.  Returns (Sensitivity, the two inputs as arrays, pair_weights as an array or None).  cells: the
        (cell_a, cell_b) of a `*_from_coords_periodic` call as `dense_cells` returns them (None: an open side); the first element
        returned is then a MinImageSensitivity."""
        if self._devices is not None:
            raise NotImplementedError("a sensitivity call applies to one device (a device group has no sensitivity call): drop devices=[...]")
        coords = cells is not None or name.endswith("coords")
        if coords:
            ma, mb = self._coords(a), self._coords(b)
            if len(ma) != len(mb):
                raise ValueError(f"Expected matrices with the same length, got lengths {len(ma)} and {len(mb)}!")
            rows, cols = len(ma), (len(ma), len(mb))
        else:
            (ma, la), (mb, lb) = self._matrix(a), self._matrix(b)
            if la is not None or lb is not None:
                raise ValueError(f"{name} takes rectangular distance matrices (rows of equal length)")
            if ma.shape[0] != mb.shape[0]:
                raise ValueError(f"Expected matrices with the same length, got lengths {ma.shape[0]} and {mb.shape[0]}!")
            rows, cols = ma.shape[0], (ma.shape[1], mb.shape[1])
        if width is not None and int(width) < 1:
            raise ValueError(f"width = {width}: a row holds at least one member")
        v = None
        if weighted:
            v = np.ones(rows) if pair_weights is None else _f64(pair_weights).reshape(-1)
            if len(v) != rows:
                raise ValueError(f"pair_weights has {len(v)} entries for {rows} rows")
        idx = self._wf_indices(None if w_func_keys is None else [str(k) for k in w_func_keys], rows)
        if len(self._weights) > 64:
            raise NotImplementedError(f"a sensitivity call takes at most 64 categories (got {len(self._weights)})")
        if max(cols) > 65535:
            raise NotImplementedError(f"a sensitivity call takes dense rows of at most 65535 points (got {cols[0]} / {cols[1]})")
        ca, cb = self._cats(list(seq_a)), self._cats(list(seq_b))
        cfg, keep = self._config()
        k = max(cols) if width is None else int(width)
        scores = np.empty(rows)
        cnt = [np.empty(rows, dtype=np.int32) for _ in range(2)]
        ix = [np.empty((rows, k), dtype=np.int32) for _ in range(2)]
        ds = [np.empty((rows, k)) for _ in range(2)]
        gs = [np.empty((rows, k)) for _ in range(2)]
        dp = [np.empty((rows, k, 3)) for _ in range(2)] if cells is not None else None
        if rows:
            outs = (N.dp(scores), N.ip(cnt[0]), N.ip(ix[0]), N.dp(ds[0]), N.dp(gs[0]), N.ip(cnt[1]), N.ip(ix[1]), N.dp(ds[1]), N.dp(gs[1]))
            head = (self._context(), C.byref(cfg), N.ip(ca), ca.size, N.ip(cb), cb.size, N.dp(ma), N.dp(mb))
            if cells is not None:
                N.check(N.lib().lchd_sensitivity_coords_periodic(*head, rows, N.ip(idx), N.dp(cells[0]), N.dp(cells[1]), k, *outs,
                                                                 N.dp(dp[0]), N.dp(dp[1])))
            elif coords:
                N.check(N.lib().lchd_sensitivity_coords(*head, rows, N.ip(idx), k, *outs))
            else:
                N.check(N.lib().lchd_sensitivity_dmxs(*head, rows, cols[0], cols[1], N.ip(idx), k, *outs))
        if cells is not None:
            return MinImageSensitivity(scores, cnt[0], ix[0], ds[0], gs[0], dp[0], cnt[1], ix[1], ds[1], gs[1], dp[1]), ma, mb, v
        return Sensitivity(scores, cnt[0], ix[0], ds[0], gs[0], cnt[1], ix[1], ds[1], gs[1]), ma, mb, v

    def sensitivity_from_dmxs(self, seq_a, seq_b, dmx_a, dmx_b, w_func_keys: Optional[Sequence[str]] = None, *,
                              width: Optional[int] = None) -> Sensitivity:
        """Additive: for every row pair `from_dmxs` would score (rectangular matrices with the same number of rows), the derivative of
        its score with respect to every entry of the two rows, as a `Sensitivity`: row p is dense row p sorted by (distance, column) --
        the reference's stable co-sort of the row with seq, no forced anchor -- `idx` the column indices, `dist` the entries,
        `count` = the side's number of columns, `g` the derivatives (0 in slot 0).  Rows are max(cols_a, cols_b) wide, or `width`
        (ValueError if that is smaller).  A dense row has no threshold, so the derivative is exact for any weight function away from
        ties, and one-sided at ties.  Arguments and errors as `attribution_from_dmxs`; every statistical distance; no device groups."""
        return self._dense_sensitivity("sensitivity_from_dmxs", seq_a, seq_b, dmx_a, dmx_b, w_func_keys, width)[0]

    def sensitivity_from_coords(self, seq_a, seq_b, coords_a, coords_b, w_func_keys: Optional[Sequence[str]] = None, *,
                                width: Optional[int] = None) -> Sensitivity:
        """Additive: `sensitivity_from_dmxs` on the rows `from_coords` scores (pair r: the two structures of equal size seen from
        their atoms r).  `idx` are atom indices; slot 0 of row r is atom r, unless an atom of lower index sits on the same point.
        Open structures only (no box / cell keywords)."""
        return self._dense_sensitivity("sensitivity_from_coords", seq_a, seq_b, coords_a, coords_b, w_func_keys, width)[0]

    @staticmethod
    def _dense_scatter(idx: np.ndarray, values: np.ndarray, cols: int) -> np.ndarray:
        """out[i][idx[i][k]] = values[i][k] for the members beyond slot 0 (0 elsewhere): sorted rows back into column order.  A column
        occurs once per row, so every element has one writer."""
        out = np.zeros((idx.shape[0], cols))
        keep = idx >= 0
        keep[:, :1] = False
        r, _ = np.nonzero(keep)
        out[r, idx[keep]] = values[keep]
        return out

    def gradient_from_dmxs(self, seq_a, seq_b, dmx_a, dmx_b, w_func_keys: Optional[Sequence[str]] = None, pair_weights=None):
        """Additive: `(scores, G_a[rows, cols_a], G_b[rows, cols_b])` with G[i][j] = v_i dS_i / d dmx[i][j] in the input's column
        order, v = `pair_weights` (default: ones): the gradient of a weighted sum of row scores with respect to the matrices
        themselves, scattered from `sensitivity_from_dmxs`.  The slot-0 column of a row (its first zero) and non-finite derivatives
        give 0.  Exact for any weight function (no threshold), one-sided at ties."""
        sens, ma, mb, v = self._dense_sensitivity("gradient_from_dmxs", seq_a, seq_b, dmx_a, dmx_b, w_func_keys, None, pair_weights, True)
        grads = [self._dense_scatter(idx, np.where(np.isfinite(g), v[:, None] * g, 0.0), m.shape[1])
                 for idx, g, m in ((sens.idx_a, sens.g_a, ma), (sens.idx_b, sens.g_b, mb))]
        return sens.scores, grads[0], grads[1]

    @staticmethod
    def _dense_coords_gradient(idx: np.ndarray, dist: np.ndarray, g: np.ndarray, v: np.ndarray, xyz: np.ndarray) -> np.ndarray:
        """One side of gradient_from_coords: W = v g / d in column order (0 where d == 0), M = W + W^T, rowsum(M) x - M x."""
        n = len(xyz)
        use = (dist > 0.0) & np.isfinite(g)
        w = LoCoHD._dense_scatter(idx,np.where(use, v[:, None] * g / np.where(use, dist, 1.0), 0.0), n)
        m = w + w.T
        return m.sum(axis=1)[:, None] * xyz - m @ xyz

    def gradient_from_coords(self, seq_a, seq_b, coords_a, coords_b, w_func_keys: Optional[Sequence[str]] = None, pair_weights=None):
        """Additive: `(scores, grad_a[n, 3], grad_b[n, 3])` with grad = sum_r v_r dS_r / dx over the dense rows `from_coords` scores,
        v = `pair_weights` (default: ones): the coordinate gradient of an all-atom LoCoHD loss.  Every atom is a member of every row
        and there is no threshold, so this derivative is exact for any weight function; at ties (equal distances in a row pair) it is
        one-sided.  Members at distance 0 contribute no direction.  Assembled on the host as one dense product: with W = v g / d in atom
        order and M = W + W^T, grad = rowsum(M) x - M x."""
        sens, xa, xb, v = self._dense_sensitivity("gradient_from_coords", seq_a, seq_b, coords_a, coords_b, w_func_keys, None, pair_weights,
                                                  True)
        return (sens.scores, self._dense_coords_gradient(sens.idx_a, sens.dist_a, sens.g_a, v, xa),
                self._dense_coords_gradient(sens.idx_b, sens.dist_b, sens.g_b, v, xb))

    # ---- native coordinate gradients (additive) ---------------------------------------------------------------
    # The same gradients in one native call (include/loco_hd_hip.h, "native coordinate gradients"): the lists are reduced on the device
    # into exact fixed-point accumulators, so the result is a function of the inputs alone and no list reaches the host.
    def native_gradient_from_primitives(self, prim_a: Sequence[PrimitiveAtom], prim_b: Sequence[PrimitiveAtom], anchor_pairs,
                                        threshold_distance: float, pair_weights=None, *, tile_pairs: int = 0, box_a=None, box_b=None,
                                        cell_a=None, cell_b=None):
        """Additive: `(scores, grad_a[Na, 3], grad_b[Nb, 3])` as `gradient_from_primitives` defines them, reduced on the device
        (lchd_gradient_primitives): every term v g (x_m - x_anchor) / d is computed in float64 as that call computes it, the terms of
        an atom are summed EXACTLY (fixed point, quantum 2^-192) and rounded once.  The bits are the same for every `tile_pairs` (pairs
        per pass; 0: planned from the free device memory), in default and deterministic mode, on every run.  `scores` are those of
        `sensitivity_from_primitives`.  ValueError if a term is not finite or reaches 2^63.  Open structures on one device only."""
        if int(tile_pairs) < 0:
            raise ValueError(f"tile_pairs = {int(tile_pairs)} is negative (0: planned from the free device memory)")
        if box_a is not None or box_b is not None or cell_a is not None or cell_b is not None:
            raise NotImplementedError("native_gradient_from_primitives takes open structures: periodic boxes and cells are not supported")
        if self._devices is not None:
            raise NotImplementedError("a native gradient call applies to one device (a device group has no gradient call): drop devices=[...]")
        pairs, idx = self._anchor_arrays(anchor_pairs)
        anchors = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        n = len(anchors)
        v = None
        if pair_weights is not None:
            v = np.ascontiguousarray(_f64(pair_weights).reshape(-1))
            if len(v) != n:
                raise ValueError(f"pair_weights has {len(v)} entries for {n} anchor pairs")
        pa, pb, interner = self._packed_lists(prim_a, prim_b)
        cfg, keep = self._config(interner)
        xa, xb = _f64(pa.xyz).reshape(-1, 3), _f64(pb.xyz).reshape(-1, 3)
        scores, ga, gb = np.empty(n), np.zeros((len(xa), 3)), np.zeros((len(xb), 3))
        N.check(N.lib().lchd_gradient_primitives(self._context(), C.byref(cfg), N.dp(xa), N.ip(pa.cat), N.ip(pa.tag), len(xa), N.dp(xb),
                                                 N.ip(pb.cat), N.ip(pb.tag), len(xb), N.lp(anchors), N.ip(idx), n, float(threshold_distance),
                                                 N.dp(v), int(tile_pairs), N.dp(scores), N.dp(ga), N.dp(gb)))
        return scores, ga, gb

    def native_gradient_from_coords(self, seq_a, seq_b, coords_a, coords_b, w_func_keys: Optional[Sequence[str]] = None, pair_weights=None):
        """Additive: `(scores, grad_a[n, 3], grad_b[n, 3])` as `gradient_from_coords` defines them, reduced on the device
        (lchd_gradient_coords): row r's terms v_r g (x_m - x_r) / d are summed exactly per atom and rounded once, as
        `native_gradient_from_primitives` does.  Open structures on one device only."""
        if self._devices is not None:
            raise NotImplementedError("a native gradient call applies to one device (a device group has no gradient call): drop devices=[...]")
        xa, xb = self._coords(coords_a), self._coords(coords_b)
        if len(xa) != len(xb):
            raise ValueError(f"Expected matrices with the same length, got lengths {len(xa)} and {len(xb)}!")
        n = len(xa)
        v = None
        if pair_weights is not None:
            v = np.ascontiguousarray(_f64(pair_weights).reshape(-1))
            if len(v) != n:
                raise ValueError(f"pair_weights has {len(v)} entries for {n} rows")
        idx = self._wf_indices(None if w_func_keys is None else [str(k) for k in w_func_keys], n)
        if len(self._weights) > 64:
            raise NotImplementedError(f"a sensitivity call takes at most 64 categories (got {len(self._weights)})")
        if n > 65535:
            raise NotImplementedError(f"a sensitivity call takes dense rows of at most 65535 points (got {n} / {n})")
        ca, cb = self._cats(list(seq_a)), self._cats(list(seq_b))
        cfg, keep = self._config()
        scores, ga, gb = np.empty(n), np.zeros((n, 3)), np.zeros((n, 3))
        if n:
            N.check(N.lib().lchd_gradient_coords(self._context(), C.byref(cfg), N.ip(ca), ca.size, N.ip(cb), cb.size, N.dp(xa), N.dp(xb), n,
                                                 N.ip(idx), N.dp(v), N.dp(scores), N.dp(ga), N.dp(gb)))
        return scores, ga, gb

    # ---- ... under periodic boundaries, with the strain derivative (additive) ---------------------------------
    # include/loco_hd_hip.h, "under periodic boundaries, and the strain derivative": the lists of the periodic sensitivity calls reduced on
    # the device from their displacements; W = sum step (x) disp per side in six more exact accumulators.
    def native_gradient_from_primitives_periodic(self, prim_a: Sequence[PrimitiveAtom], prim_b: Sequence[PrimitiveAtom], anchor_pairs,
                                                 threshold_distance: float, pair_weights=None, *, tile_pairs: int = 0, box_a=None,
                                                 box_b=None, cell_a=None, cell_b=None, strain: bool = False):
        """Additive: `native_gradient_from_primitives` for structures in periodic boxes (Lx, Ly, Lz) or triclinic cells (3 x 3, lattice
        vectors as rows), given per side as `from_primitives` takes them; a side with neither is open.  `(scores, grad_a[Na, 3],
        grad_b[Nb, 3])` as `gradient_from_primitives_periodic` defines them -- every term v g disp / d in float64, the terms of a source
        atom summed exactly and rounded once (lchd_gradient_primitives_periodic).  strain=True: a `NativeGradient(scores, grad_a, grad_b,
        strain_a, strain_b)` whose (3, 3) float64 strains W are the derivative of sum_p v_p S_p with respect to a strain x -> x (I + eps)
        of the side's coordinates and cell together, symmetric, exact sums rounded once (`cell_gradient` turns one into dL/dcell).  The
        bits are the same for every `tile_pairs`, mode and run.  ValueError if a term is not finite or reaches 2^63."""
        if int(tile_pairs) < 0:
            raise ValueError(f"tile_pairs = {int(tile_pairs)} is negative (0: planned from the free device memory)")
        for side, box, cell in (("a", box_a, cell_a), ("b", box_b, cell_b)):
            if box is not None and cell is not None:
                raise ValueError(f"box_{side} and cell_{side} were both given: a structure has one periodic box or one periodic cell")
        if self._devices is not None:
            raise NotImplementedError("a native gradient call applies to one device (a device group has no gradient call): drop devices=[...]")
        thr = float(threshold_distance)
        ba = None if box_a is None else periodic_boxes(box_a, 1, thr, "box_a")
        bb = None if box_b is None else periodic_boxes(box_b, 1, thr, "box_b")
        ca = None if cell_a is None else periodic_cells(cell_a, 1, thr, "cell_a")
        cb = None if cell_b is None else periodic_cells(cell_b, 1, thr, "cell_b")
        pairs, idx = self._anchor_arrays(anchor_pairs)
        anchors = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        n = len(anchors)
        v = None
        if pair_weights is not None:
            v = np.ascontiguousarray(_f64(pair_weights).reshape(-1))
            if len(v) != n:
                raise ValueError(f"pair_weights has {len(v)} entries for {n} anchor pairs")
        pa, pb, interner = self._packed_lists(prim_a, prim_b)
        cfg, keep = self._config(interner)
        xa, xb = _f64(pa.xyz).reshape(-1, 3), _f64(pb.xyz).reshape(-1, 3)
        scores, ga, gb = np.empty(n), np.zeros((len(xa), 3)), np.zeros((len(xb), 3))
        wa, wb = (np.zeros((3, 3)), np.zeros((3, 3))) if strain else (None, None)
        N.check(N.lib().lchd_gradient_primitives_periodic(self._context(), C.byref(cfg), N.dp(xa), N.ip(pa.cat), N.ip(pa.tag), len(xa), N.dp(xb),
                                                          N.ip(pb.cat), N.ip(pb.tag), len(xb), N.lp(anchors), N.ip(idx), n, thr, N.dp(ba),
                                                          N.dp(ca), N.dp(bb), N.dp(cb), N.dp(v), int(tile_pairs), N.dp(scores), N.dp(ga),
                                                          N.dp(gb), N.dp(wa), N.dp(wb)))
        return NativeGradient(scores, ga, gb, wa, wb) if strain else (scores, ga, gb)

    def native_gradient_from_coords_periodic(self, seq_a, seq_b, coords_a, coords_b, w_func_keys: Optional[Sequence[str]] = None,
                                             pair_weights=None, *, box_a=None, box_b=None, cell_a=None, cell_b=None, strain: bool = False):
        """Additive: `native_gradient_from_coords` on the minimum-image rows `from_coords(..., box_a= / cell_a= ...)` scores; boxes and
        cells per side as `from_coords` takes them, a side with neither is open (with none at all: the bits of
        `native_gradient_from_coords`).  `(scores, grad_a[n, 3], grad_b[n, 3])`, or with strain=True a `NativeGradient` as
        `native_gradient_from_primitives_periodic` returns it (lchd_gradient_coords_periodic)."""
        if self._devices is not None:
            raise NotImplementedError("a native gradient call applies to one device (a device group has no gradient call): drop devices=[...]")
        cells = self._dense_periodic_cells(box_a, box_b, cell_a, cell_b)
        xa, xb = self._coords(coords_a), self._coords(coords_b)
        if len(xa) != len(xb):
            raise ValueError(f"Expected matrices with the same length, got lengths {len(xa)} and {len(xb)}!")
        n = len(xa)
        v = None
        if pair_weights is not None:
            v = np.ascontiguousarray(_f64(pair_weights).reshape(-1))
            if len(v) != n:
                raise ValueError(f"pair_weights has {len(v)} entries for {n} rows")
        idx = self._wf_indices(None if w_func_keys is None else [str(k) for k in w_func_keys], n)
        if len(self._weights) > 64:
            raise NotImplementedError(f"a sensitivity call takes at most 64 categories (got {len(self._weights)})")
        if n > 65535:
            raise NotImplementedError(f"a sensitivity call takes dense rows of at most 65535 points (got {n} / {n})")
        ca, cb = self._cats(list(seq_a)), self._cats(list(seq_b))
        cfg, keep = self._config()
        scores, ga, gb = np.empty(n), np.zeros((n, 3)), np.zeros((n, 3))
        wa, wb = (np.zeros((3, 3)), np.zeros((3, 3))) if strain else (None, None)
        if n:
            N.check(N.lib().lchd_gradient_coords_periodic(self._context(), C.byref(cfg), N.ip(ca), ca.size, N.ip(cb), cb.size, N.dp(xa), N.dp(xb),
                                                          n, N.ip(idx), N.dp(cells[0]), N.dp(cells[1]), N.dp(v), N.dp(scores), N.dp(ga),
                                                          N.dp(gb), N.dp(wa), N.dp(wb)))
        return NativeGradient(scores, ga, gb, wa, wb) if strain else (scores, ga, gb)

    # ---- ... of dense rows in periodic cells (additive) ------------------------------------------------------
    # The minimum-image rows of from_coords(box_a= / cell_a= ...) (include/loco_hd_hip.h, lchd_sensitivity_coords_periodic).  A row
    # stores the length of the chosen image's vector alone, so the open product rowsum(M) x - M x no longer gives the gradient: the
    # call returns the vectors (disp) and the gradient is assembled from them.
    def _dense_periodic_cells(self, box_a, box_b, cell_a, cell_b):
        """The keyword checks of from_coords for a dense sensitivity call: (cell_a, cell_b) as dense_cells returns them."""
        for side, box, cell in (("a", box_a, cell_a), ("b", box_b, cell_b)):
            if box is not None and cell is not None:
                raise ValueError(f"box_{side} and cell_{side} were both given: a structure has one periodic box or one periodic cell")
        return dense_cells(box_a, cell_a, 1, "box_a", "cell_a"), dense_cells(box_b, cell_b, 1, "box_b", "cell_b")

    def sensitivity_from_coords_periodic(self, seq_a, seq_b, coords_a, coords_b, w_func_keys: Optional[Sequence[str]] = None, *,
                                         width: Optional[int] = None, box_a=None, box_b=None, cell_a=None,
                                         cell_b=None) -> MinImageSensitivity:
        """Additive: `sensitivity_from_coords` on the minimum-image rows `from_coords(..., box_a= / cell_a= ...)` scores; boxes and
        cells per side as `from_coords` takes them, a side with neither is open.  Returns `MinImageSensitivity(scores, count_a, idx_a,
        dist_a, g_a, disp_a, count_b, ...)`: the fields of `Sensitivity` on those rows and `disp` (n, K, 3), the displacement from row
        atom r to the nearest periodic image of member idx[r, k] (on an open side x[member] - x[r]); dist = |disp| bit for bit, the
        padding is 0.  Between two images at exactly the same distance the first in the header's candidate order is taken.
        Coordinates need not be wrapped.  Device groups are not supported (NotImplementedError)."""
        cells = self._dense_periodic_cells(box_a, box_b, cell_a, cell_b)
        return self._dense_sensitivity("sensitivity_from_coords_periodic", seq_a, seq_b, coords_a, coords_b, w_func_keys, width, cells=cells)[0]

    @staticmethod
    def _min_image_side_gradient(idx: np.ndarray, dist: np.ndarray, g: np.ndarray, disp: np.ndarray, v: np.ndarray, n: int) -> np.ndarray:
        """One side of gradient_from_coords_periodic: c = v g / d (0 in slot 0, where d == 0 and where g is not finite), T = c disp
        scattered into atom order one component at a time (`_dense_scatter`: one writer per element), grad = T.sum(axis=0) -
        T.sum(axis=1): the atom as a member of every row, minus the atom as the row's own."""
        use = (dist > 0.0) & np.isfinite(g)
        c = np.where(use, v[:, None] * g / np.where(use, dist, 1.0), 0.0)
        t = np.stack([LoCoHD._dense_scatter(idx, c * disp[..., d], n) for d in range(3)], axis=-1)  # [row][atom][3]
        return t.sum(axis=0) - t.sum(axis=1)

    @staticmethod
    def _assemble_gradient_min_image(sens: "MinImageSensitivity", pair_weights=None):
        """(grad_a, grad_b) = sum_r v_r dS_r/dx from a MinImageSensitivity; no coordinates are needed: disp carries the geometry."""
        rows = len(sens.scores)
        v = np.ones(rows) if pair_weights is None else _f64(pair_weights).reshape(-1)
        if len(v) != rows:
            raise ValueError(f"pair_weights has {len(v)} entries for {rows} rows")
        return (LoCoHD._min_image_side_gradient(sens.idx_a, sens.dist_a, sens.g_a, sens.disp_a, v, rows),
                LoCoHD._min_image_side_gradient(sens.idx_b, sens.dist_b, sens.g_b, sens.disp_b, v, rows))

    def gradient_from_coords_periodic(self, seq_a, seq_b, coords_a, coords_b, w_func_keys: Optional[Sequence[str]] = None, pair_weights=None,
                                      *, box_a=None, box_b=None, cell_a=None, cell_b=None):
        """Additive: `gradient_from_coords` under minimum-image periodic boundaries: `(scores, grad_a[n, 3], grad_b[n, 3])` with grad =
        sum_r v_r dS_r / dx over the rows `from_coords(..., box_a= ...)` scores.  Exact for any weight function (a dense row has no
        threshold), one-sided at ties and where an atom sits exactly half a cell from the row's atom.  A wrap is a translation by a
        lattice vector, so this is the gradient with respect to the coordinates as given, wrapped or not; the derivative with respect
        to the box or cell is not part of it.  Assembled on the host from `sensitivity_from_coords_periodic` in a fixed order."""
        cells = self._dense_periodic_cells(box_a, box_b, cell_a, cell_b)
        sens, _, _, v = self._dense_sensitivity("gradient_from_coords_periodic", seq_a, seq_b, coords_a, coords_b, w_func_keys, None,
                                                pair_weights, True, cells=cells)
        ga, gb = self._assemble_gradient_min_image(sens, v)
        return sens.scores, ga, gb

    # ---- cross-scoring (additive) ---------------------------------------------------------------------------
    # Every anchor of one list against every anchor of another (include/loco_hd_hip.h, "cross-scoring"): the pair list is generated on the
    # device tile by tile, scored by the pass of from_primitives, and -- for nearest -- reduced to the k best columns per row there.
    def _cross_arguments(self, what: str, anchors_a, anchors_b, w_func_key, tile_rows, k=None):
        """The checks that need no device; returns (anchors_a, anchors_b, wf index or -1, tile_rows) as arrays / ints."""
        if self._devices is not None:
            raise NotImplementedError(f"{what} applies to one device (the device group {self._devices} has no cross-scoring call): "
                                      "drop devices=[...]")
        lists = []
        for anchors in (anchors_a, anchors_b):
            idx_list = [int(a) for a in anchors]
            if any(a < 0 for a in idx_list):
                raise OverflowError("can't convert negative int to unsigned")
            lists.append(np.asarray(idx_list, dtype=np.int64).reshape(-1))
        na, nb = len(lists[0]), len(lists[1])
        if k is not None and not 1 <= int(k) <= min(nb, 64):
            raise ValueError(f"k = {int(k)} is outside 1 .. min(Nb, 64) with Nb = {nb}")
        if int(tile_rows) < 0:
            raise ValueError(f"tile_rows = {int(tile_rows)} is negative (0: planned from the free device memory)")
        if na == 0 or nb == 0:  # what from_primitives makes of an empty pair list (AnchorPairSpecifier: the with-key variant)
            self._wf_indices([], 0)
            raise ValueError("Invalid pairing for the LoCoHD instance's w_func option and the method's w_func_keys parameter!")
        idx = self._wf_indices(None if w_func_key is None else [str(w_func_key)], 1)
        return lists[0], lists[1], -1 if idx is None else int(idx[0]), int(tile_rows)

    def _cross_call(self, what, prim_a, prim_b, anchors_a, anchors_b, threshold_distance, w_func_key, tile_rows, k):
        anc_a, anc_b, wf, tile_rows = self._cross_arguments(what, anchors_a, anchors_b, w_func_key, tile_rows, k)
        pa, pb, interner = self._packed_lists(prim_a, prim_b)
        cfg, keep = self._config(interner)
        xa, xb = _f64(pa.xyz).reshape(-1, 3), _f64(pb.xyz).reshape(-1, 3)
        head = (self._context(), C.byref(cfg), N.dp(xa), N.ip(pa.cat), N.ip(pa.tag), len(xa), N.dp(xb), N.ip(pb.cat), N.ip(pb.tag), len(xb),
                N.lp(anc_a), len(anc_a), N.lp(anc_b), len(anc_b), wf, float(threshold_distance), tile_rows)
        if k is None:
            out = np.empty((len(anc_a), len(anc_b)))
            N.check(N.lib().lchd_cross_primitives(*head, N.dp(out)))
            return out
        scores, cols = np.empty((len(anc_a), int(k))), np.empty((len(anc_a), int(k)), dtype=np.int32)
        N.check(N.lib().lchd_nearest_primitives(*head, int(k), N.dp(scores), N.ip(cols)))
        return Nearest(scores, cols)

    def cross_from_primitives(self, prim_a: Sequence[PrimitiveAtom], prim_b: Sequence[PrimitiveAtom], anchors_a, anchors_b,
                              threshold_distance: float, w_func_key: Optional[str] = None, *, tile_rows: int = 0) -> np.ndarray:
        """Additive: every anchor of `anchors_a` (indices into `prim_a`) against every anchor of `anchors_b` (indices into `prim_b`;
        repeats allowed in both) as a float64 array (Na, Nb): out[i][j] is the score `from_primitives` gives the pair (anchors_a[i],
        anchors_b[j]).  `w_func_key`: the key of one weight function for the whole call, resolved as a key in an anchor-pair specifier
        is.  `tile_rows` (keyword-only): rows of A scored per pass -- 0 lets the library plan it from the free device memory; a number
        bounds the device memory of the call and lets tests force tiling.  Open structures only; no device groups."""
        return self._cross_call("cross_from_primitives", prim_a, prim_b, anchors_a, anchors_b, threshold_distance, w_func_key, tile_rows, None)

    def nearest_from_primitives(self, prim_a: Sequence[PrimitiveAtom], prim_b: Sequence[PrimitiveAtom], anchors_a, anchors_b,
                                threshold_distance: float, k: int, w_func_key: Optional[str] = None, *, tile_rows: int = 0) -> Nearest:
        """Additive: for every anchor of `anchors_a` the `k` anchors of `anchors_b` with the smallest (score, j), ascending, as
        `Nearest(scores (Na, k) float64, cols (Na, k) int32)` -- `cols` are positions in `anchors_b`, and the secondary key j makes the
        order a function of the score matrix of `cross_from_primitives` alone.  1 <= k <= min(Nb, 64).  The score matrix is never moved
        to the host: it is reduced on the device tile by tile.  Other arguments as `cross_from_primitives`."""
        return self._cross_call("nearest_from_primitives", prim_a, prim_b, anchors_a, anchors_b, threshold_distance, w_func_key, tile_rows, int(k))

    def _no_device_group_with_box(self) -> None:
        if self._devices is not None:
            raise ValueError("a periodic box or cell applies to one device (a device group has no image clouds): drop devices=[...]")

    def _from_primitives_periodic(self, prim_a, prim_b, anchor_pairs, threshold_distance, box_a, box_b, cell_a=None, cell_b=None) -> List[float]:
        for side, box, cell in (("a", box_a, cell_a), ("b", box_b, cell_b)):
            if box is not None and cell is not None:
                raise ValueError(f"box_{side} and cell_{side} were both given: a structure has one periodic box or one periodic cell")
        self._no_device_group_with_box()
        thr = float(threshold_distance)
        ba = None if box_a is None else periodic_boxes(box_a, 1, thr, "box_a")
        bb = None if box_b is None else periodic_boxes(box_b, 1, thr, "box_b")
        ca = None if cell_a is None else periodic_cells(cell_a, 1, thr, "cell_a")
        cb = None if cell_b is None else periodic_cells(cell_b, 1, thr, "cell_b")
        pairs, idx = self._anchor_arrays(anchor_pairs)
        pa, pb, interner = self._packed_lists(prim_a, prim_b)
        anchors = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        cfg, keep = self._config(interner)
        out = np.empty(len(anchors))
        if len(anchors) == 0:
            return []
        xa, xb = _f64(pa.xyz).reshape(-1, 3), _f64(pb.xyz).reshape(-1, 3)
        if ca is None and cb is None:
            N.check(N.lib().lchd_from_primitives_periodic(self._context(), C.byref(cfg), N.dp(xa), N.ip(pa.cat), N.ip(pa.tag), len(xa),
                                                          N.dp(xb), N.ip(pb.cat), N.ip(pb.tag), len(xb), N.lp(anchors), N.ip(idx),
                                                          len(anchors), thr, N.dp(ba), N.dp(bb), N.dp(out)))
        elif ba is None and bb is None:
            N.check(N.lib().lchd_from_primitives_periodic_cell(self._context(), C.byref(cfg), N.dp(xa), N.ip(pa.cat), N.ip(pa.tag), len(xa),
                                                               N.dp(xb), N.ip(pb.cat), N.ip(pb.tag), len(xb), N.lp(anchors), N.ip(idx),
                                                               len(anchors), thr, N.dp(ca), N.dp(cb), N.dp(out)))
        else:  # a box on one side, a cell on the other: no single C call takes both families, a session does
            from .device import DeviceSession

            # (as in the two C calls above: an index beyond the structure would name a ghost atom of the image cloud)
            if anchors.min() < 0 or anchors[:, 0].max() >= len(xa) or anchors[:, 1].max() >= len(xb):
                raise N.PanicException("index out of bounds: an anchor index is outside its structure (src/locohd.rs:521)")

            sess = DeviceSession(self, device=None if self._device < 0 else self._device, interner=interner)
            try:
                torch = sess.torch
                sides = []
                for pk, x, box, cell in ((pa, xa, ba, ca), (pb, xb, bb, cb)):
                    cl = sess.upload(x, pk.cat, pk.tag)
                    sides.append(sess.periodic_images(cl, box, thr) if box is not None else sess.periodic_images(cl, reach=thr, cell=cell))
                dev = torch.device("cuda", sess.device)
                d_idx = None if idx is None else torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32)).to(dev)
                out = sess.from_primitives(sides[0], sides[1], torch.from_numpy(anchors).to(dev), thr, wf_index=d_idx).cpu().numpy()
            finally:
                sess.close()
        return out.tolist()

    # The reference's callers score the same structures over and over (one native structure against every decoy,
    # python_codes/casp14/casp14_extend_with_locohd.py:72-79; one reference frame against a trajectory,
    # python_codes/trajectory_analyzer.py:112-120), and extracting a few thousand Python objects costs several times the device
    # call.  The packed form of a list is therefore kept: an entry is valid while the list still holds the very same atom
    # objects (compared by identity in native code; the entry keeps them alive, so an address cannot be re-used) and no
    # PrimitiveAtom setter has run since.  Only plain lists / tuples of exactly PrimitiveAtom are cached.
    _CACHE_ENTRIES = 8

    def _cache_lookup(self, prims, parent):
        with self._cache_lock:
            for k, e in enumerate(self._pack_cache):
                if e[0] is prims and e[3] is parent and e[2] == _ATOM_MUTATIONS[0] and _fastpack.same_items(prims, e[1]):
                    if k:
                        self._pack_cache.insert(0, self._pack_cache.pop(k))
                    return e
        return None

    def _type_map(self) -> np.ndarray:
        """primitive-type id (the process-wide table of PrimitiveAtom) -> category index of THIS instance, -1: not in its map"""
        m = self._pid_map
        if len(m) < len(_TYPE_NAMES):
            get = self._categories.get
            ext = [get(nm if type(nm) is str else str(nm), -1) for nm in _TYPE_NAMES[len(m):]]
            m = self._pid_map = np.concatenate([m, np.asarray(ext, dtype=np.int32)])
        return m

    def _pack_global(self, prims) -> _Packed:
        """Packed form with tags from the process-wide table: the gather over interned ids when the list holds exactly PrimitiveAtom
        objects, else the general extraction (strings looked up per atom) into the same id space."""
        n = len(prims)
        if _fastpack is not None and hasattr(_fastpack, "pack_atoms"):
            xyz, cat, tag = np.empty((n, 3), dtype=np.float64), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
            if _fastpack.pack_atoms(prims, PrimitiveAtom, self._type_map(), xyz, cat, tag):
                return _Packed(xyz, cat, tag)
        with _INTERN_LOCK:  # (new tags enter the process-wide table)
            return self.pack(prims, _TAG_IDS)

    def _packed_lists(self, prim_a, prim_b):
        """(packed A, packed B, interner): tags of both lists (and of the tag rule, _config) are ids of ONE table, the process-wide
        one of PrimitiveAtom -- only their equality matters (tag_pairing_rule.rs:49-75)."""
        if _fastpack is None or not hasattr(_fastpack, "same_items"):
            with _INTERN_LOCK:
                return self.pack(prim_a, _TAG_IDS), self.pack(prim_b, _TAG_IDS), _TAG_IDS
        entries = []
        for prims in (prim_a, prim_b):
            e = self._cache_lookup(prims, None)
            if e is None:
                stamp = _ATOM_MUTATIONS[0]  # before the atoms are read (see _ATOM_MUTATIONS)
                items = _fastpack.items_tuple(prims, PrimitiveAtom)
                packed = self._pack_global(prims)
                e = (prims, items, stamp, None, packed, _TAG_IDS)
                if items is not None:
                    with self._cache_lock:
                        self._pack_cache.insert(0, e)
                        del self._pack_cache[self._CACHE_ENTRIES:]
            entries.append(e)
        return entries[0][4], entries[1][4], _TAG_IDS

    def _anchor_arrays(self, anchor_pairs):
        """([P][2] int64 anchors, weight-function indices or None); the conversion of an unchanged list of tuples is kept."""
        c = self._anchor_cache
        if c is not None and c[0] is anchor_pairs and _fastpack is not None and hasattr(_fastpack, "same_items") and _fastpack.same_items(anchor_pairs, c[1]):
            return c[2], c[3]
        # (the items are taken BEFORE the conversion: a list changed in between then fails same_items rather than hit a stale entry)
        items = _fastpack.items_tuple(anchor_pairs, tuple) if (_fastpack is not None and hasattr(_fastpack, "items_tuple")) else None
        if _fastpack is not None and hasattr(_fastpack, "pairs_into") and hasattr(anchor_pairs, "__len__"):
            arr = np.empty((len(anchor_pairs), 2), dtype=np.int64)
            keys = _fastpack.pairs_into(anchor_pairs, arr)  # (AnchorPairSpecifier in native code, like the PyO3 derive)
            idx = self._wf_indices(keys, len(arr))
        else:
            pairs, keys = self._split_anchor_pairs(anchor_pairs)
            idx = self._wf_indices(keys, len(pairs))
            arr = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        self._anchor_cache = (anchor_pairs, items, arr, idx) if items is not None else None
        return arr, idx

    def from_primitives_batch(self, structures: Sequence[Sequence[PrimitiveAtom]],
                              jobs: Sequence[Tuple[int, int, Sequence[Tuple[int, int]]]],
                              threshold_distance: float, *, boxes=None, cells=None) -> List[List[float]]:
        """Additive: many `from_primitives` calls in one device pass.  `structures` are lists of
        PrimitiveAtoms; a job `(a, b, anchor_pairs)` asks for `from_primitives(structures[a], structures[b],
        anchor_pairs, threshold_distance)`.  Returns one score list per job, each bit-identical to the single call.
        Replaces loops such as python_codes/casp14/casp14_extend_with_locohd.py:42-88 (every decoy against the native
        structure): all structures are uploaded once as one batch
        object, the anchor pairs of all jobs are scored by one kernel sequence.

        It does NOT reproduce the dense numbers of python_codes/ensembles/compare_ensembles.py:277-296: that script scores
        whole-structure rows (from_dmxs), this call thresholded from_primitives environments.  The script's call is
        `from_dmxs_ensemble` / `from_coords_ensemble`.

        ``boxes`` (keyword-only, additive): one orthorhombic periodic box (Lx, Ly, Lz) for all structures, or one per structure;
        every environment then holds the periodic images within ``threshold_distance`` as in ``from_primitives(..., box_a=...)``.
        ``cells`` (keyword-only, additive): the same with one triclinic cell (3 x 3) for all structures, or one per structure."""
        if boxes is not None and cells is not None:
            raise ValueError("boxes and cells were both given: a batch is periodic in boxes or in cells")
        if boxes is not None:  # (checked before anything touches a device)
            self._no_device_group_with_box()
            boxes = periodic_boxes(boxes, len(structures), float(threshold_distance), "boxes")
        if cells is not None:
            self._no_device_group_with_box()
            cells = periodic_cells(cells, len(structures), float(threshold_distance), "cells")
        from .device import DeviceSession  # torch is only needed on this path

        if isinstance(self._w_func, dict):
            raise ValueError("from_primitives_batch needs a single weight function (no per-pair keys)")
        interner: Dict[str, int] = {}
        packed = [self.pack(st, interner) for st in structures]
        sizes = [len(pk.cat) for pk in packed]
        flat, spans = [], []
        offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        for a, b, pairs in jobs:
            if not (0 <= int(a) < len(packed) and 0 <= int(b) < len(packed)):
                raise IndexError(f"job refers to structure {a} / {b} of {len(packed)}")
            pr = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
            if len(pr) and (pr.min() < 0 or pr[:, 0].max() >= sizes[int(a)] or pr[:, 1].max() >= sizes[int(b)]):
                raise N.PanicException("index out of bounds: an anchor index is outside its structure (src/locohd.rs:521)")
            spans.append((len(flat), len(pr)))
            flat.extend([pr + np.asarray([offsets[int(a)], offsets[int(b)]], dtype=np.int64)] if len(pr) else [])
        total = sum(n for _, n in spans)
        if total == 0:
            return [[] for _ in jobs]
        sess = DeviceSession(self, device=None if self._device < 0 else self._device, interner=interner)
        try:
            torch = sess.torch
            batch, _ = sess.upload_batch([(pk.xyz, pk.cat, pk.tag) for pk in packed])
            if boxes is not None:
                batch = sess.periodic_images(batch, boxes, float(threshold_distance))
            if cells is not None:
                batch = sess.periodic_images(batch, reach=float(threshold_distance), cell=cells)
            anchors = torch.from_numpy(np.concatenate(flat)).to(torch.device("cuda", sess.device))
            scores = sess.from_primitives(batch, batch, anchors, float(threshold_distance)).cpu().numpy()
        finally:
            sess.close()
        out, pos = [], 0
        for _, n in spans:
            out.append(scores[pos:pos + n].tolist())
            pos += n
        return out

    # ---- additive array-level entry (no per-atom Python objects; used by bench.py and batch callers) --------
    def pack(self, prims: Sequence[PrimitiveAtom], interner: Optional[Dict[str, int]] = None) -> _Packed:
        interner = {} if interner is None else interner
        n = len(prims)
        if _fastpack is not None:  # native extraction (what PyO3 does for the reference), same results as the loop below
            xyz, cat, tag = np.empty((n, 3), dtype=np.float64), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
            _fastpack.pack_into(prims, self._categories, interner, xyz, cat, tag)
            return _Packed(xyz, cat, tag)
        xyz = np.array([p._coordinates if type(p) is PrimitiveAtom else p.coordinates for p in prims], dtype=np.float64).reshape(n, 3)
        cat = self._cats([p.primitive_type for p in prims])
        intern = interner.setdefault
        tag = np.fromiter((intern(p.tag, len(interner)) for p in prims), dtype=np.int32, count=n)
        return _Packed(xyz, cat, tag)

    def from_packed(self, pa: _Packed, pb: _Packed, pairs, threshold_distance: float, wf_index: Optional[np.ndarray] = None,
                    interner: Optional[Dict[str, int]] = None) -> np.ndarray:
        anchors = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        cfg, keep = self._config(interner)
        out = np.empty(len(anchors))
        if len(anchors) == 0:
            return out
        xa, xb = _f64(pa.xyz).reshape(-1, 3), _f64(pb.xyz).reshape(-1, 3)
        if self._devices is not None and len(self._devices) > 1:  # the instance's device group (the reference: its thread pool)
            N.check(N.lib().lchd_group_from_primitives(self._device_group(), C.byref(cfg), N.dp(xa), N.ip(pa.cat), N.ip(pa.tag), len(xa),
                                                       N.dp(xb), N.ip(pb.cat), N.ip(pb.tag), len(xb), N.lp(anchors), N.ip(wf_index),
                                                       len(anchors), float(threshold_distance), N.dp(out)))
            return out
        N.check(N.lib().lchd_from_primitives(self._context(), C.byref(cfg), N.dp(xa), N.ip(pa.cat), N.ip(pa.tag), len(xa),
                                             N.dp(xb), N.ip(pb.cat), N.ip(pb.tag), len(xb), N.lp(anchors), N.ip(wf_index),
                                             len(anchors), float(threshold_distance), N.dp(out)))
        return out

    # ---- argument conversion helpers ------------------------------------------------------------------------
    @staticmethod
    def _matrix(m):
        """Vec<Vec<f64>> -> (rectangular f64 matrix, row lengths or None).  Ragged rows (the reference sorts each row with a
        prefix of seq, utils.rs:25-39) are padded and travel with their lengths (lchd_from_dmxs_ragged)."""
        lens = None
        try:
            arr = _f64(m)
        except ValueError:
            rows = [_f64(r).reshape(-1) for r in m]
            width = max((len(r) for r in rows), default=0)
            if any(len(r) == 0 for r in rows):
                raise N.PanicException("index out of bounds: empty distance row (src/locohd.rs:74)")
            arr = np.zeros((len(rows), width))
            for k, r in enumerate(rows):
                arr[k, : len(r)] = r
            lens = np.asarray([len(r) for r in rows], dtype=np.int32)
        if arr.ndim == 1 and arr.size == 0:
            arr = arr.reshape(0, 0)
        if arr.ndim != 2:
            raise TypeError("a distance matrix must be a 2-D sequence of floats")
        return arr, lens

    @staticmethod
    def _coords(x) -> np.ndarray:
        arr = _f64(x)
        if arr.size == 0:
            return arr.reshape(0, 3)
        if arr.ndim != 2 or arr.shape[1] != 3:
            raise TypeError("coordinates must be a sequence of [x, y, z] triples")
        return arr

    @staticmethod
    def _split_anchor_pairs(anchor_pairs) -> Tuple[List[Tuple[int, int]], Optional[List[str]]]:
        """AnchorPairSpecifier (src/locohd.rs:34-40): 3-tuples are tried first, so an EMPTY list is the
        with-key variant (and then fails against a single weight function, :276-281)."""
        ap = list(anchor_pairs)
        if len(ap) == 0 or all(len(p) == 3 for p in ap):
            pairs, keys = [(int(p[0]), int(p[1])) for p in ap], [str(p[2]) for p in ap]
        elif all(len(p) == 2 for p in ap):
            pairs, keys = [(int(p[0]), int(p[1])) for p in ap], None
        else:
            raise TypeError("failed to extract enum AnchorPairSpecifier ('WithWeightFunctionKey | WithoutWeightFunctionKey')")
        if any(a < 0 or b < 0 for a, b in pairs):
            raise OverflowError("can't convert negative int to unsigned")
        return pairs, keys
