"""The rows of the four per-pair profile kernels (radial profiles, score attribution, category-weight gradients, neighbour
sensitivities), bit for bit against a recording: tests/golden/profile_kernel_bits.npz holds what every instantiation returned for one
fixed case before the kernels were moved onto the shared column-tile skeleton (loco_hd_amd/csrc/lchd_pair_columns.h).  The kernels sum
in a fixed shape without atomics, so a stored pair has one answer; a change of these bytes is a change of evaluation order.

The recording names the toolchain it was made with (`rocm`): the library's pow / log are part of the bytes of the general-exponent and
Kullback-Leibler rows.  Re-record with `python tests/test_gpu_profile_bits.py tests/golden/profile_kernel_bits.npz` on an MI355X."""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "profile_kernel_bits.npz"
CATS = [f"c{k}" for k in range(7)]
N_ATOMS, N_PAIRS, EDGE, THR = 60, 24, 12.0, 6.0
EDGES = [0.0, 1.5, 3.0, 4.0, 5.0, 5.5, 6.0, float("inf")]
WF = ("hyper_exp", [1.0, 0.5, 0.2, 0.05])


def _case(lh):
    rng = np.random.default_rng(20260)
    clouds = []
    for _ in range(2):
        xyz = np.round(rng.uniform(0.0, EDGE, (N_ATOMS, 3)), 1)  # one decimal: exact ties within and across the sides
        cat = rng.integers(0, len(CATS), N_ATOMS)
        clouds.append([lh.PrimitiveAtom(CATS[k], f"t{t}", list(x)) for k, t, x in zip(cat, rng.integers(0, 3, N_ATOMS), xyz)])
    pairs = [(int(i), int(j)) for i, j in rng.integers(0, N_ATOMS, (N_PAIRS, 2))]
    weights = list(rng.uniform(0.3, 3.0, len(CATS)))
    return clouds[0], clouds[1], pairs, weights


def compute(lh):
    """name -> array, one entry per instantiation (the fields of a sensitivity call one entry each)."""
    a, b, pairs, weights = _case(lh)

    def l(distance, params, w=None):
        return lh.LoCoHD(CATS, lh.WeightFunction(*WF), category_weights=w, statistical_distance=lh.StatisticalDistance(distance, params))

    out = {
        "attribution_h2u": l("Hellinger", [2.0]).attribution_from_primitives(a, b, pairs, THR),
        "attribution_h2w": l("Hellinger", [2.0], weights).attribution_from_primitives(a, b, pairs, THR),
        "attribution_pow": l("Hellinger", [3.5], weights).attribution_from_primitives(a, b, pairs, THR),
        "category_gradient_h2": l("Hellinger", [2.0], weights).category_gradient_from_primitives(a, b, pairs, THR),
        "category_gradient_pow": l("Hellinger", [3.5], weights).category_gradient_from_primitives(a, b, pairs, THR),
        "category_gradient_kl": l("Kullback-Leibler", [1e-3], weights).category_gradient_from_primitives(a, b, pairs, THR),
        "radial_h2u": l("Hellinger", [2.0]).radial_from_primitives(a, b, pairs, THR, EDGES),
        "radial_ks": l("Kolmogorov-Smirnov", [], weights).radial_from_primitives(a, b, pairs, THR, EDGES),
    }
    for name, loc in (("sensitivity_h2", l("Hellinger", [2.0])), ("sensitivity_kl", l("Kullback-Leibler", [1e-3], weights))):
        s = loc.sensitivity_from_primitives(a, b, pairs, THR)
        for field in s._fields:
            out[f"{name}_{field}"] = getattr(s, field)
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


@pytest.fixture(scope="module")
def computed():
    import loco_hd_amd as lh

    return compute(lh)


@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


MODES = ["attribution_h2u", "attribution_h2w", "attribution_pow", "category_gradient_h2", "category_gradient_pow", "category_gradient_kl",
         "radial_h2u", "radial_ks", "sensitivity_h2", "sensitivity_kl"]


@pytest.mark.parametrize("mode", MODES)
def test_rows_are_the_recorded_bytes(computed, recorded, mode):
    names = sorted(k for k in recorded if k == mode or k.startswith(mode + "_"))
    assert names and names == sorted(k for k in computed if k == mode or k.startswith(mode + "_"))
    for name in names:
        got, want = computed[name], recorded[name]
        assert got.shape == want.shape and got.dtype == want.dtype, name
        assert np.array_equal(got.reshape(-1).view(np.uint8), want.reshape(-1).view(np.uint8)), f"{name} (recorded under ROCm {recorded['rocm']})"
    if not mode.startswith("sensitivity"):
        assert np.isfinite(computed[mode]).all() and np.any(computed[mode] != 0.0)  # (the case exercises the kernel: no refused rows)


if __name__ == "__main__":
    import torch

    import loco_hd_amd

    arrays = compute(loco_hd_amd)
    np.savez_compressed(sys.argv[1], rocm=np.asarray(str(torch.version.hip)), **arrays)
    print({k: (v.shape, str(v.dtype)) for k, v in arrays.items()}, Path(sys.argv[1]).stat().st_size, "bytes")
