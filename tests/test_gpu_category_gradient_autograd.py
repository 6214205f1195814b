"""loco_hd_amd.autograd.locohd_scores_weighted: backward against the numpy restatement of the category-weight gradient
(tests/category_gradient_util.py, longdouble) -- not against differences of its own forward -- and the session's weights afterwards
against the CPU oracle.  Bound: the project's parity bound, 1e-11, on scores and on the log-weight form w_c * dL/dw_c with |v_p| <= 1
(a sum over P pairs of terms that each meet it: P * 1e-11)."""
import numpy as np
import pytest

import category_gradient_util as cg

pytestmark = pytest.mark.gpu

CATS7 = [f"c{k}" for k in range(7)]
UNI = ("uniform", [3.0, 10.0])


@pytest.mark.parametrize("distance", [("Hellinger", 2.0), ("Hellinger", 3.5), ("Kullback-Leibler", 1e-3)])
def test_backward_is_the_restated_gradient_and_the_session_keeps_the_weights(oracle, distance):
    import torch

    import loco_hd_amd as lh
    from loco_hd_amd.autograd import locohd_scores_weighted
    from loco_hd_amd.device import DeviceSession

    rng = np.random.default_rng(61)
    n, n_pairs = 200, 24
    xa, xb = rng.uniform(0.0, 16.0, (n, 3)), rng.uniform(0.0, 16.0, (n, 3))
    ca, cb = rng.integers(0, 7, n), rng.integers(0, 7, n)
    pairs = rng.integers(0, n, (n_pairs, 2))
    w = rng.uniform(0.3, 3.0, 7)
    v = rng.uniform(-1.0, 1.0, n_pairs)
    sd = lh.StatisticalDistance(distance[0], [distance[1]])
    sess = DeviceSession(lh.LoCoHD(CATS7, lh.WeightFunction(*UNI), statistical_distance=sd))  # (unit weights until forward sets others)
    try:
        cloud_a, cloud_b = sess.upload(xa, ca.astype(np.int32)), sess.upload(xb, cb.astype(np.int32))
        anchors = torch.from_numpy(pairs).cuda()
        weights = torch.tensor(w, dtype=torch.float64, requires_grad=True)
        scores = locohd_scores_weighted(sess, cloud_a, cloud_b, anchors, 8.0, weights)
        (scores * torch.from_numpy(v).to(scores.device)).sum().backward()
        want_log = (cg.from_primitives(ca, xa, None, cb, xb, None, pairs, 8.0, 7, UNI, distance, w) * v[:, None].astype(np.longdouble)).sum(0)
        err = float(np.max(np.abs(weights.grad.numpy().astype(np.longdouble) * w - want_log)))
        print(f"{distance}: max |w (backward - restated)| = {err:.3g}")
        assert weights.grad.shape == (7,) and err <= n_pairs * 1e-11

        def atoms(types, xyz):
            return [oracle.PrimitiveAtom(CATS7[k], "x", list(x)) for k, x in zip(types, xyz)]

        ref = oracle.LoCoHD(CATS7, oracle.WeightFunction(*UNI), category_weights=list(w),
                            statistical_distance=oracle.StatisticalDistance(distance[0], [distance[1]]))
        want = np.asarray(ref.from_primitives(atoms(ca, xa), atoms(cb, xb), [(int(i), int(j)) for i, j in pairs], 8.0))
        assert float(np.max(np.abs(scores.detach().cpu().numpy() - want))) <= 1e-11
        again = sess.from_primitives(cloud_a, cloud_b, anchors, 8.0)  # the session scores with the weights of the call
        assert float(np.max(np.abs(again.cpu().numpy() - want))) <= 1e-11
    finally:
        sess.close()
