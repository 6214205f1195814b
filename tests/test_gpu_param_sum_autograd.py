"""loco_hd_amd.autograd.locohd_scores_weighted / locohd_scores_wf with native=True: backward is one reduced call with grad_output as the
pair weights.  It must equal the model of tests/param_sum_util.py on the session's own per-pair rows bit for bit, leave the forward scores
unchanged, agree with the torch reduction (native=False) within the worst-case rounding of a P-term float64 sum,
P * 2^-52 * sum_p |v_p row[p][k]| per column, and restore the forward's weights when the session's were set to something else since."""
import numpy as np
import pytest

import gradient_native_util as gn
import param_sum_util as ps

pytestmark = pytest.mark.gpu

CATS5 = [f"c{k}" for k in range(5)]
CW = [1.0, 0.5, 2.0, 1.5, 0.75]
THETA = [3.0, 10.0]
THR = 10.0
P = 12


def _case(seed=7, n=40):
    rng = np.random.default_rng(seed)
    xa, xb = rng.uniform(0.0, 12.0, (n, 3)), rng.uniform(0.0, 12.0, (n, 3))
    ca, cb = rng.integers(0, 5, n).astype(np.int32), rng.integers(0, 5, n).astype(np.int32)
    return xa, xb, ca, cb, rng.integers(0, n, (P, 2)), rng.uniform(-1.0, 1.0, P)


def _session(weights, theta):
    import loco_hd_amd as lh
    from loco_hd_amd.device import DeviceSession

    return DeviceSession(lh.LoCoHD(CATS5, lh.WeightFunction("uniform", theta), category_weights=weights))


def _bound(rows, v):
    return P * 2.0 ** -52 * np.abs(rows * v[:, None]).sum(0)


def _check(param_grad, torch_grad, rows, v):
    want, flag = ps.param_sum(rows, v)
    assert flag == 0 and np.any(want != 0.0)
    assert gn.bits(param_grad).tolist() == gn.bits(want[0]).tolist()
    err, bound = np.abs(param_grad - torch_grad), _bound(rows, v)
    print("max |native - torch| / bound =", float(np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound)


def test_category_weights_backward():
    import torch

    from loco_hd_amd.autograd import locohd_scores_weighted

    xa, xb, ca, cb, pairs, v = _case()
    sess = _session([1.0] * 5, THETA)  # (other weights until forward sets these)
    try:
        a, b = sess.upload(xa, ca), sess.upload(xb, cb)
        anchors, vt = torch.from_numpy(pairs).cuda(), torch.from_numpy(v).cuda()
        grads, scores = {}, {}
        for native in (False, True):
            w = torch.tensor(CW, dtype=torch.float64, requires_grad=True)
            s = locohd_scores_weighted(sess, a, b, anchors, THR, w, native=native)
            scores[native] = s.detach().cpu().numpy()
            sess.set_category_weights([2.0, 1.0, 1.0, 1.0, 3.0])  # backward has to put the forward's weights back
            (s * vt).sum().backward()
            grads[native] = w.grad.numpy().copy()
        assert scores[True].tobytes() == scores[False].tobytes()
        assert scores[True].tobytes() == sess.from_primitives(a, b, anchors, THR).cpu().numpy().tobytes()  # (the session is left at CW)
        rows = sess.category_gradient(a, b, anchors, THR).cpu().numpy()
        _check(grads[True], grads[False], rows, v)
    finally:
        sess.close()


def test_weight_function_backward():
    import torch

    from loco_hd_amd.autograd import locohd_scores_wf

    xa, xb, ca, cb, pairs, v = _case()
    sess = _session(CW, [2.0, 8.0])  # (other parameters until forward sets these)
    try:
        a, b = sess.upload(xa, ca), sess.upload(xb, cb)
        anchors, vt = torch.from_numpy(pairs).cuda(), torch.from_numpy(v).cuda()
        grads, scores = {}, {}
        for native in (False, True):
            theta = torch.tensor(THETA, dtype=torch.float64, requires_grad=True)
            s = locohd_scores_wf(sess, a, b, anchors, THR, theta, native=native)
            scores[native] = s.detach().cpu().numpy()
            sess.set_weight_function([1.0, 6.0])  # backward has to put the forward's parameters back
            (s * vt).sum().backward()
            grads[native] = theta.grad.numpy().copy()
        assert scores[True].tobytes() == scores[False].tobytes()
        assert scores[True].tobytes() == sess.from_primitives(a, b, anchors, THR).cpu().numpy().tobytes()  # (the session is left at THETA)
        per = sess.weight_gradient(a, b, anchors, THR)
        _check(grads[True], grads[False], per.grad.cpu().numpy(), v)
    finally:
        sess.close()
