"""DeviceSession.weight_gradient(_coords), set_weight_function and loco_hd_amd.autograd.locohd_scores_wf: the session calls against the
host-array methods bit for bit, the parameters a session keeps against a fresh LoCoHD, backward against (grad * v[:, None]).sum(0) of
the session's own rows (which tests/test_gpu_weight_gradient.py pins to the restatement) and against the restatement itself, and a
descent on (a, b) of a uniform function that has to lower its loss."""
import numpy as np
import pytest

import weight_gradient_util as wg

pytestmark = pytest.mark.gpu

CATS7 = [f"c{k}" for k in range(7)]


def _case(seed=61, n=200, n_pairs=24):
    rng = np.random.default_rng(seed)
    xa, xb = rng.uniform(0.0, 16.0, (n, 3)), rng.uniform(0.0, 16.0, (n, 3))
    ca, cb = rng.integers(0, 7, n), rng.integers(0, 7, n)
    return xa, xb, ca, cb, rng.integers(0, n, (n_pairs, 2)), rng.uniform(-1.0, 1.0, n_pairs)


def _atoms(lh, types, xyz):
    return [lh.PrimitiveAtom(CATS7[k], "x", list(x)) for k, x in zip(types, xyz)]


@pytest.mark.parametrize("wf", [("uniform", [3.0, 10.0]), ("kumaraswamy", [2.0, 11.0, 2.0, 3.0])])
def test_session_calls_are_the_host_array_calls_and_keep_the_parameters_set(wf):
    import torch

    import loco_hd_amd as lh
    from loco_hd_amd.device import DeviceSession

    xa, xb, ca, cb, pairs, _ = _case()
    sd = lh.StatisticalDistance("Kullback-Leibler", [1e-3])
    host = lh.LoCoHD(CATS7, lh.WeightFunction(*wf), statistical_distance=sd)
    pa, pb, plist = _atoms(lh, ca, xa), _atoms(lh, cb, xb), [(int(i), int(j)) for i, j in pairs]
    sess = DeviceSession(host)
    try:
        cloud_a, cloud_b = sess.upload(xa, ca.astype(np.int32)), sess.upload(xb, cb.astype(np.int32))
        anchors = torch.from_numpy(pairs).cuda()
        got, want = sess.weight_gradient(cloud_a, cloud_b, anchors, 8.0), host.weight_gradient_from_primitives(pa, pb, plist, 8.0)
        assert got.grad.shape == (24, len(wf[1])) and got.scores.shape == (24,)
        assert got.grad.cpu().numpy().tobytes() == want.grad.tobytes() and got.scores.cpu().numpy().tobytes() == want.scores.tobytes()
        seq_a, seq_b = [CATS7[k] for k in ca], [CATS7[k] for k in cb]
        got, want = sess.weight_gradient_coords(cloud_a, cloud_b), host.weight_gradient_from_coords(seq_a, seq_b, xa, xb)
        assert got.grad.cpu().numpy().tobytes() == want.grad.tobytes() and got.scores.cpu().numpy().tobytes() == want.scores.tobytes()
        # other parameters: the session against a fresh LoCoHD with them; the uploaded clouds stay valid
        other = [p * f for p, f in zip(wf[1], (1.25, 0.9, 1.1, 0.8))]
        sess.set_weight_function(other)
        fresh = lh.LoCoHD(CATS7, lh.WeightFunction(wf[0], other), statistical_distance=sd)
        got, want = sess.weight_gradient(cloud_a, cloud_b, anchors, 8.0), fresh.weight_gradient_from_primitives(pa, pb, plist, 8.0)
        assert got.grad.cpu().numpy().tobytes() == want.grad.tobytes() and got.scores.cpu().numpy().tobytes() == want.scores.tobytes()
        assert sess.from_primitives(cloud_a, cloud_b, anchors, 8.0).cpu().numpy().tolist() == list(fresh.from_primitives(pa, pb, plist, 8.0))
        assert host.w_func.parameters == wf[1]  # (the LoCoHD object keeps its own)
    finally:
        sess.close()


def test_backward_is_the_weighted_sum_of_the_rows():
    import torch

    import loco_hd_amd as lh
    from loco_hd_amd.autograd import locohd_scores_wf
    from loco_hd_amd.device import DeviceSession

    xa, xb, ca, cb, pairs, v = _case()
    wf = ("dagum", [4.0, 6.0, 1.5])
    sess = DeviceSession(lh.LoCoHD(CATS7, lh.WeightFunction("dagum", [3.0, 5.0, 1.0])))  # (other parameters until forward sets these)
    try:
        cloud_a, cloud_b = sess.upload(xa, ca.astype(np.int32)), sess.upload(xb, cb.astype(np.int32))
        anchors = torch.from_numpy(pairs).cuda()
        theta = torch.tensor(wf[1], dtype=torch.float64, requires_grad=True)
        scores = locohd_scores_wf(sess, cloud_a, cloud_b, anchors, 8.0, theta)
        (scores * torch.from_numpy(v).to(scores.device)).sum().backward()
        rows = sess.weight_gradient(cloud_a, cloud_b, anchors, 8.0).grad
        want = (rows * torch.from_numpy(v).to(rows.device)[:, None]).sum(0)  # (the same expression on the same device: the same bits)
        assert theta.grad.shape == (3,) and theta.grad.tolist() == want.cpu().tolist()
        s_want, g_want = wg.from_primitives(ca, xa, None, cb, xb, None, pairs, 8.0, 7, wf)
        err = float(np.max(np.abs(theta.grad.numpy().astype(np.longdouble) - (g_want * v[:, None]).sum(0)) * np.asarray(wf[1])))
        print(f"max |theta (backward - restated)| = {err:.3g}")
        assert err <= 24 * 1e-11 and float(np.max(np.abs(scores.detach().cpu().numpy() - s_want))) <= 1e-11
    finally:
        sess.close()


def test_twenty_steps_of_descent_on_a_uniform_range_lower_the_loss():
    import torch

    import loco_hd_amd as lh
    from loco_hd_amd.autograd import locohd_scores_wf
    from loco_hd_amd.device import DeviceSession

    xa, xb, ca, cb, pairs, _ = _case(n_pairs=40)
    sess = DeviceSession(lh.LoCoHD(CATS7, lh.WeightFunction("uniform", [2.0, 7.0])))
    try:
        cloud_a, cloud_b = sess.upload(xa, ca.astype(np.int32)), sess.upload(xb, cb.astype(np.int32))
        anchors = torch.from_numpy(pairs).cuda()
        target = locohd_scores_wf(sess, cloud_a, cloud_b, anchors, 8.0, torch.tensor([2.0, 7.0], dtype=torch.float64)).detach()
        theta = torch.tensor([3.0, 6.0], dtype=torch.float64, requires_grad=True)
        losses = []
        for _ in range(21):
            loss = ((locohd_scores_wf(sess, cloud_a, cloud_b, anchors, 8.0, theta) - target) ** 2).sum()
            losses.append(float(loss.detach()))
            theta.grad = None
            loss.backward()
            with torch.no_grad():
                theta -= 2.0 * theta.grad
        print("loss:", " ".join(f"{x:.3g}" for x in losses), "theta:", theta.tolist())
        assert losses[0] > 0.0 and losses[-1] < 0.5 * losses[0]
    finally:
        sess.close()
