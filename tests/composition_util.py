"""The local composition profile restated in numpy (test infrastructure).

    P_c = sum_k (F(d_{k+1}) - F(d_k)) * w_c n_c(k) / sum_c' w_c' n_c'(k),   d_n = +inf

for one environment sorted by distance.  tests/test_composition_model.py pins this restatement to the CPU oracle through the
total-variation identity  P_X = (F(inf) - F(0)) - score_TV(environment, a lone anchor of category X);  the GPU tests then use it
wherever a whole (anchors x categories) table is needed."""
import numpy as np


def profile(dists, cats, weights, cdf):
    """Profile of one environment: `dists` (the anchor's 0 included) and integer `cats` in any order, `weights` [C], `cdf` a callable
    on float64 arrays that takes +inf."""
    d = np.asarray(dists, dtype=np.float64)
    order = np.argsort(d, kind="stable")
    d, c = d[order], np.asarray(cats)[order]
    w = np.asarray(weights, dtype=np.float64)
    f = np.asarray(cdf(np.concatenate([d, [np.inf]])), dtype=np.float64)
    counts = np.cumsum(np.eye(len(w))[c], axis=0)          # n_c(k)
    pmf = counts * w
    pmf /= pmf.sum(axis=1, keepdims=True)
    return (np.diff(f)[:, None] * pmf).sum(axis=0)


def profiles_of_rows(dmx, cats, weights, cdfs):
    """One profile per distance row; `cdfs`: one callable, or one per row."""
    return np.stack([profile(row, cats, weights, cdfs[r] if isinstance(cdfs, (list, tuple)) else cdfs) for r, row in enumerate(dmx)])


def environment(xyz, tags, anchor, threshold, accept_same=True):
    """Indices of the thresholded environment of `anchor`: strict radius test on squared distances, the tag rule {"accept_same": ...}
    on every other atom, the anchor itself always."""
    x = np.asarray(xyz, dtype=np.float64)
    dx = x - x[anchor]
    d2 = dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1] + dx[:, 2] * dx[:, 2]
    t = np.asarray(tags)
    keep = (d2 < threshold * threshold) & ((t == t[anchor]) == bool(accept_same))
    keep[anchor] = True
    idx = np.flatnonzero(keep)
    return idx, np.sqrt(d2[idx])


def profiles_of_cloud(xyz, cats, tags, anchors, threshold, weights, cdfs, accept_same=True):
    """Table (len(anchors), C) of a thresholded call; `cdfs`: one callable, or one per anchor."""
    out = []
    for k, a in enumerate(anchors):
        idx, d = environment(xyz, tags, a, threshold, accept_same)
        out.append(profile(d, np.asarray(cats)[idx], weights, cdfs[k] if isinstance(cdfs, (list, tuple)) else cdfs))
    return np.stack(out)


def tv_identity(orc, categories, weights, w_func, seq, dists, key=None):
    """The oracle side of the identity for one environment: [(F(inf) - F(0)) - from_anchors(env, lone X) for X in categories] with
    the total-variation distance (Hellinger, exponent 1).  `w_func`: an oracle WeightFunction or a dict of them (`key` picks one)."""
    lchd = orc.LoCoHD(categories, w_func, category_weights=weights, statistical_distance=orc.StatisticalDistance("Hellinger", [1.0]))
    wf = w_func[key] if isinstance(w_func, dict) else w_func
    f0, finf = wf.integral_vec([0.0, np.inf])
    return np.asarray([(finf - f0) - lchd.from_anchors(list(seq), [x], list(dists), [0.0], key) for x in categories])
