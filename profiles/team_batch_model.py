"""CPU model of the team sweep's wave-uniform trip counts: how many event-loop trips and staging rounds a wavefront of k_sweep_duo
issues per iteration when its teams are (a) the consecutive pairs of the list, (b) the pairs of a batch of 16 / 32 / 64 consecutive
pairs sorted by chunk length, (c) alone.  numpy only; the workloads are bench.py's (C2a: 10^6 pairs, two teams of 32 lanes, tile 480;
C3: 1.225 * 10^6 pairs, four teams of 16 lanes, tile 240).  Environment sizes are brute-force counts (anchor included).

    python3 profiles/team_batch_model.py

epl  = ceil(T / TL), T = n_A + n_B - 2 merged events: the event loop runs max(epl) over the wavefront's teams
epl2 = ceil((((n_A - 1) + 1) & ~1) + (n_B - 1)) / (2 TL)): staging rounds, likewise the maximum
Pairs the kernel does not sweep (more events than the tile, an environment beyond 255 points in the 480 form) count as 0, like the
sort key of k_sweep_duo; an iteration whose teams are all 0 is skipped and not counted."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import bench  # noqa: E402


def env_sizes(xyz, thr, anchors, tag=None):
    """points within thr of every anchor, the anchor included; with tags: atoms of the anchor's own tag excluded (accept_same=False)"""
    out = np.empty(len(anchors), dtype=np.int64)
    for s in range(0, len(anchors), 500):
        a = anchors[s:s + 500]
        d2 = ((xyz[a, None, :] - xyz[None, :, :]) ** 2).sum(-1)
        near = d2 <= thr * thr
        if tag is not None:
            near &= tag[a, None] != tag[None, :]
            out[s:s + 500] = near.sum(1) + 1
        else:
            out[s:s + 500] = near.sum(1)
    return out


def trips(na, nb, tl, tile, teams, c8):
    """-> rows (label, event-loop trips per iteration, staging rounds per iteration, iterations)"""
    t = na + nb - 2
    mine = t <= tile
    if c8:
        mine &= np.maximum(na, nb) <= 255
    epl = np.where(mine, -(-t // tl), 0)
    tb = ((na - 1 + 1) & ~1) + (nb - 1)
    epl2 = np.where(mine, -(-tb // (2 * tl)), 0)

    def per_iteration(e, e2):
        pad = (-len(e)) % teams
        e, e2 = np.concatenate([e, np.zeros(pad, e.dtype)]), np.concatenate([e2, np.zeros(pad, e2.dtype)])
        w, w2 = e.reshape(-1, teams).max(1), e2.reshape(-1, teams).max(1)
        run = w2 > 0  # (a swept pair has at least the pad entry to stage; an iteration of zeros is skipped)
        return w[run].mean(), w2[run].mean(), int(run.sum())

    rows = [("pairs p, p+1, ..: today", *per_iteration(epl, epl2))]
    for kb in (16, 32, 64):
        pad = (-len(epl)) % kb
        e = np.concatenate([epl, np.zeros(pad, epl.dtype)]).reshape(-1, kb)
        e2 = np.concatenate([epl2, np.zeros(pad, epl2.dtype)]).reshape(-1, kb)
        order = np.argsort(e, axis=1, kind="stable")
        rows.append((f"sorted by epl inside {kb}", *per_iteration(np.take_along_axis(e, order, 1).ravel(), np.take_along_axis(e2, order, 1).ravel())))
    n = int(mine.sum())
    rows.append(("every team alone", epl[mine].mean(), epl2[mine].mean(), -(-n // teams)))
    return rows, (t[mine].mean(), t[mine].std(), epl[mine].min(), epl[mine].max(), n)


def report(name, na, nb, tl, tile, teams, c8):
    rows, (tm, ts, e0, e1, n) = trips(na, nb, tl, tile, teams, c8)
    print(f"{name}: {len(na)} pairs, {n} swept by the team kernel ({teams} teams of {tl} lanes, tile {tile}); environments "
          f"{np.concatenate([na, nb]).mean():.0f} +- {np.concatenate([na, nb]).std():.0f} ({min(na.min(), nb.min())} .. {max(na.max(), nb.max())}), "
          f"T = {tm:.0f} +- {ts:.0f}, epl {e0} .. {e1}")
    base = rows[0]
    for label, w, w2, it in rows:
        print(f"  {label:28s} trips {w:6.2f} ({100 * (w / base[1] - 1):+5.1f} %)   staging rounds {w2:5.2f} ({100 * (w2 / base[2] - 1):+5.1f} %)   iterations {it}")


def main():
    w = bench.make_workload("c2a", 0, 10**6)
    idx = np.arange(len(w["xyz_a"]))
    sa, sb = env_sizes(w["xyz_a"], w["thr"], idx), env_sizes(w["xyz_b"], w["thr"], idx)
    report("C2a", sa[w["pairs"][:, 0]], sb[w["pairs"][:, 1]], 32, 480, 2, True)

    c3 = bench.make_c3(0, True)
    la = np.arange(0, c3["n"], 3)
    sizes = [env_sizes(xyz, c3["thr"], la, tag) for xyz, _, tag in c3["decoys"]]
    na = np.concatenate([sizes[a] for a, b in c3["spairs"]])
    nb = np.concatenate([sizes[b] for a, b in c3["spairs"]])
    report("C3", na, nb, 16, 240, 4, False)


if __name__ == "__main__":
    main()
