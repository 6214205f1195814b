"""CPU model of the team tile's merge-path search (merge_path / merge_path_fixed, loco_hd_amd/csrc/lchd_kcommon.h), numpy only.

    python3 profiles/merge_path_model.py

Lane tl of a team asks how many of the first d = min((tl + 1) epl, T) merged events come from list A (A first on ties).
  plain   `while (lo < hi)` bisection per lane; the wavefront runs until its slowest lane is done: trips = the maximum over its lanes,
          every trip with exec-mask bookkeeping
  fixed   pos = lo; for step = 2^k, 2^(k-1), .., 1: m = pos + step - 1; if (m < hi and A[m] <= B[d - 1 - m]) pos = m + 1 -- k from the
          widest window the wavefront's teams can have, min(mA, mB): trips = bits(max over teams of min(mA, mB)), no branch
Both give the same partition for every input (tests/test_merge_path_model.py).  main() counts the trips per iteration of k_sweep_duo for
bench.py's C2a and C3 environment sizes, teams co-scheduled like the kernel's batches (sorted by chunk length inside 16 / 32 pairs);
the keys are random, with ties."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def plain(A, B, d):
    """-> (i1, trips) of the bisection"""
    lo, hi, trips = max(0, d - len(B)), min(d, len(A)), 0
    while lo < hi:
        mid = (lo + hi) >> 1
        if A[mid] <= B[d - 1 - mid]:
            lo = mid + 1
        else:
            hi = mid
        trips += 1
    return lo, trips


def fixed_trips(wmax):
    return int(wmax).bit_length()


def fixed(A, B, d, wmax):
    """-> (i1, trips); wmax >= the window's width.  Reads stay inside [0, max(len - 1, 0)] of A and [0, len(B)] of B, like the kernel's"""
    lo, hi = max(0, d - len(B)), min(d, len(A))
    assert hi - lo <= wmax
    mcl, dm1, pos = max(hi - 1, 0), max(d - 1, 0), lo
    step = 1 << (fixed_trips(wmax) - 1) if wmax > 0 else 0
    trips = 0
    while step > 0:
        m = pos + step - 1
        mc = min(m, mcl)
        assert 0 <= mc <= max(len(A) - 1, 0) and 0 <= dm1 - mc <= len(B)
        a = A[mc] if mc < len(A) else 0
        b = B[dm1 - mc] if dm1 - mc < len(B) else 0
        if m < hi and a <= b:
            pos = m + 1
        step >>= 1
        trips += 1
    return pos, trips


def team_diagonals(mA, mB, tl):
    T = mA + mB
    epl = -(-T // tl)
    return [min(min(k * epl, T) + epl, T) for k in range(tl)]


def count(name, na, nb, tl, tile, teams, kb, c8, sample, rng):
    t = na + nb - 2
    mine = t <= tile
    if c8:
        mine &= np.maximum(na, nb) <= 255
    epl = np.where(mine, -(-t // tl), 0)
    n = len(epl) // kb * kb
    order = (np.argsort(epl[:n].reshape(-1, kb), axis=1, kind="stable") + np.arange(0, n, kb)[:, None]).reshape(-1, teams)
    order = order[(epl[order] > 0).any(1)]
    before, after = [], []
    for it in order[rng.choice(len(order), sample, replace=False)]:
        worst, wmax = 0, 0
        for p in it:
            if not mine[p]:
                continue
            mA, mB = int(na[p]) - 1, int(nb[p]) - 1
            A, B = np.sort(rng.integers(0, 4 * (mA + mB) + 1, mA)), np.sort(rng.integers(0, 4 * (mA + mB) + 1, mB))
            for d in team_diagonals(mA, mB, tl):
                i1, trips = plain(A, B, d)
                assert fixed(A, B, d, min(mA, mB))[0] == i1
                worst = max(worst, trips)
            wmax = max(wmax, min(mA, mB))
        before.append(worst)
        after.append(fixed_trips(wmax))
    print(f"{name}: {sample} iterations of {teams} teams of {tl} lanes (batches of {kb}): merge-path trips per iteration "
          f"plain {np.mean(before):.2f} (divergent exit), fixed {np.mean(after):.2f} (wave-uniform, no branch)")


def main():
    import bench
    from team_batch_model import env_sizes

    rng = np.random.default_rng(0)
    w = bench.make_workload("c2a", 0, 10**6)
    idx = np.arange(len(w["xyz_a"]))
    sa, sb = env_sizes(w["xyz_a"], w["thr"], idx), env_sizes(w["xyz_b"], w["thr"], idx)
    count("C2a", sa[w["pairs"][:, 0]], sb[w["pairs"][:, 1]], 32, 480, 2, 16, True, 2000, rng)
    c3 = bench.make_c3(0, True)
    la = np.arange(0, c3["n"], 3)
    sizes = [env_sizes(xyz, c3["thr"], la, tag) for xyz, _, tag in c3["decoys"]]
    na = np.concatenate([sizes[a] for a, b in c3["spairs"]])
    nb = np.concatenate([sizes[b] for a, b in c3["spairs"]])
    count("C3", na, nb, 16, 240, 4, 32, False, 2000, rng)


if __name__ == "__main__":
    main()
