#!/usr/bin/env python3
"""Merge-time importance: V views of a model in ONE launch chain (hierarchy.calc_importance(views_per_call=8): gsr_forward_views +
gsr_importance_accumulate_views) against a forward and a pass per view (views_per_call=1), timed in ONE process.

The rule, written down before the run: after a warm-up of both arms the two alternate -- A, B, A, B, ... -- for `--rounds` rounds (at
least 20); a host clock around a device synchronise.  Per case the median and the min-max of each arm are printed, the spread of ONE
arm against itself (the difference of the medians of its odd and its even rounds), and the peak allocation of each arm above what was
allocated before it ran.  The views route is "faster" at a case only where its median lies below the per-view route's by more than the
LARGER of the two same-arm spreads; anything else is "not faster", a loss included, and is recorded as such.  The defaults
(hierarchy.DEFAULT_IMPORTANCE_VIEWS, GSR_AUTOPATCH_IMPORTANCE_VIEWS, run_segments' --importance-views-per-call) stay 1 whatever this
prints: changing them is a decision of its own that cites the recorded output.

Cases: eight views at 980x545 on bench.py's headline scene (1 M Gaussians, SH degree 3) and on stage A's (130 k Gaussians, degree 0 with
16 coefficients stored), and the merge leg of `bench.py --full`: two views of 256x256 at both sizes.

    python tools/importance_views_probe.py > profiles/importance_views.txt
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
hier = importlib.import_module("3dgs_hierarchical_training_amd.hierarchy")
ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
syn = importlib.import_module("3dgs_hierarchical_training_amd.synthetic")
L = importlib.import_module("3dgs_hierarchical_training_amd._lib")

# (name, N, W, H, degree, seed, views)
CASES = [("headline 1M/980x545/deg3, 8 views", 1_000_000, 980, 545, 3, 0, 8),
         ("stage A 130k/980x545/deg0 (16 stored), 8 views", 130_000, 980, 545, 0, 3, 8),
         ("merge leg 1M/256x256/deg3, 2 views", 1_000_000, 256, 256, 3, 0, 2),
         ("merge leg 130k/256x256/deg0 (16 stored), 2 views", 130_000, 256, 256, 0, 3, 2)]


def build(N, W, H, deg, seed, n_views, dev):
    """importance_probe.py's scenes; every view carries the SAME background tensor (group_views compares identities: no device read)."""
    scene = syn.make_scene(N, W, H, sh_degree=deg, seed=seed)
    bg = scene["bg"].to(dev).float()
    views = [ts.make_settings(scene, dev, deg)._replace(bg=bg)]
    for v in range(1, n_views):
        cam = syn.make_scene(8, W, H, sh_degree=deg, seed=76 + v, posed=True)        # only its camera is used
        sc = dict(scene)
        for k in ("viewmatrix", "projmatrix", "campos"):
            sc[k] = cam[k]
        views.append(ts.make_settings(sc, dev, deg)._replace(bg=bg))
    p = ts.GaussianParams(scene, dev, optimizer="torch")
    seg = {k: getattr(p, k).detach() for k in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")}
    return seg, views


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return 1e3 * (time.perf_counter() - t0)


def peak_mib(fn, dev):
    """Peak allocation of one call above what was allocated before it."""
    torch.cuda.synchronize(dev)
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    fn()
    torch.cuda.synchronize(dev)
    return (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20


def arm_stats(x):
    odd, even = x[0::2], x[1::2]
    return statistics.median(x), min(x), max(x), abs(statistics.median(odd) - statistics.median(even))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--per-call", type=int, default=8)
    args = ap.parse_args()
    rounds = max(20, args.rounds)
    dev = torch.device("cuda:0")
    lib = L.load()
    print(f"importance_views_probe: {torch.cuda.get_device_name(dev)}, rounds {rounds}, views per call {args.per_call} against 1, "
          f"library version {lib.gsr_version()}")
    print("rule: the views route is FASTER at a case only where its median lies below the per-view route's by more than the larger same-arm spread")
    verdicts = []
    for name, N, W, H, deg, seed, n_views in CASES:
        seg, views = build(N, W, H, deg, seed, n_views, dev)
        plan = [len(g) for g in hier.group_views(views, args.per_call, N)]
        arms = {"per-view": lambda: hier.calc_importance(seg, views, route="kernel", views_per_call=1),
                "views": lambda: hier.calc_importance(seg, views, route="kernel", views_per_call=args.per_call)}
        a, b = arms["per-view"](), arms["views"]()
        rel = float((a - b).abs().max()) / max(float(a.max()), 1e-30)
        del a, b
        for _ in range(args.warmup):
            for fn in arms.values():
                fn()
        t = {k: [] for k in arms}
        for _ in range(rounds):
            for k in ("per-view", "views"):                      # A, B, A, B, ...
                t[k].append(timed(arms[k], dev))
        st = {k: arm_stats(v) for k, v in t.items()}
        peaks = {k: peak_mib(arms[k], dev) for k in arms}
        print(f"\n{name}: ms per call; the views arm's call plan {plan}; max difference of the two results {rel:.2e} of the maximum")
        for k in ("per-view", "views"):
            med, lo, hi, spread = st[k]
            print(f"  {k:9s} median {med:8.3f}   min {lo:8.3f}   max {hi:8.3f}   odd/even rounds' medians differ by {spread:.3f}   "
                  f"peak allocation {peaks[k]:9.1f} MiB")
        spread = max(st["per-view"][3], st["views"][3])
        faster = st["views"][0] < st["per-view"][0] - spread
        verdicts.append((name, faster))
        print(f"  views - per-view = {st['views'][0] - st['per-view'][0]:+.3f} ms; larger same-arm spread {spread:.3f} ms -> views route "
              f"{'FASTER' if faster else 'NOT faster'} at this case")
        del seg, views, arms
        torch.cuda.empty_cache()
    print("\nsummary: " + "; ".join(f"{n}: {'faster' if f else 'not faster'}" for n, f in verdicts))
    print(f"the defaults stay 1 (the tree has hierarchy.DEFAULT_IMPORTANCE_VIEWS = {hier.DEFAULT_IMPORTANCE_VIEWS})")


if __name__ == "__main__":
    main()
