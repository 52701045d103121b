#!/usr/bin/env python3
"""Merge-time importance: the kernel route (a forward + gsr_importance_accumulate per view) against the autograd route (a render and
a full backward per view) of hierarchy.calc_importance, timed in ONE process.

After a warm-up of both routes the two arms alternate -- A, B, A, B, ... -- for `--rounds` rounds (at least 20); a host clock around
a device synchronise.  Per size the median and the min-max of each arm are printed, and the spread of ONE arm against itself: the
difference of the medians of its odd and its even rounds.  The kernel route is "faster" only when its median lies below the autograd
route's by more than that same-arm spread (the larger of the two arms'); hierarchy.DEFAULT_IMPORTANCE_ROUTE may be "kernel" only if
that holds at BOTH sizes.  The two new kernels' own times come from the library's profile stages in a separate pass.

Sizes: bench.py's headline scene (1 M Gaussians, 980x545, SH degree 3, 8 views) and stage A's (130 k Gaussians, SH degree 0 with 16
coefficients stored, 8 views).

    python tools/importance_probe.py > profiles/importance_probe.txt
"""
import argparse
import ctypes as C
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

# (name, N, W, H, degree, seed, brightened).  The plain synthetic scenes are dark on a black background: nearly every pixel has its
# three gates open and the walk takes its one-sum path; the brightened arms (DC colour 2 dc + 1.5, background (0.2, 0.5, 0.9), as in
# tests/importance_common.py: 25-30 % of the gates closed, over half of the pixels with differing gates) time the three-sum path.
SIZES = [("headline 1M/980x545/deg3", 1_000_000, 980, 545, 3, 0, False), ("stage A 130k/980x545/deg0 (16 stored)", 130_000, 980, 545, 0, 3, False),
         ("headline, brightened", 1_000_000, 980, 545, 3, 0, True), ("stage A, brightened", 130_000, 980, 545, 0, 3, True)]


def build(N, W, H, deg, seed, n_views, dev, bright=False):
    scene = syn.make_scene(N, W, H, sh_degree=deg, seed=seed)
    bg = None
    if bright:
        scene["shs"][:, 0] = 2.0 * scene["shs"][:, 0] + 1.5
        bg = torch.tensor([0.2, 0.5, 0.9])
    views = [ts.make_settings(scene, dev, deg, bg=bg)]
    for v in range(1, n_views):
        cam = syn.make_scene(8, W, H, sh_degree=deg, seed=76 + v, posed=True)        # only its camera is used
        sc = dict(scene)
        for k in ("viewmatrix", "projmatrix", "campos"):
            sc[k] = cam[k]
        views.append(ts.make_settings(sc, dev, deg, bg=bg))
    p = ts.GaussianParams(scene, dev, optimizer="torch")
    seg = {k: getattr(p, k).detach() for k in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")}
    return seg, views


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return 1e3 * (time.perf_counter() - t0)


def arm_stats(x):
    odd, even = x[0::2], x[1::2]
    return statistics.median(x), min(x), max(x), abs(statistics.median(odd) - statistics.median(even))


def stage(lib, name):
    tot, cnt = C.c_double(0), C.c_int64(0)
    lib.gsr_profile_read(name.encode(), C.byref(tot), C.byref(cnt))
    return tot.value, int(cnt.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    rounds = max(20, args.rounds)
    dev = torch.device("cuda:0")
    lib = L.load()
    print(f"importance_probe: {torch.cuda.get_device_name(dev)}, rounds {rounds}, views {args.views}, library version {lib.gsr_version()}")
    verdicts = []
    R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    for name, N, W, H, deg, seed, bright in SIZES:
        seg, views = build(N, W, H, deg, seed, args.views, dev, bright)
        with torch.no_grad():      # what the gates look like on this scene (first view): which path of the walk is timed
            m2d = torch.zeros_like(seg["_xyz"])
            c = R.rasterize_gaussians_raw(seg["_xyz"], m2d, seg["_features_dc"], seg["_features_rest"], seg["_opacity"], seg["_scaling"],
                                          seg["_rotation"], views[0])[0]
            g = (c >= 0) & (c <= 1)
            Hp, Wp = (H + 7) // 8 * 8, (W + 7) // 8 * 8
            same = torch.ones(Hp, Wp, dtype=torch.bool, device=dev)
            same[:H, :W] = (g[0] == g[1]) & (g[1] == g[2])
            uni = same.view(Hp // 8, 8, Wp // 8, 8).permute(0, 2, 1, 3).reshape(-1, 64).all(1).float().mean().item()
            closed = 1.0 - g.float().mean().item()
        gate_note = f"closed gate elements {closed:.3f}, 8x8 blocks whose pixels' three gates agree (one-sum path) {uni:.3f}"
        arms = {"kernel": lambda: hier.calc_importance(seg, views, route="kernel"),
                "autograd": lambda: hier.calc_importance(seg, views, route="autograd")}
        for _ in range(args.warmup):
            for fn in arms.values():
                fn()
        t = {"kernel": [], "autograd": []}
        for _ in range(rounds):
            for k in ("kernel", "autograd"):                      # A, B, A, B, ...
                t[k].append(timed(arms[k], dev))
        st = {k: arm_stats(v) for k, v in t.items()}
        print(f"\n{name}: {args.views} views per call, ms per call   [{gate_note}]")
        for k in ("kernel", "autograd"):
            med, lo, hi, spread = st[k]
            print(f"  {k:9s} median {med:8.3f}   min {lo:8.3f}   max {hi:8.3f}   odd/even rounds' medians differ by {spread:.3f}")
        spread = max(st["kernel"][3], st["autograd"][3])
        faster = st["kernel"][0] < st["autograd"][0] - spread
        verdicts.append(faster)
        print(f"  kernel - autograd = {st['kernel'][0] - st['autograd'][0]:+.3f} ms; same-arm spread {spread:.3f} ms -> kernel route "
              f"{'FASTER' if faster else 'NOT faster'} at this size")
        # the two kernels' own times (profile stages; a pass of its own: the event records sit in the stream)
        lib.gsr_set_option(b"profile", 1)
        try:
            for s in ("importance_blend", "importance_finish", "blend_fwd"):
                stage(lib, s)
            for _ in range(3):
                arms["kernel"]()
            torch.cuda.synchronize(dev)
            for s in ("importance_blend", "importance_finish", "blend_fwd"):
                tot, cnt = stage(lib, s)
                print(f"  stage {s:18s} {1e3 * tot / max(cnt, 1):8.1f} us per view over {cnt} launches")
        finally:
            lib.gsr_set_option(b"profile", 0)
        del seg, views, arms
        torch.cuda.empty_cache()
    print(f"\nrule: DEFAULT_IMPORTANCE_ROUTE = \"kernel\" only if FASTER at both sizes (here: on both gate patterns of both) -> {'kernel' if all(verdicts) else 'autograd'}"
          f"   (the tree has {hier.DEFAULT_IMPORTANCE_ROUTE!r})")


if __name__ == "__main__":
    main()
