#!/usr/bin/env python3
"""Pose fit against a frozen model: 8 frames per launch chain (pose_fit.fit_poses(views_per_call=8): gsr_forward_views +
gsr_backward_views + gsr_pose_step_many) against frame by frame (views_per_call=1: the single-view frozen call + gsr_pose_step), timed
in ONE process.

The rule, written down before the run (the method of tools/importance_views_probe.py): after a warm-up of both arms the two alternate --
A, B, A, B, ... -- for `--rounds` rounds (at least 20); a host clock around a device synchronise.  One timed call is fit_poses over the 8
frames for `--iters` iterations (its set-up included), printed per iteration.  Per case the median and the min-max of each arm are
printed, the spread of ONE arm against itself (the difference of the medians of its odd and its even rounds), and the peak allocation of
each arm above what was allocated before it ran.  The views route is "faster" at a case only where its median lies below the
frame-by-frame route's by more than the LARGER of the two same-arm spreads; anything else is "not faster", a loss included, and is
recorded as such.  The defaults (fit_poses' views_per_call, run_segments' --eval-views-per-call) stay 1 whatever this prints: flipping
them is a follow-up that cites the recorded output, and only if the views arm is faster at BOTH sizes.

Cases: eight frames at 980x545 on bench.py's headline scene (1 M Gaussians, SH degree 3) and on stage A's (130 k Gaussians, degree 0 with
16 coefficients stored).

    python tools/pose_fit_views_probe.py > profiles/pose_fit_views.txt
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
bt = importlib.import_module("3dgs_hierarchical_training_amd.batched")
syn = importlib.import_module("3dgs_hierarchical_training_amd.synthetic")
pose = importlib.import_module("3dgs_hierarchical_training_amd.pose")
pose_fit = importlib.import_module("3dgs_hierarchical_training_amd.pose_fit")
R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
L = importlib.import_module("3dgs_hierarchical_training_amd._lib")

FRAMES = 8
# (name, N, W, H, degree, seed)
CASES = [("headline 1M/980x545/deg3, 8 frames", 1_000_000, 980, 545, 3, 0),
         ("stage A 130k/980x545/deg0 (16 stored), 8 frames", 130_000, 980, 545, 0, 3)]


def build(N, W, H, deg, seed, dev):
    """The model, its camera, 8 true transforms near the identity, the model's images under them and starts a small tangent away."""
    scene = syn.make_scene(N, W, H, sh_degree=deg, seed=seed)
    settings = ts.make_settings(scene, dev, deg)
    p = ts.GaussianParams(scene, dev, optimizer="torch")
    raw = p.raw()
    g = torch.Generator().manual_seed(5)
    truth = torch.stack([pose.se3_exp(0.02 * torch.randn(6, generator=g))[:3] for _ in range(FRAMES)]).float().to(dev).contiguous()
    start = torch.stack([pose.se3_exp(0.004 * torch.randn(6, generator=g)) for _ in range(FRAMES)]).float().to(dev)
    start = (start @ torch.cat([truth, torch.tensor([0.0, 0.0, 0.0, 1.0], device=dev).expand(FRAMES, 1, 4)], dim=1))[:, :3].contiguous()
    vs = bt.batch_settings([settings] * FRAMES, dev)
    color = R.forward_views(raw["_xyz"], raw["_features_dc"], raw["_opacity"], raw["_scaling"], raw["_rotation"], vs,
                            sh_rest=raw["_features_rest"], raw_params=True, points_transform=truth)[0]
    return raw, settings, color.clamp(0, 1).contiguous(), start


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
    ap.add_argument("--iters", type=int, default=4, help="pose iterations of one timed call (the times are printed per iteration)")
    ap.add_argument("--per-call", type=int, default=8)
    args = ap.parse_args()
    rounds, iters = max(20, args.rounds), max(1, args.iters)
    dev = torch.device("cuda:0")
    lib = L.load()
    print(f"pose_fit_views_probe: {torch.cuda.get_device_name(dev)}, rounds {rounds}, {iters} iterations per timed call, views per call "
          f"{args.per_call} against 1, library version {lib.gsr_version()}")
    print("rule: the views route is FASTER at a case only where its median lies below the frame-by-frame route's by more than the larger same-arm spread")
    verdicts = []
    for name, N, W, H, deg, seed in CASES:
        raw, settings, targets, start = build(N, W, H, deg, seed, dev)
        fit = lambda V: pose_fit.fit_poses(raw, settings, targets, init=start, iters=iters, lr=5e-4, views_per_call=V)
        arms = {"per-frame": lambda: fit(1), "views": lambda: fit(args.per_call)}
        a, b = arms["per-frame"]()[0], arms["views"]()[0]
        diff = float((a - b).abs().max())
        del a, b
        for _ in range(args.warmup):
            for fn in arms.values():
                fn()
        t = {k: [] for k in arms}
        for _ in range(rounds):
            for k in ("per-frame", "views"):                     # A, B, A, B, ...
                t[k].append(timed(arms[k], dev) / iters)
        st = {k: arm_stats(v) for k, v in t.items()}
        peaks = {k: peak_mib(arms[k], dev) for k in arms}
        print(f"\n{name}: ms per pose iteration of the {FRAMES} frames; largest difference of the two routes' poses after {iters} iterations "
              f"{diff:.2e} (default accumulation)")
        for k in ("per-frame", "views"):
            med, lo, hi, spread = st[k]
            print(f"  {k:9s} median {med:8.3f}   min {lo:8.3f}   max {hi:8.3f}   odd/even rounds' medians differ by {spread:.3f}   "
                  f"peak allocation {peaks[k]:9.1f} MiB")
        spread = max(st["per-frame"][3], st["views"][3])
        faster = st["views"][0] < st["per-frame"][0] - spread
        verdicts.append((name, faster))
        print(f"  views - per-frame = {st['views'][0] - st['per-frame'][0]:+.3f} ms; larger same-arm spread {spread:.3f} ms -> views route "
              f"{'FASTER' if faster else 'NOT faster'} at this case")
        del raw, settings, targets, start, arms, fit
        torch.cuda.empty_cache()
    print("\nsummary: " + "; ".join(f"{n}: {'faster' if f else 'not faster'}" for n, f in verdicts))
    print("the defaults stay 1 (fit_poses' views_per_call, run_segments' --eval-views-per-call): flipping them is a follow-up"
          + ("" if all(f for _, f in verdicts) else ", and this run does not support it"))


if __name__ == "__main__":
    main()
