#!/usr/bin/env python3
"""The single-image initialisation on the device, timed in ONE process with alternating arms.

A 980x545 depth map (smooth, every pixel valid) is un-projected once (pointcloud.depth_to_points: 534 100 points) and then reduced
to one point per voxel of 0.01 by two routes:

  kernels   pointcloud.voxel_down_sample        (csrc/voxel_kernels.hip: keys, two stable 32-bit sorts, head scan, fixed-order float64 means)
  torch     the restatement a user would write on the device without it: floor((p - origin) / voxel_size) in float64,
            torch.unique(dim=0, return_inverse=True, return_counts=True), float64 index_add_, one rounding to float32

Both give ascending (ix, iy, iz) order (torch.unique sorts its rows); the torch route's index_add_ adds with float64 atomics, so
its last bits may change from run to run.  After a warm-up the arms alternate -- A, B, A, B, ... -- for `--rounds` rounds (at least
20).  One sample is one call under a host clock that ends in a device synchronise (either route synchronises anyway: M is read
back).  Per arm the median, the min-max and the spread of the arm against itself (the difference of the medians of its odd and even
rounds) are printed; a difference between the arms below the larger same-arm spread is no difference.  Then the whole chain,
pointcloud.scene_from_depth (un-projection, voxel grid, distCUDA2, create_from_pcd's tensors), and its steps alone.

The reference's own host leg (kornia + a copy to the host + open3d + a copy back) cannot be timed where neither library is installed;
no estimate of it is made here.

    python tools/voxel_init_probe.py > profiles/voxel_init.txt
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pc = importlib.import_module("3dgs_hierarchical_training_amd.pointcloud")
syn = importlib.import_module("3dgs_hierarchical_training_amd.synthetic")
L = importlib.import_module("3dgs_hierarchical_training_amd._lib")


def depth_map(H, W, dev):
    """A smooth scene 1 - 2.6 units deep with a step edge and fine ripples: most voxels of 0.01 hold a few pixels, a near patch many."""
    yy, xx = torch.meshgrid(torch.linspace(0.0, 1.0, H), torch.linspace(0.0, 1.0, W), indexing="ij")
    d = 1.8 + 0.6 * torch.sin(5.0 * xx) * torch.cos(3.0 * yy) + 0.2 * yy + 0.01 * torch.sin(90.0 * xx + 40.0 * yy)
    d = torch.where((xx - 0.3) ** 2 + (yy - 0.6) ** 2 < 0.02, torch.full_like(d, 0.35), d)      # a near, fronto-parallel patch: long segments
    g = torch.Generator().manual_seed(3)
    return d.float().to(dev), torch.rand(3, H, W, generator=g).to(dev)


def torch_route(points, colors, voxel_size):
    finite = torch.isfinite(points).all(dim=1)
    p, c = points[finite].double(), colors[finite].double()
    origin = p.min(dim=0).values - 0.5 * voxel_size
    index = torch.floor((p - origin) / voxel_size).long()
    uniq, inverse, counts = torch.unique(index, dim=0, return_inverse=True, return_counts=True)
    n = counts.double()[:, None]
    out_p = torch.zeros((uniq.shape[0], 3), dtype=torch.float64, device=p.device).index_add_(0, inverse, p) / n
    out_c = torch.zeros((uniq.shape[0], 3), dtype=torch.float64, device=p.device).index_add_(0, inverse, c) / n
    return out_p.float(), out_c.float(), counts


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return 1e3 * (time.perf_counter() - t0)


def arm_stats(x):
    return statistics.median(x), min(x), max(x), abs(statistics.median(x[0::2]) - statistics.median(x[1::2]))


def line(name, st):
    med, lo, hi, spread = st
    print(f"  {name:34s} median {med:8.3f}   min {lo:8.3f}   max {hi:8.3f}   odd/even rounds' medians differ by {spread:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--voxel-size", type=float, default=0.01)
    args = ap.parse_args()
    rounds = max(20, args.rounds)
    dev = torch.device("cuda:0")
    H, W, vs = 545, 980, args.voxel_size
    print(f"voxel_init_probe: {torch.cuda.get_device_name(dev)}, {W}x{H}, voxel_size {vs}, rounds {rounds}, warm-up {args.warmup}, "
          f"library version {L.load().gsr_version()}")
    depth, image = depth_map(H, W, dev)
    cam = syn.make_camera(W, H)
    K = (cam["fx"], cam["fy"], 0.5 * W - 0.5, 0.5 * H - 0.5)
    points, colors = pc.depth_to_points(depth, image, K)

    kp, kc, kn, dropped = pc.voxel_down_sample(points, colors, vs, return_counts=True)
    tp, tc, tn = torch_route(points, colors, vs)
    same = kp.shape == tp.shape and torch.equal(kn.long(), tn)
    print(f"  N = {points.shape[0]}, M = {kp.shape[0]} voxels, longest segment {int(kn.max())}, mean {points.shape[0] / max(1, kp.shape[0]):.2f} points per voxel, "
          f"dropped {dropped}")
    print(f"  the two routes agree on M and on every count: {same}" +
          (f"; max |difference| points {float((kp - tp).abs().max()):.3e}, colours {float((kc - tc).abs().max()):.3e}" if same else ""))
    again = pc.voxel_down_sample(points, colors, vs)
    print(f"  kernels, a second call bit-identical: {torch.equal(again[0], kp) and torch.equal(again[1], kc)}")

    arms = {"kernels (voxel_down_sample)": lambda: pc.voxel_down_sample(points, colors, vs),
            "torch (unique + index_add_)": lambda: torch_route(points, colors, vs)}
    for _ in range(args.warmup):
        for fn in arms.values():
            fn()
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():                           # A, B, A, B, ...
            t[k].append(timed(fn, dev))
    st = {k: arm_stats(v) for k, v in t.items()}
    print(f"\nvoxel grid of {points.shape[0]} points at {vs}   [ms per call, host clock around a device synchronise]")
    for k in arms:
        line(k, st[k])
    a, b = list(arms)
    spread, diff = max(st[a][3], st[b][3]), st[a][0] - st[b][0]
    verdict = "no difference beyond the spread" if abs(diff) <= spread else ("kernels are FASTER" if diff < 0 else "kernels are SLOWER")
    print(f"  kernels - torch = {diff:+.3f}; same-arm spread {spread:.3f} -> {verdict}")

    print(f"\nthe chain and its steps, kernels route   [ms per call, {rounds} calls each after the warm-up]")
    sp, sc = pc.voxel_down_sample(points, colors, vs)
    steps = {"scene_from_depth (end to end)": lambda: pc.scene_from_depth(depth, image, K, voxel_size=vs),
             "  depth_to_points": lambda: pc.depth_to_points(depth, image, K),
             "  voxel_down_sample": lambda: pc.voxel_down_sample(points, colors, vs),
             "  scene_from_points (distCUDA2 ...)": lambda: pc.scene_from_points(sp, sc)}
    for k, fn in steps.items():
        for _ in range(args.warmup):
            fn()
        line(k, arm_stats([timed(fn, dev) for _ in range(rounds)]))


if __name__ == "__main__":
    main()
