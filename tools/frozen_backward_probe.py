#!/usr/bin/env python3
"""Frozen backward: a pose iteration against a model that does not move (render + loss + backward + pose_step, the fused pose loop of
stage_a.fit_pair / fit_pairs_batched) with the full backward (`frozen=False`) against the frozen call taken by inference
(`frozen=None`: include/gsr.h GsrBackwardArgs, rasterizer.frozen_backward_route), timed in ONE process on the same forward inputs.

After a warm-up of both arms they alternate -- A, B, A, B, ... -- for `--rounds` rounds (at least 20); a host clock around a device
synchronise.  Per size the median and the min-max of each arm are printed, and the spread of ONE arm against itself: the difference
of the medians of its odd and its even rounds.  The frozen route is "faster" only when its median lies below the full route's by more
than that same-arm spread (the larger of the two arms'); rasterizer.FROZEN_BY_INFERENCE may be True only if that holds at EVERY size.
The backward's peak allocation (growth of torch's allocated bytes over backward()) and the per-Gaussian kernel's own time (the
library's "preprocess_bwd" profile stage) come from passes of their own.

Sizes: bench.py's headline scene (1 M Gaussians, SH degree 3), stage A's model (130 k Gaussians, degree 0 with 16 coefficients
stored) and a batch of 8 such models in one launch chain, all at 980x545.  One size per process (`--size`), so that a job runs every
size under a time limit of its own:

    for s in headline stage_a batch8; do timeout 300 python tools/frozen_backward_probe.py --size $s; done > profiles/frozen_backward.txt
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
ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
bt = importlib.import_module("3dgs_hierarchical_training_amd.batched")
syn = importlib.import_module("3dgs_hierarchical_training_amd.synthetic")
R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
E = importlib.import_module("3dgs_hierarchical_training_amd._ext")
L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
loss_mod = importlib.import_module("3dgs_hierarchical_training_amd.loss")

W, H = 980, 545
# name -> (description, Gaussians per model, models, active SH degree, seed)
SIZES = {"headline": ("headline 1M/980x545/deg3", 1_000_000, 1, 3, 0),
         "stage_a": ("stage A 130k/980x545/deg0 (16 stored)", 130_000, 1, 0, 3),
         "batch8": ("batch of 8 x 130k/980x545/deg0 (16 stored)", 130_000, 8, 0, 3)}


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


class PoseLoop:
    """The fused pose loop on detached parameters: one `step(frozen)` is one pose iteration."""

    def __init__(self, n, models, deg, seed, dev):
        self.dev, self.B, self.ops = dev, models, E.load()
        scenes = [syn.make_scene(n, W, H, sh_degree=deg, seed=seed + k) for k in range(models)]
        view = ts.make_settings(scenes[0], dev, deg)
        if models > 1:
            params = bt.BatchedGaussianParams(scenes, dev, optimizer="torch")
            self.first_block = params.first_block
            self.settings = bt.batch_settings([view] * models, dev)
            self.target = torch.stack([syn.target_image(W, H, seed=10 + k) for k in range(models)]).to(dev)
        else:
            params = ts.GaussianParams(scenes[0], dev, optimizer="torch")
            self.first_block = None
            self.settings = view
            self.target = syn.target_image(W, H, seed=10).to(dev)
        self.raw = params.raw()
        self.N = params.num_points
        self.m2d = torch.zeros_like(self.raw["_xyz"])
        shape = (models, 6) if models > 1 else (6,)
        self.delta, self.m, self.v = (torch.zeros(shape, device=dev) for _ in range(3))
        self.none = torch.empty(0, device=dev)
        self.M = torch.zeros((models, 3, 4) if models > 1 else (3, 4), device=dev)
        self.it = 0
        self._pose_step(None)

    def _pose_step(self, g):
        for b in range(self.B):
            sel = (lambda x: x[b]) if self.B > 1 else (lambda x: x)
            self.ops.pose_step(sel(self.delta), sel(self.m), sel(self.v), self.none if g is None else sel(g), self.none, sel(self.M), 2e-3, 0.9,
                               0.999, 1e-8, self.it)

    def forward(self, frozen):
        r = self.raw
        Mi = self.M.detach().requires_grad_(True)
        out = R.rasterize_gaussians_raw(r["_xyz"], self.m2d, r["_features_dc"], r["_features_rest"], r["_opacity"], r["_scaling"], r["_rotation"],
                                        self.settings, points_transform=Mi, batch_first_block=self.first_block, frozen=frozen)
        return Mi, loss_mod.fused_photometric_loss(out[0], self.target, 0.2, clamp=True)

    def step(self, frozen):
        Mi, loss = self.forward(frozen)
        loss.backward()
        self.it += 1
        self._pose_step(Mi.grad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", choices=sorted(SIZES), required=True)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    rounds = max(20, args.rounds)
    dev = torch.device("cuda:0")
    lib = L.load()
    name, n, models, deg, seed = SIZES[args.size]
    print(f"frozen_backward_probe: {torch.cuda.get_device_name(dev)}, rounds {rounds}, library version {lib.gsr_version()}, "
          f"FROZEN_BY_INFERENCE {R.FROZEN_BY_INFERENCE}")
    loop = PoseLoop(n, models, deg, seed, dev)
    arms = {"frozen": None if R.FROZEN_BY_INFERENCE else True, "full": False}
    count = lambda: int(lib.gsr_get_counter(b"frozen_backward_calls"))
    for _ in range(args.warmup):
        for f in arms.values():
            loop.step(f)
    t = {k: [] for k in arms}
    c0 = count()
    for _ in range(rounds):
        for k, f in arms.items():                      # A, B, A, B, ...
            t[k].append(timed(lambda: loop.step(f), dev))
    assert count() - c0 == rounds, "the frozen arm did not take the frozen call every time (or the full arm took it)"
    st = {k: arm_stats(v) for k, v in t.items()}
    print(f"\n{name}: N = {loop.N}, ms per pose iteration (render + loss + backward + pose_step)")
    for k in arms:
        med, lo, hi, spread = st[k]
        print(f"  {k:7s} median {med:8.3f}   min {lo:8.3f}   max {hi:8.3f}   odd/even rounds' medians differ by {spread:.3f}")
    spread = max(st["frozen"][3], st["full"][3])
    faster = st["frozen"][0] < st["full"][0] - spread
    print(f"  frozen - full = {st['frozen'][0] - st['full'][0]:+.3f} ms; same-arm spread {spread:.3f} ms -> frozen route "
          f"{'FASTER' if faster else 'NOT faster'} at this size")
    # the backward's peak allocation: growth of torch's allocated bytes over backward()
    for k, f in arms.items():
        Mi, loss = loop.forward(f)
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        loss.backward()
        torch.cuda.synchronize(dev)
        grow = torch.cuda.max_memory_allocated(dev) - before
        print(f"  {k:7s} backward peak allocation {grow / 2 ** 20:9.1f} MiB  ({grow / loop.N:6.1f} bytes per Gaussian)")
        del Mi, loss
    # the per-Gaussian kernel's own time (profile stages; a pass of its own: the event records sit in the stream)
    lib.gsr_set_option(b"profile", 1)
    try:
        for k, f in arms.items():
            for s in ("preprocess_bwd", "blend_bwd"):
                stage(lib, s)
            for _ in range(5):
                loop.step(f)
            torch.cuda.synchronize(dev)
            for s in ("preprocess_bwd", "blend_bwd"):
                tot, cnt = stage(lib, s)
                print(f"  {k:7s} stage {s:15s} {1e3 * tot / max(cnt, 1):8.1f} us per call over {cnt} calls")
    finally:
        lib.gsr_set_option(b"profile", 0)
    print(f"verdict {args.size}: {'FASTER' if faster else 'NOT faster'}")


if __name__ == "__main__":
    main()
