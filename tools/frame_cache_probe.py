#!/usr/bin/env python3
"""The frame loader of the unmodified trainer, original against cached, timed in ONE process with alternating arms.

The reference calls `GaussianTrainer.load_viewpoint_cam` before every iteration (/root/reference/trainer/trainer.py:989-1142) with a pose
that went through `get_RT(fidx).detach().cpu()`.  `gsr_autopatch` caches the frame on the device, builds posed cameras with one kernel
(gsr_camera_from_pose) and keeps the pose on the device (`DevicePose`).  Three measurements at 980x545, each at stage A's size (130 k
Gaussians, SH degree 0 with 16 coefficients stored) and at the headline size (1 M, degree 3) where a model is involved:

  (a) the loader alone     refstub.StubTrainer.load_viewpoint_cam (the 'custom' branch: the frame converted on every call; the 'preloaded'
                           branch: the float image copied back to the host on every call), original against cached; cached with
                           pose=None and with a pose.  One sample = one pass over the ring of frames, per call.
  (b) a whole iteration    load -> patched render -> fused loss -> backward -> deferred Adam, original loader against cached.  One sample =
                           a block of `--block` iterations, per iteration: the host may run ahead of the device inside a block, as in training.
  (c) the harness          a phase-1 virtual-view step of run_segments.RankRunner (pose interpolation, the teacher's camera and render, the
                           model's camera and step), host cameras against --device-cameras.  One sample = one phase 1 of 24 steps, per step.

Every sample is taken with the host clock around a device synchronise; the arms alternate A, B, A, B, ...; per arm the median, the min-max and
the spread of the arm against itself (the difference of the medians of its odd and even rounds) are printed.  The decision rule of the other
routes: a difference below the larger same-arm spread is no difference.

    python tools/frame_cache_probe.py > profiles/frame_cache.txt
"""
import argparse
import importlib
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
syn = importlib.import_module("3dgs_hierarchical_training_amd.synthetic")
ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
refstub = importlib.import_module("3dgs_hierarchical_training_amd.refstub")
L = importlib.import_module("3dgs_hierarchical_training_amd._lib")

W, H = 980, 545
SIZES = [("stage A 130k/deg0 (16 stored)", 130_000, 0), ("headline 1M/deg3", 1_000_000, 3)]


def sample(fn, dev, per):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return 1e3 * (time.perf_counter() - t0) / per


def arm_stats(x):
    return statistics.median(x), min(x), max(x), abs(statistics.median(x[0::2]) - statistics.median(x[1::2]))


def line(name, st):
    med, lo, hi, spread = st
    print(f"  {name:44s} median {med:8.3f}   min {lo:8.3f}   max {hi:8.3f}   odd/even rounds' medians differ by {spread:.3f}")


def alternate(arms, dev, rounds, warmup, per):
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            t[k].append(sample(fn, dev, per))
    st = {k: arm_stats(v) for k, v in t.items()}
    for k in arms:
        line(k, st[k])
    return st


def verdict(st, a, b, what):
    spread, diff = max(st[a][3], st[b][3]), st[b][0] - st[a][0]
    word = "no difference beyond the spread" if abs(diff) <= spread else (f"{what} is FASTER" if diff < 0 else f"{what} is SLOWER")
    print(f"  {what} - original = {diff:+.3f} ms; same-arm spread {spread:.3f} -> {word}")
    return diff < -spread


class FixedPose:
    """Stands for a lietorch pose: `retr().matrix()` is device work only."""

    def __init__(self, M):
        self.M = M

    def retr(self):
        return self

    def matrix(self):
        return self.M[None]


def frame_pose(f, dev):
    ang = 0.006 * f
    M = torch.eye(4)
    M[0, 0] = M[2, 2] = float(np.cos(ang)); M[0, 2] = float(np.sin(ang)); M[2, 0] = -float(np.sin(ang))
    M[0, 3] = 0.02 * f
    return M.to(dev)


def patched_classes(A):
    class GaussianTrainer(refstub.StubTrainer):
        pass

    class HTGaussianModel(refstub.StubGaussians):
        pass
    tmod, gmod = types.ModuleType("trainer.trainer"), types.ModuleType("scene.gaussian_model_ht")
    tmod.GaussianTrainer, gmod.HTGaussianModel = GaussianTrainer, HTGaussianModel
    A._patch_frames_module(tmod)
    A._patch_frames_module(gmod)
    return GaussianTrainer, HTGaussianModel


def loader_alone(A, dev, frames, K, rounds, warmup):
    T, _ = patched_classes(A)
    poses = [frame_pose(f, dev) for f in range(len(frames))]
    dposes = [p.as_subclass(A.DevicePose) for p in poses]
    n = len(frames)
    for data_type in ("custom", "preloaded"):
        orig, cached = refstub.StubTrainer(frames, K, data_type=data_type, device=dev), T(frames, K, data_type=data_type, device=dev)
        print(f"\n(a) the loader alone, '{data_type}' branch, {n} frames of {W}x{H}   [ms per call]")
        st = alternate({
            "original, pose=None": lambda: [orig.load_viewpoint_cam(f) for f in range(n)],
            "cached,   pose=None": lambda: [cached.load_viewpoint_cam(f) for f in range(n)],
            "original, pose=get_RT(f).detach().cpu()": lambda: [orig.load_viewpoint_cam(f, pose=poses[f].detach().cpu()) for f in range(n)],
            "cached,   pose=get_RT(f).detach().cpu()": lambda: [cached.load_viewpoint_cam(f, pose=dposes[f].detach().cpu()) for f in range(n)],
        }, dev, rounds, warmup, n)
        verdict(st, "original, pose=None", "cached,   pose=None", "cached")
        verdict(st, "original, pose=get_RT(f).detach().cpu()", "cached,   pose=get_RT(f).detach().cpu()", "cached")


def whole_iteration(A, dev, frames, rounds, warmup, block):
    T, G = patched_classes(A)
    cam0 = syn.make_camera(W, H)
    K = np.array([[cam0["fx"], 0, W / 2.0], [0, cam0["fy"], H / 2.0], [0, 0, 1]])
    n = len(frames)

    class Loss:
        class cfg:
            lambda_dssim, lambda_depth = 0.2, 0.0
    wins = []
    for name, N, deg in SIZES:
        sc = syn.make_scene(N, W, H, sh_degree=deg, seed=3)
        p = ts.GaussianParams(sc, dev, optimizer="torch")            # the reference's Adam construction: FusedAdam under the patch
        r = refstub.StubRender(p)
        g = r.gaussians = G(p)
        g.P = [FixedPose(frame_pose(f, dev)) for f in range(n)]
        plain_get_RT = refstub.StubGaussians.get_RT
        orig, cached = refstub.StubTrainer(frames, K, data_type="preloaded", device=dev), T(frames, K, data_type="preloaded", device=dev)
        state = {"k": 0}

        def iteration(trainer, get_RT):
            f = state["k"] % n
            state["k"] += 1
            cam = trainer.load_viewpoint_cam(f, pose=get_RT(f).detach().cpu())
            pkg = A.render_fused(r, cam)
            A.loss_forward(Loss(), pkg["image"], cam.original_image)["loss"].backward()
            g.optimizer.step()
            g.optimizer.zero_grad(set_to_none=True)
        print(f"\n(b) a whole iteration, {name}, {W}x{H}, blocks of {block}   [ms per iteration]")
        st = alternate({"original loader": lambda: [iteration(orig, lambda f: plain_get_RT(g, f)) for _ in range(block)],
                        "cached loader": lambda: [iteration(cached, g.get_RT) for _ in range(block)]}, dev, rounds, warmup, block)
        wins.append(verdict(st, "original loader", "cached loader", "cached"))
        del p, r, g
        torch.cuda.empty_cache()
    print(f"\n  decision rule: the cache patch stays on by default only if (b)'s median lies below the original's by more than the same-arm "
          f"spread at both sizes -> {'ON' if all(wins) else 'OFF'}")


def harness(dev, rounds, warmup):
    rs = importlib.import_module("3dgs_hierarchical_training_amd.run_segments")
    seg_mod = importlib.import_module("3dgs_hierarchical_training_amd.segments")
    sequence = importlib.import_module("3dgs_hierarchical_training_amd.sequence")
    for name, N, deg in SIZES:
        cfg = rs.HTConfig(frames=6, width=W, height=H, gt_gaussians=100_000, leaf_gaussians=N, leaf_iters_per_frame=1, phase1_iters_per_frame=4,
                          phase1_ratio=1.0, phase2_iters_per_frame=[0], prune_ratio=0.5, start_sh_degree=deg, sh_up_every=0)
        seq = sequence.FrameSequence(cfg.frames, cfg.gt_gaussians, W, H, dev, seed=6)
        tr = seg_mod.LocalTransport(2)
        log = []
        runners = [rs.RankRunner(r, 2, tr, seq, cfg, dev, log=log.append) for r in range(2)]
        for rr in runners:
            rr.train_leaf()
        runners[1].merge_send(0)
        runners[0].merge_recv(0)
        root, teachers = runners[0], runners[0].teachers
        runners[1] = None

        def phase1(device_cameras):
            cfg.device_cameras = device_cameras
            root.teachers = teachers
            root.train_nonleaf(0)
            assert log[-1]["virtual_views"] == log[-1]["phase1_steps"] == 24
        print(f"\n(c) a phase-1 virtual-view step of the harness, merged model of {root.seg.params.num_points} Gaussians ({name}), {W}x{H}   [ms per step]")
        st = alternate({"host cameras": lambda: phase1(False), "--device-cameras": lambda: phase1(True)}, dev, rounds, warmup, 24)
        verdict(st, "host cameras", "--device-cameras", "--device-cameras")
        del runners, root, teachers, seq
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--parts", default="abc")
    a = ap.parse_args()
    import gsr_autopatch as A
    dev = torch.device("cuda:0")
    rounds = max(10, a.rounds)
    print(f"frame_cache_probe: {torch.cuda.get_device_name(dev)}, {W}x{H}, rounds {rounds}, warm-up {a.warmup}, library version {L.load().gsr_version()}, "
          f"host threads {torch.get_num_threads()}")
    g = np.random.default_rng(0)
    frames = [g.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(a.frames)]
    K = np.array([[611.3, 0, 490.0], [0, 611.3, 272.5], [0, 0, 1]])
    A.apply()
    try:
        if "a" in a.parts:
            loader_alone(A, dev, frames, K, rounds, a.warmup)
        if "b" in a.parts:
            whole_iteration(A, dev, frames, rounds, a.warmup, a.block)
    finally:
        A.remove()
    if "c" in a.parts:
        harness(dev, rounds, a.warmup)


if __name__ == "__main__":
    main()
