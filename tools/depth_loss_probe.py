#!/usr/bin/env python3
"""What depth supervision costs the autopatched trainer's step: wall time per step of the trainer's own calls (render_fused ->
Loss.forward -> backward -> step -> zero_grad) at the headline size (1 M Gaussians, SH degree 3, 980x545) and at stage A's size (130 k,
SH degree 0), in three arms:
    lambda_depth = 0                                        the photometric step
    lambda_depth = 0.1, fused                               the depth term on the kernels (gsr_depth_loss_*), no host synchronisation
    lambda_depth = 0.1, GSR_AUTOPATCH_DEPTH_LOSS=0          the reference's torch statements (three host synchronisations) -- what the
                                                            trainer ran before the depth kernels existed
Every arm is a fresh process (the environment switch is read per call, but a fresh process keeps the arms' allocator and view-cache
states apart); the arms of one size run back to back on the same device, `--rounds` times interleaved, and the median is reported.
  python tools/depth_loss_probe.py [--steps 300] [--rounds 3] [--kind invariant] [--out profiles/depth_loss_probe.txt]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [("headline", 1_000_000, 3), ("stage A", 130_000, 0)]
ARMS = [("lambda_depth = 0", 0.0, "1"), ("lambda_depth = 0.1, fused", 0.1, "1"), ("lambda_depth = 0.1, torch statements", 0.1, "0")]


def arm(n, deg, lambda_depth, kind, steps, warmup):
    """One arm, in this process: prints one JSON line."""
    import torch
    sys.path.insert(0, REPO)
    syn = importlib.import_module("3dgs_hierarchical_training_amd.synthetic")
    ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
    refstub = importlib.import_module("3dgs_hierarchical_training_amd.refstub")
    import gsr_autopatch
    dev = torch.device("cuda:0")
    W, H = 980, 545
    sc = syn.make_scene(n, W, H, sh_degree=deg, seed=3)
    st = ts.make_settings(sc, dev, deg)
    gt = syn.target_image(W, H, seed=2).to(dev)
    gsr_autopatch.apply()
    p = ts.GaussianParams(sc, dev, optimizer="torch")
    r = refstub.StubRender(p, bg=(0.0, 0.0, 0.0))
    cam = refstub.StubCamera(W, H, st.tanfovx, st.tanfovy, st.viewmatrix, st.projmatrix, st.campos, original_image=gt)
    with torch.no_grad():      # a monocular-depth stand-in: an affine image of the first render's depth, 10 % invalid
        d0 = gsr_autopatch.render_fused(r, cam)["depth"].detach().clone()
        g = torch.Generator(device="cpu").manual_seed(4)
        depth_gt = 1.4 * d0 + 0.3
        depth_gt[(torch.rand(d0.shape, generator=g) < 0.1).to(dev)] = 0.0
    loss_obj = refstub.StubLoss(kind, 0.2, lambda_depth)

    def step():
        pkg = gsr_autopatch.render_fused(r, cam)
        d = gsr_autopatch.loss_forward(loss_obj, pkg["image"], gt, pkg["depth"], depth_gt)
        d["loss"].backward()
        with torch.no_grad():
            p.optimizer.step()
            p.optimizer.zero_grad(set_to_none=True)

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    print(json.dumps({"ms_per_step": 1e3 * (time.perf_counter() - t0) / steps}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kind", default="invariant", choices=["l1", "invariant"])
    ap.add_argument("--timeout", type=int, default=240, help="seconds per arm")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "depth_loss_probe.txt"))
    ap.add_argument("--arm", nargs=3, metavar=("N", "DEG", "LAMBDA"), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.arm:
        arm(int(a.arm[0]), int(a.arm[1]), float(a.arm[2]), a.kind, a.steps, a.warmup)
        return
    lines = [f"tools/depth_loss_probe.py: autopatched trainer step, 980x545, depth_loss_type '{a.kind}', {a.steps} steps per arm, "
             f"median of {a.rounds} interleaved rounds (ms per step; every round's figure in brackets)"]
    for name, n, deg in SIZES:
        got = {label: [] for label, _, _ in ARMS}
        for _ in range(a.rounds):
            for label, lam, fused in ARMS:
                env = dict(os.environ, GSR_AUTOPATCH_DEPTH_LOSS=fused)
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", str(n), str(deg), str(lam), "--kind", a.kind,
                                      "--steps", str(a.steps), "--warmup", str(a.warmup)], env=env, cwd=REPO, capture_output=True,
                                     text=True, timeout=a.timeout, check=True)      # (a failed or hung arm ends the probe)
                got[label].append(json.loads(out.stdout.strip().splitlines()[-1])["ms_per_step"])
        lines.append(f"{name}: {n} Gaussians, SH degree {deg}")
        base = statistics.median(got[ARMS[0][0]])
        for label, _, _ in ARMS:
            med = statistics.median(got[label])
            lines.append(f"  {label:<40s} {med:8.3f}   ({med - base:+.3f} against lambda_depth = 0)   [{', '.join(f'{v:.3f}' for v in got[label])}]")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
