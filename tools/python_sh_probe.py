#!/usr/bin/env python3
"""ms per iteration of the reference's `convert_SHs_python` renders under gsr_autopatch, on the kernels (GSR_AUTOPATCH_PYTHON_SH=1:
sh_origin) and on the original method (=0: torch eval_sh over [N,3,16], torch activations, the drop-in rasterizer with colors_precomp,
the torch backward of all of it).  Device-synchronised wall time over the timed iterations.

  init_leaf  ~130 k Gaussians, degree 0, one camera, identity frame poses with rotate_seq off (init_leaf_3DGS,
             trainer/ht3dgs_trainer.py:186-206): render, loss, backward, the model's Adam step
  eval_nvs   1 M Gaussians, degree 3, rotate_seq, pose-only steps (update_gaussians=False; eval_nvs, :1010-1036): render, loss,
             backward, the frame pose's Adam step

Usage: python tools/python_sh_probe.py [--shape init_leaf|eval_nvs|both] [--iters 30] [--warmup 5]
Prints one JSON line per (shape, route)."""
import argparse
import importlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402


def run(shape, route, iters, warmup):
    import gsr_autopatch
    from test_gpu_python_sh import register_original
    from test_python_sh_cpu import PythonShRender
    syn = importlib.import_module("3dgs_hierarchical_training_amd.synthetic")
    ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
    refstub = importlib.import_module("3dgs_hierarchical_training_amd.refstub")
    dev = torch.device("cuda:0")
    W, H = 980, 545
    N, deg = (130_000, 0) if shape == "init_leaf" else (1_000_000, 3)
    sc = syn.make_scene(N, W, H, sh_degree=deg, seed=3)
    gt = syn.target_image(W, H, seed=1).to(dev)
    os.environ["GSR_AUTOPATCH_PYTHON_SH"] = "1" if route == "kernels" else "0"

    class _LossCfg:
        class cfg:
            lambda_dssim, lambda_depth = 0.2, 0.0
    gsr_autopatch.apply()
    register_original(gsr_autopatch)      # (the stub's render() is the original method the patched one serves or falls back to)
    try:
        p = ts.GaussianParams(sc, dev, optimizer="torch")       # the reference's Adam construction (FusedAdam under the patch)
        r = PythonShRender(p)
        g = r.gaussians
        cam = refstub.StubCamera.from_scene(sc, dev, original_image=gt, uid=1)
        lie = lambda: refstub.LieGroupParameter(refstub.SE3(torch.tensor([[0.0, 0, 0, 0, 0, 0, 1]], device=dev)))
        g.P = [lie(), lie()]
        popt = None
        if shape == "eval_nvs":
            g.rotate_seq, g.seq_idx = True, 1
            popt = torch.optim.Adam([{"params": [g.P[1]], "lr": 1e-3, "name": "R"}], lr=0.0, eps=1e-15)

        def step():
            pkg = r.render(cam, convert_SHs_python=True)
            gsr_autopatch.loss_forward(_LossCfg(), pkg["image"], gt)["loss"].backward()
            if popt is None:
                p.optimizer.step()
            else:
                popt.step()
                popt.zero_grad(set_to_none=True)
            p.optimizer.zero_grad(set_to_none=True)
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / iters
        assert (r.calls == 0) == (route == "kernels"), r.calls
    finally:
        gsr_autopatch.remove()
    return {"shape": shape, "route": route, "N": N, "sh_degree": deg, "W": W, "H": H, "iters": iters, "ms_per_iter": round(ms, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["init_leaf", "eval_nvs", "both"])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    for shape in (["init_leaf", "eval_nvs"] if a.shape == "both" else [a.shape]):
        for route in ("kernels", "original"):
            print(json.dumps(run(shape, route, a.iters, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
