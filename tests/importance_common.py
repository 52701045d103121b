"""Scenes and float64 references of the merge-time importance tests (tests/test_importance_cpu.py, tests/test_gpu_importance.py).

Built like test_gpu_fused.py::test_calc_importance_matches_oracle: a base cloud seen from two cameras, the DC colour brightened
(2 dc + 1.5) so that pixels exceed 1, background (0.2, 0.5, 0.9).  Every reference is computed once per process and shared."""
import functools
import importlib

import numpy as np
import torch

import parity
from oracle import binding

hier = importlib.import_module("3dgs_hierarchical_training_amd.hierarchy")
BG = (0.2, 0.5, 0.9)
CAM_SEEDS = (101, 102)
SCENE_A = (6000, 100, 75, 3)          # N, W, H, degree: partial tiles on both edges
SCENE_B = (2000, 72, 40)              # degrees 0, 1, 2 with 16 coefficients stored
SCENE_C = (20000, 320, 240, 3)        # the existing importance test's shape
RTOL = 1e-3                           # the project's bar for this quantity: max|imp - ref| <= 1e-3 ref.max() (test_gpu_fused.py:319)


@functools.lru_cache(maxsize=None)
def scene(N, W, H, deg, dark=False):
    """(base scene with 16 stored coefficients and active degree `deg`, [per-view scene dicts]).
    dark=True: every tenth Gaussian's DC coefficient of one channel (its index mod 3) is set to -3, so that channel's SH colour is
    clamped at 0 -- the brightened construction alone clamps a channel of only 0.15-0.3 % of the visible rows (colour = 0.92 +- 0.3),
    too few to hold the SH clamp gate to anything."""
    base = parity.syn.make_scene(N, W, H, sh_degree=3, seed=31, posed=False)
    base["shs"] = base["shs"].clone()
    base["shs"][:, 0] = 2.0 * base["shs"][:, 0] + 1.5
    if dark:
        idx = torch.arange(0, N, 10)
        base["shs"][idx, 0, idx % 3] = -3.0
    base["sh_degree"] = deg
    views = []
    for s in CAM_SEEDS:
        cam = parity.syn.make_scene(8, W, H, sh_degree=3, seed=s, posed=True)      # only its camera is used
        sc = dict(base)
        for k in ("viewmatrix", "projmatrix", "campos", "tanfovx", "tanfovy"):
            sc[k] = cam[k]
        views.append(sc)
    return base, views


def gate_of(color):
    """d clamp(x, 0, 1).sum() / dx on the image (NaN closes it)."""
    return ((color >= 0) & (color <= 1)).astype(np.float32)


def conditions(color, rgb, radii):
    """The shares that make a comparison on this view meaningful."""
    g = gate_of(color)
    closed = 1.0 - float(g.mean())
    mixed = float(((g.min(0) != g.max(0))).mean())
    near = float(((np.abs(color) < 1e-4) | (np.abs(color - 1.0) < 1e-4)).mean())     # gate elements within 1e-4 of a bound
    vis = radii > 0
    clamped = float((rgb[vis] <= 0).any(1).mean()) if vis.any() else 0.0
    return dict(closed=closed, mixed=mixed, near=near, clamped_rows=clamped)


def assert_meaningful(c, what="", dark=False):
    """closed share of the gate elements in [0.15, 0.45], pixels whose three gates differ >= 0.3, elements within 1e-4 of a bound
    <= 0.1 %, visible rows with an SH-clamped channel >= 3 % on the `dark` scenes.  On the plain scenes that last share cannot be 3 %:
    their colours are 0.92 +- 0.3, so the float64 oracle clamps a channel on 0.15-0.3 % of the visible rows (at least one row is asked);
    the `dark` scenes exist to hold the SH clamp gate to the 3 %."""
    print(f"[importance] {what}: " + ", ".join(f"{k} {v:.4f}" for k, v in c.items()))
    assert 0.15 <= c["closed"] <= 0.45, (what, c)
    assert c["mixed"] >= 0.3, (what, c)
    assert c["near"] <= 1e-3, (what, c)
    assert c["clamped_rows"] >= 0.03 if dark else c["clamped_rows"] > 0, (what, c)


@functools.lru_cache(maxsize=None)
def oracle_views(N, W, H, deg, dark=False):
    """Per view of scene(N, W, H, deg): the float64 oracle's image, |backward(gate)["shs"]| [N,16,3], the SH colours and radii."""
    _, views = scene(N, W, H, deg, dark)
    out = []
    for sc in views:
        o = binding.OracleRender(**parity.scene_kwargs(sc, "sh", bg=BG))
        color, radii = o.forward()[:2]
        color, radii = color.copy(), radii.copy()
        g = gate_of(color)
        ref = np.abs(o.backward(g, None, None)["shs"])
        rgb = o.geom()["rgb"].copy()
        o.close()
        out.append(dict(color=color, gate=g, ref=ref, rgb=rgb, radii=radii))
    return out


def oracle_importance(N, W, H, deg, dark=False):
    """[N, 48]: sum over the views of |backward(gate)["shs"]| / pixels."""
    vs = oracle_views(N, W, H, deg, dark)
    return sum(v["ref"] for v in vs).reshape(N, 48) / (len(vs) * W * H)


def segment(base, dev):
    ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
    p = ts.GaussianParams(base, dev, optimizer="torch")
    return {k: getattr(p, k).detach() for k in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")}


def settings(views, dev, deg):
    ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
    return [ts.make_settings(sc, dev, deg, bg=torch.tensor(BG)) for sc in views]
