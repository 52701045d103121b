"""Scenes and float64 references of the tests of V views of one model (tests/test_views_cpu.py, tests/test_gpu_views.py; include/gsr.h
gsr_forward_views, gsr_importance_accumulate_views).

Built on tests/importance_common.py: the same brightened base cloud and the same oracle binding, seen from up to eight cameras -- the
two of importance_common first, then six more of the same construction (synthetic.make_scene's posed camera under further seeds).
Every reference is computed once per process and shared."""
import functools
import importlib

import numpy as np
import torch

import importance_common as ic
import parity
from oracle import binding

hier = ic.hier
syn = parity.syn
# importance_common.CAM_SEEDS first: a two-view scene here IS importance_common's
CAM_SEEDS = ic.CAM_SEEDS + (103, 104, 105, 106, 107, 108)
MAX_VIEWS = len(CAM_SEEDS)


@functools.lru_cache(maxsize=None)
def scene(N, W, H, deg, V, dark=False):
    """(base scene, [V per-view scene dicts]): importance_common.scene's cloud under the first V cameras of CAM_SEEDS."""
    assert 1 <= V <= MAX_VIEWS
    base, two = ic.scene(N, W, H, deg, dark)
    views = list(two[:V])
    for s in CAM_SEEDS[2:V]:
        cam = syn.make_scene(8, W, H, sh_degree=3, seed=s, posed=True)      # only its camera is used
        sc = dict(base)
        for k in ("viewmatrix", "projmatrix", "campos", "tanfovx", "tanfovy"):
            sc[k] = cam[k]
        views.append(sc)
    return base, views


@functools.lru_cache(maxsize=None)
def _oracle_view(N, W, H, deg, v, dark):
    if v < 2:
        return ic.oracle_views(N, W, H, deg, dark)[v]
    sc = scene(N, W, H, deg, v + 1, dark)[1][v]
    o = binding.OracleRender(**parity.scene_kwargs(sc, "sh", bg=ic.BG))
    color, radii = o.forward()[:2]
    color, radii = color.copy(), radii.copy()
    g = ic.gate_of(color)
    ref = np.abs(o.backward(g, None, None)["shs"])
    rgb = o.geom()["rgb"].copy()
    o.close()
    return dict(color=color, gate=g, ref=ref, rgb=rgb, radii=radii)


def oracle_views(N, W, H, deg, V, dark=False):
    """Per view: the float64 oracle's image, |backward(gate)["shs"]| [N,16,3], the SH colours and radii (importance_common's records)."""
    return [_oracle_view(N, W, H, deg, v, dark) for v in range(V)]


def oracle_importance(N, W, H, deg, V, dark=False):
    """[N, 48]: sum over the V views of |backward(gate)["shs"]| / pixels (importance_common.oracle_importance for V views)."""
    vs = oracle_views(N, W, H, deg, V, dark)
    return sum(v["ref"] for v in vs).reshape(N, 48) / (V * W * H)


def settings(views, dev, deg, bg=None):
    """One settings tuple per view, all carrying the SAME background tensor (group_views then compares identities: no device read)."""
    ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
    bg = torch.tensor(ic.BG, dtype=torch.float32, device=dev) if bg is None else bg
    return [ts.make_settings(sc, dev, deg, bg=bg)._replace(bg=bg) for sc in views]


def away_camera(sc):
    """The camera of `sc` turned by 180 degrees about its own y axis and moved 20 units along its new viewing direction: the whole
    cloud (depths -1 .. 10 in front of `sc`, the few points behind its near plane included) lies behind it -- a view that sees nothing."""
    w2c = sc["viewmatrix"].t().clone()
    flip = torch.diag(torch.tensor([-1.0, 1.0, -1.0]))
    cam = syn.make_camera(sc["image_width"], sc["image_height"], syn.FOVX_FRANCIS, flip @ w2c[:3, :3],
                          flip @ w2c[:3, 3] - torch.tensor([0.0, 0.0, 20.0]))
    out = dict(sc)
    for k in ("viewmatrix", "projmatrix", "campos", "tanfovx", "tanfovy"):
        out[k] = cam[k]
    return out
