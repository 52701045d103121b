"""GPU: the default blend backward equals the fixed-order one, bit for bit.

The default backward and the fixed-order mode ("deterministic_backward") run the same kernel, k_blend_bwd2 (the only backward blend),
whose two waves add into a tile's LDS row commutatively: both form the same float32 part per (tile, Gaussian).  They differ only in how those parts are summed into the Gaussian's 10-double row (kGG, csrc/blend_common.h): float64 atomics in arrival
order (default: the flush of k_blend_bwd2, the prologue's fill of the rows, the `v != 0` skip) or float64 in list order (k_det_reduce
over a slot per (tile, instance)).  Exact sums give the same bits either way, so every gradient the product returns -- means2D and
the camera / points_transform gradients included -- must be equal, apart from rare rounding-boundary flips of inexact sums
(tests/parity.py same_accumulation: at most 4 entries per tensor, each within 1e-5 of itself).  A lost or doubled tile part, a wrong
row stride or a fill that misses a ragged tail moves an entry by a share of itself.  Each case reaches a different part of the route.
Measured on MI355X: no differing entry in any case, in two runs."""
import importlib

import numpy as np
import pytest
import torch

import parity

pytestmark = pytest.mark.gpu
L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
raster = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
bt = importlib.import_module("3dgs_hierarchical_training_amd.batched")
ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")


def _fixed_order(fn):
    lib = L.load()
    assert lib.gsr_set_option(b"deterministic_backward", 1) == 0
    try:
        return fn()
    finally:
        lib.gsr_set_option(b"deterministic_backward", 0)


def _both(kw, grads, what):
    """Default backward, then the fixed-order one, of the same render; every gradient compared."""
    import hip_runner
    a = hip_runner.run_hip(kw, grads, cam_grad=True)
    b = _fixed_order(lambda: hip_runner.run_hip(kw, grads, cam_grad=True))
    for x, y in zip(a["fwd"], b["fwd"]):
        assert np.array_equal(x, y), what
    assert set(a["grads"]) == set(b["grads"]) and {"means2D", "viewmatrix", "projmatrix", "campos"} <= set(a["grads"])
    assert any(np.abs(v).max() > 0 for v in b["grads"].values()), what
    return parity.same_accumulation(a["grads"], b["grads"], what)


def _scene_case(N, W, H, deg, posed=True, seed=None, smod=1.0, mode="sh", color_only=False, needles=False):
    sc = parity.syn.make_scene(N, W, H, sh_degree=deg, seed=N % 97 if seed is None else seed, posed=posed)
    sc["scale_modifier"] = smod
    if needles:    # the scene of test_gpu_parity.py::test_faint_elongated_splats: parts of opposite sign cancel over a needle's tiles
        g = torch.Generator().manual_seed(8)
        sc["scales"] = sc["scales"] * torch.tensor([12.0, 0.6, 0.6])
        sc["opacities"] = torch.sigmoid(-3.0 + torch.randn(N, 1, generator=g))
    kw = parity.scene_kwargs(sc, mode, bg=(0.1, 0.2, 0.3))
    gc, gd, ga = parity.upstream_grads(H, W, seed=4)
    if color_only:      # HAS_DA = false: the row's gz slot stays unused
        gd = ga = None
    return kw, (gc, gd, ga)


CASES = {
    "ragged-330x250-deg2": dict(N=20000, W=330, H=250, deg=2),
    "headline-300k-980x545-deg3": dict(N=300000, W=980, H=545, deg=3),
    "colour-only": dict(N=20000, W=320, H=240, deg=3, color_only=True),
    "large-splats-x12": dict(N=3000, W=320, H=240, deg=1, smod=12.0),
    "needles": dict(N=8000, W=320, H=240, deg=3, seed=55, needles=True),
    "N4097-precomp": dict(N=4097, W=256, H=192, deg=0, mode="pre"),
    "N30001-mixed": dict(N=30001, W=256, H=256, deg=0, mode="mixed"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_default_accumulation_equals_fixed_order(name):
    kw, grads = _scene_case(**CASES[name])
    _both(kw, grads, name)


@pytest.mark.parametrize("tile_sort", [0, 1])
def test_default_accumulation_equals_fixed_order_on_both_binning_routes(tile_sort):
    lib = L.load()
    kw, grads = _scene_case(60000, 640, 360, 3)
    assert lib.gsr_set_option(b"tile_sort", tile_sort) == 0
    try:
        _both(kw, grads, f"tile_sort={tile_sort}")
    finally:
        lib.gsr_set_option(b"tile_sort", 1)


def test_default_accumulation_equals_fixed_order_on_split_deep_tiles():
    """The scene of test_deep_lists_split_backward: the pieces of a split tile flush their parts separately."""
    lib = L.load()
    N, W, H = 60000, 128, 96
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=77, posed=True)
    g = torch.Generator().manual_seed(3)
    sc["opacities"] = torch.sigmoid(-3.8 + 0.5 * torch.randn(N, 1, generator=g))
    kw = parity.scene_kwargs(sc, "sh", bg=(0.3, 0.1, 0.2))
    grads = parity.upstream_grads(H, W, seed=6)
    try:
        for split in (1, 4, 7):
            assert lib.gsr_set_option(b"bwd_split", split) == 0
            _both(kw, grads, f"deep lists, bwd_split {split}")
    finally:
        lib.gsr_set_option(b"bwd_split", 0)
    assert raster.last_call_info()["staged"] > 48 * 600, "scene not deep enough to exercise the split"


def test_default_accumulation_equals_fixed_order_after_a_larger_model():
    """A large model's backward, then a smaller model's in the same process: the smaller one reuses the row buffer, whose rows the
    prologue must clear up to the smaller N (30001: not a multiple of 4 or of 128)."""
    import hip_runner
    big, gbig = _scene_case(300000, 980, 545, 3, seed=5)
    hip_runner.run_hip(big, gbig, cam_grad=True)
    kw, grads = _scene_case(30001, 980, 545, 3, seed=6)
    _both(kw, grads, "30001 after 300k")


def test_default_accumulation_equals_fixed_order_on_a_batched_render():
    """Three models of one store (rasterize_gaussians_raw(..., batch_first_block=...)), each under its own camera and pose transform:
    every raw-parameter gradient, means2D and dL/d(points_transform)."""
    dev = torch.device("cuda:0")
    W, H = 330, 250
    sizes = (5000, 12800, 7001)
    scenes = [parity.syn.make_scene(n, W, H, sh_degree=3, seed=40 + k, posed=True) for k, n in enumerate(sizes)]
    batch = bt.BatchedGaussianParams(scenes, dev, optimizer="torch")
    bset = bt.batch_settings([ts.make_settings(sc, dev, 3) for sc in scenes], dev)
    pose = importlib.import_module("3dgs_hierarchical_training_amd.pose")
    Ms = torch.stack([pose.se3_exp(torch.tensor(v))[:3] for v in
                      ([0.0] * 6, [0.02, -0.01, 0.015, 0.004, -0.003, 0.002], [-0.015, 0.01, 0.02, -0.002, 0.004, 0.001])]).to(dev)
    w = torch.rand(len(sizes), 3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    wd = torch.rand(len(sizes), 1, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(2))

    def run():
        raw = {k: v.detach().clone().requires_grad_(True) for k, v in batch.raw().items()}
        M = Ms.clone().requires_grad_(True)
        m2d = torch.zeros_like(raw["_xyz"], requires_grad=True)
        img, _, depth, alpha = raster.rasterize_gaussians_raw(raw["_xyz"], m2d, raw["_features_dc"], raw["_features_rest"], raw["_opacity"],
                                                              raw["_scaling"], raw["_rotation"], bset, points_transform=M,
                                                              batch_first_block=batch.first_block)[:4]
        ((img * w).sum() + 0.1 * (depth * wd).sum() + 0.2 * (alpha * wd).sum()).backward()
        out = {k: v.grad for k, v in raw.items()}
        out["means2D"], out["points_transform"] = m2d.grad, M.grad
        return out

    a = run()
    b = _fixed_order(run)
    assert all(v is not None for v in a.values()) and float(b["points_transform"].abs().max()) > 0
    parity.same_accumulation(a, b, "batched, three models")
