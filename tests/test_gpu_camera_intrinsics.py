"""GPU: the kernels under cameras with real intrinsics -- fx != fy, principal point off the image centre, frustum clamp acting on visible
splats (tests/camera_common.py; tests/test_camera_intrinsics_cpu.py holds the oracle and gsr_math.h to known answers under them).

Every other test of this suite renders through synthetic.make_camera (fy = fx, principal point at the centre): the principal-point
entries of projmatrix are exactly zero there, and fx / fy, limx / limy, tanfovx / tanfovy are interchangeable.  The GPU-only parts --
binning and direct binning, the list cut and its pose-keyed cache, both blends, the camera-gradient reduction, the batched tall image,
the render-only and frozen calls, the pose step on the camera -- had never seen another camera.  All comparisons go through
parity.oracle_case / check_grads at the suite's bars, or are the equalities the corresponding test of the centred camera asserts.

Measured on MI355X, next to the host emulation of gsr_math.h on the same inputs (bars: 5 % edge pixels, 1e-4 norm-wise).  A =
20 000 / 330x250 / deg 3 / sh, B = 5 000 / 160x120 / deg 0 / pre, C = 8 000 / 200x150 / deg 1 / mixed; "worst" is the largest norm-wise
relative error of any gradient tensor -- dL/dviewmatrix in every row but both-B (opacities) -- and "per-Gaussian" the largest among
means3D, means2D, opacities, colour, scales, rotations, cov3D:

    case          edge pixels GPU / host   worst GPU / host     per-Gaussian worst GPU / host
    aniso A       0.744 % / 0.746 %        4.3e-5 / 4.5e-5      4.1e-6 (opacities) / 1.5e-5 (scales)
    aniso C       0.397 % / 0.400 %        9.0e-6 / 6.8e-6      3.6e-6 (opacities) / 1.7e-6 (opacities)
    offcentre A   0.658 % / 0.659 %        2.7e-5 / 2.3e-5      5.6e-6 (opacities) / 1.8e-5 (scales)
    offcentre C   0.433 % / 0.433 %        4.3e-6 / 6.8e-6      2.4e-6 (opacities) / 3.2e-6 (opacities)
    both A        0.670 % / 0.675 %        6.5e-6 / 1.3e-5      4.9e-6 (opacities) / 3.7e-6 (rotations)
    both B        0.354 % / 0.349 %        3.8e-6 / 3.9e-6      3.8e-6 (opacities) / 3.9e-6 (opacities)
    both C        0.483 % / 0.483 %        8.2e-6 / 1.2e-5      3.1e-6 (opacities) / 3.2e-6 (opacities)
    far A         0.737 % / 0.733 %        1.1e-5 / 1.8e-5      5.0e-6 (opacities) / 5.6e-6 (opacities)
    far C         0.420 % / 0.420 %        1.3e-5 / 2.7e-5      1.6e-6 (opacities) / 1.9e-6 (rotations)
    far-both A    0.678 % / 0.676 %        1.4e-5 / 3.5e-5      7.8e-6 (opacities) / 8.2e-6 (opacities)
    far-both B    0.365 % / 0.370 %        1.3e-5 / 1.0e-5      7.2e-6 (opacities) / 8.5e-6 (opacities)
    far-both C    0.467 % / 0.467 %        3.1e-6 / 1.4e-5      2.3e-6 (opacities) / 4.8e-6 (rotations)

No pixel is unresolved in any case; the stage-A model under "both" (250x188, every pixel)
has 0.33 % edge pixels and 1.3e-5 at worst, the cut renders 0.24 % / 0.37 % and 8.9e-6."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import camera_common as cc
import parity
from oracle import binding

pytestmark = pytest.mark.gpu
L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
DEV = torch.device("cuda:0")

# N, W, H, degree, mode
SHAPE_A = (20000, 330, 250, 3, "sh")          # ragged tile grid, every SH band
SHAPE_B = (5000, 160, 120, 0, "pre")          # colors_precomp + cov3D_precomp
SHAPE_C = (8000, 200, 150, 1, "mixed")        # colors_precomp + scales / rotations
BG = (0.2, 0.1, 0.3)


def parity_inputs(name, shape):
    """(kwargs, upstream gradients) of the parity case `name` x `shape`: the posed general scene of seed 1."""
    N, W, H, deg, mode = shape
    sc = cc.general_scene(N, W, H, deg, 1, name, posed=True)
    return parity.scene_kwargs(sc, mode, bg=BG), parity.upstream_grads(H, W, seed=3)


def _oracle_parity(kw, upstream, what, mode, prepare=None):
    """Forward and backward, camera gradients included, against the float64 oracle at the suite's bars."""
    import hip_runner
    o = binding.OracleRender(**kw)
    if prepare is not None:
        prepare()
    rep, out, ref = parity.oracle_case(o, lambda g: hip_runner.run_hip(kw, g, cam_grad=True), upstream, what)
    got = dict(out["grads"])
    if mode != "sh":
        got.pop("campos")                      # (the camera centre reaches the image through the SH view direction alone)
    grep = parity.check_grads(got, ref, what)
    assert np.all(out["grads"]["projmatrix"].reshape(16)[2::4] == 0)     # clip-z row is unused
    assert float(np.abs(out["grads"]["viewmatrix"]).max()) > 0 and float(np.abs(out["grads"]["projmatrix"]).max()) > 0
    assert (out["fwd"][1] > 0).sum() > kw["means3D"].shape[0] // 2
    print(f"[intrinsics] {what}: edge pixels {rep['ambig_frac']:.4%}, unresolved {rep['unresolved_frac']:.4%}, worst rel err "
          + ", ".join(f"{k} {v:.1e}" for k, v in grep.items() if "/" not in k))
    o.close()
    return out


@pytest.mark.parametrize("shape", [SHAPE_A, SHAPE_C], ids=lambda s: f"{s[0]}-{s[1]}x{s[2]}-d{s[3]}-{s[4]}")
@pytest.mark.parametrize("name", cc.CAMERA_NAMES)
def test_parity_vs_oracle_under_real_intrinsics(name, shape):
    """Forward, every input's gradient and dL/d(viewmatrix, projmatrix, campos) under each camera of the table."""
    kw, up = parity_inputs(name, shape)
    _oracle_parity(kw, up, f"hip {name} {shape[0]}/{shape[1]}x{shape[2]}/deg{shape[3]}/{shape[4]}", shape[4])


def test_parity_vs_oracle_precomputed_covariance_under_real_intrinsics():
    """colors_precomp + cov3D_precomp (the second shape) under "both" and "far-both"."""
    for name in ("both", "far-both"):
        kw, up = parity_inputs(name, SHAPE_B)
        _oracle_parity(kw, up, f"hip {name} {SHAPE_B[0]}/{SHAPE_B[1]}x{SHAPE_B[2]}/deg0/pre", "pre")


# option, value, value that restores the default
ROUTES = [("tile_sort", 0, 1), ("tile_sort", 2, 1), ("direct_binning", 0, 1), ("blend_fwd_ppt", 7, 0),
          ("deterministic_backward", 1, 0)]


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: f"{r[0]}={r[1]}")
@pytest.mark.parametrize("name", ["both", "far"])
def test_routes_vs_oracle_under_real_intrinsics(name, route):
    """Each list-building route, the forward blend selected explicitly and the fixed-order accumulation against the oracle."""
    lib = L.load()
    opt, val, default = route
    kw, up = parity_inputs(name, SHAPE_A)
    try:
        assert lib.gsr_set_option(opt.encode(), val) == 0
        _oracle_parity(kw, up, f"hip {name} {opt}={val}", "sh")
    finally:
        lib.gsr_set_option(opt.encode(), default)


def _cut_stats(lib, W, H):
    out = (C.c_int64 * 5)()
    assert lib.gsr_debug_list_cut_stats(W, H, out) == 0
    return [int(v) for v in out]


@pytest.mark.parametrize("name", ["both", "far"])
def test_cut_render_vs_oracle_under_real_intrinsics(name):
    """`list_cut` 2 on the depth-sort route: the third render of the frame (the first sight of a frame is never cut) against the
    oracle, as test_gpu_listcut.py::test_oracle_parity_of_a_cut_render does for the centred camera."""
    import hip_runner
    lib = L.load()
    N, W, H, deg, mode = SHAPE_A
    sc = cc.general_scene(N, W, H, deg, 1, name, posed=True)
    sc["scale_modifier"] = 4.0                      # (dense: the cut leaves whole chunks of the depth order out)
    kw = parity.scene_kwargs(sc, mode, bg=BG)
    assert lib.gsr_set_option(b"view_cache_reset", 1) == 0
    assert lib.gsr_set_option(b"tile_sort", 0) == 0
    assert lib.gsr_set_option(b"list_cut", 2) == 0
    try:
        s0 = [None]

        def two_renders_first():
            hip_runner.run_hip(kw); hip_runner.run_hip(kw)
            s0[0] = _cut_stats(lib, W, H)
        _oracle_parity(kw, parity.upstream_grads(H, W, seed=2), f"hip {name} list_cut=2", mode, prepare=two_renders_first)
        s1 = _cut_stats(lib, W, H)
    finally:
        lib.gsr_set_option(b"tile_sort", 1)
        lib.gsr_set_option(b"list_cut", 1)
    s0 = s0[0]
    print(f"[intrinsics] {name} list_cut=2: counters before {s0}, after {s1}")
    assert s1[0] - s0[0] == 2 and s1[3] > s0[3] and s1[1] == s0[1]       # both oracle_case renders ran cut, chunks were skipped, no repair


@pytest.mark.parametrize("W,H,stride,surface", [(250, 188, 1, "waves"), (250, 188, 2, "plane")], ids=["waves-every-pixel", "plane-stride2"])
def test_stage_a_model_under_real_intrinsics(W, H, stride, surface):
    """Stage A's single-image model (one Gaussian per strided pixel, un-projected through the frame's OWN intrinsics) under "both":
    against the oracle on the route these models take by default and on the global depth sort; the two routes' images equal.
    The scales are the reference's neighbour-distance scale on this grid (x 0.817 of z / fx): with z / fx taken literally the "waves"
    case misses the element-wise bar on the host emulation too -- a matter of splat density, camera_common.pixel_gaussian_scene."""
    import hip_runner
    lib = L.load()
    sc = cc.pixel_gaussian_scene(W, H, stride, surface, cam="both")
    kw = parity.scene_kwargs(sc, "sh", bg=(0.05, 0.1, 0.15))
    imgs = {}
    try:
        for tsort in (1, 0):
            assert lib.gsr_set_option(b"tile_sort", tsort) == 0
            out = _oracle_parity(kw, parity.upstream_grads(H, W, seed=5), f"pixel-Gaussians both {W}x{H}/{stride}/{surface}/tile_sort={tsort}", "sh")
            # every Gaussian of the grid lands on its own pixel: visible, none culled by a misplaced principal point
            assert (out["fwd"][1] > 0).all()
            imgs[tsort] = hip_runner.run_hip(kw)["fwd"]
    finally:
        lib.gsr_set_option(b"tile_sort", 1)
    for a, b in zip(imgs[0], imgs[1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("fixed_order", [True, False], ids=["fixed-order", "default-accumulation"])
def test_one_pose_two_intrinsics_share_a_cache_entry(fixed_order):
    """The per-frame cache (visit counts, the list cut's remembered depths) identifies a frame by view matrix and points transform
    alone: the centred camera and "both" at ONE pose share an entry, so each is cut by the depths the OTHER needed.  The device-side
    repair is what keeps the image exact: rendered alternately, three times each, with backward, every render equals the same render
    with full lists -- image, depth, alpha, radii, R, range starts, list prefixes, and the gradients (equal bits in fixed-order mode,
    parity.same_accumulation on the default accumulation).

    One diagnostic is NOT an equality here, unlike in test_gpu_listcut.py: last_call_info()["staged"], the sum of the tiles' staged
    depths min(list length, batches x batch size).  Under its own frame's cut a tile's list ends at or behind what its waves staged;
    under the OTHER camera's cut a list may end inside the batch in which the wave's last pixel saturates -- the wave is not live, the
    tile needs no repair, every pixel has blended exactly what it blends on the full list, and the counter says `list length` where
    the full list says `batches x batch size`.  The counter only bounds the backward's walk from above: it may be smaller, never
    larger, and the gradients below are still held to equal bits."""
    import test_gpu_listcut as lc
    lib = L.load()
    N, W, H, deg, mode = SHAPE_A
    sc = cc.general_scene(N, W, H, deg, 1, "both", posed=True)
    sc["scale_modifier"] = 4.0                      # (dense: tiles saturate long before their lists end)
    w2c = sc["viewmatrix"].t()
    centred = parity.syn.make_camera(W, H, R=w2c[:3, :3], t=w2c[:3, 3])
    sc_c = dict(sc)
    for k in ("viewmatrix", "projmatrix", "campos", "tanfovx", "tanfovy"):
        sc_c[k] = centred[k]
    assert torch.equal(sc_c["viewmatrix"], sc["viewmatrix"]) and not torch.equal(sc_c["projmatrix"], sc["projmatrix"])
    kws = [parity.scene_kwargs(s, mode, bg=BG) for s in (sc_c, sc)]
    grads = parity.upstream_grads(H, W, seed=5)
    assert lib.gsr_set_option(b"deterministic_backward", 1 if fixed_order else 0) == 0
    assert lib.gsr_set_option(b"tile_sort", 0) == 0          # (the cut serves the depth-sort route: forced, as in test_gpu_listcut.py)
    try:
        assert lib.gsr_set_option(b"list_cut", 0) == 0
        assert lib.gsr_set_option(b"view_cache_reset", 1) == 0 and lib.gsr_set_option(b"reset_speculation", 1) == 0
        full = [lc._render(kw, grads) for kw in kws]
        assert lib.gsr_set_option(b"list_cut", 2) == 0
        assert lib.gsr_set_option(b"view_cache_reset", 1) == 0 and lib.gsr_set_option(b"reset_speculation", 1) == 0
        cut, stats = [], [_cut_stats(lib, W, H)]
        for i in range(6):
            cut.append(lc._render(kws[i % 2], grads))
            stats.append(_cut_stats(lib, W, H))
    finally:
        lib.gsr_set_option(b"list_cut", 1)
        lib.gsr_set_option(b"tile_sort", 1)
        lib.gsr_set_option(b"deterministic_backward", 0)
    for i, st in enumerate(stats):
        print(f"[intrinsics] shared cache entry, after {i} renders: cut renders {st[0]}, repaired renders {st[1]}, repaired tiles {st[2]}, "
              f"chunks skipped {st[3]}, deep tiles {st[4]}")
    assert float(np.abs(full[0][0]["fwd"][0].astype(np.float64) - full[1][0]["fwd"][0]).max()) > 0.1      # two different images
    for i, r in enumerate(cut):
        what = f"render {i} ({'centred' if i % 2 == 0 else 'both'})"
        print(f"[intrinsics] {what}: R {r[3]}, staged {r[4]} (full lists: {full[i % 2][4]})")
        assert r[4] <= full[i % 2][4], (what, r[4], full[i % 2][4])
        lc._equal_renders(r[:4] + (full[i % 2][4],), full[i % 2], what, fixed_order)
    assert stats[-1][0] == 6          # every render ran the cut machinery
    # ... and the test is about something: lists WERE cut by the other camera's depths (chunks of the depth order left out), tiles
    # DID run out of them and were repaired, on more than one render
    assert stats[-1][3] > stats[0][3] and stats[-1][2] > stats[0][2] and stats[-1][1] - stats[0][1] >= 2, stats


@pytest.mark.parametrize("fixed_order", [True, False], ids=["fixed-order", "default-accumulation"])
def test_batched_models_with_a_principal_point_each(fixed_order):
    """Three models in one batch under shared focal lengths ("aniso") and a principal point of their own each (it lives in projmatrix
    alone, so batch_settings accepts it): each model equals the model trained alone, by test_gpu_batched.py's assertions, over 3 steps."""
    import test_gpu_batched as tb
    W, H = 330, 250
    fx, fy = cc.intrinsics("aniso", W, H)[:2]
    pps = [cc.intrinsics(n, W, H)[2:] for n in ("centred", "both", "far-both")]
    assert len(set(pps)) == 3
    tb._batched_training_case((5000, 12800, 7001), 3, fixed_order, camera=lambda k: dict(fx=fx, fy=fy, cx=pps[k][0], cy=pps[k][1]), steps=3)


def test_render_only_equals_the_full_forward_under_real_intrinsics():
    """The render-only call against the full forward under "both": test_gpu_render_only.py's equalities, on every list-building route."""
    import test_gpu_render_only as ro
    sc = cc.general_scene(1000, ro.W, ro.H, 3, 17, "both", posed=True)
    ro._check_on_every_route(ro.Case(sc, "raw", 3), "raw-d3 under both")


def test_frozen_backward_equals_the_full_backward_under_real_intrinsics():
    """The frozen call's camera and transform gradients against the full backward of the same forward under "both", bit for bit in fixed
    order: test_gpu_frozen_backward.py::test_frozen_equals_full_bit_for_bit_in_fixed_order's equalities."""
    import test_gpu_frozen_backward as fb
    N, deg = 1000, 3
    t = fb._tensors(N, deg, True, "split", sc=cc.general_scene(N, fb.W, fb.H, deg, 5, "both", posed=True))
    up = fb._upstream(True)
    xf = torch.tensor(fb.XF, device=DEV)
    with fb.fixed_order():
        f = fb._forward(t, xf)
        assert int(f["meta"][0]) > 0 and int((f["radii"] > 0).sum()) > N // 4
        n0 = fb._frozen_calls()
        runs = [fb._backward(t, f, up, frozen, fb.CAMERA)[1] for frozen in (False, True, True, False)]
        assert fb._frozen_calls() == n0 + 2
    full = runs[0]
    for k in fb.CAMERA + ("d_means2D",):
        assert float(full[k].abs().max()) > 0, k
        for r in runs[1:]:
            assert torch.equal(r[k], full[k]), (k, float((r[k] - full[k]).abs().max()))
    for k in fb.PER_GAUSSIAN:
        if k in full:
            assert torch.equal(runs[3][k], full[k]), k


@pytest.mark.parametrize("route", ["kernel", "autograd"])
def test_importance_matches_the_oracle_under_real_intrinsics(route):
    """Merge-time importance (sum over two views of |dL/dSH| through the clamp gate, / pixels) against the float64 oracle under "both",
    at the project's bar for this quantity (importance_common.RTOL): test_gpu_fused.py::test_calc_importance_matches_oracle's comparison
    on importance_common's brightened scene A."""
    import importance_common as ic
    N, W, H, deg = ic.SCENE_A
    views, ref = _importance_case(N, W, H, deg)
    seg = ic.segment(views[0], DEV)
    imp = ic.hier.calc_importance(seg, ic.settings(views, DEV, deg), route=route).cpu().numpy()
    assert imp.shape == (N, 48) and np.isfinite(imp).all()
    err, top = float(np.abs(imp.astype(np.float64) - ref).max()), float(ref.max())
    print(f"[intrinsics] importance under both, {route} route: max err {err:.3e} = {err / top:.2e} of the maximum entry")
    assert err <= ic.RTOL * top


_IMPORTANCE = {}


def _importance_case(N, W, H, deg):
    """(per-view scenes, oracle importance [N,48]) -- computed once, shared by the two routes."""
    import importance_common as ic
    if not _IMPORTANCE:
        base = cc.general_scene(N, W, H, deg, 31, "both", posed=False)
        base["shs"] = base["shs"].clone()
        base["shs"][:, 0] = 2.0 * base["shs"][:, 0] + 1.5           # brightened, as importance_common.scene: pixels exceed 1
        views, ref = [], np.zeros((N, 16, 3))
        for s in ic.CAM_SEEDS:
            w2c = parity.syn.make_scene(8, W, H, sh_degree=3, seed=s, posed=True)["viewmatrix"].t()     # only its pose is used
            cam = cc.named_camera("both", W, H, R=w2c[:3, :3], t=w2c[:3, 3])
            sc = dict(base)
            sc.update(cam)
            views.append(sc)
            o = binding.OracleRender(**parity.scene_kwargs(sc, "sh", bg=ic.BG))
            color, radii = o.forward()[:2]
            ic.assert_meaningful(ic.conditions(color, o.geom()["rgb"], radii), f"importance under both, view {s}")
            ref += np.abs(o.backward(ic.gate_of(color), None, None)["shs"])
            o.close()
        _IMPORTANCE["case"] = (views, ref.reshape(N, 48) / (len(views) * W * H))
    return _IMPORTANCE["case"]
