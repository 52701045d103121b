"""GPU: merge-time importance without a backward (include/gsr.h gsr_importance_accumulate, hierarchy.calc_importance route="kernel")
against the float64 oracle's  sum_views |backward(gate)["shs"]| / pixels  at the project's bar for this quantity
(max|imp - ref| <= 1e-3 ref.max(), tests/test_gpu_fused.py:319).  Scenes and references: tests/importance_common.py."""
import ctypes as C
import importlib
import math
import types

import numpy as np
import pytest
import torch

import importance_common as ic
import parity
from oracle import binding
from test_python_sh_cpu import PythonShRender, python_sh_colour

pytestmark = pytest.mark.gpu
hier = ic.hier
ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
E = importlib.import_module("3dgs_hierarchical_training_amd._ext")
L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
refstub = importlib.import_module("3dgs_hierarchical_training_amd.refstub")
DEV = torch.device("cuda:0")
N_B, W_B, H_B = ic.SCENE_B


def _case(N, W, H, deg, dark=False):
    """(segment on the device, settings per view, oracle importance [N,48]); the views' conditions are asserted first."""
    base, views = ic.scene(N, W, H, deg, dark)
    for i, v in enumerate(ic.oracle_views(N, W, H, deg, dark)):
        ic.assert_meaningful(ic.conditions(v["color"], v["rgb"], v["radii"]), f"{N}/{W}x{H}/deg{deg}{'/dark' if dark else ''} view {i}", dark)
    return ic.segment(base, DEV), ic.settings(views, DEV, deg), ic.oracle_importance(N, W, H, deg, dark)


def _within_bar(imp, ref, what):
    err, top = float(np.abs(np.asarray(imp, np.float64) - ref).max()), float(ref.max())
    print(f"[importance] {what}: max err {err:.3e} = {err / top:.2e} of the maximum entry")
    assert np.isfinite(np.asarray(imp)).all() and err <= ic.RTOL * top, (what, err, top)


def _acc_views(seg, views, fill=0.0, **kw):
    acc = torch.full((seg["_xyz"].shape[0], 16, 3), fill, dtype=torch.float32, device=DEV)
    for rs in views:
        R.importance_accumulate(acc, seg["_xyz"], seg["_features_dc"], seg["_opacity"], seg["_scaling"], seg["_rotation"], rs,
                                sh_rest=seg["_features_rest"], raw_params=True, **kw)
    return acc


PARITY = [ic.SCENE_A, ic.SCENE_B + (0,), ic.SCENE_B + (1,), ic.SCENE_B + (2,), ic.SCENE_B + (2, True)]


@pytest.mark.parametrize("case", PARITY, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-d{c[3]}" + ("-dark" if len(c) > 4 else ""))
def test_kernel_route_matches_the_oracle(case):
    """1. Kernel route against the oracle on scene A and on scene B at degrees 0, 1, 2 (and on scene B with a tenth of the rows
    SH-clamped in one channel); for D < 3 the entries of the coefficients >= (D+1)^2 are exactly 0.0."""
    seg, views, ref = _case(*case)
    imp = hier.calc_importance(seg, views, route="kernel")
    assert tuple(imp.shape) == (case[0], 48) and imp.dtype == torch.float32 and not imp.requires_grad
    _within_bar(imp.cpu().numpy(), ref, f"kernel route {case}")
    nc = (case[3] + 1) ** 2
    assert float(imp.view(-1, 16, 3)[:, nc:].abs().max() if nc < 16 else 0.0) == 0.0
    assert all(seg[k].grad is None for k in seg)


@pytest.mark.parametrize("dark", [False, True], ids=["A", "A-dark"])
def test_zero_rows_are_neither_read_nor_written(dark):
    """2. Rows whose oracle importance is zero come out exactly 0.0; with the accumulator prefilled with 7.0 those rows still hold
    7.0 bit for bit, the others 7.0 + their sum within the bar.  (A-dark: a tenth of the rows SH-clamped in one channel.)"""
    N, W, H, deg = ic.SCENE_A
    seg, views, ref = _case(N, W, H, deg, dark)
    zero = ref.max(1) == 0
    assert 0.3 < zero.mean() < 0.7
    imp = hier.calc_importance(seg, views, route="kernel").cpu().numpy()
    assert (imp[zero] == 0.0).all()
    acc = _acc_views(seg, views, fill=7.0).cpu().numpy().reshape(N, 48)
    assert (acc[zero] == np.float32(7.0)).all()
    sums = (acc.astype(np.float64) - 7.0) / (2 * W * H)
    err = np.abs(sums - ref)[~zero].max()
    # (7 + x carries an absolute rounding of 2^-22 per entry on top of the bar)
    assert err <= ic.RTOL * ref.max() + 2.0 ** -22 / (2 * W * H), err


def test_two_views_in_one_call_equal_two_calls():
    """3. Two views in one call against the sum of two one-view calls: equal within 1e-6 of the maximum (float atomics: the order of
    the adds differs from run to run); num_pixels is divided once."""
    N, W, H, deg = ic.SCENE_A
    seg, views, _ = _case(N, W, H, deg)
    both = hier.calc_importance(seg, views, route="kernel")
    one = [hier.calc_importance(seg, [v], route="kernel") for v in views]
    want = (one[0] + one[1]) / 2
    assert float((both - want).abs().max()) <= 1e-6 * float(want.max())


@pytest.mark.parametrize("case,ratio", [(ic.SCENE_A, 0.75), (ic.SCENE_B + (2,), 0.6), (ic.SCENE_A + (True,), 0.75), (ic.SCENE_B + (2, True), 0.6)],
                         ids=["A", "B", "A-dark", "B-dark"])
def test_kernel_route_against_autograd_route(case, ratio):
    """4. Both routes within the bar of the oracle; their prune masks differ only in Gaussians whose oracle score lies within 5e-3
    of the threshold score, and in < 1 % of the rows (the pattern of tests/test_gpu_segments.py:99-109)."""
    seg, views, ref = _case(*case)
    N = case[0]
    k_imp = hier.calc_importance(seg, views, route="kernel")
    a_imp = hier.calc_importance(seg, views, route="autograd")
    _within_bar(k_imp.cpu().numpy(), ref, "kernel route")
    _within_bar(a_imp.cpu().numpy(), ref, "autograd route")
    dk, da = hier.prune_mask(k_imp, ratio).cpu().numpy(), hier.prune_mask(a_imp, ratio).cpu().numpy()
    score = ref.max(1)
    thr = np.sort(score)[int(N * ratio) - 1]
    assert thr > 0                                    # the ratio lies above the zero-row share
    diff = dk != da
    assert diff.mean() < 0.01
    assert (np.abs(score[diff] - thr) <= 5e-3 * max(thr, 1e-30)).all()


def _fwd_args(seg, rs, xf=None):
    e = torch.empty(0, device=DEV)
    return (seg["_xyz"], seg["_features_dc"], e, seg["_opacity"], seg["_scaling"], seg["_rotation"], e, seg["_features_rest"],
            rs.viewmatrix, rs.projmatrix, rs.campos, rs.bg, e if xf is None else xf)


def test_the_pass_disturbs_nothing():
    """5. out_color / out_depth / out_alpha / radii cloned before the pass equal those after it bit for bit, and an ordinary backward
    of that forward run after the pass gives gradients within parity.py's bars of a backward with no pass in between."""
    N, W, H, deg = ic.SCENE_A
    seg, views, _ = _case(N, W, H, deg)
    ops, rs = E.load(), views[0]
    e, eb = torch.empty(0, device=DEV), torch.empty(0, dtype=torch.uint8, device=DEV)
    geo = (H, W, float(rs.tanfovx), float(rs.tanfovy), 1.0, deg, True)
    with torch.no_grad():
        out = ops.rasterize_forward(*_fwd_args(seg, rs), *geo, False, False, eb, [], 0, 0, None)
        color, radii, depth, alpha, geom, image, binning, meta = out[:8]
        before = [t.clone() for t in (color, radii, depth, alpha)]
        gc, gd, ga = (torch.from_numpy(g).to(DEV) for g in parity.upstream_grads(H, W, seed=3))
        names = ("means3D", "means2D", "shs", "colors", "opacities", "scales", "rotations", "cov", "shs_rest")

        def backward():
            g = ops.rasterize_backward(*_fwd_args(seg, rs), geom, image, binning, meta, gc, gd.reshape(1, H, W), ga.reshape(1, H, W), *geo,
                                       False, False, False, False, [], radii, [], None)
            return {k: v.cpu().numpy() for k, v in zip(names, g) if v is not None and v.numel()}
        plain = backward()
        acc = torch.zeros(N, 16, 3, device=DEV)
        ops.importance_pass(acc, seg["_xyz"], seg["_features_dc"], seg["_features_rest"], rs.campos, e, color, geom, image, binning, meta,
                            H, W, deg, None)
        assert float(acc.max()) > 0
        for a, b in zip(before, (color, radii, depth, alpha)):
            assert torch.equal(a, b)
        after = backward()
    assert set(after) == set(plain) and "shs_rest" in after
    parity.check_grads(after, plain, "backward behind the importance pass")
    # and the pass on the forward's own buffers is what the one-call op computes
    acc2 = _acc_views(seg, [rs])
    assert float((acc2 - acc).abs().max()) <= 1e-6 * float(acc.max())


def _rigid():
    """20 degrees about an oblique axis plus a translation, [3,4]."""
    ax = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    ax = ax / ax.norm()
    K = torch.tensor([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]], dtype=torch.float64)
    a = math.radians(20.0)
    Rm = torch.eye(3, dtype=torch.float64) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    t = torch.tensor([0.3, -0.2, 0.4], dtype=torch.float64)
    return Rm, t


def test_variant_points_transform():
    """6a. A rigid points_transform: the stored means are the scene's moved by the inverse, the kernels move them back; against the
    oracle on the moved means (the kernel's own rounding of the move) with the unmoved SH."""
    deg = 2
    base, views = ic.scene(N_B, W_B, H_B, deg)
    Rm, t = _rigid()
    raw = ((base["means3D"].double() - t) @ Rm).float()                 # R^T (p - t)
    xf = torch.cat((Rm, t[:, None]), 1).float()
    from test_gpu_python_sh import _posed_as_the_kernel
    posed = _posed_as_the_kernel(raw, xf)
    ref = np.zeros((N_B, 16, 3))
    for i, sc in enumerate(views):
        sc2 = dict(sc)
        sc2["means3D"] = posed
        o = binding.OracleRender(**parity.scene_kwargs(sc2, "sh", bg=ic.BG))
        color, radii = o.forward()[:2]
        ic.assert_meaningful(ic.conditions(color, o.geom()["rgb"], radii), f"points_transform view {i}")
        ref += np.abs(o.backward(ic.gate_of(color), None, None)["shs"])
        o.close()
    ref = ref.reshape(N_B, 48) / (2 * W_B * H_B)
    b2 = dict(base)
    b2["means3D"] = raw
    seg = ic.segment(b2, DEV)
    acc = _acc_views(seg, ic.settings(views, DEV, deg), points_transform=xf.to(DEV))
    _within_bar(acc.cpu().numpy().reshape(N_B, 48) / (2 * W_B * H_B), ref, "points_transform")


def test_variant_sh_origin():
    """6b. sh_origin set: against the oracle's `convert_SHs_python` statement (tests/test_gpu_python_sh.py) -- the oracle renders the
    formulation's colours as colors_precomp, its colour gradient under the gate is chained through the formulation to the SH tensor
    in float64."""
    deg = 2
    base, views = ic.scene(N_B, W_B, H_B, deg)
    seg = ic.segment(base, DEV)
    x64, sh64 = base["means3D"].double(), base["shs"].double()
    ref, origins = np.zeros((N_B, 16, 3)), []
    for i, sc in enumerate(views):
        o3 = sc["campos"].double() + torch.tensor([0.3, -0.25, 0.2], dtype=torch.float64)
        origins.append(o3.float())
        leaf = sh64.clone().requires_grad_(True)
        col = python_sh_colour(x64, leaf, origins[-1].double(), deg)
        kw = parity.scene_kwargs(sc, "sh", bg=ic.BG)
        kw.pop("shs")
        o = binding.OracleRender(**kw, colors_precomp=col.detach().float())
        color, radii = o.forward()[:2]
        ic.assert_meaningful(ic.conditions(color, col.detach().numpy(), radii), f"sh_origin view {i}")
        S = torch.from_numpy(o.backward(ic.gate_of(color), None, None)["colors_precomp"])
        o.close()
        ref += torch.autograd.grad(col, leaf, S)[0].abs().numpy()
    ref = ref.reshape(N_B, 48) / (2 * W_B * H_B)
    acc = torch.zeros(N_B, 16, 3, device=DEV)
    for rs, o3 in zip(ic.settings(views, DEV, deg), origins):
        R.importance_accumulate(acc, seg["_xyz"], seg["_features_dc"], seg["_opacity"], seg["_scaling"], seg["_rotation"], rs,
                                sh_rest=seg["_features_rest"], raw_params=True, sh_origin=o3.to(DEV))
    _within_bar(acc.cpu().numpy().reshape(N_B, 48) / (2 * W_B * H_B), ref, "sh_origin")


def test_variant_activated_parameters_and_ctypes_binding(monkeypatch):
    """6c-d. Activated parameters (one [N,16,3] SH tensor, sigmoid / exp / normalize in torch) instead of raw ones, within the bar of
    the oracle; GSR_BINDING=ctypes against the extension within 1e-6 of the maximum (the order of the atomic adds differs)."""
    deg = 2
    seg, views, ref = _case(N_B, W_B, H_B, deg)
    acc = torch.zeros(N_B, 16, 3, device=DEV)
    shs = torch.cat((seg["_features_dc"], seg["_features_rest"]), 1).contiguous()
    for rs in views:
        R.importance_accumulate(acc, seg["_xyz"], shs, torch.sigmoid(seg["_opacity"]), torch.exp(seg["_scaling"]),
                                torch.nn.functional.normalize(seg["_rotation"]), rs, raw_params=False)
    _within_bar(acc.cpu().numpy().reshape(N_B, 48) / (2 * W_B * H_B), ref, "activated parameters")
    ext = hier.calc_importance(seg, views, route="kernel")
    monkeypatch.setenv("GSR_BINDING", "ctypes")
    assert E.use_ctypes()
    ct = hier.calc_importance(seg, views, route="kernel")
    monkeypatch.delenv("GSR_BINDING")
    assert float((ct - ext).abs().max()) <= 1e-6 * float(ext.max())
    _within_bar(ct.cpu().numpy(), ref, "ctypes binding")


def test_variant_refusals(monkeypatch):
    """6e. colors_precomp (no SH) or a batch of two: the error, not a result -- on both bindings where they serve the call."""
    deg = 2
    seg, views, _ = _case(N_B, W_B, H_B, deg)
    rs = views[0]
    acc = torch.zeros(N_B, 16, 3, device=DEV)
    col = torch.rand(N_B, 3, device=DEV)
    with pytest.raises(RuntimeError, match="SH coefficients"):
        R.importance_accumulate(acc, seg["_xyz"], None, seg["_opacity"], seg["_scaling"], seg["_rotation"], rs, raw_params=True, colors_precomp=col)
    with pytest.raises(RuntimeError, match="batch"):
        R.importance_accumulate(acc, seg["_xyz"], seg["_features_dc"], seg["_opacity"], seg["_scaling"], seg["_rotation"], rs,
                                sh_rest=seg["_features_rest"], raw_params=True, batch_first_block=[0, 8, 16])
    monkeypatch.setenv("GSR_BINDING", "ctypes")
    with pytest.raises(RuntimeError):          # the C ABI's own refusal (GSR_ERR_ARG): acc has no SH layout to add to
        R.importance_accumulate(torch.zeros(N_B, 0, 3, device=DEV), seg["_xyz"], None, torch.sigmoid(seg["_opacity"]), torch.exp(seg["_scaling"]),
                                torch.nn.functional.normalize(seg["_rotation"]), rs, colors_precomp=col)
    assert float(acc.abs().max()) == 0.0
    # the C entry itself: a batch of two and colors_precomp are GSR_ERR_ARG (-1)
    lib = L.load()
    a, out = L.GsrForwardArgs(), L.GsrForwardOut()
    a.N, a.M, a.D, a.W, a.H = N_B, 16, deg, W_B, H_B
    a.shs, a.campos, a.colors_precomp = seg["_features_dc"].data_ptr(), rs.campos.data_ptr(), col.data_ptr()
    assert lib.gsr_importance_accumulate(C.byref(a), C.byref(out), acc.data_ptr(), acc.data_ptr(), None) == -1
    a.colors_precomp = None
    fb = (C.c_int32 * 3)(0, 8, 16)

    class _Batch(C.Structure):
        _fields_ = [("B", C.c_int32), ("first_block", C.POINTER(C.c_int32))]
    bt = _Batch(2, fb)
    a.batch = C.cast(C.pointer(bt), C.c_void_p)
    assert lib.gsr_importance_accumulate(C.byref(a), C.byref(out), acc.data_ptr(), acc.data_ptr(), None) == -1
    assert float(acc.abs().max()) == 0.0


def _prof(lib, name):
    tot, cnt = C.c_double(0), C.c_int64(0)
    assert lib.gsr_profile_read(name.encode(), C.byref(tot), C.byref(cnt)) == 0
    return int(cnt.value)


def test_no_backward_runs():
    """7. With the `profile` option on, the profile counts of the backward blend and of the per-Gaussian backward do not move across
    a kernel-route calc_importance; the new stages' counts rise by the number of views."""
    seg, views, _ = _case(N_B, W_B, H_B, 2)
    lib = L.load()
    hier.calc_importance(seg, views, route="kernel")
    torch.cuda.synchronize()
    lib.gsr_set_option(b"profile", 1)
    try:
        for n in ("blend_bwd", "preprocess_bwd", "importance_blend", "importance_finish", "blend_fwd"):
            _prof(lib, n)                      # (reading drains a stage)
        hier.calc_importance(seg, views, route="kernel")
        torch.cuda.synchronize()
        counts = {n: _prof(lib, n) for n in ("blend_bwd", "preprocess_bwd", "importance_blend", "importance_finish", "blend_fwd")}
    finally:
        lib.gsr_set_option(b"profile", 0)
    assert counts == {"blend_bwd": 0, "preprocess_bwd": 0, "importance_blend": len(views), "importance_finish": len(views),
                      "blend_fwd": len(views)}, counts


def test_existing_tests_shape():
    """8. 20 000 Gaussians, 320x240, degree 3, brightened as above, at the bar."""
    N, W, H, deg = ic.SCENE_C
    seg, views, ref = _case(N, W, H, deg)
    imp = hier.calc_importance(seg, views, route="kernel").cpu().numpy()
    _within_bar(imp, ref, "20000/320x240/deg3")
    zero = ref.max(1) == 0
    assert (imp[zero] == 0.0).all()


def _lie(pose7, delta):
    p = refstub.LieGroupParameter(refstub.SE3(torch.tensor([pose7], device=DEV)))
    with torch.no_grad():
        p.copy_(torch.tensor([delta], device=DEV))
    return p


@pytest.mark.parametrize("posed", [False, True], ids=["identity", "frame-pose"])
@pytest.mark.parametrize("python_sh", [False, True], ids=["module-sh", "convert_SHs_python"])
def test_autopatch_on_trainer_shaped_objects(posed, python_sh):
    """9. The patched `calc_importance` on refstub's trainer-shaped objects equals hierarchy's kernel route on the same tensors within
    1e-6 of the maximum: the identity camera, the frame pose through get_xyz, convert_SHs_python on and off.  It leaves .grad None."""
    import gsr_autopatch
    deg = 2
    base, views = ic.scene(N_B, W_B, H_B, deg)
    p = ts.GaussianParams(base, DEV, optimizer="torch")
    p.active_sh_degree = deg
    r = PythonShRender(p, bg=ic.BG)
    g = r.gaussians
    if posed:
        g.P = [_lie([0.0, 0, 0, 0, 0, 0, 1], [0.0] * 6), _lie([0.02, -0.03, 0.01, 0.01, 0.0, -0.01, 1.0], [0.01, -0.02, 0.015, 0.004, -0.003, 0.002])]
        g.rotate_seq, g.seq_idx = True, 1
    cams = [refstub.StubCamera.from_scene(sc, DEV, uid=1) for sc in views]
    pipe = types.SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=python_sh)
    p._features_dc.grad = torch.ones_like(p._features_dc)
    got = gsr_autopatch.calc_importance_fused(r, cams, pipe)
    assert p._features_dc.grad is None and p._features_rest.grad is None and tuple(got.shape) == (N_B, 48) and not got.requires_grad
    seg = {k: getattr(p, k).detach() for k in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")}
    with torch.no_grad():
        M = gsr_autopatch._pose_matrix(g) if posed else None
        o = gsr_autopatch._sh_origin(g, cams[0], DEV) if python_sh else None
    want = hier._calc_importance_kernel(seg, ic.settings(views, DEV, deg), points_transform=M, sh_origin=o)
    assert float(want.max()) > 0 and float((got - want).abs().max()) <= 1e-6 * float(want.max())
    if not posed and not python_sh:
        _within_bar(got.cpu().numpy(), ic.oracle_importance(N_B, W_B, H_B, deg), "patched calc_importance")
