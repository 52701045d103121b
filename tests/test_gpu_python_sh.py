"""The SH view origin (include/gsr.h GsrForwardArgs::sh_origin): the reference's `convert_SHs_python` render
(/root/reference/scene/gaussian_model_ht.py:845-865) on the kernels.  The colour's direction is normalize(_xyz - o) of the UNposed
means, o = the camera centre in the model's frame (detached); the geometry is posed by points_transform as ever."""
import ctypes as C
import importlib
import types
import numpy as np
import pytest
import torch

import parity
from oracle import binding
from test_python_sh_cpu import GOLD, PythonShRender, RAW, fixture_case, python_sh_colour

pytestmark = pytest.mark.gpu
ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
refstub = importlib.import_module("3dgs_hierarchical_training_amd.refstub")
L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
DEV = torch.device("cuda:0")


def _transform(seed):
    """A non-identity rigid transform [3,4] (small rotation + shift) and an origin near the camera centre it implies."""
    g = torch.Generator().manual_seed(seed)
    Rm = parity.syn.random_rotation(g, 0.1)
    t = 0.1 * torch.randn(3, generator=g, dtype=torch.float64)
    xf = torch.cat((Rm.double(), t[:, None]), 1).float()
    o = (-(Rm.double().t() @ t) + 0.05 * torch.randn(3, generator=g, dtype=torch.float64)).float()
    return xf, o


def _settings(sc, deg, bg=(0.0, 0.0, 0.0), cam_grad=False):
    t = lambda k: sc[k].to(DEV).requires_grad_(cam_grad)
    return R.GaussianRasterizationSettings(image_height=sc["image_height"], image_width=sc["image_width"], tanfovx=sc["tanfovx"],
                                           tanfovy=sc["tanfovy"], bg=torch.tensor(bg, device=DEV), scale_modifier=1.0,
                                           viewmatrix=t("viewmatrix"), projmatrix=t("projmatrix"), sh_degree=deg,
                                           campos=t("campos"), prefiltered=False, debug=False)


def _raw_leaves(sc):
    p = ts.GaussianParams(sc, DEV, optimizer="torch")
    return {k: getattr(p, k).detach().clone().requires_grad_(True) for k in RAW}


def _run_raw(t, xf, o, rs, grads=None, **kw):
    """rasterize_gaussians_raw with sh_origin; grads = (gc, gd, ga) numpy or None."""
    for v in t.values():
        v.grad = None
    xfl = None if xf is None else xf.to(DEV).clone().requires_grad_(True)
    m2d = torch.zeros(t["_xyz"].shape[0], 3, device=DEV, requires_grad=True)
    color, radii, depth, alpha = R.rasterize_gaussians_raw(t["_xyz"], m2d, t["_features_dc"], t["_features_rest"], t["_opacity"],
                                                           t["_scaling"], t["_rotation"], rs, points_transform=xfl,
                                                           sh_origin=None if o is None else o.to(DEV), **kw)
    out = {"fwd": (color.detach().cpu().numpy(), radii.cpu().numpy(), depth.detach().cpu().numpy(), alpha.detach().cpu().numpy())}
    if grads is not None:
        gc, gd, ga = (None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in grads)
        loss = (color * gc).sum()
        if gd is not None:
            loss = loss + (depth * gd.reshape(depth.shape)).sum()
        if ga is not None:
            loss = loss + (alpha * ga.reshape(alpha.shape)).sum()
        loss.backward()
        out["grads"] = {k: t[k].grad.cpu().numpy() for k in RAW}
        out["grads"]["means2D"] = m2d.grad.cpu().numpy()
        if xfl is not None:
            out["grads"]["points_transform"] = xfl.grad.cpu().numpy()
    return out


def _oracle_chain(t, xf, o, deg, ref):
    """The oracle's gradients w.r.t. (posed means, colours, activated opacity / scale / rotation) chained in float64 through the
    formulation (colour from the UNposed means and the origin; means posed by xf; the activations) to the raw tensors and xf."""
    lv = {k: t[k].detach().cpu().double().requires_grad_(True) for k in RAW}
    x = lv["_xyz"]
    X = None if xf is None else xf.double().requires_grad_(True)
    posed = x if X is None else x @ X[:, :3].t() + X[:, 3]
    col = python_sh_colour(x, torch.cat((lv["_features_dc"], lv["_features_rest"]), 1), o.double(), deg)
    op, sc, rot = torch.sigmoid(lv["_opacity"]), torch.exp(lv["_scaling"]), torch.nn.functional.normalize(lv["_rotation"])
    outs = [posed, col, op, sc, rot]
    gouts = [torch.from_numpy(np.asarray(ref[k], np.float64)).reshape(v.shape) for k, v in
             zip(("means3D", "colors_precomp", "opacities", "scales", "rotations"), outs)]
    leaves = [lv[k] for k in RAW] + ([] if X is None else [X])
    gs = torch.autograd.grad(outs, leaves, gouts)
    res = {k: g.numpy() for k, g in zip(RAW, gs)}
    if X is not None:
        res["points_transform"] = gs[-1].numpy()
    res["means2D"] = ref["means2D"]
    return res


def _posed_as_the_kernel(x, xf):
    """x [N,3] float32 moved by xf [3,4] with the kernel's rounding (apply_points_transform: three nested fmaf per row; an f32 x f32
    product is exact in float64, so each fmaf is one rounding of a float64 sum).  The full-size images are sensitive to the last bit
    of a mean."""
    x = x.double()
    X = xf.double()
    rows = []
    for r in range(3):
        v = (X[r, 2] * x[:, 2] + X[r, 3]).float().double()
        v = (X[r, 1] * x[:, 1] + v).float().double()
        rows.append((X[r, 0] * x[:, 0] + v).float())
    return torch.stack(rows, 1)


def _oracle_inputs(t, xf, o, deg, sc, bg=(0.0, 0.0, 0.0)):
    with torch.no_grad():
        x = t["_xyz"].detach().cpu()
        posed = x if xf is None else _posed_as_the_kernel(x, xf)
        col = python_sh_colour(x.double(), torch.cat((t["_features_dc"], t["_features_rest"]), 1).detach().cpu().double(), o.double(), deg)
        return dict(means3D=posed.float(), opacities=torch.sigmoid(t["_opacity"].detach().cpu()), viewmatrix=sc["viewmatrix"],
                    projmatrix=sc["projmatrix"], campos=sc["campos"], bg=torch.tensor(bg), image_height=sc["image_height"],
                    image_width=sc["image_width"], tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"], sh_degree=0,
                    colors_precomp=col.float(), scales=torch.exp(t["_scaling"].detach().cpu()),
                    rotations=torch.nn.functional.normalize(t["_rotation"].detach().cpu()))


CASES = [   # N, W, H, deg, posed, seed, ambiguity bound (as tests/test_gpu_parity.py)
    (10000, 256, 256, 1, True, 1, None),
    (20000, 330, 250, 2, False, 2, None),
    (20000, 320, 240, 3, True, 3, None),
    (300000, 980, 545, 3, True, 4, 0.0280),
    (1000000, 980, 545, 3, True, 5, 0.0283),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-d{c[3]}-{'posed' if c[4] else 'plain'}")
def test_forward_and_raw_gradients_against_the_oracle(case):
    """Image within 1e-5 of the float64 oracle fed with the formulation's colours, every raw gradient and d_points_transform within
    1e-4 of the oracle's gradients chained through the formulation (tests/parity.py rules)."""
    N, W, H, deg, posed, seed, amb = case
    sc = parity.syn.make_scene(N, W, H, sh_degree=deg, seed=seed, posed=False)
    t = _raw_leaves(sc)
    xf, o = _transform(seed)
    if not posed:
        xf = None
    rs = _settings(sc, deg)
    o_ = binding.OracleRender(**_oracle_inputs(t, xf, o, deg, sc))
    up = parity.upstream_grads(H, W, seed=3)
    if N > 100000:
        up = (up[0], None, None)     # (the full-size cases: the loss on the image, as tests/test_gpu_parity.py's)
    what = f"sh_origin {N}/{W}x{H}/deg{deg}"
    rep, out, ref = parity.oracle_case(o_, lambda g: _run_raw(t, xf, o, rs, g), up, what, ambig_max_frac=amb)
    want = _oracle_chain(t, xf, o, deg, ref)
    grep = parity.check_grads(out["grads"], want, what)
    rep.pop("grad_mask")
    print(rep, {k: "%.1e" % v for k, v in grep.items()})
    o_.close()


def test_colour_sends_nothing_to_the_camera():
    """With camera gradients requested the colour contributes nothing to d_campos (exactly zero: the geometry does not read campos)
    and d_viewmatrix / d_projmatrix are those of rendering the same colours precomputed."""
    N, W, H, deg = 20000, 320, 240, 3
    sc = parity.syn.make_scene(N, W, H, sh_degree=deg, seed=8, posed=True)
    t = _raw_leaves(sc)
    xf, o = _transform(8)
    rs = _settings(sc, deg, cam_grad=True)
    gc = torch.from_numpy(parity.upstream_grads(H, W, seed=4)[0]).to(DEV)
    m2d = torch.zeros(N, 3, device=DEV, requires_grad=True)
    color = R.rasterize_gaussians_raw(t["_xyz"], m2d, t["_features_dc"], t["_features_rest"], t["_opacity"], t["_scaling"],
                                      t["_rotation"], rs, points_transform=xf.to(DEV), sh_origin=o.to(DEV))[0]
    (color * gc).sum().backward()
    assert float(rs.campos.grad.abs().max()) == 0.0
    a = (rs.viewmatrix.grad.clone(), rs.projmatrix.grad.clone())
    rs2 = _settings(sc, deg, cam_grad=True)
    with torch.no_grad():
        col = python_sh_colour(t["_xyz"], torch.cat((t["_features_dc"], t["_features_rest"]), 1), o.to(DEV), deg)
    c2 = R.rasterize_gaussians(t["_xyz"].detach(), torch.zeros(N, 3, device=DEV, requires_grad=True), None, col,
                               torch.sigmoid(t["_opacity"]).detach(), torch.exp(t["_scaling"]).detach(),
                               torch.nn.functional.normalize(t["_rotation"]).detach(), None, rs2, points_transform=xf.to(DEV))[0]
    (c2 * gc).sum().backward()
    for g, g2 in zip(a, (rs2.viewmatrix.grad, rs2.projmatrix.grad)):
        assert float((g - g2).abs().max()) <= 1e-4 * float(g2.abs().max()), (g, g2)


def test_degree_zero_is_bit_identical_to_no_origin():
    N, W, H = 20000, 320, 240
    sc = parity.syn.make_scene(N, W, H, sh_degree=0, seed=9, posed=True)
    t = _raw_leaves(sc)
    xf, o = _transform(9)
    rs = _settings(sc, 0)
    up = parity.upstream_grads(H, W, seed=5)
    a = _run_raw(t, xf, o, rs, up)
    b = _run_raw(t, xf, None, rs, up)
    for x, y in zip(a["fwd"], b["fwd"]):
        assert np.array_equal(x, y)
    parity.same_accumulation(a["grads"], b["grads"], "degree 0: sh_origin vs none")


def test_deferred_fused_adam_equals_backward_then_step(monkeypatch):
    """The patched render with convert_SHs_python on the deferred route (Adam update into shadow buffers by the backward kernel,
    adopted by optimizer.step()) ends in the same model as gradients to .grad + FusedAdam.step()."""
    import gsr_autopatch
    W, H, N = 256, 192, 6000
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=12)
    gt = parity.syn.target_image(W, H, seed=3).to(DEV)
    cam = refstub.StubCamera.from_scene(sc, DEV, original_image=gt, uid=1)
    monkeypatch.setenv("GSR_AUTOPATCH_DEFERRED_MIN_N", "0")
    res = []
    for deferred in (True, False):
        monkeypatch.setenv("GSR_AUTOPATCH_DEFERRED", "1" if deferred else "0")
        gsr_autopatch.apply()
        try:
            p = ts.GaussianParams(sc, DEV, optimizer="hip")
            r = PythonShRender(p)
            r.gaussians.P = [_lie([0.05, -0.03, 0.1, 0.02, -0.03, 0.01, 1.0]), _lie([-0.1, 0.04, 0.2, -0.04, 0.02, 0.05, 1.0])]
            for _ in range(3):
                pkg = gsr_autopatch.render_fused(r, cam, convert_SHs_python=True)
                gsr_autopatch.loss_forward(_LossCfg(), pkg["image"], gt)["loss"].backward()
                p.optimizer.step()
                p.optimizer.zero_grad(set_to_none=True)
            assert r.calls == 0 and bool(p.optimizer._shadow) == deferred
            res.append({k: getattr(p, k).detach().clone() for k in RAW})
        finally:
            gsr_autopatch.remove()
    parity.same_accumulation(res[0], res[1], "sh_origin: deferred vs separate step")


def _lie(pose7, delta=None):
    p = refstub.LieGroupParameter(refstub.SE3(torch.tensor([pose7], device=DEV)))
    if delta is not None:
        with torch.no_grad():
            p.copy_(torch.tensor([delta], device=DEV))
    return p


def test_fixture_through_the_kernels_matches_its_captured_colours():
    """python_sh.npz (the reference's real render): its raw tensors and poses through the kernels (sh_origin from P[uid],
    points_transform from P[seq_idx]) give the image of its captured colors_precomp and means3D through the existing path."""
    d = np.load(f"{GOLD}/python_sh.npz")
    W, H = int(d["image_width"]), int(d["image_height"])
    sc = dict(image_width=W, image_height=H, tanfovx=float(d["tanfovx"]), tanfovy=float(d["tanfovy"]),
              viewmatrix=torch.from_numpy(d["viewmatrix"].copy()), projmatrix=torch.from_numpy(d["projmatrix"].copy()),
              campos=torch.from_numpy(d["campos"].copy()))
    rs = _settings(sc, 3, bg=(0.1, 0.2, 0.3))
    for name in [str(c) for c in d["cases"]]:
        p, P = fixture_case(d, name, DEV)
        t = {k: getattr(p, k) for k in RAW}
        uid, seq_idx, seq = int(d[name + "_uid"]), int(d[name + "_seq_idx"]), bool(d[name + "_rotate_seq"])
        M = P[uid].retr().matrix().reshape(4, 4).detach().double()
        o = (-(M[:3, :3].t() @ M[:3, 3])).float()
        xf = P[seq_idx].retr().matrix().reshape(4, 4)[:3].detach().float() if seq else None
        a = _run_raw(t, xf, o, rs)["fwd"][0]
        n = t["_xyz"].shape[0]
        b = R.GaussianRasterizer(rs)(means3D=torch.from_numpy(d[name + "_means3D"]).to(DEV), means2D=torch.zeros(n, 3, device=DEV),
                                     colors_precomp=torch.from_numpy(d[name + "_colors_precomp"]).to(DEV),
                                     opacities=torch.sigmoid(t["_opacity"]).detach(), scales=torch.exp(t["_scaling"]).detach(),
                                     rotations=torch.nn.functional.normalize(t["_rotation"]).detach())[0].detach().cpu().numpy()
        diff = np.abs(a - b)
        assert float(b.std()) > 0.01
        assert float(diff.mean()) <= 1e-6 and float((diff > 1e-5).mean()) <= 2e-4, (name, float(diff.max()))


def test_abi_refuses_what_it_does_not_serve():
    """sh_origin without shs, with a batch of B > 1, with a prepared buffer (forward) or a next_view (backward): GSR_ERR_ARG."""
    lib = L.load()
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    ptr = buf.data_ptr()
    fb = (C.c_int32 * 3)(0, 1, 2)

    class GsrBatch(C.Structure):
        _fields_ = [("B", C.c_int32), ("first_block", C.c_void_p)]
    bt = GsrBatch(2, C.cast(fb, C.c_void_p))
    alloc = L.ALLOC_FN(lambda n, tag, user: None)

    def fwd(**kw):
        a = L.GsrForwardArgs()
        a.N, a.M, a.D, a.W, a.H = 256, 16, 3, 64, 48
        a.tanfovx = a.tanfovy = 0.5
        a.scale_modifier = 1.0
        for f in ("means3D", "scales", "rotations", "opacities", "shs", "viewmatrix", "projmatrix", "campos", "bg", "out_color",
                  "out_depth", "out_alpha", "radii", "geom", "image", "sh_origin"):
            setattr(a, f, ptr)
        a.alloc = alloc
        for k, v in kw.items():
            setattr(a, k, v)
        out = L.GsrForwardOut()
        return lib.gsr_forward(C.byref(a), C.byref(out), None)

    def bwd(**kw):
        a = L.GsrBackwardArgs()
        a.N, a.M, a.D, a.W, a.H = 256, 16, 3, 64, 48
        for f in ("means3D", "scales", "rotations", "opacities", "shs", "viewmatrix", "projmatrix", "campos", "bg", "geom", "image",
                  "binning", "d_means3D", "d_means2D", "d_opacities", "scratch", "sh_origin"):
            setattr(a, f, ptr)
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.gsr_backward(C.byref(a), None)
    for rc in (fwd(shs=None, colors_precomp=ptr), fwd(batch=C.cast(C.byref(bt), C.c_void_p)), fwd(prepared=ptr),
               bwd(shs=None, colors_precomp=ptr), bwd(batch=C.cast(C.byref(bt), C.c_void_p)), bwd(next_view=ptr)):
        assert rc == -1 and b"sh_origin" in lib.gsr_last_error()
    torch.cuda.synchronize()
    assert lib.gsr_version() >= 111


class _LossCfg:
    class cfg:
        lambda_dssim, lambda_depth = 0.2, 0.0


def register_original(gsr_autopatch):
    """Patch PythonShRender as gsr_autopatch patches scene.gaussian_model_ht.CF3DGS_Render (its render() becomes the original the
    patched method falls back to); gsr_autopatch.remove() restores it."""
    mod = types.ModuleType("python_sh_stub_scene")
    mod.CF3DGS_Render = PythonShRender
    gsr_autopatch._patch_render_module(mod)


@pytest.mark.parametrize("shape", ["init_leaf", "eval_nvs"])
def test_fifty_iterations_track_the_original_route(shape, monkeypatch):
    """The patched render trained for 50 iterations with convert_SHs_python=True -- an init_leaf-shaped run (degree 0, one camera,
    the model's own Adam) and an eval_nvs-shaped one (degree 3, rotate_seq, only the frame's pose stepped: update_gaussians=False) --
    tracks the original route (GSR_AUTOPATCH_PYTHON_SH=0: torch eval_sh + colors_precomp) loss for loss; the fused run never calls
    the original method."""
    import gsr_autopatch
    W, H = 256, 192
    N, deg = (20000, 0) if shape == "init_leaf" else (30000, 3)
    sc = parity.syn.make_scene(N, W, H, sh_degree=deg, seed=14)
    gt = parity.syn.target_image(W, H, seed=3).to(DEV)
    losses = {}
    for fused in (True, False):
        monkeypatch.setenv("GSR_AUTOPATCH_PYTHON_SH", "1" if fused else "0")
        gsr_autopatch.apply()
        register_original(gsr_autopatch)
        try:
            p = ts.GaussianParams(sc, DEV, optimizer="torch")
            r = PythonShRender(p)
            g = r.gaussians
            cam = refstub.StubCamera.from_scene(sc, DEV, original_image=gt, uid=1)
            if shape == "init_leaf":
                g.P = [_lie([0.0, 0, 0, 0, 0, 0, 1]), _lie([0.05, -0.03, 0.1, 0.02, -0.03, 0.01, 1.0])]
                popt = None
            else:
                g.P = [_lie([0.0, 0, 0, 0, 0, 0, 1]), _lie([0.02, -0.01, 0.03, 0.01, -0.02, 0.01, 1.0], [0.01, 0.0, -0.01, 0.0, 0.01, 0.0])]
                g.rotate_seq, g.seq_idx = True, 1
                popt = torch.optim.Adam([{"params": [g.P[1]], "lr": 1e-3, "name": "R"}], lr=0.0, eps=1e-15)
            ls = []
            for _ in range(50):
                pkg = r.render(cam, convert_SHs_python=True)
                loss = gsr_autopatch.loss_forward(_LossCfg(), pkg["image"], gt)["loss"]
                loss.backward()
                ls.append(float(loss.detach()))
                if popt is None:
                    p.optimizer.step()
                else:
                    popt.step()
                    popt.zero_grad(set_to_none=True)
                p.optimizer.zero_grad(set_to_none=True)
            assert (r.calls == 0) == fused, r.calls
            losses[fused] = np.array(ls)
        finally:
            gsr_autopatch.remove()
    a, b = losses[True], losses[False]
    assert b[-1] < b[0]
    rel = np.abs(a - b) / np.abs(b)
    print(shape, "max rel loss diff", rel.max(), "first / last", a[0], a[-1])
    assert rel.max() <= 1e-4, rel
