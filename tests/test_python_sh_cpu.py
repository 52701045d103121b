"""The reference's `convert_SHs_python` render (/root/reference/scene/gaussian_model_ht.py:845-865) on the kernels -- its formulation
against the captured fixture, and the dispatch of the patched `CF3DGS_Render.render`, on CPU.

With `view_dependent` (the trainer's default) the colour is `clamp_min(eval_sh(D, features, normalize(_xyz - o)) + 0.5, 0)`, where
`o = get_RT(uid).inverse()[:3, 3].detach()` is the camera centre in the model's own frame and `_xyz` the UNposed means.  The kernels
take `o` as `sh_origin` (include/gsr.h GsrForwardArgs::sh_origin); their numbers are checked on the GPU (tests/test_gpu_python_sh.py).
The HIP ops cannot run here: `gsr_autopatch._ops` is a recorder whose `pose_matrix` is pose.py's torch statement."""
import importlib
import os
import types

import numpy as np
import pytest
import torch

from oracle import torch_oracle

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
refstub = importlib.import_module("3dgs_hierarchical_training_amd.refstub")
pose = importlib.import_module("3dgs_hierarchical_training_amd.pose")
RAW = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def python_sh_colour(xyz, features, origin, deg):
    """The formulation of gaussian_model_ht.py:849-862, in the dtype of its inputs: [N,3] colours."""
    d = xyz - origin.reshape(1, 3)
    d = d / d.norm(dim=1, keepdim=True)
    return torch.clamp_min(torch_oracle.sh_basis_eval(deg, features, d) + 0.5, 0.0)


class _Gaussians(refstub.StubGaussians):
    def get_RT(self, idx=None):                # gaussian_model_ht.py:150-165
        if getattr(self, "P", None) is None:
            return torch.eye(4, device=self._xyz.device)
        if self.rotate_xyz:
            Rt = self.P[0].retr().matrix()
        else:
            Rt = self.P[self.seq_idx if idx is None else idx].retr().matrix()
        return Rt.squeeze()


class PythonShRender(refstub.StubRender):
    """`CF3DGS_Render` with `view_dependent` whose `render` also restates the reference's `convert_SHs_python` branch (:845-865):
    the colour computed in torch from the UNposed means and the pose's camera centre, handed to the rasterizer as colors_precomp."""
    view_dependent = True

    def __init__(self, params, bg=(0.0, 0.0, 0.0)):
        super().__init__(params, bg)
        self.gaussians.__class__ = _Gaussians
        self.calls = 0

    def render(self, viewpoint_camera, scaling_modifier=1.0, invert_bg_color=False, override_color=None,
               compute_cov3D_python=False, convert_SHs_python=False):
        self.calls += 1
        if not convert_SHs_python or override_color is not None:
            return super().render(viewpoint_camera, scaling_modifier, invert_bg_color, override_color, compute_cov3D_python, False)
        g = self.gaussians
        o = g.get_RT(viewpoint_camera.uid).inverse()[:3, 3].detach()
        colour = python_sh_colour(g._xyz, g.get_features, o, g.active_sh_degree) if self.view_dependent else g.get_features[:, 0]
        return super().render(viewpoint_camera, scaling_modifier, invert_bg_color, colour, compute_cov3D_python, False)


def _lie(pose7, delta):
    p = refstub.LieGroupParameter(refstub.SE3(torch.tensor([pose7], dtype=torch.float32)))
    with torch.no_grad():
        p.copy_(torch.tensor([delta], dtype=torch.float32))
    return p


def fixture_case(d, name, dev="cpu"):
    """(params, poses) of one case of python_sh.npz: raw tensors as HTGaussianModel keeps them, P as refstub SE3 parameters."""
    p = types.SimpleNamespace(optimizer=None, max_sh_degree=3, active_sh_degree=int(d[name + "_active_sh_degree"]))
    for k in RAW:
        setattr(p, k, torch.from_numpy(d[name + "_" + k].copy()).to(dev).requires_grad_(True))
    P = [_lie(d["pose7"][q].tolist(), d["delta"][q].tolist()) for q in range(len(d["pose7"]))]
    return p, P


def test_formulation_reproduces_the_captured_colours():
    """The f64 statement above, fed with the fixture's raw tensors and the origin of the reference's get_RT(uid) (built from the pose
    tensors, not read from the fixture), gives the colors_precomp the real CF3DGS_Render.render handed to the rasterizer; means3D is
    get_xyz, posed by P[seq_idx] under rotate_seq -- not P[uid]."""
    d = np.load(os.path.join(GOLD, "python_sh.npz"))
    for name in [str(c) for c in d["cases"]]:
        p, P = fixture_case(d, name)
        uid, seq_idx, seq = int(d[name + "_uid"]), int(d[name + "_seq_idx"]), bool(d[name + "_rotate_seq"])
        M = P[uid].retr().matrix().reshape(4, 4).detach().double()
        o = -(M[:3, :3].t() @ M[:3, 3])
        assert torch.allclose(o.float(), torch.from_numpy(d[name + "_origin"]), atol=1e-6)
        feats = torch.cat((p._features_dc, p._features_rest), 1).detach().double()
        col = python_sh_colour(p._xyz.detach().double(), feats, o, p.active_sh_degree)
        np.testing.assert_allclose(col.numpy(), d[name + "_colors_precomp"], atol=1e-6, rtol=0)
        want = P[seq_idx].retr().act(p._xyz.detach()) if seq else p._xyz.detach()
        np.testing.assert_allclose(want.detach().numpy(), d[name + "_means3D"], atol=1e-6, rtol=0)
        # the direction is NOT the posed mean's: the same statement from get_xyz differs (non-identity poses)
        wrong = python_sh_colour(torch.from_numpy(d[name + "_means3D"]).double(), feats, o, p.active_sh_degree)
        assert float((wrong - col).abs().max()) > 1e-3 or not seq


class _RecordingOps:
    def __init__(self):
        self.calls = []

    def pose_matrix(self, delta, base):
        self.calls.append(("pose_matrix", delta, base))
        B = torch.cat((base, torch.tensor([[0.0, 0.0, 0.0, 1.0]])), 0)
        return (pose.se3_exp(delta.reshape(6)) @ B)[:3]


@pytest.fixture
def autopatch(monkeypatch):
    import gsr_autopatch
    gsr_autopatch.apply()
    gsr_autopatch._REQUIRE_CUDA = False
    ops = _RecordingOps()
    monkeypatch.setattr(gsr_autopatch, "_ops", lambda: ops)
    monkeypatch.setattr(gsr_autopatch, "_ext_binding", lambda: True)
    # the stub class stands for scene.gaussian_model_ht.CF3DGS_Render: its render() is the original the patch falls back to
    mod = types.ModuleType("python_sh_stub_scene")
    mod.CF3DGS_Render = PythonShRender
    gsr_autopatch._patch_render_module(mod)
    yield gsr_autopatch
    gsr_autopatch._REQUIRE_CUDA = True
    gsr_autopatch.remove()


def _recording_raster(rec, H, W):
    def fake(means3D, means2D, f_dc, f_rest, opacity, scaling, rotation, settings, **kw):
        rec.update(t=(means3D, f_dc, f_rest), kw=kw, st=settings)
        xf = kw.get("points_transform")
        z = means3D.sum() * 0 + (0 if xf is None else xf.sum() * 0)
        out = (torch.zeros(3, H, W) + z, torch.ones(means3D.shape[0], dtype=torch.int32), torch.zeros(1, H, W), torch.zeros(1, H, W))
        if kw.get("extras"):
            out = out + (out[0].clamp(0, 1), (out[1] > 0).to(torch.uint8))
        return out
    return fake


def _stub(d, name="seq"):
    p, P = fixture_case(d, name)
    r = PythonShRender(p)
    W, H = int(d["image_width"]), int(d["image_height"])
    cam = refstub.StubCamera(W, H, float(d["tanfovx"]), float(d["tanfovy"]), torch.from_numpy(d["viewmatrix"].copy()),
                             torch.from_numpy(d["projmatrix"].copy()), torch.from_numpy(d["campos"].copy()), uid=2)
    return p, P, r, cam, W, H


@pytest.mark.parametrize("mode", ["rotate_seq", "no_pose_flag", "rotate_xyz", "P_none"])
def test_dispatch_hands_the_kernels_the_references_origin(autopatch, mode):
    """convert_SHs_python=True with view_dependent reaches rasterize_gaussians_raw (not the original method) with the raw tensors,
    sh_origin = the reference's get_RT(uid).inverse()[:3, 3] (identity when P is None, P[0] under rotate_xyz, P[uid] otherwise) and
    points_transform = get_xyz's pose P[seq_idx] -- two different slots when uid != seq_idx."""
    d = np.load(os.path.join(GOLD, "python_sh.npz"))
    p, P, r, cam, W, H = _stub(d)
    g = r.gaussians
    g.P = P
    if mode == "rotate_seq":
        g.rotate_seq, g.seq_idx = True, 1
    elif mode == "rotate_xyz":
        g.rotate_xyz = True
    elif mode == "P_none":
        g.P = None
    R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    rec = {}
    orig, R.rasterize_gaussians_raw = R.rasterize_gaussians_raw, _recording_raster(rec, H, W)
    try:
        pkg = r.render(cam, convert_SHs_python=True)
    finally:
        R.rasterize_gaussians_raw = orig
    assert r.calls == 0 and "kw" in rec, "the original method ran"
    assert rec["t"][0] is p._xyz and rec["t"][1] is p._features_dc and rec["t"][2] is p._features_rest
    o = rec["kw"]["sh_origin"]
    assert o is not None and tuple(o.shape) == (3,) and not o.requires_grad
    want = g.get_RT(cam.uid).inverse()[:3, 3]
    assert torch.allclose(o, want, atol=2e-6), (o, want)
    xf = rec["kw"].get("points_transform")
    if mode == "rotate_seq":
        assert torch.allclose(xf.reshape(-1, 4)[:3], P[1].retr().matrix().reshape(4, 4)[:3], atol=1e-6)      # seq_idx, not uid
        assert not torch.allclose(o, -(P[1].retr().matrix().reshape(4, 4)[:3, :3].t() @ P[1].retr().matrix().reshape(4, 4)[:3, 3]), atol=1e-3)
    elif mode == "rotate_xyz":
        assert torch.allclose(xf.reshape(-1, 4)[:3], P[0].retr().matrix().reshape(4, 4)[:3], atol=1e-6)
    else:
        assert xf is None
    if mode == "P_none":
        assert float(o.abs().max()) == 0.0
    assert pkg["image"].shape == (3, H, W)
    # the same stub without convert_SHs_python: no origin (today's direction, posed mean - campos)
    rec.clear()
    orig, R.rasterize_gaussians_raw = R.rasterize_gaussians_raw, _recording_raster(rec, H, W)
    try:
        r.render(cam)
    finally:
        R.rasterize_gaussians_raw = orig
    assert rec["kw"].get("sh_origin") is None


def test_other_configurations_reach_the_original_method(autopatch, monkeypatch):
    """view_dependent=False (raw DC as colour), compute_cov3D_python, override_color and GSR_AUTOPATCH_PYTHON_SH=0 keep
    convert_SHs_python renders on the original method."""
    d = np.load(os.path.join(GOLD, "python_sh.npz"))
    p, P, r, cam, W, H = _stub(d)
    R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    rec = {}
    orig, R.rasterize_gaussians_raw = R.rasterize_gaussians_raw, _recording_raster(rec, H, W)
    calls = []
    orig_render = refstub.StubRender.render

    def counting(self, *a, **k):
        calls.append(1)
        return {"image": torch.zeros(3, H, W)}
    try:
        refstub.StubRender.render = counting
        for kw in ({"compute_cov3D_python": True}, {"override_color": torch.zeros(p._xyz.shape[0], 3)}):
            r.render(cam, convert_SHs_python=True, **kw)
        r.view_dependent = False
        r.render(cam, convert_SHs_python=True)
        r.view_dependent = True
        monkeypatch.setenv("GSR_AUTOPATCH_PYTHON_SH", "0")
        r.render(cam, convert_SHs_python=True)
    finally:
        refstub.StubRender.render = orig_render
        R.rasterize_gaussians_raw = orig
    assert r.calls == 4 and len(calls) == 4 and "kw" not in rec
