"""Merge-time importance without a backward (include/gsr.h gsr_importance_accumulate): the identity behind it against the float64
oracle, the route keyword of hierarchy.calc_importance and the patch of `HTGaussianTrainer.calc_importance`, on CPU.
(The kernels' numbers are checked on the GPU: tests/test_gpu_importance.py.)"""
import importlib
import sys
import types

import numpy as np
import pytest
import torch

import importance_common as ic
import parity
from oracle import binding

hier = ic.hier
refstub = importlib.import_module("3dgs_hierarchical_training_amd.refstub")


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_importance_from_sums_reproduces_the_oracle_gradient(deg):
    """With L = sum clamp(image, 0, 1):  |dL/dSH[n,k,c]| = |basis_k(dir_n)| [colour_{n,c} > 0] S[n,c],  S = the gradient of the SAME
    image w.r.t. a precomputed colour (sum over pixels of alpha T under the gate).  S is taken from the oracle rendering the scene with
    its SH colours as colors_precomp and the gate as upstream gradient; importance_from_sums in float64 must then reproduce the
    oracle's |d shs| of the SH render to 1e-10 of its maximum, on scene B at every degree, both views."""
    N, W, H = ic.SCENE_B
    _, views = ic.scene(N, W, H, deg)
    for sc, v in zip(views, ic.oracle_views(N, W, H, deg)):
        kw = parity.scene_kwargs(sc, "sh", bg=ic.BG)
        kw.pop("shs")
        o = binding.OracleRender(**kw, colors_precomp=torch.from_numpy(v["rgb"]))
        o.forward()
        S = torch.from_numpy(o.backward(v["gate"], None, None)["colors_precomp"])          # float64 [N,3]
        o.close()
        d = sc["means3D"].double() - sc["campos"].double().reshape(1, 3)
        dirs = d / d.norm(dim=1, keepdim=True)
        got = hier.importance_from_sums(S, dirs, torch.from_numpy(v["rgb"]), deg, 16)
        assert got.dtype == torch.float64 and tuple(got.shape) == (N, 16, 3)
        ref = v["ref"]
        assert ref.max() > 0 and (S >= 0).all()
        err = np.abs(got.numpy() - ref).max()
        print(f"[importance] identity deg {deg}: err {err:.3e}, max {ref.max():.3e}")
        assert err <= 1e-10 * ref.max()
        assert float(got[:, (deg + 1) ** 2:].abs().max() if deg < 3 else 0.0) == 0.0


def test_importance_without_the_pixel_gate_is_far_off():
    """What the pixel gate is worth on these scenes: sums taken with every gate open miss the oracle by a large share of the maximum
    entry (so a kernel that ignored the gate could not pass the 1e-3 bar)."""
    N, W, H = ic.SCENE_B
    deg = 2
    _, views = ic.scene(N, W, H, deg)
    sc, v = views[0], ic.oracle_views(N, W, H, deg)[0]
    ic.assert_meaningful(ic.conditions(v["color"], v["rgb"], v["radii"]), "scene B deg 2 view 0")
    kw = parity.scene_kwargs(sc, "sh", bg=ic.BG)
    kw.pop("shs")
    o = binding.OracleRender(**kw, colors_precomp=torch.from_numpy(v["rgb"]))
    o.forward()
    S = torch.from_numpy(o.backward(np.ones_like(v["gate"]), None, None)["colors_precomp"])
    o.close()
    d = sc["means3D"].double() - sc["campos"].double().reshape(1, 3)
    got = hier.importance_from_sums(S, d / d.norm(dim=1, keepdim=True), torch.from_numpy(v["rgb"]), deg, 16).numpy()
    assert np.abs(got - v["ref"]).max() >= 0.3 * v["ref"].max()


def test_route_keyword(monkeypatch):
    calls = []
    monkeypatch.setattr(hier, "_calc_importance_kernel", lambda seg, views: calls.append("kernel") or "K")
    monkeypatch.setattr(hier, "_calc_importance_autograd", lambda seg, views: calls.append("autograd") or "A")
    assert hier.calc_importance({}, [], route="kernel") == "K" and hier.calc_importance({}, [], route="autograd") == "A"
    assert hier.DEFAULT_IMPORTANCE_ROUTE in hier.IMPORTANCE_ROUTES
    monkeypatch.setattr(hier, "DEFAULT_IMPORTANCE_ROUTE", "kernel")
    assert hier.calc_importance({}, []) == "K" and hier.calc_importance({}, [], None) == "K"
    monkeypatch.setattr(hier, "DEFAULT_IMPORTANCE_ROUTE", "autograd")
    assert hier.calc_importance({}, []) == "A"
    assert calls == ["kernel", "autograd", "kernel", "kernel", "autograd"]
    with pytest.raises(ValueError, match="unknown route"):
        hier.calc_importance({}, [], route="backward")


def test_exports_and_version():
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    assert "gsr_importance_accumulate" in L.EXPORTS and "gsr_importance_scratch_bytes" in L.EXPORTS
    lib = L.load()
    assert lib.gsr_version() >= 113
    assert lib.gsr_importance_scratch_bytes(1000) >= 1000 * 12 and lib.gsr_importance_scratch_bytes(0) > 0


class _Params:
    def __init__(self, n=12):
        g = torch.Generator().manual_seed(1)
        r = lambda *s: torch.randn(*s, generator=g).requires_grad_(True)
        self._xyz, self._features_dc, self._features_rest = r(n, 3), r(n, 1, 3), r(n, 15, 3)
        self._opacity, self._scaling, self._rotation = r(n, 1), r(n, 3), r(n, 4)
        self.active_sh_degree, self.max_sh_degree, self.optimizer = 3, 3, None


def test_autopatch_replaces_calc_importance_and_falls_back(tmp_path, monkeypatch):
    """`trainer.ht3dgs_trainer` imported under gsr_autopatch gets `HTGaussianTrainer.calc_importance` (a staticmethod) replaced
    through the post-import hook; the patched form accumulates every camera through rasterizer.importance_accumulate on the model's
    raw tensors, divides once, leaves `.grad` None; `compute_cov3D_python` and an override colour run the original; remove() restores
    it.  The module is a stand-in with the reference's module path, class and method name (all the hook keys on), written here so
    that the test needs nothing outside the repository."""
    import gsr_autopatch
    gsr_autopatch.remove()
    pkg = tmp_path / "trainer"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    (pkg / "ht3dgs_trainer.py").write_text(
        "class HTGaussianTrainer:\n    @staticmethod\n    def calc_importance(gs_render, cameras, pipe, *extra):\n"
        "        return ('original', len(cameras)) + tuple(extra)\n")
    sys.path.insert(0, str(tmp_path))
    R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    try:
        for m in ("trainer.ht3dgs_trainer", "trainer"):
            sys.modules.pop(m, None)
        gsr_autopatch.apply()
        monkeypatch.setenv("GSR_AUTOPATCH_IMPORTANCE", "0")                    # the switch leaves the method alone
        T = importlib.import_module("trainer.ht3dgs_trainer")
        assert T.HTGaussianTrainer.calc_importance(None, [1, 2], None) == ("original", 2) and not gsr_autopatch._patched_trainer_classes
        gsr_autopatch.remove()
        sys.modules.pop("trainer.ht3dgs_trainer", None)
        monkeypatch.delenv("GSR_AUTOPATCH_IMPORTANCE")
        gsr_autopatch.apply()
        T = importlib.import_module("trainer.ht3dgs_trainer")
        cls = T.HTGaussianTrainer
        assert isinstance(vars(cls)["calc_importance"], staticmethod) and cls.calc_importance is gsr_autopatch.calc_importance_fused
        p = _Params()
        r = refstub.StubRender(p, bg=(0.2, 0.5, 0.9))
        cams = [refstub.StubCamera(64, 48, 0.5, 0.4, torch.eye(4), torch.eye(4), torch.zeros(3), uid=u) for u in (0, 1, 2)]
        rec = []

        def fake(acc, xyz, dc, op, sc, rot, settings, **kw):
            rec.append((xyz, dc, op, sc, rot, settings, kw))
            acc += 1.0
        monkeypatch.setattr(R, "importance_accumulate", fake)
        monkeypatch.setattr(gsr_autopatch, "_REQUIRE_CUDA", False)
        pipe = types.SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False)
        p._features_dc.grad = torch.ones_like(p._features_dc)
        imp = cls.calc_importance(r, cams, pipe)
        assert tuple(imp.shape) == (12, 48) and not imp.requires_grad
        assert torch.allclose(imp, torch.full((12, 48), 3.0 / (3 * 64 * 48)))               # three views, ONE division
        assert p._features_dc.grad is None and p._features_rest.grad is None
        assert len(rec) == 3 and rec[0][0] is p._xyz and rec[0][1] is p._features_dc and rec[0][6]["sh_rest"] is p._features_rest
        assert rec[0][6]["raw_params"] is True and rec[0][6]["points_transform"] is None and rec[0][6]["sh_origin"] is None
        assert rec[1][5].image_width == 64 and rec[1][5].sh_degree == 3 and torch.equal(rec[1][5].bg, r.bg_color)
        assert [x[6]["view_id"] for x in rec] == [1, 3, 5]
        # what render_fused would not serve goes to the original method
        n = len(rec)
        assert cls.calc_importance(r, cams, types.SimpleNamespace(compute_cov3D_python=True, convert_SHs_python=False)) == ("original", 3)
        assert gsr_autopatch.calc_importance_fused(r, cams, pipe, override_color=torch.zeros(12, 3))[:2] == ("original", 3)
        assert cls.calc_importance(r, cams, types.SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=True)) == ("original", 3)
        r.gaussians.rotate_seq, r.gaussians.P = True, [object()]                            # an unknown pose object
        assert cls.calc_importance(r, cams, pipe) == ("original", 3)
        assert len(rec) == n
        gsr_autopatch.remove()
        assert cls.calc_importance(r, cams, pipe) == ("original", 3) and isinstance(vars(cls)["calc_importance"], staticmethod)
        gsr_autopatch.apply()
        assert cls.calc_importance is gsr_autopatch.calc_importance_fused                   # already imported: patched in place
    finally:
        gsr_autopatch.remove()
        sys.path.remove(str(tmp_path))
        for m in ("trainer.ht3dgs_trainer", "trainer"):
            sys.modules.pop(m, None)
        gsr_autopatch.apply()
