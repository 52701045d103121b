"""CPU: the host side of V views of one model (include/gsr.h version 123: gsr_forward_views, gsr_geom_bytes_views,
gsr_importance_accumulate_views, gsr_importance_scratch_bytes_views) -- exports and signatures, the refusals that come before a device
is touched with their rule in gsr_last_error(), the op schemas, the wrappers refusing CPU tensors, hierarchy.group_views on hand-worked
lists, the views_per_call keyword, run_segments' option, the autopatch's switch, and calc_importance's call plan with the device calls
replaced by stand-ins.  (The kernels' numbers are checked on the GPU: tests/test_gpu_views.py.)"""
import ctypes as C
import importlib
import sys
import types

import numpy as np
import pytest
import torch

hier = importlib.import_module("3dgs_hierarchical_training_amd.hierarchy")
L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
E = importlib.import_module("3dgs_hierarchical_training_amd._ext")
R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
rs_mod = importlib.import_module("3dgs_hierarchical_training_amd.run_segments")
refstub = importlib.import_module("3dgs_hierarchical_training_amd.refstub")
FAKE = 0x1000          # a non-NULL "device pointer" for calls that must be refused before anything reads it


def test_version_exports_and_signatures():
    lib = L.load()
    assert lib.gsr_version() >= 123
    for name in ("gsr_forward_views", "gsr_geom_bytes_views", "gsr_importance_accumulate_views", "gsr_importance_scratch_bytes_views"):
        assert name in L.EXPORTS and hasattr(lib, name)
    P, O = C.POINTER(L.GsrForwardArgs), C.POINTER(L.GsrForwardOut)
    assert lib.gsr_forward_views.argtypes == [P, C.c_int32, O, C.c_void_p] and lib.gsr_forward_views.restype == C.c_int
    assert lib.gsr_importance_accumulate_views.argtypes == [P, C.c_int32, O, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.gsr_importance_accumulate_views.restype == C.c_int
    for fn in (lib.gsr_geom_bytes_views, lib.gsr_importance_scratch_bytes_views):
        assert fn.argtypes == [C.c_int32, C.c_int32] and fn.restype == C.c_size_t
    assert (L.GSR_FWD_FLAG_VIEWS, L.GSR_MAX_VIEWS) == (1 << 15, 16) and hier.MAX_VIEWS_PER_CALL == L.GSR_MAX_VIEWS
    # V * Npad records, Npad = 128 ceil(N / 128): the sizes of the single-model calls at that many Gaussians
    for N, V in ((1, 1), (127, 3), (128, 16), (129, 2), (1000, 8)):
        npad = (N + 127) // 128 * 128
        assert lib.gsr_geom_bytes_views(N, V) == lib.gsr_geom_bytes(V * npad)
        assert lib.gsr_importance_scratch_bytes_views(N, V) == lib.gsr_importance_scratch_bytes(V * npad)
    # GsrForwardArgs is unchanged: render_only is still its last field
    assert L.GsrForwardArgs._fields_[-1][0] == "render_only" and lib.gsr_struct_bytes(0) == C.sizeof(L.GsrForwardArgs)


def _args(N=1000):
    a = L.GsrForwardArgs()
    a.N, a.M, a.D, a.W, a.H = N, 16, 3, 64, 48
    return a


def _refused(rc, text, code=-1):
    msg = L.load().gsr_last_error().decode()
    assert rc == code and text in msg, (rc, msg)


def test_forward_views_refusals_come_before_a_device_is_touched():
    """V outside [1, 16], a batch, a prepared buffer, render_only and V * Npad >= 2^31, each with its rule in gsr_last_error() -- on a
    machine without a GPU, so nothing of them can have reached a device.  colors_precomp passes these rules."""
    lib = L.load()
    out = L.GsrForwardOut()
    call = lambda a, V: lib.gsr_forward_views(C.byref(a), V, C.byref(out), None)
    for V in (0, -1, 17):
        _refused(call(_args(), V), "views: 1..16 views expected")

    class _Batch(C.Structure):
        _fields_ = [("B", C.c_int32), ("first_block", C.POINTER(C.c_int32))]
    a = _args()
    keep = _Batch(1, (C.c_int32 * 2)(0, 8))
    a.batch = C.cast(C.pointer(keep), C.c_void_p)          # set at all: views of a batch are out of scope, whatever its B
    _refused(call(a, 2), "views: not served with a batch")
    a = _args()
    a.prepared = FAKE
    _refused(call(a, 2), "views: not served with a prepared buffer")
    a = _args()
    a.render_only = 1
    _refused(call(a, 2), "views: not served with render_only")
    _refused(call(_args(0), 2), "views: at least one Gaussian expected")
    _refused(call(_args(2 ** 27), 16), "views: V * Npad must stay below 2^31 records", code=-4)          # exactly 2^31
    _refused(call(_args(2 ** 27 - 127), 16), "views: V * Npad must stay below 2^31 records", code=-4)    # Npad rounds up to 2^27
    # below the limit, and with colors_precomp: the V rules pass; the call ends at the ordinary pointer check (still no device)
    a = _args(2 ** 27 - 128)
    a.colors_precomp = FAKE
    _refused(call(a, 16), "missing output / workspace pointer")
    _refused(lib.gsr_forward_views(None, 2, C.byref(out), None), "null args")


def test_importance_views_refusals_come_before_a_device_is_touched():
    """The single-view entry's refusals (colors_precomp, render-only flags), flags without GSR_FWD_FLAG_VIEWS, and the V rules."""
    lib = L.load()
    flags = 1 | (7 << 1) | (2 << 4) | (1 << 6) | (1 << 13)          # what a forward writes (the one blend variant and tile map)

    def call(a, V, f):
        out = L.GsrForwardOut()
        out.forward_flags = f
        return lib.gsr_importance_accumulate_views(C.byref(a), V, C.byref(out), FAKE, FAKE, None)
    a = _args()
    a.shs, a.campos = FAKE, FAKE
    _refused(call(a, 2, flags), "forward_flags do not come from gsr_forward_views")
    _refused(call(a, 2, flags | L.GSR_FWD_FLAG_VIEWS | L.GSR_FWD_FLAG_RENDER_ONLY), "render-only forward")
    vf = flags | L.GSR_FWD_FLAG_VIEWS
    for V in (0, 17):
        _refused(call(a, V, vf), "views: 1..16 views expected")
    a.render_only = 1
    _refused(call(a, 2, vf), "views: not served with render_only")
    a.render_only, a.prepared = 0, FAKE
    _refused(call(a, 2, vf), "views: not served with a prepared buffer")
    a.prepared = None
    a.colors_precomp = FAKE
    _refused(call(a, 2, vf), "the model must carry SH coefficients")
    a.colors_precomp, a.shs = None, None
    _refused(call(a, 2, vf), "the model must carry SH coefficients")
    a.shs, a.D, a.M = FAKE, 3, 9
    _refused(call(a, 2, vf), "M >= (D+1)^2")
    a.M = 16
    _refused(call(a, 2, vf), "missing workspace / accumulator pointer")          # every rule passed: the pointer check, still no device
    # the single-view entry and the backward refuse the flags of a views forward
    out = L.GsrForwardOut()
    out.forward_flags = vf
    _refused(lib.gsr_importance_accumulate(C.byref(a), C.byref(out), FAKE, FAKE, None), "use gsr_importance_accumulate_views")
    b = L.GsrBackwardArgs()
    b.N, b.M, b.D, b.W, b.H, b.forward_flags = 1000, 16, 3, 64, 48, vf
    _refused(lib.gsr_backward(C.byref(b), None), "a backward over views is not served")


def test_op_schemas():
    ops = E.load()
    head = ("Tensor means3D, Tensor sh, Tensor colors_precomp, Tensor opacities, Tensor scales, Tensor rotations, Tensor cov3D_precomp, "
            "Tensor sh_rest, Tensor viewmatrix, Tensor projmatrix, Tensor campos, Tensor bg, Tensor points_transform, int image_height, "
            "int image_width, float tanfovx, float tanfovy, float scale_modifier, int sh_degree, bool raw_params, ")
    assert str(ops.rasterize_forward_views.default._schema) == \
        "gsr::rasterize_forward_views(" + head + "int extras=0, Tensor? sh_origin=None) -> " \
        "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)"
    assert str(ops.importance_accumulate_views.default._schema) == \
        "gsr::importance_accumulate_views(Tensor(a!) acc, " + head + "Tensor? sh_origin=None) -> Tensor[]"
    # neither op registers autograd: there is no backward over a views forward
    for name in ("gsr::rasterize_forward_views", "gsr::importance_accumulate_views"):
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(name, "Autograd")
        assert torch._C._dispatch_has_kernel_for_dispatch_key(name, "CUDA")


def test_fake_kernels_describe_the_outputs():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.symbolic_shapes import ShapeEnv
    E.load()
    with FakeTensorMode(allow_non_fake_inputs=True, shape_env=ShapeEnv()):
        f = lambda *s: torch.empty(s, device="cuda")
        N, V, H, W = 129, 3, 40, 72
        args = (f(N, 3), f(N, 1, 3), f(0), f(N, 1), f(N, 3), f(N, 4), f(0), f(N, 15, 3), f(V, 4, 4), f(V, 4, 4), f(V, 3), f(3), f(0), H, W,
                1.0, 1.0, 1.0, 3, True)
        out = torch.ops.gsr.rasterize_forward_views(*args, 3, None)
        assert tuple(out[0].shape) == (V, 3, H, W) and tuple(out[1].shape) == (V * 256,) and out[1].dtype == torch.int32
        assert tuple(out[2].shape) == (V, 1, H, W) and tuple(out[8].shape) == (V, 3, H, W) and tuple(out[9].shape) == (V * 256,)
        assert out[4].shape[0] == L.load().gsr_geom_bytes_views(N, V)
        res = torch.ops.gsr.importance_accumulate_views(f(N, 16, 3), *args, None)
        assert len(res) == 8 and tuple(res[0].shape) == (V, 3, H, W)


def _settings(H=48, W=64, V=None, bg=None, **kw):
    bg = torch.zeros(3) if bg is None else bg
    lead = () if V is None else (V,)
    base = dict(image_height=H, image_width=W, tanfovx=0.8, tanfovy=0.6, bg=bg, scale_modifier=1.0, viewmatrix=torch.eye(4).expand(*lead, 4, 4),
                projmatrix=torch.eye(4).expand(*lead, 4, 4), sh_degree=3, campos=torch.zeros(*lead, 3), prefiltered=False, debug=False)
    base.update(kw)
    return R.GaussianRasterizationSettings(**base)


def test_wrappers_refuse_cpu_tensors():
    t = lambda *s: torch.zeros(*s)
    model = (t(10, 3), t(10, 1, 3), t(10, 1), t(10, 3), t(10, 4))
    with pytest.raises(RuntimeError, match="forward_views: tensors must be on a ROCm/HIP device"):
        R.forward_views(*model, _settings(V=2), sh_rest=t(10, 15, 3), raw_params=True)
    with pytest.raises(RuntimeError, match="importance_accumulate_views: tensors must be on a ROCm/HIP device"):
        R.importance_accumulate_views(t(10, 16, 3), *model, _settings(V=2), sh_rest=t(10, 15, 3), raw_params=True)


def test_group_views_on_hand_worked_lists():
    bg = torch.tensor([0.2, 0.5, 0.9])
    a = lambda **kw: _settings(**{"bg": bg, **kw})
    seven = [a() for _ in range(7)]
    assert hier.group_views(seven, 1, 1000) == [[i] for i in range(7)]
    assert hier.group_views(seven, 3, 1000) == [[0, 1, 2], [3, 4, 5], [6]]
    assert hier.group_views(seven, 16, 1000) == [list(range(7))]
    assert hier.group_views([a() for _ in range(20)], 17, 1000) == [list(range(16)), [16, 17, 18, 19]]          # never more than 16
    assert hier.group_views([], 8, 1000) == []
    # mixed sizes: only CONSECUTIVE views that agree share a call
    mixed = [a(), a(), a(H=32), a(H=32), a(H=32), a(), a(W=80), a(W=80)]
    assert hier.group_views(mixed, 8, 1000) == [[0, 1], [2, 3, 4], [5], [6, 7]]
    assert hier.group_views(mixed, 2, 1000) == [[0, 1], [2, 3], [4], [5], [6, 7]]
    # every shared field cuts a run: field of view, degree, scale modifier
    cut = [a(), a(tanfovx=0.81), a(tanfovx=0.81, tanfovy=0.61), a(tanfovx=0.81, tanfovy=0.61, sh_degree=2),
           a(tanfovx=0.81, tanfovy=0.61, sh_degree=2, scale_modifier=0.5)]
    assert hier.group_views(cut, 8, 1000) == [[0], [1], [2], [3], [4]]
    # a background that differs cuts; an equal one in another tensor does not
    other, same = torch.tensor([0.2, 0.5, 0.8]), bg.clone()
    assert hier.group_views([a(), a(bg=same), a(bg=other), a(bg=other), a()], 8, 1000) == [[0, 1], [2, 3], [4]]
    # the record guard: at most VIEWS_MAX_RECORDS // Npad views share a call
    assert hier.VIEWS_MAX_RECORDS == 8 * 2 ** 20
    ten = [a() for _ in range(10)]
    assert hier.group_views(ten, 16, 2 ** 20) == [list(range(8)), [8, 9]]                       # 1 M Gaussians: eight views
    assert hier.group_views(ten, 16, 2 ** 20 + 1) == [[0, 1, 2, 3, 4, 5, 6], [7, 8, 9]]         # Npad = 2^20 + 128: seven
    assert hier.group_views(ten, 16, 3 * 2 ** 20) == [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9]]
    assert hier.group_views(ten[:3], 16, 9 * 2 ** 20) == [[0], [1], [2]]                        # the guard never goes below one view
    with pytest.raises(ValueError, match="per_call"):
        hier.group_views(ten, 0, 1000)


def test_views_per_call_keyword(monkeypatch):
    calls = []
    monkeypatch.setattr(hier, "_calc_importance_kernel", lambda seg, views: calls.append("per-view") or "K")
    monkeypatch.setattr(hier, "_calc_importance_views", lambda seg, views, n: calls.append(("views", n)) or "V")
    monkeypatch.setattr(hier, "_calc_importance_autograd", lambda seg, views: calls.append("autograd") or "A")
    assert hier.DEFAULT_IMPORTANCE_VIEWS == 1          # the default stays 1 (profiles/importance_views.txt)
    assert hier.calc_importance({}, [], route="kernel") == "K" and hier.calc_importance({}, [], route="kernel", views_per_call=1) == "K"
    assert hier.calc_importance({}, [], route="kernel", views_per_call=2) == "V" and hier.calc_importance({}, [], route="kernel", views_per_call=16) == "V"
    monkeypatch.setattr(hier, "DEFAULT_IMPORTANCE_VIEWS", 8)          # what GSR_IMPORTANCE_VIEWS=8 sets at import
    assert hier.calc_importance({}, [], route="kernel") == "V" and hier.calc_importance({}, [], route="kernel", views_per_call=1) == "K"
    monkeypatch.setattr(hier, "DEFAULT_IMPORTANCE_VIEWS", 1)
    assert hier.calc_importance({}, [], route="autograd") == "A" and hier.calc_importance({}, [], route="autograd", views_per_call=1) == "A"
    assert calls == ["per-view", "per-view", ("views", 2), ("views", 16), ("views", 8), "per-view", "autograd", "autograd"]
    for bad in (2, 8, 16):
        with pytest.raises(ValueError, match="kernel route only"):
            hier.calc_importance({}, [], route="autograd", views_per_call=bad)
    for bad in (0, 17, -1):
        with pytest.raises(ValueError, match="views_per_call must be 1..16"):
            hier.calc_importance({}, [], route="kernel", views_per_call=bad)


def test_environment_variable_is_read_at_import():
    import subprocess
    code = ("import importlib; h = importlib.import_module('3dgs_hierarchical_training_amd.hierarchy'); print(h.DEFAULT_IMPORTANCE_VIEWS)")
    env = dict(__import__("os").environ, GSR_IMPORTANCE_VIEWS="4")
    root = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))
    assert subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, check=True).stdout.strip() == "4"
    bad = subprocess.run([sys.executable, "-c", code], env=dict(env, GSR_IMPORTANCE_VIEWS="17"), cwd=root, capture_output=True, text=True)
    assert bad.returncode != 0 and "GSR_IMPORTANCE_VIEWS=17" in bad.stderr


def test_run_segments_option(capsys):
    """`--importance-views-per-call` (the name `--importance-views` has long meant how MANY of a child's frames are scored, and keeps
    that meaning): parsed, refused outside 1 .. 16, carried by HTConfig, and handed to calc_importance by the merge."""
    a = rs_mod.parse_args([])
    assert a.importance_views_per_call == 1 and a.importance_views == 0
    assert rs_mod.parse_args(["--importance-views-per-call", "8", "--importance-views", "3"]).importance_views_per_call == 8
    assert rs_mod.parse_args(["--importance-views-per-call", "16"]).importance_views_per_call == 16
    for bad in ("0", "17", "-2"):
        with pytest.raises(SystemExit):
            rs_mod.parse_args(["--importance-views-per-call", bad])
        assert "--importance-views-per-call: 1..16 expected" in capsys.readouterr().err
    assert rs_mod.HTConfig().importance_views_per_call == 1
    for bad in (0, 17):
        with pytest.raises(ValueError, match="importance_views_per_call"):
            rs_mod.check_importance_views_per_call(rs_mod.HTConfig(importance_views_per_call=bad))
    seq = types.SimpleNamespace()
    tr = types.SimpleNamespace()
    dev = torch.device("cpu")
    plain = rs_mod.RankRunner(0, 2, tr, seq, rs_mod.HTConfig(frames=10), dev)
    assert plain.importance_fn is hier.calc_importance
    four = rs_mod.RankRunner(0, 2, tr, seq, rs_mod.HTConfig(frames=10, importance_views_per_call=4), dev)
    assert four.importance_fn.func is hier.calc_importance and four.importance_fn.keywords == {"views_per_call": 4}
    own = lambda seg, views: None
    assert rs_mod.RankRunner(0, 2, tr, seq, rs_mod.HTConfig(frames=10, importance_views_per_call=4), dev, importance_fn=own).importance_fn is own
    with pytest.raises(ValueError, match="importance_views_per_call"):
        rs_mod.RankRunner(0, 2, tr, seq, rs_mod.HTConfig(frames=10, importance_views_per_call=17), dev)


def _seg(n=12):
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"_xyz": r(n, 3), "_features_dc": r(n, 1, 3), "_features_rest": r(n, 15, 3), "_opacity": r(n, 1), "_scaling": r(n, 3), "_rotation": r(n, 4)}


def test_calc_importance_issues_the_planned_calls_and_divides_once(monkeypatch):
    """The device calls replaced by numpy stand-ins that add a known amount per view: calc_importance(views_per_call=k) issues exactly
    the calls group_views plans -- a group of one through the single-view call -- in view order, into ONE accumulator, and divides by
    the pixel count once."""
    bg = torch.tensor([0.2, 0.5, 0.9])
    views = [_settings(bg=bg, campos=torch.full((3,), float(i))) for i in range(5)] + [_settings(H=32, bg=bg, campos=torch.full((3,), 5.0))] + \
            [_settings(bg=bg, campos=torch.full((3,), 6.0))]
    seg = _seg()
    rec = []

    def single(acc, xyz, dc, op, sc, rot, rs, **kw):
        # (views_per_call=1 is the per-view route as it was: it also names points_transform, sh_origin and view_id, all unset)
        assert xyz is seg["_xyz"] and kw["sh_rest"].data_ptr() == seg["_features_rest"].data_ptr() and kw["raw_params"] is True and rs.viewmatrix.dim() == 2
        assert all(not kw.get(k) for k in ("points_transform", "sh_origin", "view_id"))
        rec.append(("single", [float(rs.campos[0])]))
        acc += torch.from_numpy(np.full(tuple(acc.shape), 1.0, np.float32))

    def many(acc, xyz, dc, op, sc, rot, st, **kw):
        V = st.viewmatrix.shape[0]
        assert xyz is seg["_xyz"] and sorted(kw) == ["raw_params", "sh_rest"] and kw["raw_params"] is True
        assert tuple(st.projmatrix.shape) == (V, 4, 4) and tuple(st.campos.shape) == (V, 3) and st.bg is bg
        rec.append(("views", [float(c) for c in st.campos[:, 0]]))
        acc += torch.from_numpy(np.full(tuple(acc.shape), float(V), np.float32))
    monkeypatch.setattr(hier, "importance_accumulate", single)
    monkeypatch.setattr(hier, "importance_accumulate_views", many)
    pixels = 6 * 48 * 64 + 32 * 64
    for k, plan in ((3, [("views", [0, 1, 2]), ("views", [3, 4]), ("single", [5]), ("single", [6])]),
                    (16, [("views", [0, 1, 2, 3, 4]), ("single", [5]), ("single", [6])]),
                    (2, [("views", [0, 1]), ("views", [2, 3]), ("single", [4]), ("single", [5]), ("single", [6])]),
                    (1, [("single", [i]) for i in range(7)])):
        rec.clear()
        imp = hier.calc_importance(seg, views, route="kernel", views_per_call=k)
        assert rec == plan, (k, rec)
        assert [len(g) for g in hier.group_views(views, k, 12)] == [len(p[1]) for p in plan]
        assert tuple(imp.shape) == (12, 48) and torch.equal(imp, torch.full((12, 48), np.float32(7.0)) / pixels)          # seven views, ONE division


class _Params:
    def __init__(self, n=12):
        g = torch.Generator().manual_seed(1)
        r = lambda *s: torch.randn(*s, generator=g).requires_grad_(True)
        self._xyz, self._features_dc, self._features_rest = r(n, 3), r(n, 1, 3), r(n, 15, 3)
        self._opacity, self._scaling, self._rotation = r(n, 1), r(n, 3), r(n, 4)
        self.active_sh_degree, self.max_sh_degree, self.optimizer = 3, 3, None


def test_autopatch_switch_is_read_through_the_import_hook(tmp_path, monkeypatch):
    """`trainer.ht3dgs_trainer` imported under gsr_autopatch (a stand-in with the reference's module path, class and method name) gets
    `calc_importance` replaced; with GSR_AUTOPATCH_IMPORTANCE_VIEWS=3 the patched method sends runs of cameras through
    rasterizer.importance_accumulate_views (a group of one through importance_accumulate), divides once and leaves .grad None; unset, it
    is the per-camera route; outside 1 .. 16 it is an error; every fall-back still reaches the original."""
    import gsr_autopatch
    gsr_autopatch.remove()
    pkg = tmp_path / "trainer"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    (pkg / "ht3dgs_trainer.py").write_text(
        "class HTGaussianTrainer:\n    @staticmethod\n    def calc_importance(gs_render, cameras, pipe, *extra):\n"
        "        return ('original', len(cameras)) + tuple(extra)\n")
    sys.path.insert(0, str(tmp_path))
    try:
        for m in ("trainer.ht3dgs_trainer", "trainer"):
            sys.modules.pop(m, None)
        gsr_autopatch.apply()
        cls = importlib.import_module("trainer.ht3dgs_trainer").HTGaussianTrainer
        assert cls.calc_importance is gsr_autopatch.calc_importance_fused
        p = _Params()
        r = refstub.StubRender(p, bg=(0.2, 0.5, 0.9))
        cams = [refstub.StubCamera(64, 48, 0.5, 0.4, torch.eye(4) * (u + 1), torch.eye(4), torch.full((3,), float(u)), uid=u) for u in range(4)]
        rec = []

        def single(acc, xyz, dc, op, sc, rot, settings, **kw):
            rec.append(("single", 1, kw))
            acc += 1.0

        def many(acc, xyz, dc, op, sc, rot, st, **kw):
            assert xyz is p._xyz and dc is p._features_dc and kw["sh_rest"] is p._features_rest and kw["raw_params"] is True
            assert kw["points_transform"] is None and kw["sh_origin"] is None and st.bg is r.bg_color and st.sh_degree == 3
            rec.append(("views", [float(c) for c in st.campos[:, 0]], [float(m[0, 0]) for m in st.viewmatrix]))
            acc += float(st.viewmatrix.shape[0])
        monkeypatch.setattr(R, "importance_accumulate", single)
        monkeypatch.setattr(R, "importance_accumulate_views", many)
        monkeypatch.setattr(gsr_autopatch, "_REQUIRE_CUDA", False)
        pipe = types.SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=False)
        monkeypatch.delenv("GSR_AUTOPATCH_IMPORTANCE_VIEWS", raising=False)
        cls.calc_importance(r, cams, pipe)
        assert [x[:2] for x in rec] == [("single", 1)] * 4                                   # the default: a call per camera
        rec.clear()
        monkeypatch.setenv("GSR_AUTOPATCH_IMPORTANCE_VIEWS", "3")
        p._features_dc.grad = torch.ones_like(p._features_dc)
        imp = cls.calc_importance(r, cams, pipe)
        assert rec[0] == ("views", [0.0, 1.0, 2.0], [1.0, 2.0, 3.0]) and rec[1][:2] == ("single", 1) and len(rec) == 2
        assert rec[1][2]["view_id"] == 7 and rec[1][2]["points_transform"] is None           # the group of one: the call as it was
        assert torch.allclose(imp, torch.full((12, 48), 4.0 / (4 * 64 * 48))) and not imp.requires_grad          # ONE division
        assert p._features_dc.grad is None and p._features_rest.grad is None
        # every fall-back still reaches the original
        n = len(rec)
        assert cls.calc_importance(r, cams, types.SimpleNamespace(compute_cov3D_python=True, convert_SHs_python=False)) == ("original", 4)
        assert gsr_autopatch.calc_importance_fused(r, cams, pipe, override_color=torch.zeros(12, 3))[:2] == ("original", 4)
        assert cls.calc_importance(r, cams, types.SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=True)) == ("original", 4)
        r.gaussians.rotate_seq, r.gaussians.P = True, [object()]                             # an unknown pose object
        assert cls.calc_importance(r, cams, pipe) == ("original", 4) and len(rec) == n
        r.gaussians.rotate_seq, r.gaussians.P = False, None
        monkeypatch.setenv("GSR_AUTOPATCH_IMPORTANCE_VIEWS", "17")
        with pytest.raises(ValueError, match="GSR_AUTOPATCH_IMPORTANCE_VIEWS=17"):
            cls.calc_importance(r, cams, pipe)
    finally:
        gsr_autopatch.remove()
        sys.path.remove(str(tmp_path))
        for m in ("trainer.ht3dgs_trainer", "trainer"):
            sys.modules.pop(m, None)
        gsr_autopatch.apply()
