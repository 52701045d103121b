"""CPU: the host side of the frozen call over V views of one model (include/gsr.h version 124: gsr_backward_views,
gsr_backward_scratch_bytes_views, gsr_pose_step_many) -- exports and signatures, every refusal that comes before a device is touched
with its rule in gsr_last_error(), the op schemas and fake kernels, rasterize_views / fit_poses refusing what they do not serve, and
run_segments' two switches.  (The kernels' numbers are checked on the GPU: tests/test_gpu_backward_views.py.)"""
import ctypes as C
import importlib

import pytest
import torch

L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
E = importlib.import_module("3dgs_hierarchical_training_amd._ext")
R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
pose_fit = importlib.import_module("3dgs_hierarchical_training_amd.pose_fit")
rs_mod = importlib.import_module("3dgs_hierarchical_training_amd.run_segments")
FAKE = 0x1000          # a non-NULL "device pointer" for calls that must be refused before anything reads it
FLAGS = 1 | (7 << 1) | (2 << 4) | (1 << 6) | (1 << 13)          # what a forward writes (tests/test_views_cpu.py)
VIEWS_FLAGS = FLAGS | L.GSR_FWD_FLAG_VIEWS
PER_GAUSSIAN = ("d_means3D", "d_opacities", "d_colors_precomp", "d_shs", "d_shs_rest", "d_scales", "d_rotations", "d_cov3D_precomp")


def test_version_exports_and_signatures():
    lib = L.load()
    assert lib.gsr_version() >= 124
    for name in ("gsr_backward_views", "gsr_backward_scratch_bytes_views", "gsr_pose_step_many"):
        assert name in L.EXPORTS and hasattr(lib, name)
    assert lib.gsr_backward_views.argtypes == [C.POINTER(L.GsrBackwardArgs), C.c_int32, C.c_void_p] and lib.gsr_backward_views.restype == C.c_int
    assert lib.gsr_backward_scratch_bytes_views.argtypes == [C.c_int32, C.c_int32] and lib.gsr_backward_scratch_bytes_views.restype == C.c_size_t
    assert lib.gsr_pose_step_many.argtypes == [C.c_void_p] * 6 + [C.c_int32] + [C.c_float] * 4 + [C.c_int64, C.c_void_p]
    assert lib.gsr_pose_step_many.restype == C.c_int
    # V * Npad records: the single-model call's scratch at that many Gaussians
    for N, V in ((1, 1), (127, 3), (128, 16), (129, 2), (1000, 8)):
        assert lib.gsr_backward_scratch_bytes_views(N, V) == lib.gsr_backward_scratch_bytes(V * ((N + 127) // 128 * 128))
    # GsrBackwardArgs keeps its layout
    assert lib.gsr_struct_bytes(1) == C.sizeof(L.GsrBackwardArgs)


def _args(N=1000, flags=VIEWS_FLAGS, out="d_points_transform", workspace=True):
    a = L.GsrBackwardArgs()
    a.N, a.M, a.D, a.W, a.H, a.forward_flags = N, 16, 3, 72, 40, flags
    if out:
        setattr(a, out, FAKE)
    if workspace:
        a.geom = a.image = a.binning = a.scratch = FAKE
    return a


def _refused(rc, text, code=-1):
    msg = L.load().gsr_last_error().decode()
    assert rc == code and text in msg, (rc, msg)


def test_backward_views_refusals_come_before_a_device_is_touched():
    """Every rule of the entry, with fake non-NULL pointers on a machine without a GPU: nothing of a refused call can have reached a
    device."""
    lib = L.load()
    call = lambda a, V=2: lib.gsr_backward_views(C.byref(a), V, None)
    _refused(lib.gsr_backward_views(None, 2, None), "null args")
    for V in (0, -1, 17):
        _refused(call(_args(), V), "1..16 views expected")
    _refused(call(_args(2 ** 27), 16), "V * Npad must stay below 2^31 records", code=-4)
    _refused(call(_args(2 ** 27 - 127), 16), "V * Npad must stay below 2^31 records", code=-4)
    _refused(call(_args(flags=FLAGS)), "forward_flags do not come from gsr_forward_views")
    _refused(call(_args(flags=0)), "forward_flags do not come from gsr_forward_views")
    _refused(call(_args(flags=VIEWS_FLAGS | L.GSR_FWD_FLAG_RENDER_ONLY)), "render-only forward")
    for name in PER_GAUSSIAN:      # a full backward over views stays refused by name
        a = _args()
        setattr(a, name, FAKE)
        _refused(call(a), "a backward over views serves the frozen call only")
        assert "a full backward over views is not served" in lib.gsr_last_error().decode()
    a = _args()
    keep = L.GsrFusedAdam() if hasattr(L, "GsrFusedAdam") else (C.c_char * 1024)()
    a.fused_adam = C.addressof(keep)
    _refused(call(a), "a backward over views serves the frozen call only")
    for name, text in (("next_view", "next_view / prepared_out"), ("prepared_out", "next_view / prepared_out"), ("densify_stats", "densify_stats"),
                       ("retired_at", "retired_at"), ("batch", "not served with a batch")):
        a = _args()
        setattr(a, name, FAKE)
        _refused(call(a), text)
    _refused(call(_args(out=None)), "no gradient output")
    for miss in ("geom", "image", "binning", "scratch"):
        a = _args()
        setattr(a, miss, None)
        _refused(call(a), "missing workspace pointer")
    a = _args(workspace=False)
    _refused(call(a), "missing workspace pointer")
    # every output alone passes the output rule (the call then ends at a later check or would go on to the device: not made here)
    for out in ("d_viewmatrix", "d_projmatrix", "d_campos", "d_points_transform"):
        _refused(call(_args(out=out, workspace=False)), "missing workspace pointer")
    # gsr_backward itself keeps refusing the flags of a views forward, in its own words
    _refused(lib.gsr_backward(C.byref(_args()), None), "a backward over views is not served")


def test_pose_step_many_refuses_bad_arguments():
    lib = L.load()
    call = lambda d, m, v, g, out, P, step: lib.gsr_pose_step_many(d, m, v, g, None, out, P, 1e-3, 0.9, 0.999, 1e-8, step, None)
    assert call(None, FAKE, FAKE, FAKE, FAKE, 2, 1) == -1
    assert call(FAKE, FAKE, FAKE, FAKE, None, 2, 1) == -1
    assert call(FAKE, FAKE, FAKE, FAKE, FAKE, 0, 1) == -1
    assert call(FAKE, FAKE, FAKE, FAKE, FAKE, 2, -1) == -1
    assert call(FAKE, None, FAKE, FAKE, FAKE, 2, 1) == -1
    assert call(FAKE, FAKE, FAKE, None, FAKE, 2, 1) == -1


def test_op_schemas():
    ops = E.load()
    assert str(ops.rasterize_backward_views.default._schema) == \
        ("gsr::rasterize_backward_views(Tensor means3D, Tensor sh, Tensor colors_precomp, Tensor opacities, Tensor scales, Tensor rotations, "
         "Tensor cov3D_precomp, Tensor sh_rest, Tensor viewmatrix, Tensor projmatrix, Tensor campos, Tensor bg, Tensor points_transform, "
         "Tensor geom, Tensor image, Tensor binning, Tensor meta, Tensor grad_color, Tensor grad_depth, Tensor grad_alpha, "
         "int image_height, int image_width, float tanfovx, float tanfovy, float scale_modifier, int sh_degree, bool raw_params, "
         "bool need_means2D, bool need_viewmatrix, bool need_projmatrix, bool need_campos, bool need_points_transform, "
         "Tensor? sh_origin=None) -> Tensor[]")
    assert str(ops.pose_step_many.default._schema) == \
        ("gsr::pose_step_many(Tensor(a!) delta, Tensor(b!) exp_avg, Tensor(c!) exp_avg_sq, Tensor d_xf, Tensor base, Tensor(d!) xf, float lr, "
         "float beta1, float beta2, float eps, int step) -> ()")
    for name in ("gsr::rasterize_backward_views", "gsr::pose_step_many", "gsr::rasterize_forward_views"):
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(name, "Autograd")
        assert torch._C._dispatch_has_kernel_for_dispatch_key(name, "CUDA")


def test_fake_kernels_describe_the_outputs():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from torch.fx.experimental.symbolic_shapes import ShapeEnv
    E.load()
    with FakeTensorMode(allow_non_fake_inputs=True, shape_env=ShapeEnv()):
        f = lambda *s: torch.empty(s, device="cuda")
        b = lambda n: torch.empty((n,), dtype=torch.uint8, device="cuda")
        N, V, H, W = 129, 3, 40, 72
        model = (f(N, 3), f(N, 1, 3), f(0), f(N, 1), f(N, 3), f(N, 4), f(0), f(N, 15, 3), f(V, 4, 4), f(V, 4, 4), f(V, 3), f(3))
        tail = (b(64), b(64), b(64), torch.empty(3, dtype=torch.int64), f(V, 3, H, W), f(V, 1, H, W), f(0), H, W, 1.0, 1.0, 1.0, 3, True)
        out = torch.ops.gsr.rasterize_backward_views(*model, f(V, 3, 4), *tail, True, True, True, True, True, None)
        assert [tuple(x.shape) for x in out] == [(V * 256, 3), (V, 4, 4), (V, 4, 4), (V, 3), (V, 3, 4)]
        out = torch.ops.gsr.rasterize_backward_views(*model, f(V, 3, 4), *tail, False, False, False, True, True, None)
        assert [tuple(x.shape) for x in out] == [(0,), (0,), (0,), (V, 3), (V, 3, 4)]
        out = torch.ops.gsr.rasterize_backward_views(*model, f(0), *tail, False, True, False, False, True, None)      # no transform given
        assert [tuple(x.shape) for x in out] == [(0,), (V, 4, 4), (0,), (0,), (0,)]
        assert torch.ops.gsr.pose_step_many(f(V, 6), f(V, 6), f(V, 6), f(V, 3, 4), f(0), f(V, 3, 4), 1e-3, 0.9, 0.999, 1e-8, 1) is None


def _settings(H=40, W=72, V=None, **kw):
    lead = () if V is None else (V,)
    base = dict(image_height=H, image_width=W, tanfovx=0.8, tanfovy=0.6, bg=torch.zeros(3), scale_modifier=1.0,
                viewmatrix=torch.eye(4).expand(*lead, 4, 4).clone(), projmatrix=torch.eye(4).expand(*lead, 4, 4).clone(), sh_degree=3,
                campos=torch.zeros(*lead, 3), prefiltered=False, debug=False)
    base.update(kw)
    return R.GaussianRasterizationSettings(**base)


def _model(grad=None):
    t = lambda *s: torch.zeros(*s)
    m = dict(means3D=t(10, 3), sh=t(10, 1, 3), opacities=t(10, 1), scales=t(10, 3), rotations=t(10, 4), sh_rest=t(10, 15, 3))
    if grad:
        m[grad].requires_grad_(True)
    return m


def _views(m, vs, **kw):
    return R.rasterize_views(m["means3D"], m["sh"], m["opacities"], m["scales"], m["rotations"], vs, sh_rest=m["sh_rest"], raw_params=True, **kw)


def test_rasterize_views_refuses_before_a_device_is_touched():
    xf = torch.eye(4)[:3].repeat(2, 1, 1).requires_grad_(True)
    with pytest.raises(RuntimeError, match="rasterize_views: tensors must be on a ROCm/HIP device"):
        _views(_model(), _settings(V=2), points_transform=xf)
    for name in ("means3D", "sh", "opacities", "scales", "rotations", "sh_rest"):
        with pytest.raises(RuntimeError, match="only the frozen call is served over views"):
            _views(_model(grad=name), _settings(V=2), points_transform=xf)
    with pytest.raises(RuntimeError, match="nothing differentiable requires grad"):
        _views(_model(), _settings(V=2), points_transform=xf.detach())
    with pytest.raises(RuntimeError, match="nothing differentiable requires grad"):
        _views(_model(), _settings(V=2))
    # a camera that requires grad is something differentiable: the call gets as far as the device check
    vs = _settings(V=2)
    vs = vs._replace(viewmatrix=vs.viewmatrix.requires_grad_(True))
    with pytest.raises(RuntimeError, match="tensors must be on a ROCm/HIP device"):
        _views(_model(), vs)


def test_fit_poses_refuses_before_a_device_is_touched():
    raw = {k: torch.zeros(10, 3) for k in pose_fit.RAW_KEYS}
    targets = torch.zeros(4, 3, 40, 72)
    for bad in (0, -1, 17, 2.5, "4", None, True):
        with pytest.raises(ValueError, match="views_per_call"):
            pose_fit.fit_poses(raw, _settings(), targets, views_per_call=bad)
        with pytest.raises(ValueError, match="views_per_call"):
            pose_fit.check_views_per_call(bad)
    assert [pose_fit.check_views_per_call(v) for v in (1, 8, 16)] == [1, 8, 16]
    for V in (1, 4):
        with pytest.raises(RuntimeError, match="fit_poses: tensors must be on a ROCm/HIP device"):
            pose_fit.fit_poses(raw, _settings(), targets, views_per_call=V)
    with pytest.raises(ValueError, match="raw lacks"):
        pose_fit.fit_poses({"_xyz": torch.zeros(10, 3)}, _settings(), targets)


def test_run_segments_switches():
    a = rs_mod.parse_args(["--local"])
    assert (a.eval_pose_iters, a.eval_views_per_call) == (0, 1)          # the defaults: today's evaluation
    a = rs_mod.parse_args(["--local", "--eval-pose-iters", "10", "--eval-views-per-call", "4"])
    assert (a.eval_pose_iters, a.eval_views_per_call) == (10, 4)
    for bad in (["--eval-views-per-call", "0"], ["--eval-views-per-call", "17"], ["--eval-pose-iters", "-1"]):
        with pytest.raises(SystemExit):
            rs_mod.parse_args(["--local"] + bad)
    cfg = rs_mod.HTConfig()
    assert (cfg.eval_pose_iters, cfg.eval_views_per_call) == (0, 1)
    rs_mod.check_eval_pose(cfg)
    for kw in (dict(eval_views_per_call=0), dict(eval_views_per_call=17), dict(eval_pose_iters=-1)):
        with pytest.raises(ValueError):
            rs_mod.check_eval_pose(rs_mod.HTConfig(**kw))


def test_run_segments_as_a_script_knows_the_switches():
    """Executed as a script the module imports its siblings by name, pose_fit included: the range check answers (exit code 2) before
    anything looks for a device."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "3dgs_hierarchical_training_amd", "run_segments.py"), "--local",
                        "--eval-pose-iters", "10", "--eval-views-per-call", "17"], cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--eval-views-per-call: 1..16 expected, got 17" in r.stderr, r.stderr[-1000:]
