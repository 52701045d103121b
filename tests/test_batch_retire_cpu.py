"""CPU: the host side of per-model retirement inside a launch chain (include/gsr.h version 117: gsr_forward_retire, GsrBackwardArgs ends with
retired_at + retire_step, gsr_batch_retire) -- the library version, the exports and the struct mirror, the refusals of the C ABI and of the
Python layer (all before a device is touched: null or fake device pointers, CPU tensors), the early_exit keyword of stage A, and the float64
numpy restatement of the rule that the GPU tests hold the kernels against."""
import ctypes as C
import importlib
import inspect

import numpy as np
import pytest
import torch

import batch_retire_common as BR

R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
E = importlib.import_module("3dgs_hierarchical_training_amd._ext")
L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
stage_a = importlib.import_module("3dgs_hierarchical_training_amd.stage_a")

FAKE = 0x1000      # a non-NULL "device pointer": the refusals come before any use of it


def test_library_version_exports_and_struct_mirror():
    lib = L.load()
    assert lib.gsr_version() >= 117
    for name in ("gsr_batch_retire", "gsr_batch_retire_scratch_bytes", "gsr_forward_retire"):
        assert name in L.EXPORTS and hasattr(lib, name), name
    assert lib.gsr_struct_bytes(0) == C.sizeof(L.GsrForwardArgs) and lib.gsr_struct_bytes(1) == C.sizeof(L.GsrBackwardArgs)
    # appended: every earlier field keeps its offset
    assert L.GsrBackwardArgs._fields_[-2:] == [("retired_at", C.c_void_p), ("retire_step", C.c_int64)]
    # the forward's table travels beside GsrForwardArgs (gsr_forward_retire): that struct keeps its version-116 layout
    assert L.GsrForwardArgs._fields_[-1] == ("render_only", C.c_int32) and not hasattr(L.GsrForwardArgs, "retired_at")
    assert L.GsrBackwardArgs.retired_at.offset == L.GsrBackwardArgs.sh_origin.offset + C.sizeof(C.c_void_p)
    assert lib.gsr_batch_retire_scratch_bytes(3) >= 3 * 8 and lib.gsr_batch_retire_scratch_bytes(3) % 8 == 0


def test_the_new_ops_exist_and_the_old_schemas_are_unchanged():
    ops = E.load()
    assert str(ops.batch_retire.default._schema) == \
        "gsr::batch_retire(Tensor render, Tensor target, Tensor(a!) retired_at, float mse_bar, int exit_after, int step) -> Tensor"
    assert str(ops.retire_attach.default._schema) == "gsr::retire_attach(Tensor retired_at, int step) -> ()"
    assert str(ops.rasterize.default._schema).count("Tensor? sh_origin=None, int frozen=-1) -> ") == 1


def _fwd(**kw):
    a = L.GsrForwardArgs()
    a.N, a.M, a.D, a.W, a.H = 128, 16, 0, 32, 32
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _bwd(**kw):
    b = L.GsrBackwardArgs()
    b.N, b.M, b.D, b.W, b.H = 128, 16, 0, 32, 32
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _msg():
    return L.load().gsr_last_error().decode()


def test_forward_refuses_a_table_with_render_only_or_a_bad_step():
    lib = L.load()
    out = L.GsrForwardOut()
    assert lib.gsr_forward_retire(C.byref(_fwd(render_only=1, out_color=FAKE)), FAKE, 3, C.byref(out), None) == -1
    assert "retire table is not served with render_only" in _msg(), _msg()
    for step in (0, -1, 2 ** 31):
        assert lib.gsr_forward_retire(C.byref(_fwd()), FAKE, step, C.byref(out), None) == -1
        assert "retire_step must be the 1-based step" in _msg(), _msg()
    assert out.binning is None and out.num_rendered == 0
    # without a table the entry is gsr_forward: the same calls go on to their ordinary checks
    assert lib.gsr_forward_retire(C.byref(_fwd(render_only=1)), None, 0, C.byref(out), None) == -1 and "retire" not in _msg()
    assert lib.gsr_forward(C.byref(_fwd(render_only=1)), C.byref(out), None) == -1 and "retire" not in _msg()


def test_importance_and_render_only_cannot_be_given_a_table():
    """gsr_importance_accumulate takes a GsrForwardArgs, which carries no table; the Python entries of the two routes have no `retire` keyword
    (the binding refuses a table left with them through torch.ops.gsr.retire_attach: tests/test_gpu_batch_retire.py)."""
    assert not hasattr(L.GsrForwardArgs, "retired_at")
    for fn in (R.render_gaussians, R.render_gaussians_raw, R.importance_accumulate):
        assert "retire" not in inspect.signature(fn).parameters, fn


def test_backward_refuses_a_table_where_no_update_is_gated():
    lib = L.load()
    # the frozen call: no fused_adam, no per-Gaussian gradient pointer, a camera output
    assert lib.gsr_backward(C.byref(_bwd(d_viewmatrix=FAKE, retired_at=FAKE, retire_step=2)), None) == -1
    assert "not served on the frozen backward" in _msg(), _msg()
    # the plain backward (gradients out, Adam as a separate launch)
    assert lib.gsr_backward(C.byref(_bwd(d_means3D=FAKE, d_means2D=FAKE, d_opacities=FAKE, retired_at=FAKE, retire_step=2)), None) == -1
    assert "needs fused_adam" in _msg(), _msg()
    fa = L.GsrFusedAdam()
    fa.step = 1
    b = _bwd(d_means2D=FAKE, fused_adam=C.addressof(fa), retired_at=FAKE, retire_step=0)
    assert lib.gsr_backward(C.byref(b), None) == -1 and "retire_step must be the 1-based step" in _msg(), _msg()
    # the deferred step and densify_stats
    fa.param_out[0] = FAKE
    b.retire_step = 2
    assert lib.gsr_backward(C.byref(b), None) == -1 and "deferred step" in _msg(), _msg()
    fa.param_out[0] = None
    b.densify_stats = FAKE
    assert lib.gsr_backward(C.byref(b), None) == -1 and "densify_stats" in _msg(), _msg()


def test_batch_retire_argument_rules():
    lib = L.load()
    ok = dict(render=FAKE, target=FAKE, B=3, C_=3, H=4, W=4, bar=1e-3, after=500, step=1, table=FAKE, mse=FAKE, scratch=FAKE)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gsr_batch_retire(a["render"], a["target"], a["B"], a["C_"], a["H"], a["W"], a["bar"], a["after"], a["step"], a["table"], a["mse"],
                                    a["scratch"], None)
    for bad in (dict(render=None), dict(target=None), dict(table=None), dict(mse=None), dict(scratch=None), dict(B=0), dict(B=65536), dict(H=0),
                dict(step=0), dict(step=2 ** 31), dict(after=-1), dict(mse=FAKE + 4), dict(scratch=FAKE + 4)):
        assert call(**bad) == -1, bad


def test_python_routes_refuse_a_table_before_a_device_is_touched():
    n = 128
    z = lambda *s: torch.zeros(*s)
    rs = R.GaussianRasterizationSettings(image_height=16, image_width=16, tanfovx=0.5, tanfovy=0.5, bg=z(3), scale_modifier=1.0, viewmatrix=torch.eye(4),
                                         projmatrix=torch.eye(4), sh_degree=0, campos=z(3), prefiltered=False, debug=False)
    table = torch.zeros(1, dtype=torch.int32)
    args = (z(n, 3), z(n, 3), z(n, 1, 3), z(n, 15, 3), z(n, 1), z(n, 3), z(n, 4), rs)
    with pytest.raises(RuntimeError, match="needs fused_adam"):          # Adam as a separate FusedAdam.step() launch
        R.rasterize_gaussians_raw(*args, retire=(table, 1))
    opt = object()
    with pytest.raises(RuntimeError, match="deferred step"):
        R.rasterize_gaussians_raw(*args, fused_adam=opt, fused_adam_deferred=True, retire=(table, 1))
    with pytest.raises(RuntimeError, match="densify_stats"):
        R.rasterize_gaussians_raw(*args, fused_adam=opt, densify_stats=(z(n), z(n), z(n)), retire=(table, 1))
    with pytest.raises(RuntimeError, match="1-based"):
        R.rasterize_gaussians_raw(*args, fused_adam=opt, retire=(table, 0))
    with pytest.raises(RuntimeError, match="int32"):
        R.rasterize_gaussians_raw(*args, fused_adam=opt, retire=(torch.zeros(1), 1))
    with pytest.raises(RuntimeError, match="frozen"):
        R._check_retire((table, 1), fused_adam=opt, frozen=True)
    for fn in (R.rasterize_gaussians_raw, ts.render, ts.train_step):
        assert inspect.signature(fn).parameters["retire"].default is None, fn


def test_train_step_refuses_a_table_off_the_fused_route():
    scene = {"means3D": torch.zeros(4, 3), "shs": torch.zeros(4, 16, 3), "scales": torch.ones(4, 3), "rotations": torch.ones(4, 4),
             "opacities": torch.full((4, 1), 0.5), "sh_degree": 0}
    params = ts.GaussianParams(scene, torch.device("cpu"))
    table = params.new_retire_table(psnr_exit=30.0, exit_after=7)
    assert table.retired_at.dtype == torch.int32 and table.retired_at.tolist() == [0] and table.step == 0
    assert table.mse_bar == BR.mse_bar(30.0) and table.exit_after == 7 and table.retired_sync() == [0]
    assert "SYNCHRONISES" in ts.RetireTable.retired_sync.__doc__ and "SYNCHRONISES" in ts.GaussianParams.retired_sync.__doc__
    with pytest.raises(RuntimeError, match="retire"):
        ts.train_step(params, None, torch.zeros(3, 4, 4), fused_optimizer=False, retire=table)
    assert table.step == 0


def test_unknown_early_exit_raises_before_anything_else():
    for fn, args in ((stage_a.fit_pair, (None, 0, None)), (stage_a.fit_pairs_batched, (None, [0, 1], None))):
        with pytest.raises(ValueError, match="early_exit"):
            fn(*args, early_exit="bogus")
        p = inspect.signature(fn).parameters
        assert (p["early_exit"].default, p["psnr_exit"].default, p["exit_after"].default) == ("host", 35.0, 500)
    assert stage_a.EARLY_EXIT_MODES == ("host", "device")


def test_the_rule_restated():
    bar = BR.mse_bar(35.0)
    assert abs(bar - 10 ** -3.5) < 1e-18
    mse = np.array([bar * 0.5, bar, bar * 2.0, np.nan])
    # nothing at s == exit_after, the passing image at s == exit_after + 1; equality and NaN do not pass (strict <)
    assert BR.retire_rule([0, 0, 0, 0], mse, 500, bar, 500).tolist() == [0, 0, 0, 0]
    assert BR.retire_rule([0, 0, 0, 0], mse, 501, bar, 500).tolist() == [501, 0, 0, 0]
    # sticky: a set entry survives a later, worse image and a later, better one
    assert BR.retire_rule([501, 0, 7, 0], np.array([1.0, 0.0, 0.0, 0.0]), 600, bar, 500).tolist() == [501, 600, 7, 600]
    # the render culls strictly after the retiring step, Adam still runs AT it
    assert [BR.render_is_culled(e, 3) for e in (0, 2, 3, 4)] == [False, True, False, False]
    assert [BR.adam_runs(e, 3) for e in (0, 2, 3, 4)] == [True, False, True, True]
    # the float64 MSE: clamp in float32, difference and square in float64
    r = np.array([[[[-1.0, 0.25], [2.0, 0.5]]]], dtype=np.float32)
    t = np.array([[[[0.5, 0.25], [0.5, 1.0]]]], dtype=np.float32)
    assert BR.image_mse(r, t).tolist() == [(0.25 + 0.0 + 0.25 + 0.25) / 4]
