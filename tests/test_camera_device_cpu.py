"""CPU: the host side of the device cameras (include/gsr.h version 119: gsr_camera_from_pose, gsr_pose_virtual_view) -- the library version,
the exports and their ctypes signatures, every refusal of the C ABI (all before a device is touched: null or fake device pointers), the op
schemas, the Python layer's refusal of CPU tensors, the harness switch, and the numpy float64 oracle the GPU tests hold the kernels
against: on the hand-worked cases, against pose.py's torch statements and against the reference's own `Camera` (tests/golden/camera.npz and
camera_general.npz hold its view matrix, intrinsics, size and the matrices it built from them)."""
import ctypes as C
import importlib
import inspect
import math
import os

import numpy as np
import pytest
import torch

import camera_device_common as CC

E = importlib.import_module("3dgs_hierarchical_training_amd._ext")
L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
cameras = importlib.import_module("3dgs_hierarchical_training_amd.cameras")
pose_mod = importlib.import_module("3dgs_hierarchical_training_amd.pose")

FAKE = 0x1000      # a non-NULL "device pointer": the refusals come before any use of it


def test_library_version_and_exports():
    lib = L.load()
    assert lib.gsr_version() >= 119
    for name in ("gsr_camera_from_pose", "gsr_pose_virtual_view"):
        assert name in L.EXPORTS and hasattr(lib, name), name
    assert lib.gsr_struct_bytes(0) == C.sizeof(L.GsrForwardArgs) and lib.gsr_struct_bytes(1) == C.sizeof(L.GsrBackwardArgs)
    assert lib.gsr_camera_from_pose.restype is C.c_int
    assert lib.gsr_camera_from_pose.argtypes == [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32,
                                                 C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.gsr_pose_virtual_view.restype is C.c_int
    assert lib.gsr_pose_virtual_view.argtypes == [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]


def test_camera_from_pose_argument_rules():
    lib = L.load()
    ok = dict(pose=FAKE, B=1, fx=50.0, fy=51.0, cx=32.0, cy=24.0, W=64, H=48, znear=0.01, zfar=100.0, view=FAKE, proj=FAKE, campos=FAKE)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gsr_camera_from_pose(a["pose"], a["B"], a["fx"], a["fy"], a["cx"], a["cy"], a["W"], a["H"], a["znear"], a["zfar"],
                                        a["view"], a["proj"], a["campos"], None)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(pose=None), dict(view=None), dict(proj=None), dict(campos=None),                   # a NULL pointer
                dict(B=0), dict(B=-1), dict(B=17), dict(B=2 ** 20),                                      # 1 <= B <= 16
                dict(fx=0.0), dict(fx=-50.0), dict(fy=0.0), dict(fy=-1.0), dict(fx=nan), dict(fy=inf),   # focal lengths positive and finite
                dict(W=0), dict(W=-64), dict(H=0), dict(H=-48),                                          # a positive size
                dict(cx=nan), dict(cy=inf), dict(znear=nan), dict(zfar=inf), dict(znear=5.0, zfar=5.0)):
        assert call(**bad) == -1, bad


def test_pose_virtual_view_argument_rules():
    lib = L.load()
    ok = dict(p0=FAKE, p1=FAKE, alpha=0.5, base=FAKE, out=FAKE, out_rel=FAKE)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gsr_pose_virtual_view(a["p0"], a["p1"], a["alpha"], a["base"], a["out"], a["out_rel"], None)
    for bad in (dict(p0=None), dict(p1=None), dict(out=None), dict(base=None), dict(out_rel=None),      # NULL; base / out_rel on one side only
                dict(alpha=-0.01), dict(alpha=1.01), dict(alpha=float("nan")), dict(alpha=float("inf")),
                dict(base=None, out_rel=None, p0=None), dict(base=None, out_rel=None, alpha=2.0)):
        assert call(**bad) == -1, bad


def test_op_schemas():
    ops = E.load()
    assert str(ops.camera_from_pose.default._schema) == \
        "gsr::camera_from_pose(Tensor pose, float fx, float fy, float cx, float cy, int W, int H, float znear=0.01, float zfar=100.) -> " \
        "(Tensor viewmatrix, Tensor projmatrix, Tensor campos)"
    assert str(ops.pose_virtual_view.default._schema) == \
        "gsr::pose_virtual_view(Tensor pose0, Tensor pose1, float alpha, Tensor? base=None) -> (Tensor out, Tensor out_rel)"


def test_ops_have_no_cpu_kernel():
    ops = E.load()
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.camera_from_pose(torch.eye(4), 50.0, 50.0, 32.0, 24.0, 64, 48)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.pose_virtual_view(torch.eye(4), torch.eye(4), 0.5)


def test_python_wrappers_refuse_cpu_tensors_before_a_device_is_touched():
    R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    tpl = R.GaussianRasterizationSettings(image_height=48, image_width=64, tanfovx=0.8, tanfovy=0.6, bg=torch.zeros(3), scale_modifier=1.0,
                                          viewmatrix=None, projmatrix=None, sh_degree=0, campos=None, prefiltered=False, debug=False)
    eye = torch.eye(4)
    for fn, args in ((cameras.camera_from_pose, (eye, 40.0, 40.0, 32.0, 24.0, 64, 48)), (cameras.settings_from_pose, (tpl, eye)),
                     (cameras.virtual_view, (eye, eye, 0.5)), (cameras.virtual_view, (eye, eye, 0.5, eye))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(*args)
    src = inspect.getsource(cameras)
    code = "\n".join(ln for ln in src.split('"""')[2::2])          # the module without its docstrings
    for word in (".cpu()", ".item()", ".numpy()", "linalg", "import oracle", "from oracle"):
        assert word not in code, word


def test_harness_switch_is_off_by_default():
    rs = importlib.import_module("3dgs_hierarchical_training_amd.run_segments")
    assert rs.HTConfig().device_cameras is False
    assert '"--device-cameras", action="store_true"' in inspect.getsource(rs)
    assert "device_cameras=a.device_cameras" in inspect.getsource(rs)


def test_the_oracle_on_the_hand_worked_cases():
    r = CC.camera_oracle(np.eye(4, dtype=np.float32), 42.0, 42.0, 32.0, 24.0, 64, 48)
    assert np.array_equal(r["view"], np.eye(4)) and np.array_equal(r["campos"], np.zeros(3))
    assert np.array_equal(r["proj"], np.array(CC.projection(42.0, 42.0, 32.0, 24.0, 64, 48)).T)      # identity view: the full projection is P^T
    r = CC.camera_oracle(CC.HAND_POSE, **CC.HAND_INTR)
    assert np.array_equal(r["view"], CC.HAND_VIEW) and np.array_equal(r["campos"], CC.HAND_CAMPOS) and np.array_equal(r["proj"], CC.HAND_FULL)
    # a batch is its poses one by one
    poses = CC.batch_poses(5)
    rb = CC.camera_oracle(poses, 611.3, 598.7, 501.25, 260.5, 980, 545)
    for b in range(5):
        one = CC.camera_oracle(poses[b], 611.3, 598.7, 501.25, 260.5, 980, 545)
        assert all(np.array_equal(rb[k][b], one[k]) for k in ("view", "proj", "campos"))
    # the camera centre of a pose that is NOT orthonormal: -A^-1 t, not -A^T t
    p = CC.make_pose((1.0, -0.4, 0.3), 0.8, (0.3, -1.2, 2.0), skew=0.05)
    want = -np.linalg.solve(p[:3, :3].astype(np.float64), p[:3, 3].astype(np.float64))
    assert np.allclose(CC.camera_oracle(p, 42.0, 42.0, 32.0, 24.0, 64, 48)["campos"], want, rtol=1e-13, atol=1e-13)
    assert not np.allclose(-p[:3, :3].T.astype(np.float64) @ p[:3, 3].astype(np.float64), want, atol=1e-3)


def test_the_virtual_view_oracle_on_hand_worked_cases_and_against_pose_py():
    eye = np.eye(4, dtype=np.float32)
    quarter = np.array([[0, 0, 1, 0], [0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, 0, 1]], dtype=np.float32)      # 90 degrees about y
    out, rel = CC.virtual_view_oracle(eye, quarter, 0.5)
    s = math.sqrt(0.5)
    assert rel is None and np.allclose(out, [[s, 0, s, 0], [0, 1, 0, 0], [-s, 0, s, 0], [0, 0, 0, 1]], rtol=0, atol=1e-15)
    # alpha = 0 is pose0 bit for bit; alpha = 1 is pose1 as float32; a base multiplies by its inverse
    for p0, p1 in ((CC.sequence_pose(3), CC.sequence_pose(4)), (CC.HAND_POSE, CC.make_pose((0.3, 1.0, -0.2), 2.5, (0.5, -1.0, 2.0)))):
        assert np.array_equal(CC.virtual_view_oracle(p0, p1, 0.0)[0], p0.astype(np.float64))
        # (Exp(Log(R)) is a rotation to float64 accuracy, pose1's block only to float32 accuracy: alpha = 1 returns pose1 as a float32 matrix)
        assert CC.ulp_distance(CC.virtual_view_oracle(p0, p1, 1.0)[0].astype(np.float32), p1.astype(np.float64))[0] <= 1.0
        for alpha in (0.25, 0.61803):
            base = CC.sequence_pose(1)
            out, rel = CC.virtual_view_oracle(p0, p1, alpha, base)
            want = pose_mod.interpolate_pose(torch.from_numpy(p0).double(), torch.from_numpy(p1).double(), alpha).numpy()
            assert np.allclose(out, want, rtol=0, atol=1e-12)
            assert np.allclose(rel, want @ np.linalg.inv(base.astype(np.float64)), rtol=0, atol=1e-12)
    # the same switches as pose.py: two identical poses take both series branches and give the pose back
    p = CC.sequence_pose(5)
    assert np.array_equal(CC.virtual_view_oracle(p, p, 0.37)[0][:3, :3].astype(np.float32), p[:3, :3])


def _golden_cameras(golden_dir):
    d = np.load(os.path.join(golden_dir, "camera.npz"))
    yield "camera.npz co3d", d["co3d_view"], d["K"], int(d["W"]), int(d["H"]), d["co3d_proj"], d["co3d_full"], d["co3d_campos"]
    g = np.load(os.path.join(golden_dir, "camera_general.npz"))
    for tag in ("both", "far_both"):
        yield f"camera_general.npz {tag}", g[f"{tag}_view"], g[f"{tag}_K"], int(g["W"]), int(g["H"]), g[f"{tag}_proj"], g[f"{tag}_full"], g[f"{tag}_campos"]


def test_the_oracle_reproduces_the_reference_camera(golden_dir):
    """The reference's `Camera(is_co3d=True)` (scene/cameras.py:76-98) computes in float32: the projection entries are rounded to float32,
    the `bmm` rounds every product and partial sum, the camera centre comes out of a float32 LU inverse of the 4x4.  The float64 oracle, fed
    the float32 view matrix the reference itself used, must agree with it to the float32 error of those statements:
      full projection   8 * 2^-24 * sum_k |view[i,k]| |P^T[k,j]|   (one rounding of P, one per product, three partial sums, one of the oracle's
                        own output: 6, with slack for the fx / w division done in float32)
      camera centre     32 * 2^-24 * cond_inf(view) * max(1, |centre|_inf)   (a 4x4 LU inverse: a small multiple of cond * eps)"""
    eps = 2.0 ** -24
    seen = 0
    for name, view, K, W, H, proj, full, campos in _golden_cameras(golden_dir):
        assert view.dtype == np.float32 and full.dtype == np.float32
        pose = view.T.copy()                                  # world_view_transform is the transposed pose
        assert np.array_equal(pose[3], [0, 0, 0, 1])
        fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
        r = CC.camera_oracle(pose, fx, fy, cx, cy, W, H)
        assert np.array_equal(r["view"].astype(np.float32), view), name
        PT = np.array(CC.projection(fx, fy, cx, cy, W, H)).T
        assert np.allclose(PT, proj.astype(np.float64), rtol=4 * eps, atol=0), name          # the pose-independent projection_matrix
        bound = 8 * eps * (np.abs(view.astype(np.float64)) @ np.abs(PT)) + 1e-30
        err = np.abs(r["proj"] - full.astype(np.float64))
        print(f"{name}: full projection {float((err / bound).max()):.3f} of its float32 bound", end="; ")
        assert (err <= bound).all(), name
        v64 = view.astype(np.float64)
        cond = np.abs(v64).sum(1).max() * np.abs(np.linalg.inv(v64)).sum(1).max()
        cb = 32 * eps * cond * max(1.0, float(np.abs(campos).max()))
        cerr = float(np.abs(r["campos"] - campos.astype(np.float64)).max())
        print(f"camera centre {cerr / cb:.3f} of its float32 bound")
        assert cerr <= cb, name
        seen += 1
        if "general" in name:
            assert fx != fy and cx != W / 2 and cy != H / 2
    assert seen == 3


# ---- gsr_autopatch: DevicePose and the frame cache, on CPU ------------------------------------------------------------------------------------
# The HIP op cannot run here, so `gsr_autopatch._ops` is replaced by a stand-in whose `camera_from_pose` is the float64 oracle rounded to
# float32 (test infrastructure: the values the GPU tests hold the kernel to), and `_REQUIRE_CUDA` is lifted so that CPU images are cached.
refstub = importlib.import_module("3dgs_hierarchical_training_amd.refstub")


class _OracleOps:
    def __init__(self):
        self.calls = 0

    def camera_from_pose(self, pose, fx, fy, cx, cy, W, H, znear=0.01, zfar=100.0):
        self.calls += 1
        r = CC.camera_oracle(pose.numpy(), fx, fy, cx, cy, W, H, znear, zfar)
        return tuple(torch.from_numpy(r[k].astype(np.float32)) for k in ("view", "proj", "campos"))


def _frames(n=3, W=64, H=48, seed=0):
    g = np.random.default_rng(seed)
    return [g.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(n)]


K_STUB = np.array([[50.0, 0, 30.5], [0, 47.0, 25.0], [0, 0, 1]])


def _stub_module(data_type):
    import types

    class GaussianTrainer(refstub.StubTrainer):
        originals = 0

        def load_viewpoint_cam(self, *a, **k):
            type(self).originals += 1
            return super().load_viewpoint_cam(*a, **k)
    mod = types.ModuleType("trainer.trainer")
    mod.GaussianTrainer = GaussianTrainer
    return mod


@pytest.fixture
def frames_patch(monkeypatch):
    import gsr_autopatch
    monkeypatch.delenv("GSR_AUTOPATCH_FRAMES", raising=False)
    monkeypatch.delenv("GSR_AUTOPATCH_FRAMES_MB", raising=False)
    gsr_autopatch.apply()
    ops = _OracleOps()
    monkeypatch.setattr(gsr_autopatch, "_REQUIRE_CUDA", False)
    monkeypatch.setattr(gsr_autopatch, "_ops", lambda: ops)
    monkeypatch.setattr(gsr_autopatch, "_test_ops", ops, raising=False)
    yield gsr_autopatch
    gsr_autopatch.remove()


def test_device_pose_semantics_on_cpu_storage():
    import gsr_autopatch
    DP = gsr_autopatch.DevicePose
    m = torch.from_numpy(CC.sequence_pose(3))
    p = m.clone().as_subclass(DP)
    assert p.cpu() is p and type(p.detach()) is DP and type(p.detach().cpu()) is DP        # the trainer's `.detach().cpu()` copies nothing
    assert type(p[:3, :3]) is DP and p[:3, :3].data_ptr() == p.data_ptr()                   # a view of the same storage
    R, t = p[:3, :3].numpy(), p[:3, 3].numpy()                                               # what the original loader does with its pose
    assert isinstance(R, np.ndarray) and np.array_equal(R, m[:3, :3].numpy()) and np.array_equal(t, m[:3, 3].numpy())
    assert np.array_equal(np.asarray(p), m.numpy())
    # an operation with a genuine CPU tensor gives the plain result
    rel = torch.from_numpy(CC.sequence_pose(1))
    out = rel @ p
    assert type(out) is torch.Tensor and torch.equal(out, rel @ m)
    assert type(p @ rel) is torch.Tensor and torch.equal(p @ rel, m @ rel)
    assert type(torch.stack([p, rel])) is torch.Tensor
    # poses combined with poses alone stay poses: `pose_dict[...]` entries are `get_RT().detach()` results themselves, and the trainer's
    # `pose_dict[...].detach().cpu() @ pose_train` must still deliver `.numpy()` to the original loader
    q = rel.clone().as_subclass(DP)
    prod = q.detach().cpu() @ p.detach().cpu()
    assert type(prod) is DP and np.array_equal(prod[:3, :3].numpy(), (rel @ m)[:3, :3].numpy())
    assert type(p.inverse()) is DP and torch.equal(p.inverse().as_subclass(torch.Tensor), m.inverse())
    assert tuple(p.shape) == (4, 4) and p.dtype == torch.float32
    # `.cpu()` of a genuine CPU tensor is the ordinary one
    assert type(m.cpu()) is torch.Tensor and m.cpu() is m
    # autograd history survives the wrapping (get_RT of a trainable pose)
    w = torch.eye(4, requires_grad=True)
    q = (w * 2.0).as_subclass(DP)
    q.sum().backward()
    assert torch.equal(w.grad, torch.full((4, 4), 2.0))


def test_patched_get_rt_returns_a_device_pose(frames_patch):
    import types
    A = frames_patch

    class HTGaussianModel(refstub.StubGaussians):
        pass
    mod = types.ModuleType("scene.gaussian_model_ht")
    mod.HTGaussianModel = HTGaussianModel
    orig = HTGaussianModel.get_RT
    A._patch_frames_module(mod)
    assert HTGaussianModel.get_RT is A.get_RT_device
    g = HTGaussianModel.__new__(HTGaussianModel)
    g.P, g._p = None, types.SimpleNamespace(_xyz=torch.zeros(2, 3))
    out = g.get_RT(0)
    assert type(out) is A.DevicePose and torch.equal(out.inverse().as_subclass(torch.Tensor), torch.eye(4)) and out.detach().cpu() is not None
    A.remove()
    assert HTGaussianModel.get_RT is orig


def test_frames_switch_off_leaves_the_classes_untouched(monkeypatch, tmp_path):
    """Through the import hook, as the other patches: a module named trainer.trainer imported AFTER apply()."""
    import sys
    import gsr_autopatch
    pkg = tmp_path / "trainer"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    (pkg / "trainer.py").write_text("class GaussianTrainer:\n    def load_viewpoint_cam(self, idx, pose=None, load_depth=False, pose_to_train=False, load_vfi=False):\n"
                                    "        return 'original'\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    for value, patched in (("0", False), ("1", True)):
        monkeypatch.setenv("GSR_AUTOPATCH_FRAMES", value)
        for name in ("trainer", "trainer.trainer"):
            monkeypatch.delitem(sys.modules, name, raising=False)      # (restored when the test ends, whatever was there)
        gsr_autopatch.apply()
        try:
            mod = importlib.import_module("trainer.trainer")
            assert (mod.GaussianTrainer.load_viewpoint_cam is gsr_autopatch.load_viewpoint_cam_cached) == patched, value
            if not patched:
                assert mod.GaussianTrainer().load_viewpoint_cam(0) == "original" and not gsr_autopatch._patched_frame_classes
        finally:
            gsr_autopatch.remove()
        assert mod.GaussianTrainer().load_viewpoint_cam(0) == "original"


@pytest.mark.parametrize("data_type", ["custom", "preloaded"])
def test_patched_loader_on_the_stand_in_trainer(frames_patch, data_type):
    A = frames_patch
    mod = _stub_module(data_type)
    T = mod.GaussianTrainer
    A._patch_frames_module(mod)
    assert T.load_viewpoint_cam is A.load_viewpoint_cam_cached
    tr = T(_frames(), K_STUB, data_type=data_type, device="cpu")
    ref = refstub.StubTrainer(_frames(), K_STUB, data_type=data_type, device="cpu")            # the unpatched route
    pose = torch.from_numpy(CC.sequence_pose(4))
    # first call: the original, cached; later calls: no original, the same plane, the same fields
    c0 = tr.load_viewpoint_cam(1)
    assert T.originals == 1 and isinstance(c0, refstub.StubCameraFull)
    c1 = tr.load_viewpoint_cam(1)
    r1 = ref.load_viewpoint_cam(1)
    assert T.originals == 1 and type(c1) is refstub.StubCameraFull and c1 is not c0 and c1.original_image is c0.original_image
    assert torch.equal(c1.original_image, r1.original_image)
    for k in ("uid", "colmap_id", "FoVx", "FoVy", "image_name", "image_width", "image_height", "znear", "zfar", "focal_x", "focal_y", "vfi"):
        assert getattr(c1, k) == getattr(r1, k), k
    assert np.array_equal(c1.intrinsics, r1.intrinsics) and torch.equal(c1.projection_matrix, r1.projection_matrix)
    for k in ("world_view_transform", "full_proj_transform", "camera_center"):                 # identity cameras: bit-equal, no launch
        assert torch.equal(getattr(c1, k), getattr(r1, k)), k
    assert A._test_ops.calls == 0 and np.array_equal(c1.R, np.eye(3)) and np.array_equal(c1.T, np.zeros(3))
    # a posed camera: one call of the kernel, within the float32 error of the original's statements
    c2 = tr.load_viewpoint_cam(1, pose=pose)
    r2 = ref.load_viewpoint_cam(1, pose=pose)
    assert T.originals == 1 and A._test_ops.calls == 1 and c2.original_image is c0.original_image
    assert torch.equal(c2.world_view_transform, r2.world_view_transform)
    assert torch.allclose(c2.full_proj_transform, r2.full_proj_transform, rtol=0, atol=1e-5) and torch.allclose(c2.camera_center, r2.camera_center, rtol=0, atol=1e-5)
    assert np.array_equal(c2.R, r2.R) and np.array_equal(c2.T, r2.T)
    # a DevicePose is taken as it is; its camera is the plain pose's
    c3 = tr.load_viewpoint_cam(1, pose=pose.clone().as_subclass(A.DevicePose).detach().cpu())
    assert T.originals == 1 and torch.equal(c3.full_proj_transform, c2.full_proj_transform) and torch.equal(c3.camera_center, c2.camera_center)
    assert np.array_equal(c3.R.numpy(), r2.R)
    # work the cache cannot know runs the original: pose_to_train, a depth or a vfi that is not there yet
    n = T.originals
    if data_type == "preloaded":
        ct = tr.load_viewpoint_cam(1, pose=pose, pose_to_train=True)
        assert T.originals == n + 1 and torch.is_tensor(ct.R)
        n = T.originals
    tr.load_viewpoint_cam(1, load_depth=True)
    assert T.originals == n + 1 and tr.depth_calls == 1 and 1 in tr.mono_depth
    tr.load_viewpoint_cam(1, load_depth=True)                                                  # the depth is there now: cached
    assert T.originals == n + 1 and tr.depth_calls == 1
    if data_type == "preloaded":
        cv = tr.load_viewpoint_cam(1, load_vfi=True)
        assert T.originals == n + 2 and tr.vfi_calls == 1 and "1_to_2" in tr.vfi
        cv2 = tr.load_viewpoint_cam(1, load_vfi=True)                                          # a vfi already there is attached as the original does
        assert T.originals == n + 2 and cv2.vfi is tr.vfi["1_to_2"] and cv.vfi is cv2.vfi
        tr.load_viewpoint_cam(2, load_vfi=True)                                                # the last frame has no pair: the original, every time
        tr.load_viewpoint_cam(2, load_vfi=True)
        assert T.originals == n + 4
    # a DevicePose handed to the original arrives as the host tensor the reference would have passed
    n = T.originals
    cd = tr.load_viewpoint_cam(0, pose=pose.clone().as_subclass(A.DevicePose), load_depth=True)
    assert T.originals == n + 1 and isinstance(cd.R, np.ndarray) and np.array_equal(cd.R, r2.R)
    # an in-place write into the cached plane makes the next call rebuild it
    n = T.originals
    c0.original_image.mul_(0.5)
    c4 = tr.load_viewpoint_cam(1)
    assert T.originals == n + 1 and c4.original_image is not c0.original_image and torch.equal(c4.original_image, r1.original_image)
    assert tr.load_viewpoint_cam(1).original_image is c4.original_image and T.originals == n + 1


def test_frame_budget(frames_patch, monkeypatch):
    A = frames_patch
    mod = _stub_module("custom")
    T = mod.GaussianTrainer
    A._patch_frames_module(mod)
    monkeypatch.setenv("GSR_AUTOPATCH_FRAMES_MB", "1")
    big = _frames(1, W=320, H=300)                       # 320 x 300 x 3 floats = 1.1 MB: over the budget
    tr = T(big + _frames(2), K_STUB, data_type="custom", device="cpu")
    tr.load_viewpoint_cam(0); tr.load_viewpoint_cam(0)
    assert T.originals == 2 and 0 not in tr._gsr_frames["entries"]
    tr.load_viewpoint_cam(1); tr.load_viewpoint_cam(1)
    assert T.originals == 3 and tr._gsr_frames["bytes"] == 64 * 48 * 3 * 4
    assert A._frame_budget_bytes() == 1 << 20
    monkeypatch.delenv("GSR_AUTOPATCH_FRAMES_MB")
    assert A._frame_budget_bytes() == 16384 << 20


def test_a_pose_product_reaches_the_original_loader_as_a_host_pose(frames_patch, monkeypatch):
    """ht3dgs_trainer.py:561-562 as stage A leaves it: `pose_dict[...]` holds a `get_RT().detach()` result, the loader gets
    `pose_dict[...].detach().cpu() @ pose_train` with load_depth and load_vfi -- on calls the patched loader hands to the original (nothing
    of the frame known yet; a frame over the budget), whose `pose[:3, :3].numpy()` needs a host pose."""
    A = frames_patch
    mod = _stub_module("preloaded")
    T = mod.GaussianTrainer
    A._patch_frames_module(mod)
    rel = torch.from_numpy(CC.sequence_pose(1)).as_subclass(A.DevicePose).detach()          # what stage A stored
    pose_train = torch.from_numpy(CC.sequence_pose(4)).as_subclass(A.DevicePose).detach().cpu()
    want = (torch.from_numpy(CC.sequence_pose(1)) @ torch.from_numpy(CC.sequence_pose(4))).numpy()
    tr = T(_frames(), K_STUB, data_type="preloaded", device="cpu")
    cam = tr.load_viewpoint_cam(0, pose=rel.detach().cpu() @ pose_train, load_depth=True, load_vfi=True)
    assert T.originals == 1 and isinstance(cam.R, np.ndarray) and np.array_equal(cam.R, want[:3, :3]) and np.array_equal(cam.T, want[:3, 3])
    monkeypatch.setenv("GSR_AUTOPATCH_FRAMES_MB", "0.01")                                       # every frame is over the budget
    tr2 = T(_frames(), K_STUB, data_type="preloaded", device="cpu")
    for _ in range(2):
        cam = tr2.load_viewpoint_cam(1, pose=rel.detach().cpu() @ pose_train, load_depth=True, load_vfi=True)
        assert isinstance(cam.R, np.ndarray) and np.array_equal(cam.R, want[:3, :3])
    assert T.originals == 3 and not tr2._gsr_frames["entries"]
