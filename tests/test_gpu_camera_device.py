"""GPU: cameras from poses that stay on the device (include/gsr.h version 119; csrc/camera_kernels.hip, cameras.py) against the numpy
float64 oracle of tests/camera_device_common.py -- whose docstring states the bars: bit equality with the oracle's value rounded to float32
for gsr_camera_from_pose; one float32 ulp of it plus the float64 oracle's own rounding error for gsr_pose_virtual_view.  Then a render under such a camera against the host route's, the frame cache of
`gsr_autopatch` on the stand-in trainer, and the harness switch."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest
import torch

import camera_device_common as CC
import parity

pytestmark = pytest.mark.gpu

L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
cameras = importlib.import_module("3dgs_hierarchical_training_amd.cameras")
sequence = importlib.import_module("3dgs_hierarchical_training_amd.sequence")
ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
syn = importlib.import_module("3dgs_hierarchical_training_amd.synthetic")

DEV = torch.device("cuda:0")


def _n(t):
    return t.detach().cpu().numpy()


# ---- gsr_camera_from_pose ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CC.INTRINSICS))
@pytest.mark.parametrize("B", [1, 2, 16])
def test_camera_from_pose_against_the_oracle(B, name):
    W, H, fx, fy, cx, cy = CC.INTRINSICS[name]
    poses = CC.batch_poses(B, seed=B)
    ref = CC.camera_oracle(poses, fx, fy, cx, cy, W, H)
    dpose = torch.from_numpy(poses).to(DEV)
    view, proj, campos = cameras.camera_from_pose(dpose, fx, fy, cx, cy, W, H)
    assert tuple(view.shape) == (B, 4, 4) and tuple(proj.shape) == (B, 4, 4) and tuple(campos.shape) == (B, 3)
    assert view.dtype == proj.dtype == campos.dtype == torch.float32 and view.is_contiguous() and proj.is_contiguous() and campos.is_contiguous()
    scale = CC.input_scale(poses)
    got = {"view": _n(view), "proj": _n(proj), "campos": _n(campos)}
    assert np.array_equal(got["view"], ref["view"].astype(np.float32))           # a transposed copy
    for k in ("view", "proj", "campos"):
        CC.assert_bit_equal(got[k], ref[k], f"B={B} {name} {k}")
        CC.assert_exact_zeros_and_ones(got[k], ref[k], f"B={B} {name} {k}")
    # the yardstick, not a bar: how far the host float32 route (Camera's own statements) sits from the same oracle
    far = {"proj": 0.0, "campos": 0.0}
    for b in range(B):
        _, hfull, hcam = CC.host_route(poses[b], fx, fy, cx, cy, W, H)
        far["proj"] = max(far["proj"], CC.ulp_distance(hfull, ref["proj"][b], scale)[0])
        far["campos"] = max(far["campos"], CC.ulp_distance(hcam, ref["campos"][b], scale)[0])
    print(f"   host float32 route, same unit: projection {far['proj']:.2f}, camera centre {far['campos']:.2f}")
    # repeats are bit-identical; a [B,16] layout and the [4,4] form of the first pose are the same numbers
    again = cameras.camera_from_pose(dpose, fx, fy, cx, cy, W, H)
    flat = cameras.camera_from_pose(dpose.reshape(B, 16), fx, fy, cx, cy, W, H)
    one = cameras.camera_from_pose(dpose[0], fx, fy, cx, cy, W, H)
    for a, b_, c, o in zip((view, proj, campos), again, flat, one):
        assert torch.equal(a, b_) and torch.equal(a, c) and torch.equal(a[0], o)
    assert tuple(one[0].shape) == (4, 4) and tuple(one[2].shape) == (3,)
    # the ctypes route equals the op
    lib = L.load()
    v2, p2, c2 = torch.empty_like(view), torch.empty_like(proj), torch.empty_like(campos)
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    L.check(lib.gsr_camera_from_pose(dpose.data_ptr(), B, fx, fy, cx, cy, W, H, CC.ZNEAR, CC.ZFAR, v2.data_ptr(), p2.data_ptr(), c2.data_ptr(),
                                     stream), "gsr_camera_from_pose")
    assert torch.equal(v2, view) and torch.equal(p2, proj) and torch.equal(c2, campos)


def test_camera_from_pose_hand_worked_and_refusals():
    i = CC.HAND_INTR
    view, proj, campos = cameras.camera_from_pose(torch.from_numpy(CC.HAND_POSE).to(DEV), i["fx"], i["fy"], i["cx"], i["cy"], i["W"], i["H"],
                                                  i["znear"], i["zfar"])
    assert np.array_equal(_n(view), CC.HAND_VIEW) and np.array_equal(_n(proj), CC.HAND_FULL) and np.array_equal(_n(campos), CC.HAND_CAMPOS)
    view, proj, campos = cameras.camera_from_pose(torch.eye(4, device=DEV), 42.0, 42.0, 32.0, 24.0, 64, 48)
    assert np.array_equal(_n(view), np.eye(4)) and np.array_equal(_n(campos), np.zeros(3))
    with pytest.raises(RuntimeError):
        cameras.camera_from_pose(torch.zeros(17, 4, 4, device=DEV), 42.0, 42.0, 32.0, 24.0, 64, 48)
    with pytest.raises(RuntimeError):
        cameras.camera_from_pose(torch.zeros(3, 4, device=DEV), 42.0, 42.0, 32.0, 24.0, 64, 48)
    with pytest.raises(ValueError):
        cameras.camera_from_pose(torch.eye(4, device=DEV), 0.0, 42.0, 32.0, 24.0, 64, 48)


# ---- gsr_pose_virtual_view ----------------------------------------------------------------------------------------------------------------
VIEW_PAIRS = {"consecutive frames (0.006 rad)": (CC.sequence_pose(3), CC.sequence_pose(4)),
              "a 2.5 rad turn": (CC.HAND_POSE, CC.make_pose((0.3, 1.0, -0.2), 2.5, (0.5, -1.0, 2.0))),
              "the same pose twice": (CC.sequence_pose(5), CC.sequence_pose(5))}


@pytest.mark.parametrize("name", list(VIEW_PAIRS))
def test_pose_virtual_view_against_the_oracle(name):
    p0, p1 = VIEW_PAIRS[name]
    base = CC.sequence_pose(1)
    d0, d1, db = (torch.from_numpy(p).to(DEV) for p in (p0, p1, base))
    scale = CC.input_scale(p0, p1, base)
    # alpha = 0 and alpha = 1 return pose0 and pose1
    out0 = cameras.virtual_view(d0, d1, 0.0)
    assert np.array_equal(_n(out0), p0)
    CC.assert_one_ulp(_n(cameras.virtual_view(d0, d1, 1.0)), p1.astype(np.float64), scale, f"{name} alpha=1 vs pose1")
    lib = L.load()
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    for alpha in (0.0, 0.25, 0.61803, 1.0):
        ref, ref_rel = CC.virtual_view_oracle(p0, p1, alpha, base)
        out = cameras.virtual_view(d0, d1, alpha)                  # base absent
        out_b, rel = cameras.virtual_view(d0, d1, alpha, base=db)  # base present
        assert tuple(out.shape) == (4, 4) and tuple(rel.shape) == (4, 4) and out.dtype == rel.dtype == torch.float32
        assert torch.equal(out, out_b)
        CC.assert_one_ulp(_n(out), ref, scale, f"{name} alpha={alpha} view")
        CC.assert_one_ulp(_n(rel), ref_rel, scale, f"{name} alpha={alpha} view relative to the base")
        assert np.array_equal(_n(out)[3], [0, 0, 0, 1]) and np.array_equal(_n(rel)[3], [0, 0, 0, 1])
        # repeats are bit-identical; the ctypes route equals the op
        o2, r2 = torch.empty_like(out), torch.empty_like(rel)
        L.check(lib.gsr_pose_virtual_view(d0.data_ptr(), d1.data_ptr(), alpha, db.data_ptr(), o2.data_ptr(), r2.data_ptr(), stream),
                "gsr_pose_virtual_view")
        assert torch.equal(o2, out) and torch.equal(r2, rel)
    with pytest.raises(ValueError):
        cameras.virtual_view(d0, d1, 1.5)


# ---- a render under a device camera ---------------------------------------------------------------------------------------------------------
def test_render_under_a_device_camera_matches_the_host_route():
    W, H, N = 64, 48, 1000
    seq = sequence.FrameSequence(4, N, W, H, DEV, sh_degree=3, seed=3)
    params = ts.GaussianParams(seq.gt_scene, DEV, optimizer="torch")
    pose = seq.w2c[3] @ torch.linalg.inv(seq.w2c[1])             # a chained product, as the segments hold them
    host = seq.settings_for_pose(pose)
    dev = seq.settings_for_pose(pose.to(DEV))
    assert dev.viewmatrix.is_cuda and dev.image_width == host.image_width and dev.tanfovx == host.tanfovx and dev.sh_degree == host.sh_degree
    assert torch.equal(dev.viewmatrix, host.viewmatrix)
    cam = syn.make_camera(W, H)
    ref = CC.camera_oracle(pose.numpy(), cam["fx"], cam["fy"], W / 2.0, H / 2.0, W, H)
    scale = CC.input_scale(pose.numpy())
    CC.assert_bit_equal(_n(dev.projmatrix), ref["proj"], "settings_for_pose(device pose) projection")
    CC.assert_bit_equal(_n(dev.campos), ref["campos"], "settings_for_pose(device pose) camera centre")
    img_h, dep_h, al_h = ts.render_image(params, host, depth_alpha=True)
    img_d, dep_d, al_d = ts.render_image(params, dev, depth_alpha=True)
    d = float((img_h - img_d).abs().max())
    print(f"render under the device camera against the host route's: max |difference| {d:.3e} (bar {parity.FWD_ATOL})")
    assert float(img_h.max()) > 0.2                              # there is an image to compare
    assert d <= parity.FWD_ATOL
    assert float((al_h - al_d).abs().max()) <= parity.FWD_ATOL
    # cameras.settings_from_pose with its default intrinsics (from the template's field of view) is the same camera
    st = cameras.settings_from_pose(host, pose.to(DEV))
    CC.assert_one_ulp(_n(st.projmatrix), ref["proj"], scale, "settings_from_pose(template) projection")
    assert torch.equal(st.campos, dev.campos) and st.bg is host.bg


# ---- the harness ----------------------------------------------------------------------------------------------------------------------------
def _phase1(device_cameras):
    rs = importlib.import_module("3dgs_hierarchical_training_amd.run_segments")
    seg_mod = importlib.import_module("3dgs_hierarchical_training_amd.segments")
    cfg = rs.HTConfig(frames=6, width=64, height=48, gt_gaussians=1500, leaf_gaussians=800, leaf_iters_per_frame=4, phase1_iters_per_frame=4,
                      phase2_iters_per_frame=[2, 2, 2], prune_ratio=0.5, device_cameras=device_cameras)
    seq = sequence.FrameSequence(cfg.frames, cfg.gt_gaussians, cfg.width, cfg.height, DEV, seed=6)
    tr = seg_mod.LocalTransport(2)
    log = []
    runners = [rs.RankRunner(r, 2, tr, seq, cfg, DEV, log=log.append) for r in range(2)]
    for rr in runners:
        rr.train_leaf()
    runners[1].merge_send(0)
    runners[0].merge_recv(0)
    runners[0].train_nonleaf(0)
    rec = [r for r in log if r["phase"] == "nonleaf"]
    assert len(rec) == 1
    return rec[0], runners[0]


def test_phase1_with_device_cameras_draws_the_same_virtual_views():
    host, _ = _phase1(False)
    dev, root = _phase1(True)
    print(f"phase 1: {host['phase1_steps']} steps, {host['virtual_views']} virtual views on the host route, {dev['virtual_views']} with device cameras")
    assert host["phase1_steps"] == dev["phase1_steps"] == 4 * 6
    assert dev["virtual_views"] == host["virtual_views"] > 0
    assert dev["gaussians"] == host["gaussians"]
    assert root.seg.__dict__.get("_device_poses")                # the device route was the one taken
    assert math.isfinite(root.evaluate())


# ---- the frame cache of gsr_autopatch on the stand-in trainer -----------------------------------------------------------------------------------
refstub = importlib.import_module("3dgs_hierarchical_training_amd.refstub")
K_STUB = np.array([[50.0, 0, 30.5], [0, 47.0, 25.0], [0, 0, 1]])


def _frames(n=3, W=64, H=48, seed=0):
    g = np.random.default_rng(seed)
    return [g.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(n)]


@pytest.fixture
def patched(monkeypatch):
    """(gsr_autopatch, the patched GaussianTrainer stand-in counting its original calls, the patched HTGaussianModel stand-in)."""
    import types
    import gsr_autopatch
    monkeypatch.delenv("GSR_AUTOPATCH_FRAMES", raising=False)
    monkeypatch.delenv("GSR_AUTOPATCH_FRAMES_MB", raising=False)

    class GaussianTrainer(refstub.StubTrainer):
        originals = 0

        def load_viewpoint_cam(self, *a, **k):
            type(self).originals += 1
            return super().load_viewpoint_cam(*a, **k)

    class HTGaussianModel(refstub.StubGaussians):
        pass
    tmod, gmod = types.ModuleType("trainer.trainer"), types.ModuleType("scene.gaussian_model_ht")
    tmod.GaussianTrainer, gmod.HTGaussianModel = GaussianTrainer, HTGaussianModel
    gsr_autopatch.apply()
    gsr_autopatch._patch_frames_module(tmod)
    gsr_autopatch._patch_frames_module(gmod)
    yield gsr_autopatch, GaussianTrainer, HTGaussianModel
    gsr_autopatch.remove()


class _FixedPose:
    """Stands for a lietorch pose whose `retr().matrix()` is device work only: a matrix that is already there."""

    def __init__(self, M):
        self.M = M

    def retr(self):
        return self

    def matrix(self):
        return self.M[None]


@pytest.mark.parametrize("data_type", ["custom", "preloaded"])
def test_frame_cache_against_the_unpatched_loader(patched, data_type, monkeypatch):
    A, T, _ = patched
    tr = T(_frames(), K_STUB, data_type=data_type, device=DEV)
    ref = refstub.StubTrainer(_frames(), K_STUB, data_type=data_type, device=DEV)       # the unpatched route
    assert T.load_viewpoint_cam is A.load_viewpoint_cam_cached
    for f in range(3):
        first = tr.load_viewpoint_cam(f)
        second = tr.load_viewpoint_cam(f)
        want = ref.load_viewpoint_cam(f)
        assert T.originals == f + 1 and second is not first and type(second) is refstub.StubCameraFull
        # images: the original's own plane, bit for bit the unpatched call's
        assert second.original_image is first.original_image and second.original_image.is_cuda
        assert torch.equal(second.original_image, want.original_image)
        # fields
        for k in ("uid", "colmap_id", "FoVx", "FoVy", "image_name", "image_width", "image_height", "znear", "zfar", "focal_x", "focal_y"):
            assert getattr(second, k) == getattr(want, k), k
        assert np.array_equal(second.intrinsics, want.intrinsics) and torch.equal(second.projection_matrix, want.projection_matrix)
        # identity cameras are bit-equal
        for k in ("world_view_transform", "full_proj_transform", "camera_center"):
            assert torch.equal(getattr(second, k), getattr(want, k)), k
    # posed cameras: the kernel's, within the bar of the oracle; the unpatched route's own distance beside it
    K32 = K_STUB.astype(np.float32)
    fx, fy, cx, cy = float(K32[0, 0]), float(K32[1, 1]), float(K32[0, 2]), float(K32[1, 2])
    n = T.originals
    for f, p in ((0, CC.sequence_pose(7)), (1, CC.batch_poses(2)[1]), (2, CC.make_pose((1.0, -0.4, 0.3), 0.8, (0.3, -1.2, 2.0)))):
        oracle = CC.camera_oracle(p, fx, fy, cx, cy, 64, 48)
        scale = CC.input_scale(p)
        for label, pose in (("host pose", torch.from_numpy(p)), ("DevicePose", torch.from_numpy(p).to(DEV).as_subclass(A.DevicePose).detach().cpu())):
            cam = tr.load_viewpoint_cam(f, pose=pose)
            assert np.array_equal(_n(cam.world_view_transform), oracle["view"].astype(np.float32))
            CC.assert_bit_equal(_n(cam.full_proj_transform), oracle["proj"], f"{data_type} frame {f} {label} projection")
            CC.assert_bit_equal(_n(cam.camera_center), oracle["campos"], f"{data_type} frame {f} {label} camera centre")
            assert cam.original_image is tr._gsr_frames["entries"][f]["image"]
        un = ref.load_viewpoint_cam(f, pose=torch.from_numpy(p))
        print(f"   unpatched loader, same unit: projection {CC.ulp_distance(_n(un.full_proj_transform), oracle['proj'], scale)[0]:.2f}, "
              f"camera centre {CC.ulp_distance(_n(un.camera_center), oracle['campos'], scale)[0]:.2f}")
    assert T.originals == n                                        # not one original call for a cached frame
    # an in-place write into the cached plane makes the next call rebuild it
    plane = tr.load_viewpoint_cam(1).original_image
    plane.mul_(0.5)
    again = tr.load_viewpoint_cam(1)
    assert T.originals == n + 1 and again.original_image is not plane and torch.equal(again.original_image, ref.load_viewpoint_cam(1).original_image)
    assert tr.load_viewpoint_cam(1).original_image is again.original_image and T.originals == n + 1
    # a frame over a 1 MB budget is not cached
    monkeypatch.setenv("GSR_AUTOPATCH_FRAMES_MB", "1")
    big = T(_frames(1, W=320, H=300), K_STUB, data_type=data_type, device=DEV)
    n = T.originals
    a, b = big.load_viewpoint_cam(0), big.load_viewpoint_cam(0)
    assert T.originals == n + 2 and a.original_image is not b.original_image and not big._gsr_frames["entries"]


def test_device_pose_with_a_cpu_matrix_gives_the_unpatched_result(patched):
    A, _, G = patched
    M = torch.from_numpy(CC.sequence_pose(4)).to(DEV)
    g = G.__new__(G)
    g.P, g.rotate_xyz, g.seq_idx = [_FixedPose(M)], False, 0
    pose = g.get_RT(0)
    assert type(pose) is A.DevicePose and pose.is_cuda and pose.detach().cpu() is not None and type(pose.detach().cpu()) is A.DevicePose
    rel = torch.from_numpy(CC.sequence_pose(1))                  # `pose_dict[...].cpu() @ pose`
    out = rel @ pose.detach().cpu()
    assert type(out) is torch.Tensor and out.device.type == "cpu" and torch.equal(out, rel @ M.cpu())
    assert np.array_equal(pose.detach().cpu()[:3, :3].numpy(), M.cpu()[:3, :3].numpy())
    both = M @ pose                                              # device with device: the plain device tensor
    assert type(both) is torch.Tensor and both.is_cuda and torch.equal(both, M @ M)


@pytest.mark.filterwarnings("ignore:Synchronization debug mode")
def test_a_pose_product_reaches_the_original_loader_as_a_host_pose(patched, monkeypatch):
    """ht3dgs_trainer.py:561-562 as stage A leaves it: `pose_dict[...]` holds a `get_RT().detach()` result (a DevicePose under the patch),
    the loader gets `pose_dict[...].detach().cpu() @ pose_train` with load_depth and load_vfi.  On calls the patched loader hands to the
    original -- a frame it knows nothing of yet, a frame over the budget -- the original's `pose[:3, :3].numpy()` needs a host pose; so does
    a plain device tensor handed in directly."""
    A, T, G = patched
    M1, M4 = torch.from_numpy(CC.sequence_pose(1)).to(DEV), torch.from_numpy(CC.sequence_pose(4)).to(DEV)
    g = G.__new__(G)
    g.P, g.rotate_xyz, g.seq_idx = [_FixedPose(M1), _FixedPose(M4)], False, 0
    rel = g.get_RT(0).detach()                                    # what stage A stored
    want = (M1 @ M4).cpu().numpy()
    product = lambda: rel.detach().cpu() @ g.get_RT(1).detach().cpu()
    assert type(product()) is A.DevicePose and product().is_cuda
    tr = T(_frames(), K_STUB, data_type="preloaded", device=DEV)
    cam = tr.load_viewpoint_cam(0, pose=product(), load_depth=True, load_vfi=True)             # uncached: depth and vfi not there yet
    assert T.originals == 1 and isinstance(cam.R, np.ndarray) and np.array_equal(cam.R, want[:3, :3]) and np.array_equal(cam.T, want[:3, 3])
    cached = tr.load_viewpoint_cam(0, pose=product(), load_depth=True, load_vfi=True)           # everything there now: the kernel
    assert T.originals == 1 and cached.vfi is tr.vfi["0_to_1"] and torch.equal(cached.world_view_transform, cam.world_view_transform)
    monkeypatch.setenv("GSR_AUTOPATCH_FRAMES_MB", "0.01")                                       # every frame is over the budget
    tr2 = T(_frames(), K_STUB, data_type="preloaded", device=DEV)
    n = T.originals
    for pose in (product(), product(), M1 @ M4):                                                # the last: a PLAIN device tensor
        cam = tr2.load_viewpoint_cam(1, pose=pose, load_depth=True, load_vfi=True)
        assert isinstance(cam.R, np.ndarray) and np.array_equal(cam.R, want[:3, :3])
    assert T.originals == n + 3 and not tr2._gsr_frames["entries"]


def test_twenty_iterations_on_cached_frames_never_wait_for_the_device(patched):
    A, T, G = patched
    W, H, N = 64, 48, 1500
    sc = syn.make_scene(N, W, H, sh_degree=3, seed=2)
    A_params = ts.GaussianParams(sc, DEV, optimizer="torch")     # (gsr_autopatch is applied: torch.optim.Adam hands out the FusedAdam)
    r = refstub.StubRender(A_params)
    g = r.gaussians = G(A_params)
    g.P = [_FixedPose(torch.from_numpy(CC.sequence_pose(f)).to(DEV)) for f in range(3)]
    cam0 = syn.make_camera(W, H)
    K = np.array([[cam0["fx"], 0, W / 2.0], [0, cam0["fy"], H / 2.0], [0, 0, 1]])
    tr = T(_frames(), K, data_type="preloaded", device=DEV)

    class _L:
        class cfg:
            lambda_dssim, lambda_depth = 0.2, 0.0

    def iteration(f):
        cam = tr.load_viewpoint_cam(f, pose=g.get_RT(f).detach().cpu())
        pkg = A.render_fused(r, cam)
        A.loss_forward(_L(), pkg["image"], cam.original_image)["loss"].backward()
        g.optimizer.step()
        g.optimizer.zero_grad(set_to_none=True)
        return cam
    for f in range(3):                                           # first calls: the original loader, once per frame
        iteration(f)
    n = T.originals
    before = A_params._xyz.detach().clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for k in range(20):
            cam = iteration(k % 3)
        with pytest.raises(RuntimeError):                        # the mode does see the wait the unpatched statement has
            refstub.StubGaussians.get_RT(g, 0).detach().cpu()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert T.originals == n and type(cam.R) is A.DevicePose
    assert not torch.equal(A_params._xyz.detach(), before)       # the model trained
