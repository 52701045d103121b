"""Stand-ins shaped like the reference's live objects, for the tests and the bench leg of `gsr_autopatch.render_fused`.

The reference's `CF3DGS_Render` / `HTGaussianModel` / `Camera` (/root/reference/scene/gaussian_model_ht.py:47-90,726-773,
/root/reference/scene/cameras.py:17-98) import lietorch, plyfile and the dataset stack, none of which exists in this image or on the
GPU box; these classes carry exactly the ATTRIBUTES the render wrapper and the train step read from them -- no behaviour of their own
beyond the reference's one-line activations -- so that the patched method can be driven the way the unmodified trainer drives it
(/root/reference/trainer/ht3dgs_trainer.py:102-166).
"""
import math

import torch


class StubCamera:
    """FoVx / FoVy / image size / the three matrices, as `Camera` keeps them (cameras.py:60-98); built from a scene dict of
    synthetic.make_scene or from raw matrices."""

    def __init__(self, W, H, tanfovx, tanfovy, viewmatrix, projmatrix, campos, uid=0, original_image=None):
        self.image_width, self.image_height = int(W), int(H)
        self.FoVx, self.FoVy = 2.0 * math.atan(float(tanfovx)), 2.0 * math.atan(float(tanfovy))
        self.world_view_transform, self.full_proj_transform, self.camera_center = viewmatrix, projmatrix, campos
        self.uid = uid
        self.original_image = original_image

    @classmethod
    def from_scene(cls, scene, device, original_image=None, uid=0):
        return cls(scene["image_width"], scene["image_height"], scene["tanfovx"], scene["tanfovy"], scene["viewmatrix"].to(device),
                   scene["projmatrix"].to(device), scene["campos"].to(device), uid, original_image)


class SE3:
    """Stand-in for `lietorch.SE3` as far as the reference's model file uses it (/root/reference/scene/gaussian_model_ht.py:135-166,
    346-386): `SE3(pose7)` with `.data` = [..., 7] (tx ty tz qx qy qz qw), `tangent_shape`, `retr(a)` = Exp(a) * self,
    `act(points)`, `matrix()`, `inv()`, `*`.  lietorch is a third-party CUDA extension that exists neither in this image nor on the
    GPU box; this class states its PUBLIC behaviour with plain torch (pose.py's closed forms), so that the trainer's pose
    statements can be driven -- and timed as a torch chain -- without it.  An element that came out of an operation carries its
    matrix only (`.data` is then None): enough for `act` / `matrix` / `inv` / `*`, which is all the reference asks of one."""

    def __init__(self, data=None, _matrix=None):
        self.data = data
        self._matrix = _matrix

    @property
    def tangent_shape(self):
        return tuple(self.data.shape[:-1]) + (6,)

    def _M(self):
        if self._matrix is None:
            from . import pose
            return pose.pose7_to_matrix(self.data.reshape(7))
        return self._matrix

    def retr(self, a):
        from . import pose
        return SE3(_matrix=pose.se3_exp(a.reshape(6)) @ self._M())

    def matrix(self):
        return self._M()[None]

    def inv(self):
        M = self._M()
        Rt = M[:3, :3].t()
        top = torch.cat((Rt, -(Rt @ M[:3, 3:4])), dim=1)
        return SE3(_matrix=torch.cat((top, M[3:4]), dim=0))

    def act(self, x):
        M = self._M()
        return x @ M[:3, :3].t() + M[:3, 3]

    def __mul__(self, other):
        return SE3(_matrix=self._M() @ other._M())


class LieGroupParameter(torch.Tensor):
    """Stand-in for `lietorch.LieGroupParameter`: a float32 tensor SUBCLASS of the group's tangent shape, zeros at construction,
    `__torch_function__` disabled, the group element in `.group`; `retr()` = Exp(self) * group (lietorch/groups.py, public API).
    A stock torch.optim.Adam updates the six tangent numbers in place (addcdiv_), the group element stays."""
    __torch_function__ = torch._C._disabled_torch_function_impl

    def __new__(cls, group, requires_grad=True):
        data = torch.zeros(group.tangent_shape, device=group.data.device, dtype=group.data.dtype, requires_grad=True)
        return torch.Tensor._make_subclass(cls, data, requires_grad)

    def __init__(self, group, requires_grad=True):
        self.group = group

    def retr(self):
        return self.group.retr(self)

    def inv(self):
        return self.retr().inv()


def pose7_identity(device):
    return torch.tensor([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]], device=device)


class StubGaussians:
    """The attributes of `HTGaussianModel` the render wrapper reads (gaussian_model_ht.py:67-90,128-188), on top of an object that
    holds the six raw tensors and the optimizer (train_step.GaussianParams)."""

    def __init__(self, params):
        self._p = params
        self.rotate_xyz = False
        self.rotate_seq = False
        self.seq_idx = 0
        self.P = None
        N, dev = params._xyz.shape[0], params._xyz.device
        self.max_radii2D = torch.zeros(N, device=dev)
        self.xyz_gradient_accum = torch.zeros(N, 1, device=dev)
        self.denom = torch.zeros(N, 1, device=dev)

    _xyz = property(lambda s: s._p._xyz)
    _features_dc = property(lambda s: s._p._features_dc)
    _features_rest = property(lambda s: s._p._features_rest)
    _opacity = property(lambda s: s._p._opacity)
    _scaling = property(lambda s: s._p._scaling)
    _rotation = property(lambda s: s._p._rotation)
    active_sh_degree = property(lambda s: s._p.active_sh_degree)
    max_sh_degree = property(lambda s: s._p.max_sh_degree)
    optimizer = property(lambda s: s._p.optimizer)

    @property
    def get_xyz(self):                       # gaussian_model_ht.py:135-148
        if self.rotate_xyz:
            return self.P[0].retr().act(self._xyz.clone())
        if self.rotate_seq:
            return self.P[self.seq_idx].retr().act(self._xyz.clone())
        return self._xyz

    def get_RT(self, idx=None):              # gaussian_model_ht.py:150-166
        if getattr(self, "P", None) is None:
            return torch.eye(4, device=self._xyz.device)
        p = self.P[0] if self.rotate_xyz else self.P[self.seq_idx if idx is None else idx]
        return p.retr().matrix().squeeze()

    get_scaling = property(lambda s: torch.exp(s._scaling))
    get_rotation = property(lambda s: torch.nn.functional.normalize(s._rotation))
    get_opacity = property(lambda s: torch.sigmoid(s._opacity))
    get_features = property(lambda s: torch.cat((s._features_dc, s._features_rest), dim=1))

    def add_densification_stats(self, viewspace_point_tensor, update_filter):      # gaussian_model_ht.py:718-721, verbatim semantics
        self.xyz_gradient_accum[update_filter] += torch.norm(viewspace_point_tensor.grad[update_filter, :2], dim=-1, keepdim=True)
        self.denom[update_filter] += 1


class StubRender:
    """`CF3DGS_Render` as far as `render` reads it: `.gaussians`, `.bg_color` (gaussian_model_ht.py:726-741).  `render` is the
    ORIGINAL wrapper's sequence of calls restated (activated tensors + cat -> GaussianRasterizer -> clamp), i.e. the unpatched route
    against which the patched one is compared."""

    def __init__(self, params, bg=(0.0, 0.0, 0.0)):
        self.gaussians = StubGaussians(params)
        self.bg_color = torch.tensor(bg, dtype=torch.float32, device=params._xyz.device)

    def render(self, viewpoint_camera, scaling_modifier=1.0, invert_bg_color=False, override_color=None,
               compute_cov3D_python=False, convert_SHs_python=False):
        from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer
        g = self.gaussians
        xyz = g.get_xyz
        screenspace_points = torch.zeros_like(xyz, requires_grad=True) + 0       # :800-808
        screenspace_points.retain_grad()
        rs = GaussianRasterizationSettings(
            image_height=int(viewpoint_camera.image_height), image_width=int(viewpoint_camera.image_width),
            tanfovx=math.tan(viewpoint_camera.FoVx * 0.5), tanfovy=math.tan(viewpoint_camera.FoVy * 0.5),
            bg=self.bg_color if not invert_bg_color else 1 - self.bg_color, scale_modifier=scaling_modifier,
            viewmatrix=viewpoint_camera.world_view_transform, projmatrix=viewpoint_camera.full_proj_transform,
            sh_degree=g.active_sh_degree, campos=viewpoint_camera.camera_center, prefiltered=False, debug=False)
        out = GaussianRasterizer(raster_settings=rs)(
            means3D=xyz, means2D=screenspace_points, shs=None if override_color is not None else g.get_features,
            colors_precomp=override_color, opacities=g.get_opacity, scales=g.get_scaling, rotations=g.get_rotation, cov3D_precomp=None)
        image, radii, depth, alpha = out
        return {"image": image.clamp(0, 1), "depth": depth, "alpha": alpha, "viewspace_points": screenspace_points,
                "visibility_filter": radii > 0, "radii": radii}


class StubLoss:
    """`trainer.losses.Loss` as far as `gsr_autopatch.loss_forward` and the trainer read it: `.cfg` (lambda_dssim, lambda_depth),
    `.depth_loss_type`, `get_depth_loss` and `forward` (losses.py:86-136), restated with the reference's sequence of torch statements --
    its three host synchronisations included (`det.nonzero()` in the 2x2 solve, `if divisor == 0` in both reductions) -- i.e. the
    unpatched route against which the fused depth term is compared and timed."""

    def __init__(self, depth_loss_type="invariant", lambda_dssim=0.2, lambda_depth=0.0):
        import types
        self.depth_loss_type = depth_loss_type
        self.cfg = types.SimpleNamespace(lambda_dssim=lambda_dssim, lambda_depth=lambda_depth, depth_loss_type=depth_loss_type)

    @staticmethod
    def _batch_mean(total, divisor):                                   # reduction_batch_based
        divisor = torch.sum(divisor)
        if divisor == 0:
            return 0
        return torch.sum(total) / divisor

    def _scale_shift_invariant(self, pred, target, mask, alpha=0.5):   # [1,H,W] each
        a00, a01, a11 = torch.sum(mask * pred * pred, (1, 2)), torch.sum(mask * pred, (1, 2)), torch.sum(mask, (1, 2))
        b0, b1 = torch.sum(mask * pred * target, (1, 2)), torch.sum(mask * target, (1, 2))
        scale, shift = torch.zeros_like(b0), torch.zeros_like(b1)
        det = a00 * a11 - a01 * a01
        ok = det.nonzero()
        scale[ok] = (a11[ok] * b0[ok] - a01[ok] * b1[ok]) / det[ok]
        shift[ok] = (-a01[ok] * b0[ok] + a00[ok] * b1[ok]) / det[ok]
        fit = scale.view(-1, 1, 1) * pred + shift.view(-1, 1, 1)
        M = torch.sum(mask, (1, 2))
        res = fit - target
        total = self._batch_mean(torch.sum(mask * res * res, (1, 2)), 2 * M)
        diff = mask * res
        gx = mask[:, :, 1:] * mask[:, :, :-1] * torch.abs(diff[:, :, 1:] - diff[:, :, :-1])
        gy = mask[:, 1:, :] * mask[:, :-1, :] * torch.abs(diff[:, 1:, :] - diff[:, :-1, :])
        return total + alpha * self._batch_mean(torch.sum(gx, (1, 2)) + torch.sum(gy, (1, 2)), M)

    def get_depth_loss(self, depth_pred, depth_gt):                    # [H,W] each
        if self.depth_loss_type == "l1":
            return torch.abs(depth_pred - depth_gt).sum() / float(depth_pred.shape[0] * depth_pred.shape[1])
        mask = (depth_gt > 0.02).float()
        return self._scale_shift_invariant(depth_pred[None], depth_gt[None], mask[None])

    def forward(self, rgb_pred, rgb_gt, depth_pred=None, depth_gt=None, rgb_loss_type='l1', **kwargs):
        from .train_step import ssim
        lambda_dssim, lambda_depth = self.cfg.lambda_dssim, self.cfg.lambda_depth
        rgb_gt = rgb_gt.to(rgb_pred.device)
        rgb_full_loss = (1 - lambda_dssim) * torch.abs(rgb_pred - rgb_gt).mean()
        dssim_loss = 1 - ssim(rgb_pred, rgb_gt)
        if lambda_depth != 0.0 and depth_pred is not None and depth_gt is not None:
            depth_gt = depth_gt.to(rgb_pred.device)
            depth_pred[depth_pred < 0.02] = 0.02
            depth_pred[depth_pred > 20.0] = 20.0
            depth_loss = self.get_depth_loss(depth_pred.squeeze(), depth_gt.squeeze())
        else:
            depth_loss = torch.zeros((), device=rgb_pred.device)
        loss = rgb_full_loss + lambda_dssim * dssim_loss + lambda_depth * depth_loss
        return {'loss': loss, 'loss_rgb': rgb_full_loss, 'loss_dssim': dssim_loss, 'loss_depth': depth_loss}

    __call__ = forward


# ---- the frame loader: `GaussianTrainer.load_viewpoint_cam` and the `Camera` it builds per call --------------------------------------------
# Written from what the reference's loader and camera DO per call (/root/reference/trainer/trainer.py:989-1142,
# /root/reference/scene/cameras.py:17-101), with this project's helpers and names: the attribute names of the camera are its interface (the
# trainer, the patched render and the frame cache read them), everything else is this file's own.
def fov_of_focal(focal, pixels):
    """Full opening angle of `pixels` seen through a pinhole of focal length `focal` (pixels)."""
    return 2.0 * math.atan(0.5 * pixels / focal)


def frame_to_float_image(frame):
    """A decoded frame, numpy uint8 [H,W,3], as the float32 [3,H,W] image the trainer works on: scaled to [0,1] in float64 on the host
    first, narrowed afterwards -- the order (and the cost: a float64 plane per call) of the reference's conversion."""
    import numpy as np
    scaled = np.true_divide(frame, 255.0)                       # float64
    return torch.from_numpy(scaled).movedim(-1, 0).to(torch.float32)


def float_image_to_frame(image):
    """The way back, as the pre-loaded branch takes it on every call: the device image to the host, to 0..255, truncated to uint8."""
    import numpy as np
    return (image.movedim(0, -1).cpu().numpy() * 255).astype(np.uint8)


def rigid_view_matrix(R, t):
    """World-to-camera 4x4 of (R, t) after the round trip through its inverse that the reference's view-matrix helper makes (with no
    recentring the two inversions cancel up to rounding, which is kept): numpy blocks -> float64 work, a float32 array; tensor blocks -> the
    tensor's own dtype and device."""
    import numpy as np
    if torch.is_tensor(R):
        M = torch.eye(4, dtype=R.dtype, device=R.device)
        M[:3, :3] = R
        M[:3, 3] = t
        return torch.linalg.inv(torch.linalg.inv(M))
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = t
    return np.linalg.inv(np.linalg.inv(M)).astype(np.float32)


def pinhole_projection_T(K32, W, H, near, far):
    """The transposed projection of a pinhole with intrinsics K32 (numpy float32 3x3, pixels) over a W x H frame and the depth range
    [near, far], as a host float32 tensor: x and y scaled by twice the focal length over the frame size and shifted by the principal
    point's offset from the centre, depth mapped to far / (far - near) * (z - near), w = z.  Entries are formed in float32, like the
    reference's."""
    import numpy as np
    P = np.zeros((4, 4), dtype=np.float32)
    two = np.float32(2.0)
    P[0, 0], P[1, 1] = two * K32[0, 0] / W, two * K32[1, 1] / H
    P[0, 2], P[1, 2] = -(W - two * K32[0, 2]) / W, -(H - two * K32[1, 2]) / H
    depth_gain = far / (far - near)
    P[2, 2], P[2, 3] = depth_gain, -near * depth_gain
    P[3, 2] = 1.0
    return torch.from_numpy(np.ascontiguousarray(P.T))


class StubCameraFull(torch.nn.Module):
    """Stand-in for the camera `load_viewpoint_cam` builds on every call (the reference's `Camera` in its co3d form): the attributes that
    class exposes, filled by the same amount of work -- the image clamped on the host, uploaded and multiplied by a plane of ones on the
    device; the view matrix and the projection built on the host and uploaded; one batched 4x4 product and one 4x4 inverse on the device,
    whose row read waits for it.  This is the unpatched route the frame cache of `gsr_autopatch` is compared with and timed against."""
    NEAR, FAR = 0.01, 100.0

    def __init__(self, uid, R, T, fov_xy, image, image_name, intrinsics, device="cuda", vfi=None, alpha_mask=None):
        import numpy as np
        super().__init__()
        self.uid = self.colmap_id = uid
        self.image_name, self.vfi = image_name, vfi
        self.R, self.T = R, T
        self.FoVx, self.FoVy = fov_xy
        self.intrinsics = np.asarray(intrinsics).astype(np.float32)
        self.depth = self.optical_flow = self.mask_for_relative_pose = self.mask = None
        self.znear, self.zfar, self.scale = self.NEAR, self.FAR, 1.0
        self.trans = torch.zeros(3, dtype=R.dtype, device=R.device) if torch.is_tensor(R) else np.zeros(3)
        self.data_device = torch.device(device)
        self._take_image(image, alpha_mask)
        self._build_matrices()
        self.focal_x = 0.5 * self.image_width / math.tan(0.5 * self.FoVx)
        self.focal_y = 0.5 * self.image_height / math.tan(0.5 * self.FoVy)

    def _take_image(self, image, alpha_mask):
        plane = torch.clamp(image, min=0.0, max=1.0).to(device=self.data_device)
        self.image_height, self.image_width = int(plane.shape[-2]), int(plane.shape[-1])
        weight = torch.ones((1, self.image_height, self.image_width), device=self.data_device) if alpha_mask is None \
            else alpha_mask.to(device=self.data_device)
        plane.mul_(weight)
        self.original_image, self.gt_alpha_mask = plane, alpha_mask

    def _build_matrices(self):
        view = rigid_view_matrix(self.R, self.T)
        view = view if torch.is_tensor(view) else torch.from_numpy(view).to(device=self.data_device)
        self.world_view_transform = view.t()
        self.projection_matrix = pinhole_projection_T(self.intrinsics, self.image_width, self.image_height, self.znear, self.zfar).to(
            device=self.world_view_transform.device)
        self.full_proj_transform = torch.bmm(self.world_view_transform[None], self.projection_matrix[None])[0]
        self.camera_center = torch.linalg.inv(self.world_view_transform)[3, :3]


class StubTrainer:
    """Stand-in for the reference's `GaussianTrainer` as far as its frame loader goes, on frames held as numpy uint8 arrays [H,W,3] (what a
    decoded image file is; the decode itself and the halving of frames above 1000 pixels have no counterpart here).  data_type 'custom':
    every call converts the frame to a float image again.  data_type 'preloaded': `data[idx]` is a camera that already holds the float image
    on the device, and every call copies that image back to the host (for the depth network) and builds a fresh camera around it.
    `predict_depth` / `predict_vfi` stand for the two networks: a cheap deterministic function each, counted.  Side effects as in the
    reference: `mono_depth[idx]` and `vfi["i_to_i+1"]` are filled the first time they are asked for."""

    def __init__(self, frames, intrinsic, data_type="custom", device="cuda", near=0.01):
        import numpy as np
        if data_type not in ("custom", "preloaded"):
            raise ValueError("data_type: 'custom' or 'preloaded'")
        self.data_type, self.device, self.near = data_type, torch.device(device), near
        self.intrinsic = np.asarray(intrinsic, dtype=np.float64)
        self.mono_depth, self.vfi, self.rgb_images = {}, {}, {}
        self.depth_calls = self.vfi_calls = 0
        frames = [np.ascontiguousarray(f, dtype=np.uint8) for f in frames]
        self.data = frames if data_type == "custom" else [self._camera(k, None, frame_to_float_image(f)) for k, f in enumerate(frames)]

    # -- the two networks ------------------------------------------------------------------------------------------------------------------
    def predict_depth(self, frame):
        self.depth_calls += 1
        return torch.from_numpy(frame.astype("float32").mean(axis=2) / 255.0 + 1.0)

    def predict_vfi(self, image1, image2):
        self.vfi_calls += 1
        return (0.5 * (image1 + image2)).squeeze(0)

    # -- pieces of a call ------------------------------------------------------------------------------------------------------------------
    def _camera(self, idx, pose, image, trainable=False, vfi=None, like=None):
        import numpy as np
        if pose is None:
            R, t = np.eye(3), np.zeros(3)
        elif trainable:
            R, t = pose[:3, :3], pose[:3, 3]                     # tensor blocks: the camera stays differentiable in the pose
        else:
            host = pose.numpy()                                  # a host pose is expected here, as in the reference: a device tensor raises
            R, t = host[:3, :3], host[:3, 3]
        if like is None:
            h, w = image.shape[-2:]
            fov, name, K = (fov_of_focal(self.intrinsic[0, 0], w), fov_of_focal(self.intrinsic[1, 1], h)), f"frame_{idx:05d}", self.intrinsic
        else:
            fov, name, K = (like.FoVx, like.FoVy), like.image_name, like.intrinsics
        return StubCameraFull(idx, R, t, fov, image, name, K, device=self.device, vfi=vfi)

    def _want_depth(self, idx, frame, floor=None):
        if idx in self.mono_depth:
            return
        depth = self.predict_depth(frame)
        if floor is not None:
            depth.clamp_(min=floor)
        self.mono_depth[idx] = depth.to(self.device)

    def _interpolated(self, idx, image):
        """The in-between image of frames idx and idx + 1, predicted once and kept; a plane of ones behind the last frame."""
        if idx + 1 >= len(self.data):
            self.vfi[idx] = torch.ones((3,) + tuple(image.shape[-2:]), device=self.device)
            return self.vfi[idx]
        key = f"{idx}_to_{idx + 1}"
        if key not in self.vfi:
            pair = [im.to(self.device)[None] for im in (image, self.data[idx + 1].original_image)]
            self.vfi[key] = self.predict_vfi(*pair).to(self.device)
        return self.vfi[key]

    # -- the loader ------------------------------------------------------------------------------------------------------------------------
    def load_viewpoint_cam(self, idx, pose=None, load_depth=False, pose_to_train=False, load_vfi=False):
        if self.data_type == "custom":
            frame = self.data[idx]
            cam = self._camera(idx, pose, frame_to_float_image(frame))            # the conversion, every call
            if load_depth:
                self._want_depth(idx, frame)
            return cam
        held = self.data[idx]
        frame = float_image_to_frame(held.original_image)                            # the float image back to the host, every call
        vfi = self._interpolated(idx, held.original_image) if load_vfi else None
        cam = self._camera(idx, pose, held.original_image, trainable=pose_to_train is True, vfi=vfi, like=held)
        if load_depth:
            self._want_depth(idx, frame, floor=self.near)
        return cam


# ---- the model's surgery: densify / prune as the unmodified trainer runs it -----------------------------------------------------------------
# Written from what `HTGaussianModel`'s surgery methods DO (/root/reference/scene/gaussian_model_ht.py:468-474, :532-716), in this file's own
# words: the method and attribute names are the interface (the trainer calls them, `gsr_autopatch` replaces two of them and reads the rest),
# the statements are this file's.  Tensors are created on the model's own device, so the same class runs on the CPU for the dispatch tests.
def build_rotation(q):
    """Rotation matrices [n,3,3] of raw quaternions [n,4] in (w,x,y,z) order; each is divided by its length first (the length formed as the
    root of the four squares added left to right, the arithmetic of the reference's helper of this name in utils/general_utils.py)."""
    length = torch.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    w, x, y, z = (q / length[:, None]).unbind(1)
    rows = (1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y))
    return torch.stack(rows, dim=1).reshape(-1, 3, 3)


def logit(p):
    return torch.log(p / (1 - p))


SURGERY_GROUPS = (("xyz", "_xyz", 0.00016), ("f_dc", "_features_dc", 0.0025), ("f_rest", "_features_rest", 0.0025 / 20.0),
                  ("opacity", "_opacity", 0.05), ("scaling", "_scaling", 0.005), ("rotation", "_rotation", 0.001))


class StubSurgeryModel:
    """Stand-in for `HTGaussianModel` as far as densification goes: the six raw tensors as `nn.Parameter` leaves, the optimizer over the six
    named groups (optimizer="adam": the stock torch.optim.Adam, "fused": this library's FusedAdam, both `lr=0.0, eps=1e-15` with per-group
    rates), the three statistics tensors, `percent_dense`, the activations, and the surgery methods with the reference's sequence of torch
    operations: boolean indexing and `torch.cat` tensor by tensor, the optimizer's state re-keyed group by group, fresh parameters every
    time.  It is the unpatched arm `gsr_autopatch`'s `densify_and_prune` / `prune_points` are compared with and timed against, and also
    carries the attributes the patched render reads (`active_sh_degree`, the pose switches, `get_xyz`).

    One deliberate difference: where the reference writes `.squeeze()` on an [N,1] tensor this class squeezes the last axis only, so that
    a model of ONE row keeps a mask of shape [1] (the reference's 0-d mask would index a new axis into every tensor)."""

    def __init__(self, raw, optimizer="adam", percent_dense=0.01, active_sh_degree=None):
        self.scaling_activation, self.scaling_inverse_activation = torch.exp, torch.log
        self.opacity_activation, self.inverse_opacity_activation = torch.sigmoid, logit
        self.rotation_activation = torch.nn.functional.normalize
        for _, attr, _ in SURGERY_GROUPS:
            setattr(self, attr, torch.nn.Parameter(raw[attr].detach().clone().contiguous().requires_grad_(True)))
        n, dev = self._xyz.shape[0], self._xyz.device
        self.max_sh_degree = int(round(math.sqrt(self._features_rest.shape[1] + 1))) - 1
        self.active_sh_degree = self.max_sh_degree if active_sh_degree is None else int(active_sh_degree)
        self.percent_dense = percent_dense
        self.empty_cache = True               # the reference ends densify_and_prune / prune with torch.cuda.empty_cache(); False: a timing arm without it
        self.rotate_xyz = self.rotate_seq = False
        self.seq_idx, self.P = 0, None
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        self.max_radii2D = torch.zeros((n,), device=dev)
        groups = [{"params": [getattr(self, attr)], "lr": lr, "name": name} for name, attr, lr in SURGERY_GROUPS]
        if optimizer == "fused":
            from .optim import FusedAdam
            self.optimizer = FusedAdam(groups, lr=0.0, eps=1e-15)
        elif optimizer == "adam":
            from torch.optim.adam import Adam          # (the stock class, also while gsr_autopatch has redirected `torch.optim.Adam`)
            self.optimizer = Adam(groups, lr=0.0, eps=1e-15)
        else:
            raise ValueError("StubSurgeryModel: optimizer is 'adam' or 'fused'")

    get_xyz = property(lambda s: s._xyz)
    get_scaling = property(lambda s: s.scaling_activation(s._scaling))
    get_rotation = property(lambda s: s.rotation_activation(s._rotation))
    get_opacity = property(lambda s: s.opacity_activation(s._opacity))
    get_features = property(lambda s: torch.cat((s._features_dc, s._features_rest), dim=1))

    def get_RT(self, idx=None):
        return torch.eye(4, device=self._xyz.device)

    def add_densification_stats(self, viewspace_point_tensor, update_filter):
        self.xyz_gradient_accum[update_filter] += torch.norm(viewspace_point_tensor.grad[update_filter, :2], dim=-1, keepdim=True)
        self.denom[update_filter] += 1

    # -- the optimizer's side of every resize: one group at a time ------------------------------------------------------------------------
    def _regroup(self, group, new_tensor, moments):
        """`new_tensor` becomes the group's parameter (a fresh `nn.Parameter`); a group that has optimizer state keeps the state's dict,
        re-keyed, with both moments passed through `moments`; a group without state stays without."""
        old = group["params"][0]
        st = self.optimizer.state.get(old, None)
        if st is not None:
            st["exp_avg"], st["exp_avg_sq"] = moments(st["exp_avg"]), moments(st["exp_avg_sq"])
            del self.optimizer.state[old]
        group["params"][0] = torch.nn.Parameter(new_tensor.requires_grad_(True))
        if st is not None:
            self.optimizer.state[group["params"][0]] = st
        return group["params"][0]

    def _adopt(self, by_name):
        for name, attr, _ in SURGERY_GROUPS:
            if name in by_name:
                setattr(self, attr, by_name[name])

    def replace_tensor_to_optimizer(self, tensor, name):
        return {g["name"]: self._regroup(g, tensor, lambda m: torch.zeros_like(tensor))
                for g in self.optimizer.param_groups if g["name"] == name}

    def _prune_optimizer(self, mask):
        return {g["name"]: self._regroup(g, g["params"][0][mask], lambda m: m[mask]) for g in self.optimizer.param_groups}

    def prune_points(self, mask):
        keep = ~mask
        self._adopt(self._prune_optimizer(keep))
        self.xyz_gradient_accum = self.xyz_gradient_accum[keep]
        self.denom = self.denom[keep]
        self.max_radii2D = self.max_radii2D[keep]

    def cat_tensors_to_optimizer(self, tensors_dict):
        out = {}
        for g in self.optimizer.param_groups:
            assert len(g["params"]) == 1
            ext = tensors_dict[g["name"]]
            out[g["name"]] = self._regroup(g, torch.cat((g["params"][0], ext), dim=0), lambda m, ext=ext: torch.cat((m, torch.zeros_like(ext)), dim=0))
        return out

    def densification_postfix(self, new_xyz, new_features_dc, new_features_rest, new_opacities, new_scaling, new_rotation):
        self._adopt(self.cat_tensors_to_optimizer({"xyz": new_xyz, "f_dc": new_features_dc, "f_rest": new_features_rest,
                                                   "opacity": new_opacities, "scaling": new_scaling, "rotation": new_rotation}))
        n, dev = self.get_xyz.shape[0], self._xyz.device
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        self.max_radii2D = torch.zeros((n,), device=dev)

    # -- the selections ---------------------------------------------------------------------------------------------------------------------
    def densify_and_clone(self, grads, grad_threshold, scene_extent):
        sel = torch.where(torch.norm(grads, dim=-1) >= grad_threshold, True, False)
        sel = torch.logical_and(sel, torch.max(self.get_scaling, dim=1).values <= self.percent_dense * scene_extent)
        self.densification_postfix(self._xyz[sel], self._features_dc[sel], self._features_rest[sel], self._opacity[sel],
                                   self._scaling[sel], self._rotation[sel])

    def densify_and_split(self, grads, grad_threshold, scene_extent, N=2):
        n, dev = self.get_xyz.shape[0], self._xyz.device
        padded = torch.zeros((n,), device=dev)
        padded[:grads.shape[0]] = grads.squeeze(-1)          # rows appended by the clone step count as zero
        sel = torch.where(padded >= grad_threshold, True, False)
        sel = torch.logical_and(sel, torch.max(self.get_scaling, dim=1).values > self.percent_dense * scene_extent)
        stds = self.get_scaling[sel].repeat(N, 1)
        means = torch.zeros((stds.size(0), 3), device=dev)
        samples = torch.normal(mean=means, std=stds)
        rots = build_rotation(self._rotation[sel]).repeat(N, 1, 1)
        new_xyz = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + self.get_xyz[sel].repeat(N, 1)
        new_scaling = self.scaling_inverse_activation(self.get_scaling[sel].repeat(N, 1) / (0.8 * N))
        self.densification_postfix(new_xyz, self._features_dc[sel].repeat(N, 1, 1), self._features_rest[sel].repeat(N, 1, 1),
                                   self._opacity[sel].repeat(N, 1), new_scaling, self._rotation[sel].repeat(N, 1))
        self.prune_points(torch.cat((sel, torch.zeros(N * sel.sum(), device=dev, dtype=torch.bool))))

    def _mean_gradient(self):
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        return grads

    def _removal_mask(self, min_opacity, extent, max_screen_size):
        mask = (self.get_opacity < min_opacity).squeeze(-1)
        if max_screen_size:
            too_big_on_screen = self.max_radii2D > max_screen_size
            too_big_in_world = self.get_scaling.max(dim=1).values > 0.1 * extent
            mask = torch.logical_or(torch.logical_or(mask, too_big_on_screen), too_big_in_world)
        return mask

    def densify(self, max_grad, min_opacity, extent, max_screen_size):
        grads = self._mean_gradient()
        self.densify_and_clone(grads, max_grad, extent)
        self.densify_and_split(grads, max_grad, extent)

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size):
        self.densify(max_grad, min_opacity, extent, max_screen_size)
        self.prune_points(self._removal_mask(min_opacity, extent, max_screen_size))
        if self._xyz.is_cuda and self.empty_cache:
            torch.cuda.empty_cache()

    def prune(self, max_grad, min_opacity, extent, max_screen_size):
        self.prune_points(self._removal_mask(min_opacity, extent, max_screen_size))
        if self._xyz.is_cuda and self.empty_cache:
            torch.cuda.empty_cache()

    def reset_opacity(self):
        capped = torch.min(self.get_opacity, torch.ones_like(self.get_opacity) * 0.01)
        self._adopt(self.replace_tensor_to_optimizer(self.inverse_opacity_activation(capped), "opacity"))


# ---- the merge: `HTGaussianTrainer.merge_two_3DGS` as the unmodified trainer runs it ----------------------------------------------------------
# Written from what the reference's method DOES (trainer/ht3dgs_trainer.py:226-272, `calc_importance` :1427-1462), in this
# file's own words over `StubSurgeryModel`: the method and attribute names are the interface (`gsr_autopatch` replaces `merge_two_3DGS` and
# calls the rest), the statements are this file's.
class StubModelRender(StubRender):
    """`StubRender` around a model that exists already (a `StubSurgeryModel`): `.gaussians`, `.bg_color`, the original wrapper's `render`."""

    def __init__(self, gaussians, bg=(0.0, 0.0, 0.0)):
        self.gaussians = gaussians
        self.bg_color = torch.tensor(bg, dtype=torch.float32, device=gaussians._xyz.device)


class _ListLogger:
    """`logger.info` that keeps its lines."""

    def __init__(self):
        self.lines = []

    def info(self, text):
        self.lines.append(str(text))


class StubMergeTrainer:
    """Stand-in for `HTGaussianTrainer` as far as a merge goes: `logger`, `pipe_cfg.prune_ratio`, a counting `load_viewpoint_cam` that hands
    out prepared cameras, `calc_importance` (a staticmethod, looked up on the class at the call -- replace it on a subclass to inject
    prepared scores) and `merge_two_3DGS` with the reference's sequence of torch operations: per model the row maximum of the score, `topk` of
    the lowest, a zero fill and an indexed store for the mask; `prune_points` on the destination between the two scores; the source's points
    through the homogeneous transform on all rows; six boolean gathers; `densification_postfix`.  It is the unpatched arm
    `gsr_autopatch.merge_two_3DGS_fused` is compared with and timed against.  Tensors are created on the model's own device, so the same
    class runs on the CPU for the dispatch tests."""

    def __init__(self, prune_ratio=0.5, cameras=None):
        import types
        self.pipe_cfg = types.SimpleNamespace(prune_ratio=prune_ratio, compute_cov3D_python=False, convert_SHs_python=False)
        self.logger = _ListLogger()
        self.cameras = {} if cameras is None else cameras            # frame index -> camera
        self.cam_calls = []                                          # (frame index, pose, load_depth) per call, in order

    def load_viewpoint_cam(self, idx, pose=None, load_depth=False, pose_to_train=False, load_vfi=False):
        self.cam_calls.append((idx, pose, load_depth))
        return self.cameras.get(idx)

    @staticmethod
    def calc_importance(gs_render, cameras, pipe):
        """Sum over the cameras of |d sum(render) / d SH coefficient|, over the pixel count: [N, 3 M]."""
        g = gs_render.gaussians
        hooks = [t.register_hook(lambda grad: grad.abs()) for t in (g._features_dc, g._features_rest)]
        g._features_dc.grad = None
        g._features_rest.grad = None
        num_pixels = 0
        for cam in cameras:
            image = gs_render.render(cam, compute_cov3D_python=pipe.compute_cov3D_python, convert_SHs_python=pipe.convert_SHs_python,
                                     override_color=None)["image"]
            image.sum().backward()
            num_pixels += image.shape[1] * image.shape[2]
        importance = torch.cat([g._features_dc.grad, g._features_rest.grad], 1).flatten(-2) / num_pixels
        for h in hooks:
            h.remove()
        if g._xyz.is_cuda:
            torch.cuda.empty_cache()
        return importance.detach()

    def _cameras_of(self, gaussians, frames):
        cams = []
        for fidx in frames:
            pose = gaussians.get_RT(fidx).detach().cpu() if not gaussians.rotate_seq else None
            cams.append(self.load_viewpoint_cam(fidx, pose=pose, load_depth=True))
        return cams

    def _lowest_mask(self, gaussians, importance):
        score = importance.amax(-1).squeeze()
        _, lowest = torch.topk(score, int(score.shape[0] * self.pipe_cfg.prune_ratio), largest=False)
        mask = torch.zeros((gaussians._xyz.shape[0], 1), device=gaussians._xyz.device)
        mask[lowest, :] = 1
        return mask.bool()

    def merge_two_3DGS(self, gs_render_dst, gs_render_src, transform_matrix, to_visit_frames_dst=None, to_visit_frames_src=None):
        dst, src = gs_render_dst.gaussians, gs_render_src.gaussians
        self.logger.info(f"The number of 3D Gaussians in the first 3DGS before merging: {dst.get_xyz.shape[0]}")
        self.logger.info(f"The number of 3D Gaussians in the second 3DGS before merging: {src.get_xyz.shape[0]}")
        importance = type(self).calc_importance(gs_render_dst, self._cameras_of(dst, to_visit_frames_dst), self.pipe_cfg)
        dst.prune_points(self._lowest_mask(dst, importance).squeeze())
        importance = type(self).calc_importance(gs_render_src, self._cameras_of(src, to_visit_frames_src), self.pipe_cfg)
        keep = ~(self._lowest_mask(src, importance).squeeze())
        n = len(src._xyz)
        homogeneous = torch.cat([src._xyz, torch.ones((n, 1), device=src._xyz.device)], dim=1)
        moved = homogeneous @ transform_matrix.T
        moved = moved[:, :3] / moved[:, 3].unsqueeze(1)
        dst.densification_postfix(moved[keep], src._features_dc[keep], src._features_rest[keep], src._opacity[keep], src._scaling[keep],
                                  src._rotation[keep])
        self.logger.info(f"The number of 3D Gaussians in the merged 3DGS: {dst.get_xyz.shape[0]}")
