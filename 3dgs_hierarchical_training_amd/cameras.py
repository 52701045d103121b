"""Cameras from poses that stay on the device.

The reference builds a new `Camera` for every iteration (/root/reference/scene/cameras.py:17-101, through `load_viewpoint_cam`,
/root/reference/trainer/trainer.py:989-1142): the pose comes to the host (`get_RT(fidx).detach().cpu()`, a wait for the device), goes back
up as three small tensors, and the camera centre is an `inverse()` on the device that waits once more.  The virtual views of the non-leaf
phase add `get_virtual_view` (/root/reference/trainer/ht3dgs_trainer.py:462-479).  Here both are one launch each on a device pose:

  camera_from_pose    gsr_camera_from_pose    view matrix, full projection and camera centre of 1..16 poses
  settings_from_pose  the same, as the `GaussianRasterizationSettings` the rasterizer takes
  virtual_view        gsr_pose_virtual_view   pose0 * Exp(alpha * Log(pose0^-1 * pose1)), and that pose relative to a base pose

Semantics in include/gsr.h (float64 inside, one rounding to float32 per output; csrc/camera_kernels.hip).  Nothing here reads a tensor
back, calls `.item()` or does matrix work on the host.  No CPU fallback: a CPU tensor raises RuntimeError before a device is touched.
"""
from typing import Optional, Sequence, Tuple

import torch

ZNEAR, ZFAR = 0.01, 100.0         # Camera.znear / zfar (cameras.py:70-71)
MAX_BATCH = 16


def _need_device(name: str, **tensors):
    for k, t in tensors.items():
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise RuntimeError(f"{name}: {k} must be a tensor on a ROCm/HIP device -- there is no CPU fallback")


def camera_from_pose(pose: torch.Tensor, fx: float, fy: float, cx: float, cy: float, W: int, H: int, znear: float = ZNEAR,
                     zfar: float = ZFAR) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(viewmatrix, projmatrix, campos) of `pose` ([4,4] world-to-camera -> [4,4], [4,4], [3]; [B,4,4] or [B,16] with B <= 16 -> [B,4,4],
    [B,4,4], [B,3]) in the layouts `Camera(is_co3d=True)` keeps (world_view_transform, full_proj_transform, camera_center)."""
    _need_device("camera_from_pose", pose=pose)
    if not (fx > 0 and fy > 0 and W > 0 and H > 0):
        raise ValueError("camera_from_pose: fx, fy, W and H must be positive")
    from . import _ext
    return _ext.load().camera_from_pose(pose.detach(), float(fx), float(fy), float(cx), float(cy), int(W), int(H), float(znear), float(zfar))


def settings_from_pose(template, pose: torch.Tensor, intrinsics: Optional[Sequence[float]] = None, znear: float = ZNEAR, zfar: float = ZFAR):
    """`template` (a GaussianRasterizationSettings: size, field of view, background, degree) with the three camera tensors of the device
    pose `pose` [4,4].  intrinsics = (fx, fy, cx, cy) in pixels; None = what the template's field of view states, principal point at the
    centre (synthetic.make_camera's camera)."""
    _need_device("settings_from_pose", pose=pose)
    W, H = int(template.image_width), int(template.image_height)
    if intrinsics is None:
        fx, fy, cx, cy = 0.5 * W / float(template.tanfovx), 0.5 * H / float(template.tanfovy), 0.5 * W, 0.5 * H
    else:
        fx, fy, cx, cy = (float(v) for v in intrinsics)
    if tuple(pose.shape) != (4, 4):
        raise ValueError("settings_from_pose: pose is one [4,4] world-to-camera matrix")
    view, proj, campos = camera_from_pose(pose, fx, fy, cx, cy, W, H, znear, zfar)
    return template._replace(viewmatrix=view, projmatrix=proj, campos=campos)


def virtual_view(p0: torch.Tensor, p1: torch.Tensor, alpha: float, base: Optional[torch.Tensor] = None):
    """The pose `alpha` of the way from p0 to p1, p0 * Exp(alpha * Log(p0^-1 * p1)) ([4,4] device tensors, alpha a host number in [0, 1]).
    With `base` returns (pose, pose * base^-1): the view and the same view in the coordinates of a model whose own frame is `base`."""
    _need_device("virtual_view", p0=p0, p1=p1, base=base)
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("virtual_view: alpha must lie in [0, 1]")
    from . import _ext
    out, out_rel = _ext.load().pose_virtual_view(p0.detach(), p1.detach(), alpha, None if base is None else base.detach())
    return out if base is None else (out, out_rel)
