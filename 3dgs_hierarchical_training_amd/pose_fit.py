"""Fit F poses, independently, against ONE model that does not move.

The workload of the reference's test-time pose fit (`eval_nvs`, trainer/ht3dgs_trainer.py:1018-1042 of the reference: 200 epochs x F
frames with update_gaussians=False, update_cam=True), of a segment's pose refinement before an evaluation and of any "register these
images against this model" task.  Every frame f owns six tangent numbers delta_f under Adam, its pose is M_f = Exp(delta_f) * base_f
and reaches the render as `points_transform`; the loss is the fused photometric loss (plus the depth term on request) -- what stage
A's pose phase uses (stage_a.fit_pair).

Two routes, chosen by `views_per_call`:
  1   frame by frame: rasterize_gaussians_raw(..., frozen=True) + gsr_pose_step -- one launch chain, one host wait and one read of the
      model's parameter rows per frame and iteration;
  V   the frames in chunks of V (the last one may be shorter): per iteration of a chunk ONE rasterize_views (gsr_forward_views +
      gsr_backward_views), ONE loss on the stack of images, ONE backward and ONE gsr_pose_step_many.
Nothing couples the frames on either route, and under the `deterministic_backward` option the returned poses are bit-identical for
every value of views_per_call.
"""
from typing import Dict, Optional, Tuple

import torch

from . import _lib as L

RAW_KEYS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def check_views_per_call(views_per_call) -> int:
    """1 .. GSR_MAX_VIEWS, a whole number: anything else raises ValueError (before a device is touched)."""
    if isinstance(views_per_call, bool) or not isinstance(views_per_call, int) or not 1 <= views_per_call <= L.GSR_MAX_VIEWS:
        raise ValueError(f"views_per_call={views_per_call!r}: a whole number from 1 to {L.GSR_MAX_VIEWS} expected")
    return views_per_call


def fit_poses(raw: Dict[str, torch.Tensor], settings, targets: torch.Tensor, init: Optional[torch.Tensor] = None, iters: int = 200,
              lr: float = 2e-3, views_per_call: int = 1, lambda_dssim: float = 0.2, depth_gt: Optional[torch.Tensor] = None,
              lambda_depth: float = 0.0, depth_loss_type: str = "invariant",
              sh_origin: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, dict]:
    """raw: the model's six raw tensors, as `GaussianParams.raw()` returns them (they are detached: the model is frozen).
    settings: ONE shared camera -- the identity camera of the pose convention the harness uses (sequence.settings_for_pose(eye)), at the
    SH degree to render with.  targets [F,3,H,W].  init [F,3,4] (or [F,4,4]): the start transforms, `base` of M = Exp(delta) * base; None
    = the identity.  lr / Adam's defaults as stage A's pose phase.  depth_gt [F,H,W] or [F,1,H,W] with lambda_depth != 0 adds the depth
    term (`depth_loss_type`: 'invariant' or 'l1').  sh_origin [F,3] (optional): per frame, the point the SH view direction is taken from, in
    the model's own coordinates and held fixed during the fit (the rasterizer's sh_origin) -- without it the colour sees the direction
    from the identity camera to the POSED mean, which is what a camera at the pose sees only at SH degree 0.
    Returns (M [F,3,4] on the device, info): info = {'frames', 'iters', 'views_per_call', 'chunks', 'launch_chains'} -- launch_chains is
    the number of render + backward chains the fit enqueued (F * iters frame by frame, chunks * iters over views)."""
    V = check_views_per_call(views_per_call)
    if int(iters) < 0:
        raise ValueError(f"iters={iters!r}: a non-negative count expected")
    missing = [k for k in RAW_KEYS if k not in raw]
    if missing:
        raise ValueError(f"fit_poses: raw lacks {missing} (GaussianParams.raw() returns all six)")
    dev = raw["_xyz"].device
    if dev.type != "cuda" or targets.device.type != "cuda":
        raise RuntimeError("fit_poses: tensors must be on a ROCm/HIP device (no CPU fallback)")
    if targets.dim() != 4 or targets.shape[1] != 3 or tuple(targets.shape[2:]) != (int(settings.image_height), int(settings.image_width)):
        raise ValueError("fit_poses: targets must be [F,3,H,W] at the settings' image size")
    F = int(targets.shape[0])
    if init is not None and tuple(init.shape) not in ((F, 3, 4), (F, 4, 4)):
        raise ValueError("fit_poses: init must be [F,3,4] or [F,4,4] (one start transform per frame)")
    if sh_origin is not None and tuple(sh_origin.shape) != (F, 3):
        raise ValueError("fit_poses: sh_origin must be [F,3] (one origin per frame)")
    with_depth = depth_gt is not None and float(lambda_depth) != 0.0
    if with_depth and int(depth_gt.shape[0]) != F:
        raise ValueError("fit_poses: depth_gt must carry one plane per frame")

    from . import _ext
    from .loss import fused_photometric_loss, fused_training_loss_report
    from .rasterizer import rasterize_gaussians_raw, rasterize_views
    ops = _ext.load()
    xyz, fdc, frest, opac, scal, rot = (raw[k].detach() for k in RAW_KEYS)
    targets = targets.detach().float().contiguous()
    if with_depth:
        depth_gt = depth_gt.detach().float().contiguous()
    none = torch.empty(0, device=dev)
    if sh_origin is not None:
        sh_origin = sh_origin.detach().to(dev).float().contiguous()
    base = none if init is None else init.detach().to(dev).float()[:, :3].contiguous()
    delta = torch.zeros(F, 6, device=dev)
    m, v = torch.zeros(F, 6, device=dev), torch.zeros(F, 6, device=dev)
    M = torch.zeros(F, 3, 4, device=dev)
    b1, b2, eps = 0.9, 0.999, 1e-8          # torch.optim.Adam's defaults, as stage A's pose phase

    def loss_of(out, lo, hi):      # out = (image, radii, depth, alpha) of frame lo (hi = lo + 1, single images) or of the stack lo .. hi
        single = out[0].dim() == 3
        tgt = targets[lo] if single else targets[lo:hi]
        if with_depth:
            dgt = depth_gt[lo] if single else depth_gt[lo:hi]
            return fused_training_loss_report(out[0], tgt, out[2], dgt, lambda_dssim, float(lambda_depth), depth_loss_type, clamp=True)[0]
        return fused_photometric_loss(out[0], tgt, lambda_dssim, clamp=True)     # a stack: the SUM of the images' losses

    chunks = 0
    if V == 1:
        m2d = torch.zeros_like(xyz)
        for f in range(F):
            chunks += 1
            bf = none if init is None else base[f]
            so = None if sh_origin is None else sh_origin[f]
            ops.pose_step(delta[f], m[f], v[f], none, bf, M[f], lr, b1, b2, eps, 0)              # M_f = Exp(0) base_f
            for it in range(1, int(iters) + 1):
                Mi = M[f].detach().requires_grad_(True)
                out = rasterize_gaussians_raw(xyz, m2d, fdc, frest, opac, scal, rot, settings, points_transform=Mi, sh_origin=so, frozen=True)
                loss_of(out, f, f + 1).backward()
                ops.pose_step(delta[f], m[f], v[f], Mi.grad, bf, M[f], lr, b1, b2, eps, it)
    else:
        from .batched import batch_settings
        for lo in range(0, F, V):
            hi = min(F, lo + V)
            chunks += 1
            vs = batch_settings([settings] * (hi - lo), dev)
            bc = none if init is None else base[lo:hi]
            d_, m_, v_, M_ = delta[lo:hi], m[lo:hi], v[lo:hi], M[lo:hi]      # (contiguous views of the F poses: updated in place)
            ops.pose_step_many(d_, m_, v_, none, bc, M_, lr, b1, b2, eps, 0)
            for it in range(1, int(iters) + 1):
                Mi = M_.detach().requires_grad_(True)
                out = rasterize_views(xyz, fdc, opac, scal, rot, vs, sh_rest=frest, raw_params=True, points_transform=Mi,
                                      sh_origin=None if sh_origin is None else sh_origin[lo:hi])
                loss_of(out, lo, hi).backward()
                ops.pose_step_many(d_, m_, v_, Mi.grad, bc, M_, lr, b1, b2, eps, it)
    info = {"frames": F, "iters": int(iters), "views_per_call": V, "chunks": chunks, "launch_chains": chunks * int(iters)}
    return M, info
