"""Fused photometric loss (1-l)*L1 + l*(1-SSIM) of the train step and its depth term, HIP kernels behind the C ABI.

Host-side mirror of what the reference computes with torch ops: `Loss.forward`
(/root/reference/trainer/losses.py:98-136) with the 11x11 Gaussian-window SSIM (:147-209), applied to the
clamped render (`rendered_image.clamp(0, 1)`, /root/reference/scene/gaussian_model_ht.py:883).  The clamp is
fused: pass the rasterizer's raw colour output.  No CPU path.
"""
import torch

from . import _ext as E


class _FusedPhotometricLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, render, target, lambda_dssim, clamp):
        if render.device.type != "cuda":
            raise RuntimeError("fused_photometric_loss: tensors must be on a ROCm/HIP device (no CPU fallback)")
        ops = E.load()
        render = render.float().contiguous()
        target = target.to(render.device).float().contiguous()
        out, ws = ops.photometric_loss_forward(render, target, float(lambda_dssim), bool(clamp))
        ctx.save_for_backward(render, target, ws)
        ctx.cfg = (float(lambda_dssim), bool(clamp))
        return out[0]

    @staticmethod
    def backward(ctx, grad_loss):
        render, target, ws = ctx.saved_tensors
        lam, clamp = ctx.cfg
        return E.load().photometric_loss_backward(render, target, ws, grad_loss, lam, clamp), None, None, None


def fused_photometric_loss(render: torch.Tensor, target: torch.Tensor, lambda_dssim: float = 0.2,
                           clamp: bool = True) -> torch.Tensor:
    """render: raw rasterizer colour [3,H,W] (clamped to [0,1] inside when clamp=True); target [3,H,W].
    One dispatcher call; the autograd node lives in the extension (csrc/torch_ext.cpp PhotometricLossFn) -- the Python
    autograd.Function above states the same thing and serves the plain-FFI binding route."""
    if render.device.type != "cuda":
        raise RuntimeError("fused_photometric_loss: tensors must be on a ROCm/HIP device (no CPU fallback)")
    if E.use_ctypes():
        return _FusedPhotometricLoss.apply(render, target, lambda_dssim, clamp)
    return E.load().photometric_loss(render, target, float(lambda_dssim), bool(clamp))


class _FusedPhotometricTerms(torch.autograd.Function):
    """The same op with its three results exposed: (loss, mean SSIM, mean L1).  Only `loss` carries a gradient."""

    @staticmethod
    def forward(ctx, render, target, lambda_dssim, clamp):
        ops = E.load()
        render = render.float().contiguous()
        target = target.to(render.device).float().contiguous()
        out, ws = ops.photometric_loss_forward(render, target, float(lambda_dssim), bool(clamp))
        ctx.save_for_backward(render, target, ws)
        ctx.cfg = (float(lambda_dssim), bool(clamp))
        loss, ssim_v, l1_v = out[0], out[1], out[2]
        ctx.mark_non_differentiable(ssim_v, l1_v)
        return loss, ssim_v, l1_v

    @staticmethod
    def backward(ctx, grad_loss, _g_ssim, _g_l1):
        render, target, ws = ctx.saved_tensors
        lam, clamp = ctx.cfg
        return E.load().photometric_loss_backward(render, target, ws, grad_loss.contiguous(), lam, clamp), None, None, None


def fused_photometric_loss_terms(render: torch.Tensor, target: torch.Tensor, lambda_dssim: float = 0.2, clamp: bool = True):
    """(loss, mean SSIM, mean L1): what `Loss.forward` of /root/reference/trainer/losses.py:98-136 reports as `loss`,
    `1 - loss_dssim` and `loss_rgb / (1 - lambda)` -- one fused forward, one fused backward (gsr_autopatch.loss_forward)."""
    if render.device.type != "cuda":
        raise RuntimeError("fused_photometric_loss: tensors must be on a ROCm/HIP device (no CPU fallback)")
    return _FusedPhotometricTerms.apply(render, target, lambda_dssim, clamp)


def fused_photometric_loss_report(render: torch.Tensor, target: torch.Tensor, lambda_dssim: float = 0.2, clamp: bool = True):
    """(loss, terms): the differentiable loss and the six-float vector {loss, mean SSIM, mean L1, loss_rgb = (1 - lambda) mean L1,
    loss_dssim = 1 - mean SSIM, loss_depth = 0} that the same finishing kernel wrote -- the whole return dict of `Loss.forward`
    (/root/reference/trainer/losses.py:128-136) from one dispatcher call; autograd node in the extension (PhotometricTermsFn),
    no gradient materialised for the vector.  Extension binding only."""
    if render.device.type != "cuda":
        raise RuntimeError("fused_photometric_loss: tensors must be on a ROCm/HIP device (no CPU fallback)")
    return E.load().photometric_loss_terms(render, target, float(lambda_dssim), bool(clamp))


# ---- the depth term of Loss.forward (/root/reference/trainer/losses.py:86-95, :114-119) -----------------------------------------------
DEPTH_LOSS_KINDS = {"l1": 0, "invariant": 1}       # GSR_DEPTH_LOSS_L1 / GSR_DEPTH_LOSS_INVARIANT of include/gsr.h
DEPTH_CLAMP = (0.02, 20.0)                         # the bounds of the reference's two masked assignments (losses.py:116-117)


def _depth_kind(kind) -> int:
    if kind not in DEPTH_LOSS_KINDS:
        raise ValueError(f"depth loss type {kind!r}: 'l1' or 'invariant' (the reference's depth_loss_type)")
    return DEPTH_LOSS_KINDS[kind]


def _depth_images(depth) -> int:
    """Images of a depth stack ([B,1,H,W] -- what a batched render returns -- or [B,H,W] with B > 1); 0 for a plane [H,W] / [1,H,W]."""
    return int(depth.shape[0]) if (depth.dim() == 4 or (depth.dim() == 3 and depth.shape[0] > 1)) else 0


def _check_depth(depth, depth_gt):
    plane = depth.dim() == 2 or (depth.dim() == 3 and depth.shape[0] == 1)
    stack = (depth.dim() == 3 and depth.shape[0] > 1) or (depth.dim() == 4 and depth.shape[1] == 1)
    if stack:       # depth_gt [B,H,W] or [B,1,H,W] of the same B
        stack = (depth_gt.dim() == 3 or (depth_gt.dim() == 4 and depth_gt.shape[1] == 1)) and depth_gt.shape[0] == depth.shape[0]
    if not (plane or stack) or tuple(depth_gt.shape[-2:]) != tuple(depth.shape[-2:]) or depth_gt.numel() != depth.numel():
        raise RuntimeError("fused_depth_loss: depth and depth_gt must be [H,W] or [1,H,W] planes of one size, or stacks [B,1,H,W] / [B,H,W] "
                           f"of one B and one plane size (got {tuple(depth.shape)} and {tuple(depth_gt.shape)})")
    if depth.device.type != "cuda":
        raise RuntimeError("fused_depth_loss: tensors must be on a ROCm/HIP device (no CPU fallback)")


class _FusedDepthLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, depth_gt, kind, lo, hi):
        ops = E.load()
        depth = depth.float().contiguous()
        depth_gt = depth_gt.to(depth.device).float().contiguous()
        ctx.cfg = (kind, lo, hi)
        if _depth_images(depth):      # a stack: the SUM of the images' terms
            total, _rows, ws = ops.depth_loss_forward_stack(depth, depth_gt, kind, lo, hi)
            ctx.save_for_backward(depth, depth_gt, ws)
            return total
        out, ws = ops.depth_loss_forward(depth, depth_gt, kind, lo, hi)
        ctx.save_for_backward(depth, depth_gt, ws)
        return out[0]

    @staticmethod
    def backward(ctx, grad_loss):
        depth, depth_gt, ws = ctx.saved_tensors
        kind, lo, hi = ctx.cfg
        return E.load().depth_loss_backward(depth, depth_gt, ws, grad_loss.contiguous(), kind, lo, hi, 1.0), None, None, None, None


def fused_depth_loss(depth: torch.Tensor, depth_gt: torch.Tensor, kind: str = "invariant", clamp=DEPTH_CLAMP) -> torch.Tensor:
    """`get_depth_loss(depth_pred, depth_gt)` of the reference after its clamp statements (losses.py:116-119, :86-95), unweighted:
    depth = the rasterizer's depth plane [H,W] or [1,H,W] (clamped to `clamp` inside; strictly clamped pixels get zero gradient),
    kind = the reference's depth_loss_type: 'l1', or 'invariant' = the scale-and-shift-invariant loss (alpha 0.5, one scale, mask
    depth_gt > 0.02) whose gradient flows through the fitted scale and shift.  Four short launches forward, one backward, float64
    fixed-order sums: bit-identical from run to run, no host synchronisation.  Autograd node in the extension (DepthLossFn); the
    Python autograd.Function above states the same thing and serves the plain-FFI binding route.
    A stack of B independent planes -- depth [B,1,H,W] (a batched render's depth) or [B,H,W], depth_gt [B,H,W] or [B,1,H,W] -- returns the
    SUM of the images' terms, as the photometric loss does on a stack: every image has its own fit and its own M, the launches stay
    four and one, and image b's term and gradient plane are bit for bit those of the plane alone (`fused_depth_loss_rows` reads the
    per-image rows)."""
    _check_depth(depth, depth_gt)
    k, lo, hi = _depth_kind(kind), float(clamp[0]), float(clamp[1])
    if E.use_ctypes():
        return _FusedDepthLoss.apply(depth, depth_gt, k, lo, hi)
    return E.load().depth_loss(depth, depth_gt, k, lo, hi)


def fused_depth_loss_rows(depth: torch.Tensor, depth_gt: torch.Tensor, kind: str = "invariant", clamp=DEPTH_CLAMP) -> torch.Tensor:
    """{loss_depth, scale s, shift t, M, data term, regulariser} of the same forward, without a gradient: (6,) for a plane, one row per
    image [B,6] for a stack (`torch.ops.gsr.depth_loss_forward`)."""
    _check_depth(depth, depth_gt)
    with torch.no_grad():
        return E.load().depth_loss_forward(depth.float().contiguous(), depth_gt.to(depth.device).float().contiguous(), _depth_kind(kind),
                                           float(clamp[0]), float(clamp[1]))[0]


def fused_training_loss_report(render: torch.Tensor, target: torch.Tensor, depth: torch.Tensor = None, depth_gt: torch.Tensor = None,
                               lambda_dssim: float = 0.2, lambda_depth: float = 0.0, kind: str = "invariant", clamp: bool = True,
                               depth_clamp=DEPTH_CLAMP):
    """(loss, terms): the whole of `Loss.forward` (losses.py:98-136) -- loss = photometric + lambda_depth * depth term, and the
    six-float vector {total loss, mean SSIM, mean L1, loss_rgb, loss_dssim, loss_depth (unweighted)}, i.e. every entry of the dict the
    reference returns -- from one dispatcher call; ONE autograd node hands back d_render and d_depth.  `clamp` is the render's
    clamp(0, 1) as in fused_photometric_loss; the depth plane is clamped to `depth_clamp` inside.  Without a depth_gt, or with
    lambda_depth = 0, this is fused_photometric_loss_report: the same launches, the same bits.  Extension binding only.
    Stacks: render / target [B,3,H,W] with depth [B,1,H,W] or [B,H,W] and depth_gt [B,H,W] or [B,1,H,W] of the same B -- loss = the SUM
    of the images' losses, terms[5] = the mean of the images' unweighted depth terms (as terms[1], terms[2] are means), still one node."""
    if depth_gt is None or depth is None or float(lambda_depth) == 0.0:
        return fused_photometric_loss_report(render, target, lambda_dssim, clamp)
    if render.device.type != "cuda":
        raise RuntimeError("fused_photometric_loss: tensors must be on a ROCm/HIP device (no CPU fallback)")
    _check_depth(depth, depth_gt)
    if (render.dim() == 4) != bool(_depth_images(depth)) or (render.dim() == 4 and render.shape[0] != depth.shape[0]) \
            or tuple(render.shape[-2:]) != tuple(depth.shape[-2:]):
        raise RuntimeError("fused_depth_loss: depth and depth_gt must be [H,W] or [1,H,W] planes of one size, or stacks [B,1,H,W] / [B,H,W] "
                           f"of one B and one plane size, matching the render (got render {tuple(render.shape)}, depth {tuple(depth.shape)})")
    return E.load().training_loss_terms(render, target, depth, depth_gt, float(lambda_dssim), float(lambda_depth), _depth_kind(kind),
                                        bool(clamp), float(depth_clamp[0]), float(depth_clamp[1]))
