"""Host-side mirror of the reference's rasterizer interface, on top of the C ABI of include/gsr.h.

Same names, argument meaning and error behaviour as the module the reference imports
(`from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer`:
/root/reference/scene/gaussian_model_ht.py:39-42, gaussian_renderer/__init__.py:12), called as at
gaussian_model_ht.py:809-880 and returning the 4-tuple unpacked at :881-894
(color[3,H,W], radii[N] int32, depth[1,H,W], alpha[1,H,W]).

PyTorch is plumbing only: device memory (caching allocator), the current HIP stream and autograd.  All
arithmetic happens in the hand-written HIP kernels of csrc/gsr_kernels.hip.  There is no CPU path: tensors
must live on a ROCm device and the libraries must be built, otherwise a RuntimeError is raised.

Binding: the PyTorch-ROCm C++ extension `torch.ops.gsr.rasterize` (csrc/torch_ext.cpp: C++ autograd function, buffers
from at::empty, no Python in the allocator path).  `GSR_BINDING=ctypes` selects the plain-FFI route over the same C ABI
(`_RasterizeGaussians` below: the example INTEGRATION.md walks through).
"""
import ctypes as C
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import _ext as E
from . import _lib as L


class GaussianRasterizationSettings(NamedTuple):
    """The 12 keywords built at gaussian_model_ht.py:809-822 / gaussian_renderer/__init__.py:38-51."""
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


# diagnostics of the most recent forward (bench.py reads R and the per-tile staged counters from here)
_LAST = {"num_rendered": 0, "image": None, "W": 0, "H": 0, "B": 1}


def _sync_last():
    """Pull the extension's record of the most recent forward into _LAST (the ctypes route fills _LAST itself)."""
    if E.use_ctypes() or not E._loaded:
        return
    rec = torch.ops.gsr.debug_last()
    if len(rec) == 4:
        image, binning, meta, dims = rec
        _LAST.update(num_rendered=int(meta[0]), binning_capacity=int(meta[1]), image=image, binning=binning if binning.numel() else None,
                     W=int(dims[0]), H=int(dims[1]), B=int(dims[2]) if dims.numel() > 2 else 1)


def last_call_info():
    """{'num_rendered': R, 'staged': R_eff} of the most recent forward on this process."""
    lib = L.load()
    _sync_last()
    img, W, H, B = _LAST["image"], _LAST["W"], _LAST["H"], _LAST.get("B", 1)
    staged = 0
    if img is not None:
        T = ((W + 15) // 16) * ((H + 15) // 16) * B          # (a batched render: B images, one tall tile grid)
        off = lib.gsr_image_bytes_batched(W, H, B) - ((T * 16 + 255) // 256) * 256
        # four counters per tile (one per 8x8 sub-tile wave; tile-level kernels use slot 0): the tile's staged depth
        # is the deepest of its waves
        staged = int(img[off:off + 16 * T].view(torch.int32).view(T, 4).max(dim=1).values.sum().item())
    return {"num_rendered": _LAST["num_rendered"], "staged": staged}


def last_binning():
    """Debug / test hook (gsr_debug_read_binning): (ranges[T,2] int64, list[R] int64) of the most recent forward on this
    process -- per-tile [begin, end) into the (tile, depth, id)-ordered list of Gaussian ids."""
    lib = L.load()
    _sync_last()
    b, W, H, R = _LAST.get("binning"), _LAST["W"], _LAST["H"], _LAST["num_rendered"]
    if b is None:
        raise RuntimeError("no forward has run yet")
    if _LAST.get("B", 1) > 1:
        raise RuntimeError("last_binning: not available for a batched render")
    T = ((W + 15) // 16) * ((H + 15) // 16)
    ranges = torch.empty((T, 2), dtype=torch.int32, device=b.device)
    lst = torch.empty((max(R, 1),), dtype=torch.int32, device=b.device)
    with torch.cuda.device(b.device):
        st = torch.cuda.current_stream(b.device).cuda_stream
        L.check(lib.gsr_debug_read_binning(b.data_ptr(), _LAST["binning_capacity"], R, W, H, ranges.data_ptr(), lst.data_ptr(),
                                           C.c_void_p(st)), "gsr_debug_read_binning")
    return ranges.long() & 0xffffffff, lst[:R].long() & 0xffffffff


def _f32c(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """float32 + contiguous (viewmatrix / campos arrive as non-contiguous views: SURVEY Appendix B)."""
    if t is None:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _ptr(t: Optional[torch.Tensor]):
    return None if (t is None or t.numel() == 0) else t.data_ptr()


def _empty_to_none(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if (t is None or t.numel() == 0) else t


# frozen=None: take the frozen backward whenever frozen_backward_route() says nobody reads a per-Gaussian gradient -- when this is True.
# OFF by measurement (profiles/frozen_backward.txt, a pose iteration, frozen against full on one box): 0.714 against 0.739 ms at 1 M /
# degree 3 and 2.135 against 2.176 ms for 8 x 130 k, but 0.439 against 0.443 ms at 130 k / degree 0, inside that size's same-arm spread of
# 0.005 ms -- not faster at every size, so the keyword stays and the inference waits.  frozen=True takes the route (and its memory saving:
# 62 against 310 bytes per Gaussian of backward allocations at 1 M) explicitly.
FROZEN_BY_INFERENCE = False


def frozen_backward_route(param_grad, means2D_grad, camera_grad, transform_grad, fused_adam=False, densify_stats=False, frozen=None) -> bool:
    """Whether a backward takes the frozen call of gsr_backward (include/gsr.h, GsrBackwardArgs): the gradients of the camera and of
    points_transform alone, no per-Gaussian gradient computed, allocated or stored.

    param_grad      some of means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, sh_rest needs a gradient
    means2D_grad    means2D needs one (it does not change the route: the frozen call writes d_means2D when asked to)
    camera_grad     some of viewmatrix, projmatrix, campos needs one
    transform_grad  points_transform is given and needs one
    frozen          None = by inference: no fused Adam, no densify_stats, no parameter wants a gradient and the camera or the transform does
                    (the reference's pose phases after fix_position(): stage A's train_relative_pose, train_pose_only);
                    False = never; True = always -- a parameter that requires grad then keeps .grad = None -- and a RuntimeError with
                    fused_adam or densify_stats, or when neither the camera nor the transform wants a gradient."""
    del means2D_grad
    wanted = bool(camera_grad or transform_grad)
    if frozen:
        if fused_adam or densify_stats:
            raise RuntimeError("frozen=True is not served together with fused_adam, prepare_next or densify_stats")
        if not wanted:
            raise RuntimeError("frozen=True: the camera or points_transform must require grad (a frozen backward computes nothing else)")
        return True
    if frozen is not None or not FROZEN_BY_INFERENCE:
        return False
    return wanted and not (param_grad or fused_adam or densify_stats)


def _check_frozen(frozen, fused_adam=None, prepare_next=None, densify_stats=None):
    """frozen=True with an argument that needs the per-Gaussian backward: refused before anything touches a device."""
    if frozen and (fused_adam is not None or prepare_next is not None or densify_stats is not None):
        raise RuntimeError("frozen=True is not served together with fused_adam, prepare_next or densify_stats")


def _check_retire(retire, fused_adam=None, fused_adam_deferred=False, densify_stats=None, frozen=None):
    """retire = (retired_at, step): the retire table of a launch chain (include/gsr.h gsr_forward_retire) and the 1-based step of this
    call.  It is applied by the fused route alone -- the optimizer-in-backward with its hand-over; every other route REFUSES it rather than
    ignore it, before anything touches a device: a separate `FusedAdam.step()` launch (no fused_adam here), the deferred step, densify_stats,
    the frozen backward.  (The render-only call and the importance pass have no `retire` keyword; a table left with them through
    torch.ops.gsr.retire_attach is refused by the library / the binding.)"""
    if retire is None:
        return None
    table, step = retire
    if not torch.is_tensor(table) or table.dtype != torch.int32 or table.dim() != 1 or not table.is_contiguous():
        raise RuntimeError("retire: retired_at must be a contiguous int32 vector (one entry per model)")
    if int(step) < 1:
        raise RuntimeError("retire: the step of a call is 1-based (the counter the fused Adam receives)")
    if fused_adam is None:
        raise RuntimeError("retire: a retire table needs fused_adam -- an update applied by a separate FusedAdam.step() launch cannot be gated per model")
    if fused_adam_deferred:
        raise RuntimeError("retire: a retire table is not served with the deferred step (fused_adam_deferred)")
    if densify_stats is not None:
        raise RuntimeError("retire: a retire table is not served with densify_stats")
    if frozen:
        raise RuntimeError("retire: a retire table is not served on the frozen backward")
    return table, int(step)


def _call_with_retire(ops, retire, fn, *args):
    """fn(*args) with the table attached to it (torch.ops.gsr.retire_attach: single use, this thread); a call that fails before it took the
    table leaves none behind."""
    if retire is None:
        return fn(*args)
    ops.retire_attach(retire[0], retire[1])
    try:
        return fn(*args)
    finally:
        ops.retire_attach(retire[0][:0], 0)


def _frozen_code(frozen) -> int:
    """The `frozen` argument of torch.ops.gsr.rasterize: -1 by inference, 0 never, 1 always."""
    if frozen is None:
        return -1 if FROZEN_BY_INFERENCE else 0
    return 1 if frozen else 0


class _Workspace:
    """Allocator handed to gsr_forward: R-sized buffers come from torch's caching allocator."""

    def __init__(self, device):
        self.device = device
        self.binning = None
        self.scratch = []
        self.cb = L.ALLOC_FN(self._alloc)

    def _alloc(self, nbytes, tag, _user):
        try:
            buf = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        except Exception:  # out of memory -> NULL -> GSR_ERR_ALLOC
            return None
        if tag == L.GSR_ALLOC_BINNING:
            self.binning = buf
        else:
            self.scratch.append(buf)
        return buf.data_ptr()


class _CtypesForward:
    """What one gsr_forward through the plain-FFI route leaves behind: outputs, the buffers a backward (or the importance pass) reads,
    the prepared inputs they were computed from and the GsrForwardOut fields."""
    __slots__ = ("means3D", "opacities", "sh", "colors_precomp", "scales", "rotations", "cov3Ds_precomp", "vm", "pm", "campos", "bg", "sh_rest",
                 "xf", "color", "radii", "depth", "alpha", "geom", "image", "binning", "num_rendered", "binning_capacity", "forward_flags",
                 "N", "M", "H", "W")


def _ctypes_forward(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, sh_rest=None,
                    raw_params=False, viewmatrix=None, projmatrix=None, campos=None, points_transform=None, view_id=0) -> _CtypesForward:
    """gsr_forward over ctypes (shared by _RasterizeGaussians.forward and importance_accumulate's ctypes route)."""
    lib = L.load()
    rs = raster_settings
    dev = means3D.device
    if dev.type != "cuda":
        raise RuntimeError("GaussianRasterizer: tensors must be on a ROCm/HIP device (no CPU fallback)")
    means3D = _f32c(means3D)
    N = means3D.shape[0]
    sh, colors_precomp = _f32c(_empty_to_none(sh)), _f32c(_empty_to_none(colors_precomp))
    scales, rotations = _f32c(_empty_to_none(scales)), _f32c(_empty_to_none(rotations))
    cov3Ds_precomp = _f32c(_empty_to_none(cov3Ds_precomp))
    opacities = _f32c(opacities)
    vm = _f32c((viewmatrix if viewmatrix is not None else rs.viewmatrix).to(dev))
    pm = _f32c((projmatrix if projmatrix is not None else rs.projmatrix).to(dev))
    campos = _f32c((campos if campos is not None else rs.campos).to(dev))
    bg = _f32c(rs.bg.to(dev))
    H, W = int(rs.image_height), int(rs.image_width)
    sh_rest = _f32c(_empty_to_none(sh_rest))
    xf = None
    if points_transform is not None:       # [3,4] or [4,4] rigid / affine transform applied to the means in-kernel
        if tuple(points_transform.shape) not in ((3, 4), (4, 4)):
            raise RuntimeError("points_transform must be a [3,4] or [4,4] tensor")
        xf = _f32c(points_transform.to(dev)[:3])
    M = (int(sh.shape[1]) + (int(sh_rest.shape[1]) if sh_rest is not None else 0)) if sh is not None else 0

    color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    depth = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    alpha = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    radii = torch.empty((N,), dtype=torch.int32, device=dev)
    geom = torch.empty(lib.gsr_geom_bytes(N), dtype=torch.uint8, device=dev)
    image = torch.empty(lib.gsr_image_bytes(W, H), dtype=torch.uint8, device=dev)
    ws = _Workspace(dev)

    a = L.GsrForwardArgs()
    a.N, a.M, a.D, a.W, a.H = N, M, int(rs.sh_degree), W, H
    a.prefiltered, a.debug = int(bool(rs.prefiltered)), int(bool(rs.debug))
    a.scale_modifier, a.tanfovx, a.tanfovy = float(rs.scale_modifier), float(rs.tanfovx), float(rs.tanfovy)
    a.means3D, a.scales, a.rotations, a.cov3D_precomp = _ptr(means3D), _ptr(scales), _ptr(rotations), _ptr(cov3Ds_precomp)
    a.opacities, a.shs, a.colors_precomp = _ptr(opacities), _ptr(sh), _ptr(colors_precomp)
    a.viewmatrix, a.projmatrix, a.campos, a.bg = _ptr(vm), _ptr(pm), _ptr(campos), _ptr(bg)
    a.out_color, a.out_depth, a.out_alpha, a.radii = color.data_ptr(), depth.data_ptr(), alpha.data_ptr(), _ptr(radii)
    a.geom, a.image = geom.data_ptr(), image.data_ptr()
    a.alloc, a.alloc_user = ws.cb, None
    a.shs_rest, a.raw_params = _ptr(sh_rest), int(bool(raw_params))
    a.points_transform = _ptr(xf)
    a.view_id = int(view_id)
    out = L.GsrForwardOut()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(lib.gsr_forward(C.byref(a), C.byref(out), C.c_void_p(stream)), "gsr_forward")
    ws.scratch.clear()  # stream-ordered reuse by the caching allocator is safe: same stream

    _LAST.update(num_rendered=int(out.num_rendered), image=image, W=W, H=H, B=1, binning=ws.binning,
                 binning_capacity=int(out.binning_capacity))
    f = _CtypesForward()
    f.means3D, f.opacities, f.sh, f.colors_precomp, f.scales, f.rotations, f.cov3Ds_precomp = means3D, opacities, sh, colors_precomp, scales, rotations, cov3Ds_precomp
    f.vm, f.pm, f.campos, f.bg, f.sh_rest, f.xf = vm, pm, campos, bg, sh_rest, xf
    f.color, f.radii, f.depth, f.alpha, f.geom, f.image, f.binning = color, radii, depth, alpha, geom, image, ws.binning
    f.num_rendered, f.binning_capacity, f.forward_flags = int(out.num_rendered), int(out.binning_capacity), int(out.forward_flags)
    f.N, f.M, f.H, f.W = N, M, H, W
    return f


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings,
                sh_rest=None, raw_params=False, viewmatrix=None, projmatrix=None, campos=None, fused_adam=None,
                points_transform=None, view_id=0, frozen=None):
        # viewmatrix / projmatrix / campos are ALSO passed as explicit tensor inputs (same objects as in
        # raster_settings) so that autograd can return their gradients: a NamedTuple cannot carry grads.
        rs = raster_settings
        f = _ctypes_forward(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs, sh_rest, raw_params,
                            viewmatrix, projmatrix, campos, points_transform, view_id)
        means3D, opacities, sh, colors_precomp, scales, rotations, cov3Ds_precomp = f.means3D, f.opacities, f.sh, f.colors_precomp, f.scales, f.rotations, f.cov3Ds_precomp
        vm, pm, campos, bg, sh_rest, xf = f.vm, f.pm, f.campos, f.bg, f.sh_rest, f.xf
        color, radii, depth, alpha, geom, image = f.color, f.radii, f.depth, f.alpha, f.geom, f.image
        N, M, H, W = f.N, f.M, f.H, f.W
        ctx.raster_settings = rs
        ctx.num_rendered = f.num_rendered
        ctx.binning_capacity = f.binning_capacity
        ctx.forward_flags = f.forward_flags
        ctx.dims = (N, M, H, W)
        ctx.has = (sh is not None, colors_precomp is not None, scales is not None, cov3Ds_precomp is not None)
        ctx.raw = (sh_rest is not None, bool(raw_params))
        ctx.fused_adam = fused_adam
        ctx.frozen = frozen
        ctx.xf_shape = tuple(points_transform.shape) if points_transform is not None else None
        z = means3D.new_empty(0)
        # NOTE: depth is deliberately NOT saved -- the caller mutates it in place (ht3dgs_trainer.py:1290-1292).
        ctx.save_for_backward(means3D, opacities, sh if sh is not None else z, colors_precomp if colors_precomp is not None else z,
                              scales if scales is not None else z, rotations if rotations is not None else z,
                              cov3Ds_precomp if cov3Ds_precomp is not None else z, vm, pm, campos, bg, geom, image,
                              f.binning, sh_rest if sh_rest is not None else z, xf if xf is not None else z)
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)   # unused depth / alpha outputs arrive as None -> specialised backward
        return color, radii, depth, alpha

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth, grad_alpha):
        lib = L.load()
        rs = ctx.raster_settings
        (means3D, opacities, sh, colors_precomp, scales, rotations, cov3Ds_precomp, vm, pm, campos, bg, geom, image,
         binning, sh_rest, xf) = ctx.saved_tensors
        has_rest, raw_params = ctx.raw
        N, M, H, W = ctx.dims
        has_sh, has_col, has_scale, has_cov = ctx.has
        dev = means3D.device
        grad_color, grad_depth, grad_alpha = _f32c(grad_color), _f32c(grad_depth), _f32c(grad_alpha)
        if grad_color is None and grad_depth is None and grad_alpha is None:
            return (None,) * 18
        need_vm, need_pm, need_cp = ctx.needs_input_grad[11], ctx.needs_input_grad[12], ctx.needs_input_grad[13]
        d_vm = torch.empty((4, 4), dtype=torch.float32, device=dev) if need_vm else None
        d_pm = torch.empty((4, 4), dtype=torch.float32, device=dev) if need_pm else None
        d_cp = torch.empty((3,), dtype=torch.float32, device=dev) if need_cp else None
        has_xf = ctx.xf_shape is not None
        d_xf = torch.zeros(ctx.xf_shape, dtype=torch.float32, device=dev) if (has_xf and ctx.needs_input_grad[15]) else None

        fused = ctx.fused_adam
        nig = ctx.needs_input_grad
        take_frozen = frozen_backward_route(any(nig[q] for q in (0, 2, 3, 4, 5, 6, 7, 9)), nig[1], need_vm or need_pm or need_cp,
                                            d_xf is not None, fused is not None, False, ctx.frozen)
        # (the frozen call: d_means2D only when somebody wants it, none of the other per-Gaussian tensors)
        d_means2D = torch.empty((N, 3), dtype=torch.float32, device=dev) if (nig[1] or not take_frozen) else None
        d_means3D = d_opac = d_sh = d_sh_rest = d_col = d_scales = d_rot = d_cov = None
        fa = None
        if take_frozen:
            pass
        elif fused is not None:
            # optimizer-in-backward: the kernel applies the Adam step to the raw parameters in place; their gradients
            # are never materialised (the corresponding .grad stay None and optimizer.step() has nothing left to do)
            if not (raw_params and has_rest and has_sh and has_scale):
                raise RuntimeError("fused_adam needs the raw-parameter path (rasterize_gaussians_raw)")
            fa = fused.fused_backward_args({"xyz": means3D, "f_dc": sh, "f_rest": sh_rest, "opacity": opacities,
                                            "scaling": scales, "rotation": rotations}, int(rs.sh_degree))
        else:
            d_means3D = torch.empty((N, 3), dtype=torch.float32, device=dev)
            d_opac = torch.empty((N, 1), dtype=torch.float32, device=dev)
            d_sh = torch.empty((N, 1 if has_rest else M, 3), dtype=torch.float32, device=dev) if has_sh else None
            d_sh_rest = torch.empty((N, M - 1, 3), dtype=torch.float32, device=dev) if (has_sh and has_rest) else None
            d_col = torch.empty((N, 3), dtype=torch.float32, device=dev) if has_col else None
            d_scales = torch.empty((N, 3), dtype=torch.float32, device=dev) if has_scale else None
            d_rot = torch.empty((N, 4), dtype=torch.float32, device=dev) if has_scale else None
            d_cov = torch.empty((N, 6), dtype=torch.float32, device=dev) if has_cov else None
        scratch = torch.empty(lib.gsr_backward_scratch_bytes(N), dtype=torch.uint8, device=dev)

        a = L.GsrBackwardArgs()
        a.N, a.M, a.D, a.W, a.H = N, M, int(rs.sh_degree), W, H
        a.scale_modifier, a.tanfovx, a.tanfovy = float(rs.scale_modifier), float(rs.tanfovx), float(rs.tanfovy)
        a.means3D, a.opacities = _ptr(means3D), _ptr(opacities)
        a.scales, a.rotations = (_ptr(scales), _ptr(rotations)) if has_scale else (None, None)
        a.cov3D_precomp = _ptr(cov3Ds_precomp) if has_cov else None
        a.shs = _ptr(sh) if has_sh else None
        a.colors_precomp = _ptr(colors_precomp) if has_col else None
        a.viewmatrix, a.projmatrix, a.campos, a.bg = _ptr(vm), _ptr(pm), _ptr(campos), _ptr(bg)
        a.geom, a.image, a.binning, a.num_rendered = geom.data_ptr(), image.data_ptr(), binning.data_ptr(), ctx.num_rendered
        a.binning_capacity = ctx.binning_capacity
        a.forward_flags = ctx.forward_flags
        a.grad_color, a.grad_depth, a.grad_alpha = _ptr(grad_color), _ptr(grad_depth), _ptr(grad_alpha)
        a.d_means3D, a.d_means2D, a.d_opacities = _ptr(d_means3D), _ptr(d_means2D), _ptr(d_opac)
        a.d_colors_precomp, a.d_shs = _ptr(d_col), _ptr(d_sh)
        a.d_scales, a.d_rotations, a.d_cov3D_precomp = _ptr(d_scales), _ptr(d_rot), _ptr(d_cov)
        a.scratch = scratch.data_ptr()
        a.shs_rest = _ptr(sh_rest) if has_rest else None
        a.d_shs_rest, a.raw_params = _ptr(d_sh_rest), int(raw_params)
        a.d_viewmatrix, a.d_projmatrix, a.d_campos = _ptr(d_vm), _ptr(d_pm), _ptr(d_cp)
        a.fused_adam = C.addressof(fa) if fa is not None else None
        a.points_transform = _ptr(xf) if has_xf else None
        a.d_points_transform = _ptr(d_xf)       # first 12 floats = rows 0..2 (a [4,4] input keeps a zero last row)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            L.check(lib.gsr_backward(C.byref(a), C.c_void_p(stream)), "gsr_backward")
        if fused is not None:
            fused.fused_backward_applied()      # the update is enqueued: the optimizer's step count advances now, not at render time
        return (d_means3D, d_means2D, d_sh, d_col, d_opac, d_scales, d_rot, d_cov, None, d_sh_rest, None, d_vm, d_pm, d_cp, None, d_xf, None, None)


def _cam_inputs(rs):
    """Only route the camera tensors through autograd when one of them wants a gradient."""
    if any(torch.is_tensor(t) and t.requires_grad for t in (rs.viewmatrix, rs.projmatrix, rs.campos)):
        return rs.viewmatrix, rs.projmatrix, rs.campos
    return None, None, None


_EMPTY = {}


def _e(dev):
    t = _EMPTY.get(dev)
    if t is None:
        t = _EMPTY[dev] = torch.empty(0, dtype=torch.float32, device=dev)
    return t


def _ecpu():
    t = _EMPTY.get("cpu_i64")
    if t is None:
        t = _EMPTY["cpu_i64"] = torch.empty(0, dtype=torch.int64)
    return t


def _rasterize_ext(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs, sh_rest, raw_params,
                   fused_adam, points_transform, prepared=None, prepare_next=None, next_points_transform=None, densify_stats=None,
                   batch_first_block=None, fused_adam_deferred=False, view_id=0, extras=0, sh_origin=None, frozen=None, retire=None):
    """torch.ops.gsr.rasterize: empty tensors stand for None; the camera tensors of the settings tuple are ordinary inputs
    (their gradients are produced when one of them requires grad)."""
    _check_frozen(frozen, fused_adam, prepare_next, densify_stats)
    retire = _check_retire(retire, fused_adam, fused_adam_deferred, densify_stats, frozen)
    ops = E.load()
    dev = means3D.device
    if dev.type != "cuda":
        raise RuntimeError("GaussianRasterizer: tensors must be on a ROCm/HIP device (no CPU fallback)")
    e = _e(dev)
    pick = lambda t: e if (t is None or t.numel() == 0) else t
    vm, pm, cp = rs.viewmatrix, rs.projmatrix, rs.campos
    cam_grad = vm.requires_grad or pm.requires_grad or cp.requires_grad
    if vm.device != dev:
        vm, pm, cp = vm.to(dev), pm.to(dev), cp.to(dev)
    bg = rs.bg if rs.bg.device == dev else rs.bg.to(dev)
    nb = (len(batch_first_block) - 1) if batch_first_block is not None else 1
    if points_transform is not None and tuple(points_transform.shape) not in (((3, 4), (4, 4)) if nb <= 1 else ((nb, 3, 4),)):
        raise RuntimeError("points_transform must be a [3,4] or [4,4] tensor ([B,3,4] for a batch of B models)")
    if nb > 1 and (tuple(vm.shape) != (nb, 4, 4) or tuple(pm.shape) != (nb, 4, 4) or tuple(cp.shape) != (nb, 3)):
        raise RuntimeError("batch: raster_settings.viewmatrix / projmatrix must be [B,4,4] and campos [B,3]")
    xf = e if points_transform is None else points_transform.to(dev)
    if sh_origin is not None:
        if sh_origin.numel() != 3:
            raise RuntimeError("sh_origin must hold three numbers (the origin of the SH view direction)")
        if sh is None or nb > 1 or prepared is not None or prepare_next is not None:
            raise RuntimeError("sh_origin needs SH coefficients and is not served with a batch, prepared or prepare_next")
        sh_origin = sh_origin.detach().to(device=dev, dtype=torch.float32).reshape(3)
    m, v, lr, b1, b2, eps, step, commit = [], [], [], 0.0, 0.0, 0.0, 0, None
    if fused_adam is not None and not (torch.is_grad_enabled() and (means3D.requires_grad or opacities.requires_grad)):
        fused_adam = None       # a render that cannot reach a backward (torch.no_grad(), detached parameters): nothing to plan
    if fused_adam is not None:
        if not (raw_params and sh_rest is not None and sh is not None and scales is not None):
            raise RuntimeError("fused_adam needs the raw-parameter path (rasterize_gaussians_raw)")
        # a PLAN only: the step count advances when the backward that applies the update runs (csrc/torch_ext.cpp increments
        # `commit`), so a forward whose graph is dropped leaves the optimizer untouched
        group_tensors = {"xyz": means3D, "f_dc": sh, "f_rest": sh_rest, "opacity": opacities, "scaling": scales, "rotation": rotations}
        if fused_adam_deferred:      # the update goes to shadow buffers; optimizer.step() adopts it (optim.FusedAdam, deferred application)
            if prepare_next is not None:
                raise RuntimeError("fused_adam_deferred: a deferred update cannot prepare a next view")
            m, v, lr, b1, b2, eps, step, commit = fused_adam.deferred_step_plan(group_tensors, int(rs.sh_degree))
        else:
            m, v, lr, b1, b2, eps, step, commit = fused_adam.fused_step_plan(group_tensors, int(rs.sh_degree),
                                                                             None if prepare_next is None else int(prepare_next.sh_degree))
    eb = _EMPTY.get(("u8", dev))
    if eb is None:
        eb = _EMPTY[("u8", dev)] = torch.empty(0, dtype=torch.uint8, device=dev)
    nx = prepare_next
    if nx is not None and fused_adam is None and not torch.is_grad_enabled():
        nx = None               # (a no_grad render has no backward that could prepare anything)
    if nx is not None:
        if fused_adam is None:
            raise RuntimeError("prepare_next needs fused_adam: the backward that applies the update prepares the next render")
        if int(nx.sh_degree) not in (int(rs.sh_degree), int(rs.sh_degree) + 1) or int(nx.sh_degree) > 3 or \
                float(nx.scale_modifier) != float(rs.scale_modifier):
            raise RuntimeError("prepare_next: the next view must use this view's sh_degree or the one above it (oneupSHdegree) and this "
                               "view's scale_modifier")
        nvm, npm, ncp = nx.viewmatrix.to(dev), nx.projmatrix.to(dev), nx.campos.to(dev)
    args = (means3D, means2D, pick(sh), pick(colors_precomp), opacities, pick(scales), pick(rotations), pick(cov3Ds_precomp),
            pick(sh_rest), vm, pm, cp, bg, xf, int(rs.image_height), int(rs.image_width), float(rs.tanfovx),
            float(rs.tanfovy), float(rs.scale_modifier), int(rs.sh_degree), bool(raw_params), bool(rs.prefiltered),
            bool(rs.debug), bool(cam_grad), m, v, lr, b1, b2, eps, step,
            eb if prepared is None else prepared, e if nx is None else nvm, e if nx is None else npm, e if nx is None else ncp,
            0 if nx is None else int(nx.image_height), 0 if nx is None else int(nx.image_width),
            0.0 if nx is None else float(nx.tanfovx), 0.0 if nx is None else float(nx.tanfovy),
            e if (nx is None or next_points_transform is None) else next_points_transform.to(dev),
            -1 if nx is None else int(nx.sh_degree), _ecpu() if commit is None else commit,
            [] if densify_stats is None else list(densify_stats), [] if nb <= 1 else [int(x) for x in batch_first_block], int(view_id), int(extras),
            sh_origin, _frozen_code(frozen))
    if not rs.debug:
        out = _call_with_retire(ops, retire, ops.rasterize, *args)
        if extras:       # (color, radii, depth, alpha, clamped colour, visibility bytes)
            return out[:4] + (out[5], out[6])
        return out[:5] if prepare_next is not None else out[:4]
    # raster_settings.debug = True: what the public module does -- on an error in the native forward, dump the arguments to
    # snapshot_fw.dump for offline inspection and re-raise (the reference always passes debug=False, gaussian_model_ht.py:821)
    try:
        out = _call_with_retire(ops, retire, ops.rasterize, *args)
        if extras:
            return out[:4] + (out[5], out[6])
        return out[:5] if prepare_next is not None else out[:4]
    except Exception:
        torch.save([a.detach().cpu() if torch.is_tensor(a) else a for a in args[:24]], "snapshot_fw.dump")
        print("\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
        raise


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings,
                        points_transform=None, view_id=0, frozen: Optional[bool] = None):
    """frozen: which backward runs -- see frozen_backward_route (None = by inference, False = the full one, True = the frozen one)."""
    if not E.use_ctypes():
        return _rasterize_ext(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings,
                              None, False, None, points_transform, view_id=view_id, frozen=frozen)
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                     raster_settings, None, False, *_cam_inputs(raster_settings), None, points_transform, view_id, frozen)


def rasterize_gaussians_raw(means3D, means2D, features_dc, features_rest, opacity_logit, log_scales, rotations_raw,
                            raster_settings, fused_adam=None, points_transform=None, prepared=None, prepare_next=None,
                            next_points_transform=None, densify_stats=None, batch_first_block=None, fused_adam_deferred=False,
                            view_id=0, extras=0, sh_origin=None, frozen: Optional[bool] = None, retire=None):
    """Extension ("next" row f-2): rasterize straight from HTGaussianModel's raw parameters (_xyz, _features_dc,
    _features_rest, _opacity, _scaling, _rotation; /root/reference/scene/gaussian_model_ht.py:74-82) with the
    activations of :49-65,128-133,176-188 fused into the HIP kernels; gradients are w.r.t. the raw tensors.

    fused_adam = a `FusedAdam` whose groups are exactly these six tensors (names xyz, f_dc, f_rest, opacity, scaling,
    rotation as at gaussian_model_ht.py:275-286): backward() then applies that optimizer's step inside the
    per-Gaussian backward kernel (include/gsr.h GsrFusedAdam) and leaves the parameter .grad unset; means2D.grad is
    still produced.  Same result as backward() followed by optimizer.step().

    points_transform = [3,4] / [4,4] tensor M: every mean is replaced by M[:3,:3] p + M[:3,3] inside the kernels -- the
    fused form of `get_xyz` under pose fitting (`self.P[k].retr().act(xyz)`, gaussian_model_ht.py:135-148); its
    gradient comes back through autograd (see pose.py for the SE3 parametrisation).

    prepare_next = the raster settings of the NEXT render of these parameters (with fused_adam): backward() then also runs
    that render's preprocess on the freshly updated parameters (include/gsr.h GsrNextView) and a FIFTH output -- a byte
    buffer, valid once backward() has run -- is returned; hand it to the next call as `prepared=` together with the same
    settings and the (in-place updated) parameter tensors, and that forward skips its preprocess kernel with a bit-identical
    result.  The caller guarantees that nothing else modifies the parameters in between.  next_points_transform = the pose
    transform of that next render when it is not this render's (per-frame poses under refinement).

    densify_stats = (xyz_gradient_accum, denom, max_radii2D), float32 tensors of N elements: backward() then also accumulates
    the per-iteration densification statistics of /root/reference/trainer/ht3dgs_trainer.py:141-147 and
    /root/reference/scene/gaussian_model_ht.py:718-721 into them, inside the per-Gaussian backward kernel (include/gsr.h
    GsrDensifyStats) -- no torch ops on N-sized tensors per step.

    fused_adam_deferred = True (with fused_adam): backward() writes the Adam-updated parameters and moments into the optimizer's
    shadow buffers instead of in place (include/gsr.h GsrFusedAdam::param_out) and `fused_adam.step()` adopts them by swapping
    storages; until then the model is untouched, so surgery or a skipped step between backward() and step() keep the reference's
    meaning (what gsr_autopatch.render_fused uses under the unmodified trainer).

    batch_first_block = [0, b1, ..., N / 128]: the tensors hold B INDEPENDENT models back to back, model k owning the 128-Gaussian
    blocks [b_k, b_k+1) (pad every model to a multiple of 128 with Gaussians that are culled); raster_settings then carries one
    camera per model (viewmatrix / projmatrix [B,4,4], campos [B,3]; points_transform [B,3,4]) and the outputs are [B,3,H,W] /
    [B,1,H,W]: B renders in one launch chain, each bit-identical with rendering its model alone (include/gsr.h GsrBatch; the
    independent single-image fits of stage A, /root/reference/trainer/ht3dgs_trainer.py:697-698).

    view_id = the caller's id of the frame shown (non-zero, the same whenever the same frame is rendered; 0 = none): speed only --
    the forward blend's balanced placement recognises the frame by it instead of by its pose (include/gsr.h GsrForwardArgs::view_id).

    extras (extension binding; not together with prepare_next): bit 0 adds the CLAMPED colour image -- `clamp(color, 0, 1)`, written by
    the blend kernel, differentiable like torch.clamp -- and bit 1 the visibility bytes `radii > 0` (uint8 [N], written by the
    preprocess) to the returned tuple: (color, radii, depth, alpha, clamped, visible) -- what the reference's render wrapper derives
    with a torch launch each (gaussian_model_ht.py:883, :905).

    sh_origin = three numbers o (detached): the SH colour is evaluated in the direction normalize(means3D - o) of the UNtransformed
    means instead of normalize(posed mean - campos) -- the reference's `convert_SHs_python` render with `view_dependent`, whose origin
    is the camera centre in the model's own frame, `get_RT(uid).inverse()[:3, 3].detach()` (gaussian_model_ht.py:845-865).  The
    colour then sends no gradient to the pose or the camera; its direction gradient reaches means3D directly (include/gsr.h
    GsrForwardArgs::sh_origin).  Not with batch_first_block, prepared or prepare_next.

    frozen = which backward runs (frozen_backward_route): None -- by inference, the frozen call of gsr_backward (include/gsr.h: camera and
    points_transform gradients alone, no per-Gaussian gradient computed or allocated) when no parameter tensor requires grad and the
    camera or points_transform does, which is every pose iteration against detached parameters (the reference after fix_position():
    /root/reference/trainer/ht3dgs_trainer.py:307-335, 916-963); False -- always the full backward; True -- the frozen one even if a
    parameter requires grad (its .grad then stays None); RuntimeError with fused_adam, prepare_next or densify_stats.

    retire = (retired_at, step): the retire table of the launch chain -- B int32 entries on the device (one for a single model), 0 = active,
    otherwise the step at which torch.ops.gsr.batch_retire retired the model -- and the 1-based step s of this call (include/gsr.h
    gsr_forward_retire; the reference's per-model exit, /root/reference/trainer/ht3dgs_trainer.py:299-300).  The forward culls every
    model with 0 < retired_at[b] < s (background image, zero depth / alpha, radii 0, no gradient); the backward skips the Adam update of
    those models bit for bit and prepares the next render with the test at s + 1.  Needs fused_adam; refused (RuntimeError, before a device is
    touched) with fused_adam_deferred, densify_stats or frozen=True."""
    _check_frozen(frozen, fused_adam, prepare_next, densify_stats)
    if not E.use_ctypes():
        return _rasterize_ext(means3D, means2D, features_dc, None, opacity_logit, log_scales, rotations_raw, None, raster_settings,
                              features_rest, True, fused_adam, points_transform, prepared, prepare_next, next_points_transform,
                              densify_stats, batch_first_block, fused_adam_deferred, view_id, extras, sh_origin, frozen, retire)
    if retire is not None:
        raise RuntimeError("retire is served by the PyTorch extension binding only")
    if prepared is not None or extras or prepare_next is not None or densify_stats is not None or batch_first_block is not None or fused_adam_deferred \
            or sh_origin is not None:
        raise RuntimeError("prepared / prepare_next / densify_stats / batch_first_block / fused_adam_deferred / sh_origin are served by the "
                           "PyTorch extension binding only")
    e = torch.Tensor([])
    return _RasterizeGaussians.apply(means3D, means2D, features_dc, e, opacity_logit, log_scales, rotations_raw, e,
                                     raster_settings, features_rest, True, *_cam_inputs(raster_settings), fused_adam, points_transform, view_id,
                                     frozen)


def _render_only(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs, sh_rest, raw_params, depth_alpha, clamped,
                 visible, points_transform, view_id, sh_origin):
    """The render-only forward (include/gsr.h GsrForwardArgs::render_only) on either binding: (color, radii, depth, alpha, clamped,
    visible), None for what was not asked.  Nothing of the call but these tensors stays allocated."""
    dev = means3D.device
    if dev.type != "cuda":
        raise RuntimeError("render_gaussians: tensors must be on a ROCm/HIP device (no CPU fallback)")
    if points_transform is not None and tuple(points_transform.shape) not in ((3, 4), (4, 4)):
        raise RuntimeError("points_transform must be a [3,4] or [4,4] tensor")
    if sh_origin is not None and (sh_origin.numel() != 3 or _empty_to_none(sh) is None):
        raise RuntimeError("sh_origin must hold three numbers (the origin of the SH view direction) and needs SH coefficients")
    H, W = int(rs.image_height), int(rs.image_width)
    with torch.no_grad():
        if not E.use_ctypes():
            ops = E.load()
            e = _e(dev)
            pick = lambda t: e if (t is None or t.numel() == 0) else t.detach()
            if sh_origin is not None:
                sh_origin = sh_origin.detach().to(device=dev, dtype=torch.float32).reshape(3)
            xf = e if points_transform is None else points_transform.detach().to(dev)
            color, radii, depth, alpha, cl, vis = ops.render(
                means3D.detach(), pick(sh), pick(colors_precomp), opacities.detach(), pick(scales), pick(rotations), pick(cov3Ds_precomp),
                pick(sh_rest), rs.viewmatrix.detach().to(dev), rs.projmatrix.detach().to(dev), rs.campos.detach().to(dev), rs.bg.detach().to(dev), xf,
                H, W, float(rs.tanfovx), float(rs.tanfovy), float(rs.scale_modifier), int(rs.sh_degree), bool(raw_params), int(view_id),
                (1 if depth_alpha else 0) | (2 if clamped else 0) | (4 if visible else 0), sh_origin)
            return (color, radii, depth if depth_alpha else None, alpha if depth_alpha else None, cl if clamped else None,
                    vis if visible else None)
        # the plain-FFI route over the same C ABI: render_only = 1, geom = image = NULL, every buffer the library asks for is scratch
        if sh_origin is not None:
            raise RuntimeError("sh_origin is served by the PyTorch extension binding only")
        lib = L.load()
        means3D = _f32c(means3D.detach())
        N = means3D.shape[0]
        prep = lambda t: _f32c(_empty_to_none(None if t is None else t.detach()))
        sh, colors_precomp, scales, rotations = prep(sh), prep(colors_precomp), prep(scales), prep(rotations)
        cov3Ds_precomp, sh_rest, opacities = prep(cov3Ds_precomp), prep(sh_rest), _f32c(opacities.detach())
        vm, pm, campos, bg = (_f32c(t.detach().to(dev)) for t in (rs.viewmatrix, rs.projmatrix, rs.campos, rs.bg))
        xf = None if points_transform is None else _f32c(points_transform.detach().to(dev)[:3])
        M = (int(sh.shape[1]) + (int(sh_rest.shape[1]) if sh_rest is not None else 0)) if sh is not None else 0
        new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
        color, radii = new((3, H, W)), new((N,), torch.int32)
        depth, alpha = (new((1, H, W)), new((1, H, W))) if depth_alpha else (None, None)
        cl = new((3, H, W)) if clamped else None
        vis = new((N,), torch.uint8) if visible else None
        ws = _Workspace(dev)
        a = L.GsrForwardArgs()
        a.N, a.M, a.D, a.W, a.H = N, M, int(rs.sh_degree), W, H
        a.scale_modifier, a.tanfovx, a.tanfovy = float(rs.scale_modifier), float(rs.tanfovx), float(rs.tanfovy)
        a.means3D, a.scales, a.rotations, a.cov3D_precomp = _ptr(means3D), _ptr(scales), _ptr(rotations), _ptr(cov3Ds_precomp)
        a.opacities, a.shs, a.colors_precomp = _ptr(opacities), _ptr(sh), _ptr(colors_precomp)
        a.viewmatrix, a.projmatrix, a.campos, a.bg = _ptr(vm), _ptr(pm), _ptr(campos), _ptr(bg)
        a.out_color, a.out_depth, a.out_alpha, a.radii = color.data_ptr(), _ptr(depth), _ptr(alpha), _ptr(radii)
        a.geom, a.image = None, None
        a.alloc, a.alloc_user = ws.cb, None
        a.shs_rest, a.raw_params = _ptr(sh_rest), int(bool(raw_params))
        a.points_transform = _ptr(xf)
        a.view_id = int(view_id)
        a.out_color_clamped, a.visible = _ptr(cl), _ptr(vis)
        a.render_only = 1
        out = L.GsrForwardOut()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            L.check(lib.gsr_forward(C.byref(a), C.byref(out), C.c_void_p(stream)), "gsr_forward")
        if ws.binning is not None or out.binning or not (int(out.forward_flags) & L.GSR_FWD_FLAG_RENDER_ONLY):
            raise RuntimeError("render_gaussians: the library did not take the render-only route")
        ws.scratch.clear()  # stream-ordered reuse by the caching allocator is safe: same stream
        return color, radii, depth, alpha, cl, vis


def render_gaussians(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, depth_alpha=False,
                     clamped=False, visible=False, points_transform=None, view_id=0, sh_origin=None):
    """The image of a model that no backward will ever visit -- a frozen teacher (/root/reference/trainer/ht3dgs_trainer.py:877-883), an
    evaluation or novel-view render (:1050-1061) -- through the render-only forward (include/gsr.h GsrForwardArgs::render_only,
    torch.ops.gsr.render): the inputs of rasterize_gaussians without means2D and the training keywords.  No autograd (inputs are
    detached), no state planes, checkpoints or binning buffer: when the call returns the allocator holds the returned tensors and
    nothing else of it.  Returns (color, radii, depth, alpha, clamped, visible): depth / alpha [1,H,W] with depth_alpha=True, the
    clamped colour `clamp(color, 0, 1)` with clamped=True, the visibility bytes `radii > 0` (uint8 [N]) with visible=True, None for
    what was not asked.  Every returned tensor is bit-identical with the full forward's.  points_transform, view_id, sh_origin: as in
    rasterize_gaussians_raw (sh_origin: extension binding only).  last_call_info() / last_binning() keep describing the last full
    forward: this call leaves them nothing to read."""
    return _render_only(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, None, False,
                        depth_alpha, clamped, visible, points_transform, view_id, sh_origin)


def render_gaussians_raw(means3D, features_dc, features_rest, opacity_logit, log_scales, rotations_raw, raster_settings, depth_alpha=False,
                         clamped=False, visible=False, points_transform=None, view_id=0, sh_origin=None):
    """render_gaussians straight from HTGaussianModel's raw parameters (the inputs of rasterize_gaussians_raw without means2D and the
    training keywords; the activations run in-kernel)."""
    return _render_only(means3D, features_dc, None, opacity_logit, log_scales, rotations_raw, None, raster_settings, features_rest, True,
                        depth_alpha, clamped, visible, points_transform, view_id, sh_origin)


def importance_accumulate(acc, means3D, sh, opacities, scales, rotations, raster_settings, sh_rest=None, raw_params=False,
                          cov3Ds_precomp=None, colors_precomp=None, points_transform=None, view_id=0, sh_origin=None,
                          batch_first_block=None):
    """One view's merge-time colour importance, added to `acc` [N, M, 3] in place WITHOUT a backward (include/gsr.h
    gsr_importance_accumulate; /root/reference/trainer/ht3dgs_trainer.py:1427-1462 per view): one forward through the code path of
    rasterize_gaussians / rasterize_gaussians_raw, a second walk of its tile lists in forward order that sums alpha T over the
    pixels whose clamp gate is open, and |basis_k| [colour not clamped] S added per Gaussian.  No autograd, no .grad.
    Returns the forward's (color, radii, depth, alpha, geom, image, binning, meta) -- an ordinary backward over them is still valid
    (the extension binding; the ctypes binding returns the first four)."""
    dev = means3D.device
    if dev.type != "cuda":
        raise RuntimeError("importance_accumulate: tensors must be on a ROCm/HIP device (no CPU fallback)")
    rs = raster_settings
    with torch.no_grad():
        if not E.use_ctypes():
            ops = E.load()
            e = _e(dev)
            pick = lambda t: e if (t is None or t.numel() == 0) else t.detach()
            vm, pm, cp = rs.viewmatrix.to(dev), rs.projmatrix.to(dev), rs.campos.to(dev)
            if sh_origin is not None:
                sh_origin = sh_origin.detach().to(device=dev, dtype=torch.float32).reshape(3)
            xf = e if points_transform is None else points_transform.detach().to(dev)[:3]
            return tuple(ops.importance_accumulate(
                acc, means3D.detach(), pick(sh), pick(colors_precomp), opacities.detach(), pick(scales), pick(rotations), pick(cov3Ds_precomp),
                pick(sh_rest), vm, pm, cp, rs.bg.to(dev), xf, int(rs.image_height), int(rs.image_width), float(rs.tanfovx), float(rs.tanfovy),
                float(rs.scale_modifier), int(rs.sh_degree), bool(raw_params),
                [] if batch_first_block is None else [int(x) for x in batch_first_block], int(view_id), sh_origin))
        # the plain-FFI route over the same C ABI: the ctypes forward above for its buffers, then the pass
        if sh_origin is not None or batch_first_block is not None:
            raise RuntimeError("sh_origin / batch_first_block are served by the PyTorch extension binding only")
        lib = L.load()
        f = _ctypes_forward(means3D.detach(), sh, colors_precomp, opacities.detach(), scales, rotations, cov3Ds_precomp, rs, sh_rest, raw_params,
                            points_transform=points_transform, view_id=view_id)
        N, M, H, W = f.N, f.M, f.H, f.W
        if tuple(acc.shape) != (N, M, 3) or acc.dtype != torch.float32 or not acc.is_contiguous():
            raise RuntimeError("importance_accumulate: acc must be a contiguous float32 [N, M, 3] tensor (M = stored SH coefficients)")
        a = L.GsrForwardArgs()
        a.N, a.M, a.D, a.W, a.H = N, M, int(rs.sh_degree), W, H
        a.means3D, a.shs, a.shs_rest, a.colors_precomp = _ptr(f.means3D), _ptr(f.sh), _ptr(f.sh_rest), _ptr(f.colors_precomp)
        a.campos, a.points_transform, a.raw_params = _ptr(f.campos), _ptr(f.xf), int(bool(raw_params))
        a.out_color, a.geom, a.image = f.color.data_ptr(), f.geom.data_ptr(), f.image.data_ptr()
        out = L.GsrForwardOut()
        out.num_rendered, out.binning_capacity, out.forward_flags = f.num_rendered, f.binning_capacity, f.forward_flags
        out.binning = _ptr(f.binning)
        scratch = torch.empty(lib.gsr_importance_scratch_bytes(N), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            L.check(lib.gsr_importance_accumulate(C.byref(a), C.byref(out), acc.data_ptr(), scratch.data_ptr(), C.c_void_p(stream)),
                    "gsr_importance_accumulate")
        return f.color, f.radii, f.depth, f.alpha


def _views_inputs(fn, means3D, view_settings, points_transform, sh_origin, sh):
    """Checks and device copies shared by forward_views / importance_accumulate_views: (V, vm, pm, campos, xf | None, sh_origin | None)."""
    dev = means3D.device
    if dev.type != "cuda":
        raise RuntimeError(f"{fn}: tensors must be on a ROCm/HIP device (no CPU fallback)")
    rs = view_settings
    if rs.viewmatrix.dim() != 3 or tuple(rs.viewmatrix.shape[1:]) != (4, 4):
        raise RuntimeError(f"{fn}: view_settings must carry stacked cameras ([V,4,4], [V,4,4], [V,3]: batched.batch_settings)")
    V = int(rs.viewmatrix.shape[0])
    if not 1 <= V <= L.GSR_MAX_VIEWS:
        raise RuntimeError(f"{fn}: 1..{L.GSR_MAX_VIEWS} views expected, got {V}")
    if tuple(rs.projmatrix.shape) != (V, 4, 4) or tuple(rs.campos.shape) != (V, 3):
        raise RuntimeError(f"{fn}: view_settings must carry stacked cameras ([V,4,4], [V,4,4], [V,3]: batched.batch_settings)")
    f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
    xf = None
    if points_transform is not None:       # one [3,4] / [4,4] transform per view
        if points_transform.dim() != 3 or tuple(points_transform.shape) not in ((V, 3, 4), (V, 4, 4)):
            raise RuntimeError(f"{fn}: points_transform must be [V,3,4] or [V,4,4] (one transform per view)")
        xf = f32(points_transform[:, :3])
    if sh_origin is not None:
        if sh_origin.numel() != 3 * V or _empty_to_none(sh) is None:
            raise RuntimeError(f"{fn}: sh_origin must be [V,3] (one origin of the SH view direction per view) and needs SH coefficients")
        sh_origin = f32(sh_origin.reshape(V, 3))
    return V, f32(rs.viewmatrix), f32(rs.projmatrix), f32(rs.campos), xf, sh_origin


class _CtypesViews:
    """What one gsr_forward_views over ctypes leaves behind (forward_views and importance_accumulate_views share it)."""
    __slots__ = ("a", "out", "keep", "color", "radii", "depth", "alpha", "clamped", "visible", "N", "M", "V", "Npad")


def _ctypes_forward_views(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs, sh_rest, raw_params, V, vm, pm, campos,
                          xf, sh_origin, extras) -> _CtypesViews:
    lib = L.load()
    dev = means3D.device
    prep = lambda t: _f32c(_empty_to_none(None if t is None else t.detach()))
    means3D, opacities = _f32c(means3D.detach()), _f32c(opacities.detach())
    sh, colors_precomp, scales, rotations = prep(sh), prep(colors_precomp), prep(scales), prep(rotations)
    cov3Ds_precomp, sh_rest = prep(cov3Ds_precomp), prep(sh_rest)
    bg = _f32c(rs.bg.detach().to(dev))
    N = int(means3D.shape[0])
    Npad = (N + 127) // 128 * 128
    H, W = int(rs.image_height), int(rs.image_width)
    M = (int(sh.shape[1]) + (int(sh_rest.shape[1]) if sh_rest is not None else 0)) if sh is not None else 0
    new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
    f = _CtypesViews()
    f.N, f.M, f.V, f.Npad = N, M, V, Npad
    f.color, f.depth, f.alpha, f.radii = new((V, 3, H, W)), new((V, 1, H, W)), new((V, 1, H, W)), new((V * Npad,), torch.int32)
    f.clamped = new((V, 3, H, W)) if (extras & 1) else None
    f.visible = new((V * Npad,), torch.uint8) if (extras & 2) else None
    geom = new((lib.gsr_geom_bytes_views(N, V),), torch.uint8)
    image = new((lib.gsr_image_bytes_batched(W, H, V),), torch.uint8)
    ws = _Workspace(dev)
    a = L.GsrForwardArgs()
    a.N, a.M, a.D, a.W, a.H = N, M, int(rs.sh_degree), W, H
    a.scale_modifier, a.tanfovx, a.tanfovy = float(rs.scale_modifier), float(rs.tanfovx), float(rs.tanfovy)
    a.means3D, a.scales, a.rotations, a.cov3D_precomp = _ptr(means3D), _ptr(scales), _ptr(rotations), _ptr(cov3Ds_precomp)
    a.opacities, a.shs, a.colors_precomp = _ptr(opacities), _ptr(sh), _ptr(colors_precomp)
    a.viewmatrix, a.projmatrix, a.campos, a.bg = _ptr(vm), _ptr(pm), _ptr(campos), _ptr(bg)
    a.out_color, a.out_depth, a.out_alpha, a.radii = f.color.data_ptr(), f.depth.data_ptr(), f.alpha.data_ptr(), f.radii.data_ptr()
    a.geom, a.image = geom.data_ptr(), image.data_ptr()
    a.alloc, a.alloc_user = ws.cb, None
    a.shs_rest, a.raw_params = _ptr(sh_rest), int(bool(raw_params))
    a.points_transform, a.sh_origin = _ptr(xf), _ptr(sh_origin)
    a.out_color_clamped, a.visible = _ptr(f.clamped), _ptr(f.visible)
    out = L.GsrForwardOut()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(lib.gsr_forward_views(C.byref(a), V, C.byref(out), C.c_void_p(stream)), "gsr_forward_views")
    ws.scratch.clear()  # stream-ordered reuse by the caching allocator is safe: same stream
    f.a, f.out = a, out
    f.keep = (means3D, opacities, sh, colors_precomp, scales, rotations, cov3Ds_precomp, sh_rest, bg, vm, pm, campos, xf, sh_origin, geom, image,
              ws.binning)
    return f


def forward_views(means3D, sh, opacities, scales, rotations, view_settings, sh_rest=None, raw_params=False, cov3Ds_precomp=None,
                  colors_precomp=None, points_transform=None, sh_origin=None, extras=0):
    """ONE model under V cameras in one launch chain (include/gsr.h gsr_forward_views, torch.ops.gsr.rasterize_forward_views): the
    preprocess reads the model's one set of parameter rows for every view, behind it the chain is a batched forward's.
    view_settings: what batched.batch_settings returns for the V settings (cameras [V,4,4], [V,4,4], [V,3]; image size, field of view,
    background, degree and scale modifier shared); points_transform [V,3,4] / [V,4,4] and sh_origin [V,3] are per view.  No autograd --
    rasterize_views is the node with a backward (the frozen call over views) -- and inputs are detached.  extras: bit 0 = the clamped colour, bit 1 = the visibility
    bytes.  Returns (color [V,3,H,W], radii [V,N], depth [V,1,H,W], alpha [V,1,H,W], clamped [V,3,H,W] | None, visible [V,N] | None);
    every view's outputs are bit-identical with rendering that view alone."""
    V, vm, pm, cp, xf, sh_origin = _views_inputs("forward_views", means3D, view_settings, points_transform, sh_origin, sh)
    rs = view_settings
    dev = means3D.device
    N = int(means3D.shape[0])
    Npad = (N + 127) // 128 * 128
    rows = lambda t: t.view(V, Npad)[:, :N]
    with torch.no_grad():
        if not E.use_ctypes():
            ops = E.load()
            e = _e(dev)
            pick = lambda t: e if (t is None or t.numel() == 0) else t.detach()
            color, radii, depth, alpha, _geom, _image, _binning, _meta, cl, vis = ops.rasterize_forward_views(
                means3D.detach(), pick(sh), pick(colors_precomp), opacities.detach(), pick(scales), pick(rotations), pick(cov3Ds_precomp),
                pick(sh_rest), vm, pm, cp, rs.bg.detach().to(dev), e if xf is None else xf, int(rs.image_height), int(rs.image_width),
                float(rs.tanfovx), float(rs.tanfovy), float(rs.scale_modifier), int(rs.sh_degree), bool(raw_params), int(extras), sh_origin)
            return color, rows(radii), depth, alpha, cl if (extras & 1) else None, rows(vis) if (extras & 2) else None
        f = _ctypes_forward_views(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs, sh_rest, raw_params, V, vm, pm,
                                  cp, xf, sh_origin, int(extras))
        return f.color, rows(f.radii), f.depth, f.alpha, f.clamped, rows(f.visible) if f.visible is not None else None


def importance_accumulate_views(acc, means3D, sh, opacities, scales, rotations, view_settings, sh_rest=None, raw_params=False,
                                cov3Ds_precomp=None, colors_precomp=None, points_transform=None, sh_origin=None):
    """importance_accumulate for V views of one model in one launch chain (include/gsr.h gsr_importance_accumulate_views): one
    forward_views, one walk over the V images' tile lists, one finishing launch that adds the views' terms to `acc` [N, M, 3] in the
    order the views are given -- the order V single-view calls would add them in.  One host wait for the instance count instead of V.
    view_settings, points_transform, sh_origin: as in forward_views.  Returns the forward's (color [V,3,H,W], radii [V,N], depth, alpha)."""
    V, vm, pm, cp, xf, sh_origin = _views_inputs("importance_accumulate_views", means3D, view_settings, points_transform, sh_origin, sh)
    rs = view_settings
    dev = means3D.device
    N = int(means3D.shape[0])
    Npad = (N + 127) // 128 * 128
    rows = lambda t: t.view(V, Npad)[:, :N]
    with torch.no_grad():
        if not E.use_ctypes():
            ops = E.load()
            e = _e(dev)
            pick = lambda t: e if (t is None or t.numel() == 0) else t.detach()
            r = ops.importance_accumulate_views(
                acc, means3D.detach(), pick(sh), pick(colors_precomp), opacities.detach(), pick(scales), pick(rotations), pick(cov3Ds_precomp),
                pick(sh_rest), vm, pm, cp, rs.bg.detach().to(dev), e if xf is None else xf, int(rs.image_height), int(rs.image_width),
                float(rs.tanfovx), float(rs.tanfovy), float(rs.scale_modifier), int(rs.sh_degree), bool(raw_params), sh_origin)
            return r[0], rows(r[1]), r[2], r[3]
        lib = L.load()
        f = _ctypes_forward_views(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs, sh_rest, raw_params, V, vm, pm,
                                  cp, xf, sh_origin, 0)
        if tuple(acc.shape) != (f.N, f.M, 3) or acc.dtype != torch.float32 or not acc.is_contiguous():
            raise RuntimeError("importance_accumulate_views: acc must be a contiguous float32 [N, M, 3] tensor (M = stored SH coefficients)")
        scratch = torch.empty(lib.gsr_importance_scratch_bytes_views(f.N, V), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            L.check(lib.gsr_importance_accumulate_views(C.byref(f.a), V, C.byref(f.out), acc.data_ptr(), scratch.data_ptr(), C.c_void_p(stream)),
                    "gsr_importance_accumulate_views")
        return f.color, rows(f.radii), f.depth, f.alpha


class _ViewsCall:
    """What one rasterize_views call carries past autograd's tensor arguments: the frozen model's (detached) tensors, the settings, the
    device copies of the cameras and, after the forward, what the backward needs of it."""
    __slots__ = ("params", "rs", "raw_params", "V", "vm", "pm", "cp", "xf", "sh_origin", "xf_shape", "ext", "ctypes")


class _RasterizeViews(torch.autograd.Function):
    """rasterize_forward_views + rasterize_backward_views (gsr_forward_views + gsr_backward_views over ctypes) as one autograd node: the
    tensor inputs are the cameras and the transforms, the only things a backward over views differentiates."""

    @staticmethod
    def forward(ctx, viewmatrix, projmatrix, campos, points_transform, call):
        means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, sh_rest = call.params
        rs, V = call.rs, call.V
        dev = means3D.device
        if not E.use_ctypes():
            ops = E.load()
            e = _e(dev)
            pick = lambda t: e if (t is None or t.numel() == 0) else t
            call.ext = [pick(means3D), pick(sh), pick(colors_precomp), pick(opacities), pick(scales), pick(rotations), pick(cov3Ds_precomp),
                        pick(sh_rest), call.vm, call.pm, call.cp, rs.bg.detach().to(dev), pick(call.xf)]
            color, radii, depth, alpha, geom, image, binning, meta, _cl, _vis = ops.rasterize_forward_views(
                *call.ext, int(rs.image_height), int(rs.image_width), float(rs.tanfovx), float(rs.tanfovy), float(rs.scale_modifier),
                int(rs.sh_degree), bool(call.raw_params), 0, call.sh_origin)
            call.ext += [geom, image, binning, meta]
        else:
            f = _ctypes_forward_views(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs, sh_rest, call.raw_params, V,
                                      call.vm, call.pm, call.cp, call.xf, call.sh_origin, 0)
            call.ctypes = f
            color, radii, depth, alpha = f.color, f.radii, f.depth, f.alpha
        ctx.call = call
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)   # unused depth / alpha outputs arrive as None
        return color, radii, depth, alpha

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth, grad_alpha):
        call = ctx.call
        if grad_color is None and grad_depth is None and grad_alpha is None:
            return (None,) * 5
        rs, V = call.rs, call.V
        need_vm, need_pm, need_cp, need_xf = ctx.needs_input_grad[:4]
        dev = call.vm.device
        if call.ext is not None:
            ops = E.load()
            e = _e(dev)
            g = lambda t: e if t is None else t
            _m2d, d_vm, d_pm, d_cp, d_xf = ops.rasterize_backward_views(
                *call.ext, g(grad_color), g(grad_depth), g(grad_alpha), int(rs.image_height), int(rs.image_width), float(rs.tanfovx),
                float(rs.tanfovy), float(rs.scale_modifier), int(rs.sh_degree), bool(call.raw_params), False, bool(need_vm), bool(need_pm),
                bool(need_cp), bool(need_xf), call.sh_origin)
        else:
            lib = L.load()
            f = call.ctypes
            grad_color, grad_depth, grad_alpha = _f32c(grad_color), _f32c(grad_depth), _f32c(grad_alpha)
            new = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
            d_vm, d_pm = (new(V, 4, 4) if need_vm else None), (new(V, 4, 4) if need_pm else None)
            d_cp, d_xf = (new(V, 3) if need_cp else None), (new(V, 3, 4) if need_xf else None)
            scratch = torch.empty(lib.gsr_backward_scratch_bytes_views(f.N, V), dtype=torch.uint8, device=dev)
            a = L.GsrBackwardArgs()
            for name in ("N", "M", "D", "W", "H", "scale_modifier", "tanfovx", "tanfovy", "means3D", "scales", "rotations", "cov3D_precomp",
                         "opacities", "shs", "colors_precomp", "viewmatrix", "projmatrix", "campos", "bg", "geom", "image", "shs_rest",
                         "raw_params", "points_transform", "sh_origin"):
                setattr(a, name, getattr(f.a, name))
            a.binning, a.num_rendered = f.out.binning, f.out.num_rendered
            a.binning_capacity, a.forward_flags = f.out.binning_capacity, f.out.forward_flags
            a.grad_color, a.grad_depth, a.grad_alpha = _ptr(grad_color), _ptr(grad_depth), _ptr(grad_alpha)
            a.d_viewmatrix, a.d_projmatrix, a.d_campos, a.d_points_transform = _ptr(d_vm), _ptr(d_pm), _ptr(d_cp), _ptr(d_xf)
            a.scratch = scratch.data_ptr()
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                L.check(lib.gsr_backward_views(C.byref(a), V, C.c_void_p(stream)), "gsr_backward_views")
        if need_xf and call.xf_shape[1] == 4:     # a [V,4,4] input: the last row takes no part in the render
            d_xf = torch.cat([d_xf, torch.zeros((V, 1, 4), dtype=torch.float32, device=dev)], dim=1)
        return (d_vm if need_vm else None, d_pm if need_pm else None, d_cp if need_cp else None, d_xf if need_xf else None, None)


def rasterize_views(means3D, sh, opacities, scales, rotations, view_settings, sh_rest=None, raw_params=False, cov3Ds_precomp=None,
                    colors_precomp=None, points_transform=None, sh_origin=None):
    """ONE frozen model under V cameras in one launch chain, WITH a backward (include/gsr.h gsr_forward_views + gsr_backward_views): a
    torch.autograd.Function over torch.ops.gsr.rasterize_forward_views and rasterize_backward_views.  Gradients reach points_transform
    ([V,3,4] or [V,4,4]) and those of view_settings.viewmatrix / projmatrix / campos that require grad -- per view, nothing is summed
    across views.  The model's tensors take no gradient: only the frozen call is served over views.  Arguments as in forward_views.
    Returns (color [V,3,H,W], radii [V,N], depth [V,1,H,W], alpha [V,1,H,W]).  Raises RuntimeError before a device is touched when a
    parameter tensor requires grad or nothing differentiable does."""
    rs = view_settings
    params = (means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, sh_rest)
    if any(torch.is_tensor(t) and t.requires_grad for t in params):
        raise RuntimeError("rasterize_views: a parameter tensor requires grad, and only the frozen call is served over views (camera and "
                           "points_transform gradients; a full backward over views is not served) -- detach the model")
    diff = (rs.viewmatrix, rs.projmatrix, rs.campos, points_transform)
    if not any(torch.is_tensor(t) and t.requires_grad for t in diff):
        raise RuntimeError("rasterize_views: nothing differentiable requires grad (points_transform, viewmatrix, projmatrix, campos): use "
                           "forward_views for a render without a backward")
    call = _ViewsCall()
    call.V, call.vm, call.pm, call.cp, call.xf, call.sh_origin = _views_inputs("rasterize_views", means3D, rs, points_transform, sh_origin, sh)
    call.params = tuple(None if t is None else t.detach() for t in params)
    call.rs, call.raw_params = rs, bool(raw_params)
    call.xf_shape = tuple(points_transform.shape) if points_transform is not None else None
    call.ext = call.ctypes = None
    N = int(means3D.shape[0])
    Npad = (N + 127) // 128 * 128
    color, radii, depth, alpha = _RasterizeViews.apply(rs.viewmatrix, rs.projmatrix, rs.campos, points_transform, call)
    return color, radii.view(call.V, Npad)[:, :N], depth, alpha


class GaussianRasterizer(nn.Module):
    """Callable exactly as at gaussian_model_ht.py:824,871-880 and gaussian_renderer/__init__.py:53,88-96."""

    def __init__(self, raster_settings: GaussianRasterizationSettings, frozen: Optional[bool] = None):
        """frozen: which backward this module's renders run (frozen_backward_route: None = by inference, False = the full one, True = the
        frozen one).  It lives here and as the attribute `frozen`: forward() keeps exactly the reference's keyword set."""
        super().__init__()
        self.raster_settings = raster_settings
        self.frozen = frozen

    def markVisible(self, positions: torch.Tensor) -> torch.Tensor:
        """Frustum (near-plane) visibility mask; present in the module's API, unused by the reference."""
        rs = self.raster_settings
        with torch.no_grad():
            dev = positions.device
            if dev.type != "cuda":
                raise RuntimeError("markVisible: tensors must be on a ROCm/HIP device (no CPU fallback)")
            return E.load().mark_visible(positions, rs.viewmatrix.to(dev), rs.projmatrix.to(dev))

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        # (the keyword set is exactly the reference's; extensions such as points_transform live on the functions
        #  rasterize_gaussians / rasterize_gaussians_raw, and `frozen` on the constructor)
        rs = self.raster_settings
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or (
                (scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        e = torch.Tensor([])
        return rasterize_gaussians(means3D, means2D, shs if shs is not None else e,
                                   colors_precomp if colors_precomp is not None else e, opacities,
                                   scales if scales is not None else e, rotations if rotations is not None else e,
                                   cov3D_precomp if cov3D_precomp is not None else e, rs, frozen=self.frozen)
