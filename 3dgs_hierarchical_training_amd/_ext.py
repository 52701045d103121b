"""Loader of the PyTorch-ROCm extension (csrc/torch_ext.cpp -> csrc/torch_build/gsr_torch.so) and the fake kernels that
make its ops traceable (torch.compile / FakeTensor).

`torch.ops.gsr.*` is the product's binding: GaussianRasterizer, the fused loss, FusedAdam and simple_knn go through
it.  The ctypes view of the same C ABI (_lib.py) stays as the plain-FFI example of INTEGRATION.md and for the debug /
profiling hooks; `GSR_BINDING=ctypes` routes the rasterizer through it (one GPU test does, to keep it honest).
No fallback: a missing gsr_torch.so raises.
"""
import os

import torch

from . import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
EXT_PATH = os.path.join(HERE, "csrc", "torch_build", "gsr_torch.so")
_loaded = False


def use_ctypes() -> bool:
    return os.environ.get("GSR_BINDING", "") == "ctypes"


def load():
    """torch.ops.load_library(gsr_torch.so) once; returns torch.ops.gsr."""
    global _loaded
    if not _loaded:
        L.load()        # libgsr_hip.so first (fails loudly when it is not built)
        if not os.path.exists(EXT_PATH):
            raise RuntimeError(f"{EXT_PATH} not found: the PyTorch extension is not built (run `python __graft_entry__.py` or "
                               "`python 3dgs_hierarchical_training_amd/build.py`).  There is no CPU fallback.")
        torch.ops.load_library(EXT_PATH)
        _register_fakes()
        _loaded = True
    return torch.ops.gsr


def _register_fakes():
    lib = L.load()

    @torch.library.register_fake("gsr::rasterize_forward")
    def _(means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, sh_rest, viewmatrix, projmatrix, campos, bg,
          points_transform, image_height, image_width, tanfovx, tanfovy, scale_modifier, sh_degree, raw_params, prefiltered, debug,
          prepared, batch_first_block, view_id=0, extras=0, sh_origin=None):
        N, H, W = means3D.shape[0], image_height, image_width
        f = lambda *s: means3D.new_empty(s, dtype=torch.float32)
        b = lambda n: means3D.new_empty((n,), dtype=torch.uint8)
        ctx = torch.library.get_ctx()
        nbin = ctx.new_dynamic_size()          # the binning buffer is R-sized: data dependent
        B = len(batch_first_block) - 1 if len(batch_first_block) >= 3 else 1
        lead = (B,) if B > 1 else ()
        return (f(*lead, 3, H, W), means3D.new_empty((N,), dtype=torch.int32), f(*lead, 1, H, W), f(*lead, 1, H, W), b(lib.gsr_geom_bytes(int(N))),
                b(lib.gsr_image_bytes_batched(int(W), int(H), B)), b(nbin), torch.empty((3,), dtype=torch.int64),
                f(*lead, 3, H, W) if (extras & 1) else f(0), b(N if ((extras & 2) and prepared.numel() == 0) else 0))

    @torch.library.register_fake("gsr::render")
    def _(means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, sh_rest, viewmatrix, projmatrix, campos, bg,
          points_transform, image_height, image_width, tanfovx, tanfovy, scale_modifier, sh_degree, raw_params, view_id=0, outputs=0,
          sh_origin=None):
        # (color, radii, depth, alpha, clamped, visible); outputs: bit 0 depth + alpha, bit 1 clamped colour, bit 2 visibility bytes
        N, H, W = means3D.shape[0], image_height, image_width
        f = lambda *s: means3D.new_empty(s, dtype=torch.float32)
        return (f(3, H, W), means3D.new_empty((N,), dtype=torch.int32), f(1, H, W) if (outputs & 1) else f(0),
                f(1, H, W) if (outputs & 1) else f(0), f(3, H, W) if (outputs & 2) else f(0),
                means3D.new_empty((N if (outputs & 4) else 0,), dtype=torch.uint8))

    @torch.library.register_fake("gsr::importance_accumulate")
    def _(acc, means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, sh_rest, viewmatrix, projmatrix, campos, bg,
          points_transform, image_height, image_width, tanfovx, tanfovy, scale_modifier, sh_degree, raw_params, batch_first_block,
          view_id=0, sh_origin=None):
        # acc is mutated in place (the schema's (a!)); the forward's {color, radii, depth, alpha, geom, image, binning, meta} come back
        N, H, W = means3D.shape[0], image_height, image_width
        f = lambda *s: means3D.new_empty(s, dtype=torch.float32)
        b = lambda n: means3D.new_empty((n,), dtype=torch.uint8)
        nbin = torch.library.get_ctx().new_dynamic_size()
        return [f(3, H, W), means3D.new_empty((N,), dtype=torch.int32), f(1, H, W), f(1, H, W), b(lib.gsr_geom_bytes(int(N))),
                b(lib.gsr_image_bytes_batched(int(W), int(H), 1)), b(nbin), torch.empty((3,), dtype=torch.int64)]

    def _views_outputs(means3D, viewmatrix, H, W, extras):
        N, V = means3D.shape[0], viewmatrix.shape[0]
        Npad = (N + 127) // 128 * 128
        f = lambda *s: means3D.new_empty(s, dtype=torch.float32)
        b = lambda n: means3D.new_empty((n,), dtype=torch.uint8)
        nbin = torch.library.get_ctx().new_dynamic_size()
        return [f(V, 3, H, W), means3D.new_empty((V * Npad,), dtype=torch.int32), f(V, 1, H, W), f(V, 1, H, W),
                b(lib.gsr_geom_bytes_views(int(N), int(V))), b(lib.gsr_image_bytes_batched(int(W), int(H), int(V))), b(nbin),
                torch.empty((3,), dtype=torch.int64), f(V, 3, H, W) if (extras & 1) else f(0), b(V * Npad if (extras & 2) else 0)]

    @torch.library.register_fake("gsr::rasterize_forward_views")
    def _(means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, sh_rest, viewmatrix, projmatrix, campos, bg,
          points_transform, image_height, image_width, tanfovx, tanfovy, scale_modifier, sh_degree, raw_params, extras=0, sh_origin=None):
        return tuple(_views_outputs(means3D, viewmatrix, image_height, image_width, extras))

    @torch.library.register_fake("gsr::importance_accumulate_views")
    def _(acc, means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, sh_rest, viewmatrix, projmatrix, campos, bg,
          points_transform, image_height, image_width, tanfovx, tanfovy, scale_modifier, sh_degree, raw_params, sh_origin=None):
        return _views_outputs(means3D, viewmatrix, image_height, image_width, 0)[:8]

    @torch.library.register_fake("gsr::importance_pass")
    def _(acc, means3D, sh, sh_rest, campos, points_transform, color, geom, image, binning, meta, image_height, image_width, sh_degree,
          sh_origin=None):
        return None

    @torch.library.register_fake("gsr::rasterize")
    def _(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, sh_rest, viewmatrix, projmatrix, campos,
          bg, points_transform, image_height, image_width, tanfovx, tanfovy, scale_modifier, sh_degree, raw_params, prefiltered, debug,
          cam_grad, adam_m, adam_v, adam_lr, beta1, beta2, eps, step, prepared, next_viewmatrix, next_projmatrix, next_campos,
          next_height, next_width, next_tanfovx, next_tanfovy, next_points_transform, next_sh_degree, adam_commit, densify_stats, batch_first_block, view_id=0, extras=0,
          sh_origin=None, frozen=-1):
        N, H, W = means3D.shape[0], image_height, image_width
        f = lambda *s: means3D.new_empty(s, dtype=torch.float32)
        nprep = lib.gsr_prepared_bytes(int(N)) if next_viewmatrix.numel() else 0
        B = len(batch_first_block) - 1 if len(batch_first_block) >= 3 else 1
        lead = (B,) if B > 1 else ()
        return (f(*lead, 3, H, W), means3D.new_empty((N,), dtype=torch.int32), f(*lead, 1, H, W), f(*lead, 1, H, W),
                means3D.new_empty((nprep,), dtype=torch.uint8), f(*lead, 3, H, W) if (extras & 1) else f(0),
                means3D.new_empty((N if ((extras & 2) and prepared.numel() == 0) else 0,), dtype=torch.uint8))

    @torch.library.register_fake("gsr::rasterize_backward")
    def _(means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, sh_rest, viewmatrix, projmatrix, campos, bg,
          points_transform, geom, image, binning, meta, grad_color, grad_depth, grad_alpha, image_height, image_width, tanfovx, tanfovy,
          scale_modifier, sh_degree, raw_params, need_viewmatrix, need_projmatrix, need_campos, need_points_transform, densify_stats, radii,
          batch_first_block, sh_origin=None):
        N = means3D.shape[0]
        f = lambda *s: means3D.new_empty(s, dtype=torch.float32)
        has = lambda t: t.numel() > 0
        M = (sh.shape[1] + (sh_rest.shape[1] if has(sh_rest) else 0)) if has(sh) else 0
        none = f(0)
        B = len(batch_first_block) - 1 if len(batch_first_block) >= 3 else 1
        lead = (B,) if B > 1 else ()           # a batch of B models: one camera gradient per model (as the real op returns them)
        return [f(N, 3), f(N, 3), f(N, 1 if has(sh_rest) else M, 3) if has(sh) else none, f(N, 3) if has(colors_precomp) else none,
                f(N, 1), f(N, 3) if has(scales) else none, f(N, 4) if has(scales) else none, f(N, 6) if has(cov3D_precomp) else none,
                f(N, M - 1, 3) if (has(sh) and has(sh_rest)) else none, f(*lead, 4, 4) if need_viewmatrix else none,
                f(*lead, 4, 4) if need_projmatrix else none, f(*lead, 3) if need_campos else none,
                f(*lead, 3, 4) if (need_points_transform and has(points_transform)) else none]

    @torch.library.register_fake("gsr::rasterize_backward_frozen")
    def _(means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, sh_rest, viewmatrix, projmatrix, campos, bg,
          points_transform, geom, image, binning, meta, grad_color, grad_depth, grad_alpha, image_height, image_width, tanfovx, tanfovy,
          scale_modifier, sh_degree, raw_params, need_means2D, need_viewmatrix, need_projmatrix, need_campos, need_points_transform,
          batch_first_block, sh_origin=None):
        f = lambda *s: means3D.new_empty(s, dtype=torch.float32)
        none = f(0)
        B = len(batch_first_block) - 1 if len(batch_first_block) >= 3 else 1
        lead = (B,) if B > 1 else ()
        return [f(means3D.shape[0], 3) if need_means2D else none, f(*lead, 4, 4) if need_viewmatrix else none,
                f(*lead, 4, 4) if need_projmatrix else none, f(*lead, 3) if need_campos else none,
                f(*lead, 3, 4) if (need_points_transform and points_transform.numel() > 0) else none]

    @torch.library.register_fake("gsr::rasterize_backward_views")
    def _(means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, sh_rest, viewmatrix, projmatrix, campos, bg,
          points_transform, geom, image, binning, meta, grad_color, grad_depth, grad_alpha, image_height, image_width, tanfovx, tanfovy,
          scale_modifier, sh_degree, raw_params, need_means2D, need_viewmatrix, need_projmatrix, need_campos, need_points_transform,
          sh_origin=None):
        # {d_means2D [V Npad,3], d_viewmatrix [V,4,4], d_projmatrix [V,4,4], d_campos [V,3], d_points_transform [V,3,4]}; empty = not wanted
        f = lambda *s: means3D.new_empty(s, dtype=torch.float32)
        none = f(0)
        N, V = means3D.shape[0], viewmatrix.shape[0]
        Npad = (N + 127) // 128 * 128
        return [f(V * Npad, 3) if need_means2D else none, f(V, 4, 4) if need_viewmatrix else none, f(V, 4, 4) if need_projmatrix else none,
                f(V, 3) if need_campos else none, f(V, 3, 4) if (need_points_transform and points_transform.numel() > 0) else none]

    @torch.library.register_fake("gsr::rasterize_backward_fused")
    def _(means3D, sh, sh_rest, opacities, scales, rotations, viewmatrix, projmatrix, campos, bg, points_transform, geom, image, binning,
          meta, grad_color, grad_depth, grad_alpha, image_height, image_width, tanfovx, tanfovy, scale_modifier, sh_degree,
          need_viewmatrix, need_projmatrix, need_campos, need_points_transform, adam_m, adam_v, adam_lr, beta1, beta2, eps, step,
          next_viewmatrix, next_projmatrix, next_campos, next_height, next_width, next_tanfovx, next_tanfovy, prepared_out,
          next_points_transform, next_sh_degree, densify_stats, radii, batch_first_block, sh_origin=None):
        f = lambda *s: means3D.new_empty(s, dtype=torch.float32)
        none = f(0)
        B = len(batch_first_block) - 1 if len(batch_first_block) >= 3 else 1
        lead = (B,) if B > 1 else ()
        return [f(means3D.shape[0], 3), f(*lead, 4, 4) if need_viewmatrix else none, f(*lead, 4, 4) if need_projmatrix else none,
                f(*lead, 3) if need_campos else none, f(*lead, 3, 4) if (need_points_transform and points_transform.numel() > 0) else none]

    # in-place ops without a return value: nothing to describe beyond the schema's (a!) annotations
    @torch.library.register_fake("gsr::adam_step")
    def _(params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step):
        return None

    @torch.library.register_fake("gsr::pose_step")
    def _(delta, exp_avg, exp_avg_sq, d_xf, base, xf, lr, beta1, beta2, eps, step):
        return None

    @torch.library.register_fake("gsr::pose_step_many")
    def _(delta, exp_avg, exp_avg_sq, d_xf, base, xf, lr, beta1, beta2, eps, step):
        return None

    @torch.library.register_fake("gsr::pose_step_camera")
    def _(delta, exp_avg, exp_avg_sq, d_viewmatrix, d_projmatrix, d_campos, projection_T, base, viewmatrix, projmatrix, campos, lr,
          beta1, beta2, eps, step):
        return None

    @torch.library.register_fake("gsr::pose_matrix_forward")
    def _(delta, base):
        return delta.new_empty((3, 4), dtype=torch.float32)

    @torch.library.register_fake("gsr::pose_matrix")
    def _(delta, base):
        return delta.new_empty((3, 4), dtype=torch.float32)

    @torch.library.register_fake("gsr::pose_matrix_backward")
    def _(delta, base, d_xf):
        return torch.empty_like(delta)

    @torch.library.register_fake("gsr::masked_max_")
    def _(dst, src, mask):
        return None

    @torch.library.register_fake("gsr::densify_stats_add_")
    def _(accum, denom, grad, mask):
        return None

    @torch.library.register_fake("gsr::psnr")
    def _(a, b):
        return a.new_empty((a.shape[0], 1), dtype=torch.float32)

    @torch.library.register_fake("gsr::mark_visible")
    def _(means3D, viewmatrix, projmatrix):
        return means3D.new_empty((means3D.shape[0],), dtype=torch.bool)

    @torch.library.register_fake("gsr::photometric_loss_forward")
    def _(render, target, lambda_dssim, clamp):
        C, H, W = render.shape[-3:]
        B = render.shape[0] if render.dim() == 4 else 1
        return render.new_empty((3,), dtype=torch.float32), render.new_empty((lib.gsr_loss_workspace_bytes(int(B * C), int(H), int(W)),), dtype=torch.uint8)

    @torch.library.register_fake("gsr::photometric_loss")
    def _(render, target, lambda_dssim, clamp):
        return render.new_empty((), dtype=torch.float32)

    @torch.library.register_fake("gsr::photometric_loss_terms")
    def _(render, target, lambda_dssim, clamp):
        return render.new_empty((), dtype=torch.float32), render.new_empty((6,), dtype=torch.float32)

    @torch.library.register_fake("gsr::photometric_loss_backward")
    def _(render, target, workspace, grad_loss, lambda_dssim, clamp):
        return torch.empty_like(render, dtype=torch.float32)

    def _depth_images(depth):
        """Images of a depth stack ([B,1,H,W], or [B,H,W] with B > 1); 0 for a plane [H,W] / [1,H,W]."""
        return int(depth.shape[0]) if (depth.dim() == 4 or (depth.dim() == 3 and depth.shape[0] > 1)) else 0

    @torch.library.register_fake("gsr::depth_loss_forward")
    def _(depth, depth_gt, kind, clamp_lo, clamp_hi):
        H, W = depth.shape[-2:]
        B = _depth_images(depth)
        nws = lib.gsr_depth_loss_workspace_bytes_batched(B, int(H), int(W)) if B else lib.gsr_depth_loss_workspace_bytes(int(H), int(W))
        return depth.new_empty((B, 6) if B else (6,), dtype=torch.float32), depth.new_empty((nws,), dtype=torch.uint8)

    @torch.library.register_fake("gsr::depth_loss_forward_stack")
    def _(depth, depth_gt, kind, clamp_lo, clamp_hi):
        H, W = depth.shape[-2:]
        B = _depth_images(depth)
        return (depth.new_empty((), dtype=torch.float32), depth.new_empty((B, 6), dtype=torch.float32),
                depth.new_empty((lib.gsr_depth_loss_workspace_bytes_batched(B, int(H), int(W)),), dtype=torch.uint8))

    @torch.library.register_fake("gsr::depth_loss_backward")
    def _(depth, depth_gt, workspace, grad_loss, kind, clamp_lo, clamp_hi, lambda_depth):
        return torch.empty_like(depth, dtype=torch.float32)

    @torch.library.register_fake("gsr::depth_loss")
    def _(depth, depth_gt, kind, clamp_lo, clamp_hi):
        return depth.new_empty((), dtype=torch.float32)

    @torch.library.register_fake("gsr::training_loss_terms")
    def _(render, target, depth, depth_gt, lambda_dssim, lambda_depth, kind, clamp, clamp_lo, clamp_hi):
        return render.new_empty((), dtype=torch.float32), render.new_empty((6,), dtype=torch.float32)

    @torch.library.register_fake("gsr::knn_mean_dist2")
    def _(points):
        return points.new_empty((points.shape[0],), dtype=torch.float32)

    @torch.library.register_fake("gsr::depth_to_points")
    def _(depth, image, fx, fy, cx, cy):
        H, W = depth.shape[-2:]
        return depth.new_empty((H * W, 3), dtype=torch.float32), depth.new_empty((H * W if image is not None else 0, 3), dtype=torch.float32)

    @torch.library.register_fake("gsr::voxel_down_sample")
    def _(points, colors, voxel_size):
        # M (the number of occupied voxels) and `dropped` depend on the data: unbacked sizes.  The real op reads them back from the device
        # (its one host synchronisation), so a compiled graph breaks here all the same.
        ctx = torch.library.get_ctx()
        M, dropped = ctx.new_dynamic_size(), ctx.new_dynamic_size()
        return (points.new_empty((M, 3), dtype=torch.float32), points.new_empty((M if colors is not None else 0, 3), dtype=torch.float32),
                points.new_empty((M,), dtype=torch.int32), dropped)

    @torch.library.register_fake("gsr::camera_from_pose")
    def _(pose, fx, fy, cx, cy, W, H, znear=0.01, zfar=100.0):
        f = lambda *s: pose.new_empty(s, dtype=torch.float32)
        if pose.dim() == 2 and tuple(pose.shape) == (4, 4):
            return f(4, 4), f(4, 4), f(3)
        B = pose.shape[0]
        return f(B, 4, 4), f(B, 4, 4), f(B, 3)

    @torch.library.register_fake("gsr::pose_virtual_view")
    def _(pose0, pose1, alpha, base=None):
        return pose0.new_empty((4, 4), dtype=torch.float32), pose0.new_empty((4, 4) if base is not None else (0,), dtype=torch.float32)

    @torch.library.register_fake("gsr::resize_plan")
    def _(flags):
        return (flags.new_empty((lib.gsr_resize_plan_bytes(int(flags.shape[0])) // 4,), dtype=torch.int32),
                flags.new_empty((L.GSR_RESIZE_META_WORDS,), dtype=torch.int64))

    @torch.library.register_fake("gsr::resize_apply")
    def _(plan, meta, N, nA, nB, nC, nSplit, src, kinds, child, check=False):
        return [t.new_empty((nA + nB + 2 * nC,) + tuple(t.shape[1:])) for t in src]

    @torch.library.register_fake("gsr::resize_plan_batched")
    def _(flags, first_block, counts):
        return (flags.new_empty((lib.gsr_resize_plan_bytes(int(flags.shape[0])) // 4,), dtype=torch.int32),
                flags.new_empty((len(counts), L.GSR_RESIZE_META_WORDS), dtype=torch.int64))

    @torch.library.register_fake("gsr::resize_apply_batched")
    def _(plan, meta, first_block, counts, counts4, new_first_block, src, kinds, child, pad, check=False):
        return [t.new_empty((L.GSR_RESIZE_BLOCK * new_first_block[-1],) + tuple(t.shape[1:])) for t in src]

    @torch.library.register_fake("gsr::select_smallest")
    def _(values, k):
        n = values.shape[0]
        return (values.new_empty((n,), dtype=torch.uint8), values.new_empty((n,), dtype=torch.uint8),
                values.new_empty((L.GSR_SELECT_META_WORDS,), dtype=torch.int64))

    @torch.library.register_fake("gsr::merge_apply")
    def _(plan_a, plan_b, meta, Na, nA, Nb, nB, src_a, src_b, kinds, check=False):
        return [t.new_empty((nA + nB,) + tuple(t.shape[1:])) for t in src_a]
