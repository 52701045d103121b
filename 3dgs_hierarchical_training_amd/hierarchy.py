"""Merge step of the hierarchical trainer on top of the MI355X rasterizer.

Mirrors, without importing the reference:
  * `HTGaussianTrainer.calc_importance`  /root/reference/trainer/ht3dgs_trainer.py:1427-1462 -- per view,
    loss = rendering.sum() on the clamped image, |grad| of `_features_dc` / `_features_rest` accumulated over the
    views (the `register_hook(lambda g: g.abs())` of :1436-1437), divided by the number of pixels;
  * `merge_two_3DGS`                     :214-272 -- amax over the 48 coefficients, `topk(largest=False)` of
    `prune_ratio * N` marks the Gaussians to drop on BOTH sides, source points moved by the 4x4, append.
Multi-GPU (segments.py): each child's importance is computed on its home rank (both ranks of a pair work in
parallel), the source ships its **un-pruned** child with the drop mask, and the mask is applied at the destination --
which therefore also holds both un-pruned children as the frozen teachers of `train_nonleaf_3DGS_phase1`
(:757, :866-883).  No collective is involved.
"""
import os
import time
from typing import Dict, List, Optional

import torch

from . import segments
from .rasterizer import (GaussianRasterizationSettings, importance_accumulate, importance_accumulate_views, rasterize_gaussians_raw,
                         render_gaussians_raw)


def _elapsed_ms(t0: float, ref: torch.Tensor) -> float:
    if ref.is_cuda:
        torch.cuda.synchronize(ref.device)
    return 1e3 * (time.perf_counter() - t0)


def render_raw(seg: Dict[str, torch.Tensor], rs: GaussianRasterizationSettings) -> torch.Tensor:
    """Clamped image of a frozen model given by its six raw tensors (the teacher render of :877-883)."""
    # the render-only forward: the kernel's own clamped image (bit-identical with `color.clamp(0, 1)`, NaN stays NaN), no zero means2D,
    # no state planes, checkpoints or binning buffer behind it -- nobody runs a backward over a teacher
    return render_gaussians_raw(seg["_xyz"], seg["_features_dc"], seg["_features_rest"], seg["_opacity"], seg["_scaling"],
                                seg["_rotation"], rs, clamped=True)[4]


# Which route calc_importance takes when its caller names none: "kernel" (a forward and the importance pass per view, include/gsr.h
# gsr_importance_accumulate) or "autograd" (a render and a full backward per view).  Chosen by tools/importance_probe.py's rule: the
# kernel route's median lies below the autograd route's by more than the same-arm spread at the headline scene and at stage A's size,
# on dark and on brightened scenes (profiles/importance_probe.txt: 4.28 against 6.97 ms and 1.97 against 3.03 ms per eight views;
# DESIGN.md section 6).  GSR_IMPORTANCE_ROUTE=autograd in the environment puts the old route back under every caller (A/B runs).
DEFAULT_IMPORTANCE_ROUTE = os.environ.get("GSR_IMPORTANCE_ROUTE", "kernel")
IMPORTANCE_ROUTES = ("kernel", "autograd")
if DEFAULT_IMPORTANCE_ROUTE not in IMPORTANCE_ROUTES:
    raise ValueError(f"GSR_IMPORTANCE_ROUTE={DEFAULT_IMPORTANCE_ROUTE!r}: one of {IMPORTANCE_ROUTES}")

# How many views of a model one call of the kernel route takes (include/gsr.h gsr_importance_accumulate_views): 1 = a forward and a pass
# per view, the route as it was; 2..16 = runs of views that share their frame go through ONE launch chain and one host wait.  The
# default stays 1 whatever tools/importance_views_probe.py measures (profiles/importance_views.txt): changing it is
# a decision of its own that cites that file.  VIEWS_MAX_RECORDS bounds what one call keeps alive -- V images of pixel state and V * Npad
# splat records: at most 8 Mi records, 8 views at 1 M Gaussians.
DEFAULT_IMPORTANCE_VIEWS = int(os.environ.get("GSR_IMPORTANCE_VIEWS", "1"))
MAX_VIEWS_PER_CALL = 16
VIEWS_MAX_RECORDS = 8 * 2 ** 20
if not 1 <= DEFAULT_IMPORTANCE_VIEWS <= MAX_VIEWS_PER_CALL:
    raise ValueError(f"GSR_IMPORTANCE_VIEWS={DEFAULT_IMPORTANCE_VIEWS}: 1..{MAX_VIEWS_PER_CALL}")

_SH_C0 = 0.28209479177387814
_SH_C1 = 0.4886025119029199
_SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
_SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
          -0.5900435899266435)


def sh_basis(dirs: torch.Tensor, degree: int) -> torch.Tensor:
    """[N, (degree+1)^2] real SH basis in the unit directions `dirs` [N,3]: the factors that multiply the coefficients in the
    kernels' colour evaluation (csrc/gsr_math.h sh_channel / sh_basis_dir), in `dirs`' dtype."""
    x, y, z = dirs[:, 0], dirs[:, 1], dirs[:, 2]
    b = [torch.full_like(x, _SH_C0)]
    if degree > 0:
        b += [-_SH_C1 * y, _SH_C1 * z, -_SH_C1 * x]
    if degree > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        b += [_SH_C2[0] * xy, _SH_C2[1] * yz, _SH_C2[2] * (2 * zz - xx - yy), _SH_C2[3] * xz, _SH_C2[4] * (xx - yy)]
    if degree > 2:
        b += [_SH_C3[0] * y * (3 * xx - yy), _SH_C3[1] * xy * z, _SH_C3[2] * y * (4 * zz - xx - yy),
              _SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy), _SH_C3[4] * x * (4 * zz - xx - yy), _SH_C3[5] * z * (xx - yy),
              _SH_C3[6] * x * (xx - 3 * yy)]
    return torch.stack(b, 1)


def importance_from_sums(S: torch.Tensor, dirs: torch.Tensor, colours: torch.Tensor, degree: int, M: int) -> torch.Tensor:
    """One view's |dL/dSH| [N, M, 3] for L = sum clamp(image, 0, 1), from the per-Gaussian sums the importance pass takes:

        |dL/dSH[n,k,c]| = |basis_k(dirs_n)| * [colours[n,c] > 0] * S[n,c],   S[n,c] = sum_pixels alpha T [0 <= out_color_c <= 1]

    (S >= 0; "colour > 0" says that channel's SH colour was not clamped at 0).  The finishing kernel's formula
    (csrc/gsr_kernels.hip k_importance_finish) in torch, in the kernel's order of operations: b = |basis_k|, then b * S[n,c] where the
    gate is open, nothing where it is closed; coefficients k >= (degree+1)^2 stay zero.  Any device, any float dtype: S, dirs [N,3]
    (unit view directions) and colours [N,3] are used in S's dtype."""
    nc = (degree + 1) ** 2
    if M < nc:
        raise ValueError(f"M = {M} stored coefficients cannot hold degree {degree}")
    b = sh_basis(dirs.to(S.dtype), degree).abs()                       # [N, nc]
    gated = torch.where(colours.to(S.device) > 0, S, torch.zeros_like(S))   # [N, 3]
    out = S.new_zeros((S.shape[0], M, 3))
    out[:, :nc] = b[:, :, None] * gated[:, None, :]
    return out


def _calc_importance_autograd(seg, views):
    dc = seg["_features_dc"].detach().clone().requires_grad_(True)
    rest = seg["_features_rest"].detach().clone().requires_grad_(True)
    acc_dc, acc_rest = torch.zeros_like(dc), torch.zeros_like(rest)
    num_pixels = 0
    for rs in views:
        dc.grad = rest.grad = None
        m2d = torch.zeros_like(seg["_xyz"])
        color = rasterize_gaussians_raw(seg["_xyz"].detach(), m2d, dc, rest, seg["_opacity"].detach(),
                                        seg["_scaling"].detach(), seg["_rotation"].detach(), rs)[0]
        color.clamp(0, 1).sum().backward()
        acc_dc += dc.grad.abs()
        acc_rest += rest.grad.abs()
        num_pixels += int(rs.image_height) * int(rs.image_width)
    return (torch.cat([acc_dc, acc_rest], 1).flatten(-2) / max(num_pixels, 1)).detach()


def _calc_importance_kernel(seg, views, points_transform=None, sh_origin=None, view_id=0):
    """Per view one forward plus the importance pass into ONE [N, M, 3] accumulator; the single division by the pixel count at the end."""
    dc, rest = seg["_features_dc"].detach(), seg["_features_rest"].detach()
    acc = torch.zeros((dc.shape[0], dc.shape[1] + rest.shape[1], 3), dtype=torch.float32, device=dc.device)
    num_pixels = 0
    for rs in views:
        importance_accumulate(acc, seg["_xyz"], dc, seg["_opacity"], seg["_scaling"], seg["_rotation"], rs, sh_rest=rest,
                              raw_params=True, points_transform=points_transform, sh_origin=sh_origin, view_id=view_id)
        num_pixels += int(rs.image_height) * int(rs.image_width)
    return acc.flatten(-2) / max(num_pixels, 1)


def _same_frame(a: GaussianRasterizationSettings, b: GaussianRasterizationSettings) -> bool:
    """Do two views share what gsr_forward_views shares: image size, field of view, SH degree, scale modifier and background?"""
    if (int(a.image_height), int(a.image_width), float(a.tanfovx), float(a.tanfovy), int(a.sh_degree), float(a.scale_modifier)) != \
            (int(b.image_height), int(b.image_width), float(b.tanfovx), float(b.tanfovy), int(b.sh_degree), float(b.scale_modifier)):
        return False
    return a.bg is b.bg or (a.bg.shape == b.bg.shape and a.bg.device == b.bg.device and bool(torch.equal(a.bg, b.bg)))


def group_views(views, per_call: int, N: int) -> List[List[int]]:
    """The call plan of the kernel route: the indices of `views`, in order, cut into the groups one call each takes.  Consecutive views that
    agree in image_height, image_width, tanfovx, tanfovy, sh_degree, scale_modifier and bg (the same tensor, or equal values) form a
    run; a run is cut into groups of at most min(per_call, 16, max(1, VIEWS_MAX_RECORDS // Npad)) views, Npad = 128 ceil(N / 128).  A
    group of one view goes through the single-view call.  Pure: nothing is rendered."""
    if per_call < 1:
        raise ValueError(f"group_views: per_call must be at least 1, got {per_call}")
    npad = max(128, (int(N) + 127) // 128 * 128)
    cap = min(int(per_call), MAX_VIEWS_PER_CALL, max(1, VIEWS_MAX_RECORDS // npad))
    plan: List[List[int]] = []
    for i, rs in enumerate(views):
        if plan and len(plan[-1]) < cap and _same_frame(views[plan[-1][0]], rs):
            plan[-1].append(i)
        else:
            plan.append([i])
    return plan


def stack_views(views, device) -> GaussianRasterizationSettings:
    """One settings tuple for the views of a group (what batched.batch_settings returns): cameras [V,4,4], [V,4,4], [V,3]."""
    v0 = views[0]
    return v0._replace(viewmatrix=torch.stack([v.viewmatrix.to(device).float() for v in views]).contiguous(),
                       projmatrix=torch.stack([v.projmatrix.to(device).float() for v in views]).contiguous(),
                       campos=torch.stack([v.campos.to(device).float() for v in views]).contiguous())


def _calc_importance_views(seg, views, per_call):
    """The kernel route with up to `per_call` views per launch chain (group_views): ONE [N, M, 3] accumulator that the groups add into in
    view order, the single division by the pixel count at the end."""
    dc, rest = seg["_features_dc"].detach(), seg["_features_rest"].detach()
    acc = torch.zeros((dc.shape[0], dc.shape[1] + rest.shape[1], 3), dtype=torch.float32, device=dc.device)
    num_pixels = 0
    for group in group_views(views, per_call, dc.shape[0]):
        if len(group) == 1:
            importance_accumulate(acc, seg["_xyz"], dc, seg["_opacity"], seg["_scaling"], seg["_rotation"], views[group[0]], sh_rest=rest,
                                  raw_params=True)
        else:
            importance_accumulate_views(acc, seg["_xyz"], dc, seg["_opacity"], seg["_scaling"], seg["_rotation"],
                                        stack_views([views[i] for i in group], dc.device), sh_rest=rest, raw_params=True)
        num_pixels += sum(int(views[i].image_height) * int(views[i].image_width) for i in group)
    return acc.flatten(-2) / max(num_pixels, 1)


def calc_importance(seg: Dict[str, torch.Tensor], views: List[GaussianRasterizationSettings], route: Optional[str] = None,
                    views_per_call: Optional[int] = None) -> torch.Tensor:
    """[N, 48] colour importance of a segment over `views` (each a full raster-settings tuple), entry k * 3 + c.
    route: "autograd" = per view a render and a full backward, |grad| of the SH tensors; "kernel" = per view a forward and the
    importance pass (no backward, no autograd, no .grad left anywhere); None = DEFAULT_IMPORTANCE_ROUTE.
    views_per_call: how many views one launch chain of the kernel route takes (group_views); 1 = the per-view route, 2..16 = the views
    entry (gsr_importance_accumulate_views); None = DEFAULT_IMPORTANCE_VIEWS (GSR_IMPORTANCE_VIEWS, 1).  The autograd route takes 1 only."""
    route = DEFAULT_IMPORTANCE_ROUTE if route is None else route
    if route not in IMPORTANCE_ROUTES:
        raise ValueError(f"calc_importance: unknown route {route!r} (one of {IMPORTANCE_ROUTES})")
    per_call = DEFAULT_IMPORTANCE_VIEWS if views_per_call is None else int(views_per_call)
    if not 1 <= per_call <= MAX_VIEWS_PER_CALL:
        raise ValueError(f"calc_importance: views_per_call must be 1..{MAX_VIEWS_PER_CALL}, got {per_call}")
    if route == "autograd":
        if per_call > 1:
            raise ValueError("calc_importance: views_per_call > 1 is served by the kernel route only (route='autograd' renders view by view)")
        return _calc_importance_autograd(seg, views)
    return _calc_importance_kernel(seg, views) if per_call == 1 else _calc_importance_views(seg, views, per_call)


def prune_mask(importance: torch.Tensor, prune_ratio: float, route: str = "torch") -> torch.Tensor:
    """True = dropped: the `prune_ratio * N` Gaussians with the smallest max-over-coefficients importance
    (ht3dgs_trainer.py:234-239).

    route: "torch" = amax, topk, a zero fill and an indexed store; "kernel" = gsr_select_smallest on the [N, 3 M] tensor as it is (merge.py;
    no amax launch, no host wait).  With distinct scores both give the same mask; among rows tied at the threshold the kernel route drops
    those with the lowest row numbers, where topk promises no rule.  The kernel route has no CPU fallback."""
    from . import merge
    if merge.check_route(route, "prune_mask") == "kernel":
        merge.need_device("prune_mask", importance=importance)
        values = importance.reshape(importance.shape[0], -1) if importance.dim() > 1 else importance
        return merge.select_smallest(values, int(values.shape[0] * prune_ratio))[0]
    score = importance.amax(-1).reshape(-1)
    k = int(score.shape[0] * prune_ratio)
    mask = torch.zeros_like(score, dtype=torch.bool)
    if k > 0:
        mask[torch.topk(score, k, largest=False).indices] = True
    return mask


def merge_send(tr, dst: int, seg: Dict[str, torch.Tensor], views, prune_ratio: float, frames=None, poses=None,
               start_fidx: int = 0, global_iteration: int = 0, importance_fn=calc_importance, drop=None, sh_degree: int = -1,
               route: str = "torch") -> Dict:
    """Source side of one pair: own importance -> drop mask; ship the UN-PRUNED child + mask + frames / poses.
    `drop`: a mask computed beforehand (then `views` is not used).  route: prune_mask's."""
    t0 = time.perf_counter()
    if drop is None:
        drop = prune_mask(importance_fn(seg, views), prune_ratio, route=route)
    imp_ms = _elapsed_ms(t0, seg["_xyz"])
    st = segments.send_child(tr, dst, seg, drop=drop, frames=frames, poses=poses, start_fidx=start_fidx,
                             global_iteration=global_iteration, sh_degree=sh_degree)
    return {"role": "src", "peer": dst, "importance_ms": imp_ms, "send_ms": st["ms"], "bytes": st["bytes"],
            "n": int(seg["_xyz"].shape[0]), "n_dropped": int(drop.sum())}


def merge_recv(tr, src: int, seg: Dict[str, torch.Tensor], views, prune_ratio: float, src_to_dst=None,
               importance_fn=calc_importance, drop=None, route: str = "torch") -> Dict:
    """Destination side: own importance (in parallel with the source's), receive the un-pruned child, apply both masks,
    move the child's points by `src_to_dst` (a [4,4] or a callable(child_message) -> [4,4]) and append.
    route: prune_mask's and segments.merge_segments'.

    Returns {'merged', 'teachers': [own un-pruned, child un-pruned], 'child': message, stats...}."""
    t0 = time.perf_counter()
    drop_dst = drop if drop is not None else prune_mask(importance_fn(seg, views), prune_ratio, route=route)
    imp_ms = _elapsed_ms(t0, seg["_xyz"])
    msg = segments.recv_child(tr, src, seg["_xyz"].device)
    child = msg["seg"]
    drop_src = msg["drop"] if msg["drop"] is not None else torch.zeros(child["_xyz"].shape[0], dtype=torch.bool,
                                                                         device=child["_xyz"].device)
    T = src_to_dst(msg) if callable(src_to_dst) else src_to_dst
    t1 = time.perf_counter()
    merged = segments.merge_segments(seg, child, ~drop_dst, ~drop_src, T, route=route)
    own = {k: seg[k].detach() for k in segments.SEGMENT_KEYS}
    return {"role": "dst", "peer": src, "merged": merged, "teachers": [own, child], "child": msg,
            "importance_ms": imp_ms, "recv_ms": msg["ms"], "bytes": msg["bytes"],
            "append_ms": _elapsed_ms(t1, seg["_xyz"]), "n": int(seg["_xyz"].shape[0]), "n_child": int(child["_xyz"].shape[0]),
            "n_merged": int(merged["_xyz"].shape[0]), "n_dropped": int(drop_dst.sum()), "n_child_dropped": int(drop_src.sum())}


def merge_level(seg: Dict[str, torch.Tensor], views: List[GaussianRasterizationSettings], level_pairs, prune_ratio: float,
                src_to_dst: Optional[torch.Tensor] = None, importance_fn=calc_importance, group=None, transport=None,
                route: str = "torch"):
    """One level of the merge tree for this rank.  Returns the merged segment on destination ranks, None on
    source ranks (their GPU is free after the send), and the unchanged segment on ranks idle at this level.
    route: merge_send's and merge_recv's."""
    from . import merge
    merge.check_route(route, "merge_level")
    tr = transport if transport is not None else segments.DistTransport(group)
    role = segments.partner(tr.rank, level_pairs)
    if role is None:
        return seg
    if role[0] == "send":
        merge_send(tr, role[1], seg, views, prune_ratio, importance_fn=importance_fn, route=route)
        return None
    return merge_recv(tr, role[1], seg, views, prune_ratio, src_to_dst, importance_fn=importance_fn, route=route)["merged"]
