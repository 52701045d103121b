"""The single-image model's initialisation on the device: depth map -> points -> voxel-grid means -> Gaussians.

The reference builds it on the host for every frame of stage A and every leaf (/root/reference/trainer/trainer.py:646-671, reached from
ht3dgs_trainer.py:188, :360, :398): `kornia.depth_to_3d`, a copy of the H*W points to the host, `open3d` (`estimate_normals`, whose
normals nothing reads, then `voxel_down_sample(voxel_size=0.01)`), a copy back, then `create_from_pcd`
(/root/reference/scene/gaussian_model_ht.py:197-233).  Here the chain stays on the device and needs neither library:

  depth_to_points     gsr_depth_to_points      (csrc/voxel_kernels.hip; semantics in include/gsr.h)
  voxel_down_sample   gsr_voxel_down_sample    (defined output order, fixed summation order: repeatable bit for bit)
  scene_from_points   create_from_pcd with distCUDA2 = gsr_knn_mean_dist2
  scene_from_depth    the three composed

The first two restate kornia's and Open3D's public definitions; neither library is available to the tests, so they are not pinned
against a run of them.  No CPU fallback: a CPU tensor raises RuntimeError before a device is touched.
"""
from typing import Dict, Optional, Sequence, Tuple, Union

import torch

C0 = 0.28209479177387814      # SH band 0 (the reference's utils/sh_utils.py RGB2SH)

Intrinsics = Union[torch.Tensor, Sequence[float]]


def _need_device(name: str, **tensors):
    for k, t in tensors.items():
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise RuntimeError(f"{name}: {k} must be a tensor on a ROCm/HIP device -- there is no CPU fallback")


def _fx_fy_cx_cy(intrinsics: Intrinsics) -> Tuple[float, float, float, float]:
    """(fx, fy, cx, cy) from a 3x3 matrix (tensor, array or nested list) or from the four numbers."""
    if isinstance(intrinsics, torch.Tensor):
        k = intrinsics.detach().to("cpu", torch.float64)
    else:
        k = torch.as_tensor(intrinsics, dtype=torch.float64)
    if tuple(k.shape) == (3, 3):
        return float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])
    if tuple(k.shape) == (4,):
        return tuple(float(v) for v in k)
    raise ValueError("intrinsics: a 3x3 matrix or (fx, fy, cx, cy)")


def depth_to_points(depth: torch.Tensor, image: Optional[torch.Tensor], intrinsics: Intrinsics) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Un-project every pixel of `depth` [H,W]: x = ((u - cx) / fx) * d, y = ((v - cy) / fy) * d, z = d in float32, row-major
    [H*W,3]; the colours of `image` [3,H,W] gathered beside them as [H*W,3] (None without an image).  No autograd."""
    _need_device("depth_to_points", depth=depth, image=image)
    fx, fy, cx, cy = _fx_fy_cx_cy(intrinsics)
    if fx == 0.0 or fy == 0.0:
        raise ValueError("depth_to_points: fx and fy must not be 0")
    from . import _ext
    points, colors = _ext.load().depth_to_points(depth.detach(), None if image is None else image.detach(), fx, fy, cx, cy)
    return points, (colors if image is not None else None)


def voxel_down_sample(points: torch.Tensor, colors: Optional[torch.Tensor] = None, voxel_size: float = 0.01,
                      return_counts: bool = False):
    """One point (and colour) per occupied voxel of a grid of `voxel_size`: the float64 mean of the voxel's points, rounded once to
    float32, in ascending (ix, iy, iz) order.  Rows with a non-finite coordinate are dropped.  Returns (points [M,3], colors [M,3] or
    None); with return_counts also (counts [M] int32, dropped).  Raises RuntimeError when extent / voxel_size needs an index of 2^21
    or more.  One host synchronisation (M is read back).  No autograd."""
    _need_device("voxel_down_sample", points=points, colors=colors)
    from . import _ext
    p, c, counts, dropped = _ext.load().voxel_down_sample(points.detach(), None if colors is None else colors.detach(), float(voxel_size))
    c = c if colors is not None else None
    return (p, c, counts, int(dropped)) if return_counts else (p, c)


def scene_from_points(points: torch.Tensor, colors: torch.Tensor, sh_degree_stored: int = 3) -> Dict:
    """`create_from_pcd` (/root/reference/scene/gaussian_model_ht.py:197-233) on the device, as the scene dict `GaussianParams` takes
    (activated values: it applies log / inverse sigmoid itself): SH band 0 = RGB2SH(colour), the other coefficients 0; scales =
    sqrt(clamp_min(distCUDA2(points), 1e-7)) on all three axes; identity rotations; opacity 0.1; active SH degree 0."""
    _need_device("scene_from_points", points=points, colors=colors)
    from . import _ext
    points = points.detach().float().contiguous()
    n = points.shape[0]
    dist2 = _ext.load().knn_mean_dist2(points).clamp_min(1e-7)
    shs = torch.zeros((n, (sh_degree_stored + 1) ** 2, 3), dtype=torch.float32, device=points.device)
    shs[:, 0] = (colors.detach().float() - 0.5) / C0
    rotations = torch.zeros((n, 4), dtype=torch.float32, device=points.device)
    rotations[:, 0] = 1.0
    return dict(means3D=points, shs=shs, scales=torch.sqrt(dist2)[:, None].repeat(1, 3),
                rotations=rotations, opacities=torch.full((n, 1), 0.1, dtype=torch.float32, device=points.device),
                sh_degree=0, bg=torch.zeros(3), scale_modifier=1.0)


def scene_from_depth(depth: torch.Tensor, image: torch.Tensor, intrinsics: Intrinsics, voxel_size: float = 0.01) -> Dict:
    """scene_from_points(voxel_down_sample(depth_to_points(depth, image, intrinsics), voxel_size)).  The depth is used as given: the
    caller clamps it to its near plane as the reference does (trainer.py:637)."""
    _need_device("scene_from_depth", depth=depth, image=image)
    if image is None:
        raise ValueError("scene_from_depth: an image is needed for the colours")
    points, colors = depth_to_points(depth, image, intrinsics)
    points, colors = voxel_down_sample(points, colors, voxel_size)
    return scene_from_points(points, colors)
