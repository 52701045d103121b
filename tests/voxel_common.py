"""The float64 numpy oracle of the voxel grid and of the un-projection (include/gsr.h, version 118), and the clouds the tests hold the
kernels against.  The oracle restates Open3D's PointCloud::VoxelDownSample with a defined output order -- np.unique(axis=0) sorts the
index rows lexicographically, which IS the library's output order -- and accumulates sequentially in input order (np.add.at)."""
import numpy as np

INDEX_LIMIT = 2 ** 21


def voxel_oracle(points, colors, voxel_size):
    """points [N,3] float32, colors [N,3] float32 or None -> dict(points [M,3] f32, colors [M,3] f32 or None, counts [M] int64,
    dropped, status, index [M,3] int64)."""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    finite = np.isfinite(points).all(axis=1)
    dropped = int((~finite).sum())
    p = points[finite].astype(np.float64)
    c = None if colors is None else np.asarray(colors, dtype=np.float32).reshape(-1, 3)[finite].astype(np.float64)
    empty = dict(points=np.zeros((0, 3), np.float32), colors=None if colors is None else np.zeros((0, 3), np.float32),
                 counts=np.zeros((0,), np.int64), dropped=dropped, status=0, index=np.zeros((0, 3), np.int64))
    if p.shape[0] == 0:
        return empty
    origin = p.min(axis=0) - 0.5 * float(voxel_size)
    ref = np.floor((p - origin) / float(voxel_size))
    if (ref.max(axis=0) >= INDEX_LIMIT).any():
        return dict(empty, status=1)
    index = ref.astype(np.int64)
    uniq, inverse, counts = np.unique(index, axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    sums = np.zeros((uniq.shape[0], 3), np.float64)
    np.add.at(sums, inverse, p)
    out_c = None
    if c is not None:
        csum = np.zeros((uniq.shape[0], 3), np.float64)
        np.add.at(csum, inverse, c)
        out_c = (csum / counts[:, None]).astype(np.float32)
    return dict(points=(sums / counts[:, None]).astype(np.float32), colors=out_c, counts=counts.astype(np.int64), dropped=dropped,
                status=0, index=uniq)


def depth_to_points_oracle(depth, image, fx, fy, cx, cy):
    """The float32 formula, evaluated with torch on the CPU: x = ((u - cx) / fx) * d, y = ((v - cy) / fy) * d, z = d."""
    import torch
    depth = torch.as_tensor(depth, dtype=torch.float32)
    H, W = depth.shape
    f32 = lambda s: torch.tensor(s, dtype=torch.float32)
    u = torch.arange(W, dtype=torch.float32)[None, :].expand(H, W)
    v = torch.arange(H, dtype=torch.float32)[:, None].expand(H, W)
    x = ((u - f32(cx)) / f32(fx)) * depth
    y = ((v - f32(cy)) / f32(fy)) * depth
    pts = torch.stack((x, y, depth), dim=-1).reshape(-1, 3)
    cols = None if image is None else torch.as_tensor(image, dtype=torch.float32).permute(1, 2, 0).reshape(-1, 3).contiguous()
    return pts, cols


# ---- the hand-worked case: eight points, three voxels, voxel_size 0.5 -------------------------------------------------------------------
# min_bound = (0,0,0), origin = (-0.25,-0.25,-0.25); per axis [-0.25,0.25) -> 0, [0.25,0.75) -> 1, [0.75,1.25) -> 2.
HAND_VOXEL_SIZE = 0.5
HAND_POINTS = np.array([
    [0.5, 0.125, 0.125],      # (1,0,0)
    [0.0, 1.0, 0.0],          # (0,2,0)
    [0.0, 0.0, 0.0],          # (0,0,0): exactly at min_bound, (p - origin) / voxel_size = 0.5 on every axis
    [0.25, 0.0, 0.0],         # (1,0,0): x exactly on the face between voxels 0 and 1, (p - origin) / voxel_size = 1.0
    [0.125, 0.125, 0.0],      # (0,0,0)
    [0.125, 0.875, 0.125],    # (0,2,0)
    [0.625, 0.0, 0.0],        # (1,0,0)
    [0.0, 0.0, 0.125],        # (0,0,0)
], dtype=np.float32)
HAND_COLORS = np.array([[0.5, 0, 0], [0, 1, 0], [0, 0, 0], [1, 0, 0], [0.25, 0, 0.5], [0, 0.5, 0], [0, 0, 0], [0.5, 0, 1]], dtype=np.float32)
HAND_INDEX = np.array([[0, 0, 0], [0, 2, 0], [1, 0, 0]])
HAND_COUNTS = np.array([3, 2, 3])
HAND_MEANS = np.array([[0.125 / 3, 0.125 / 3, 0.125 / 3], [0.0625, 0.9375, 0.0625], [1.375 / 3, 0.125 / 3, 0.125 / 3]]).astype(np.float32)
HAND_COLOR_MEANS = np.array([[0.25, 0, 0.5], [0, 0.75, 0], [0.5, 0, 0]]).astype(np.float32)


# ---- the clouds of tests/test_gpu_voxel.py: name -> (points f32, colors f32 or None, voxel_size) ----------------------------------------
def _uniform(n, seed, lo=-1.0, hi=1.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, (n, 3)).astype(np.float32), rng.uniform(0, 1, (n, 3)).astype(np.float32)


def _lattice():
    # min 0, voxel_size 0.5 -> origin -0.25, faces at 0.25, 0.75, ...: every non-zero coordinate sits exactly on a face
    g = np.array([0.0, 0.25, 0.75, 1.25, 1.75], dtype=np.float32)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    pts = np.concatenate((pts, pts[::-1]))
    return pts, np.random.default_rng(5).uniform(0, 1, pts.shape).astype(np.float32)


def _with_nonfinite(n, seed):
    pts, cols = _uniform(n, seed)
    rng = np.random.default_rng(seed + 1)
    rows = rng.choice(n, n // 20, replace=False)
    pts[rows, rng.integers(0, 3, rows.shape[0])] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), rows.shape[0])
    return pts, cols


def _far_pair(d, axes):
    pts = np.zeros((2, 3), np.float32)
    pts[1, axes] = d
    return pts, np.array([[0.25, 0.5, 0.75], [1.0, 0.0, 0.5]], np.float32)


def _build_cases():
    u20k = _uniform(20000, 20)
    one = np.random.default_rng(13).uniform(1.0, 1.004, (13000, 3)).astype(np.float32)      # spread < voxel_size / 2: one voxel
    mixed = (np.random.default_rng(9).standard_normal((3000, 3)) * 2.0 - 1.0).astype(np.float32)
    return {
        "n1": (np.array([[0.3, -0.2, 1.5]], np.float32), np.array([[0.1, 0.2, 0.3]], np.float32), 0.01),
        "two_identical": (np.full((2, 3), 0.7, np.float32), np.array([[0.0, 0.5, 1.0], [1.0, 0.5, 0.25]], np.float32), 0.01),
        "n64": _uniform(64, 64) + (0.25,),
        "n65": _uniform(65, 65) + (0.25,),
        "n4096": _uniform(4096, 4096) + (0.1,),
        "n4097": _uniform(4097, 4097) + (0.1,),
        "uniform_fine": u20k + (0.05,),
        "uniform_coarse": u20k + (0.5,),
        "one_voxel_13000": (one, np.random.default_rng(14).uniform(0, 1, one.shape).astype(np.float32), 0.01),
        "lattice_on_faces": _lattice() + (0.5,),
        "mixed_sign": (mixed, np.random.default_rng(10).uniform(0, 1, mixed.shape).astype(np.float32), 0.1),
        "extent_30": _uniform(5000, 30, -15.0, 15.0) + (0.01,),
        "index_just_under_2_21": _far_pair(20971.0, [0, 1, 2]) + (0.01,),
        "five_percent_nonfinite": _with_nonfinite(5000, 50) + (0.1,),
        "no_colors": (_uniform(3000, 77)[0], None, 0.1),
    }


CASES = _build_cases()
OVERFLOW_CASE = _far_pair(20973.0, [1]) + (0.01,)       # an index past 2^21 on the y axis: status 1
_ORACLE = {}


def oracle_of(name):
    """The oracle's answer for CASES[name]: computed once, shared, never modified."""
    if name not in _ORACLE:
        p, c, vs = CASES[name]
        r = voxel_oracle(p, c, vs)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _ORACLE[name] = r
    return _ORACLE[name]


def assert_within_one_ulp(got, ref, what):
    """|got - ref| <= one float32 ulp of ref (np.spacing), element for element."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if got.size == 0:
        return 0
    diff = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    ulp = np.abs(np.spacing(ref)).astype(np.float64)
    bad = diff > ulp
    assert not bad.any(), f"{what}: {int(bad.sum())} of {got.size} elements beyond one ulp, worst {float((diff / ulp).max()):.2f} ulp"
    return int((diff > 0).sum())
