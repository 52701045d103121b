"""What the device-camera tests share: a numpy float64 oracle of gsr_camera_from_pose and gsr_pose_virtual_view (include/gsr.h, version 119),
the bar the kernels are held to, the host float32 route as a yardstick, and the poses the tests use.

The oracle restates the header's statements scalar by scalar, in the header's operation order and without a fused multiply-add (no `@`: a
BLAS may fuse).  For gsr_camera_from_pose the kernel runs the same IEEE operations, so its float64 results -- and their float32 roundings --
are the oracle's.  gsr_pose_virtual_view also calls sin / cos / acos, whose device and host implementations may differ in the last float64
bit.

THE BARS.  gsr_camera_from_pose has no such call: its outputs are held to BIT EQUALITY with the oracle's values rounded to float32
(`assert_bit_equal`), which is inside the issue's one float32 ulp.  An output x of gsr_pose_virtual_view is held to (`assert_one_ulp`)

    |x - f32(oracle)| <= ulp32(f32(oracle)) + 64 * 2^-53 * S,      S = max(1, the largest |entry| of the inputs)

The first term is the issue's one float32 ulp: the kernel rounds a float64 result once.  The second is the float64 oracle's OWN rounding
error, which no evaluation in float64 escapes: each output is a sum of at most a few dozen products of magnitude <= S (a handful of 3x3
products and adjugates chained), each rounded to 2^-53 relative, and an entry that is small only by cancellation carries the error of the
terms that cancelled, not of its own size.  64 * 2^-53 * S is 7e-15 for S = 1: eight orders below one float32 ulp of any entry above
1e-7, so for every entry that is not such a cancellation the bar IS one float32 ulp.
"""
import math

import numpy as np

ZNEAR, ZFAR = 0.01, 100.0


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------
def _adj3(m):
    """(adjugate [3][3] as python floats, determinant) of the 3x3 block of a 4x4, in the header's order."""
    a00, a01, a02, a10, a11, a12, a20, a21, a22 = (float(m[i][j]) for i in range(3) for j in range(3))
    adj = [[a11 * a22 - a12 * a21, a02 * a21 - a01 * a22, a01 * a12 - a02 * a11],
           [a12 * a20 - a10 * a22, a00 * a22 - a02 * a20, a02 * a10 - a00 * a12],
           [a10 * a21 - a11 * a20, a01 * a20 - a00 * a21, a00 * a11 - a01 * a10]]
    return adj, (a00 * adj[0][0] + a01 * adj[1][0]) + a02 * adj[2][0]


def projection(fx, fy, cx, cy, W, H, znear=ZNEAR, zfar=ZFAR):
    """P of include/gsr.h (scene/cameras.py:87-90), float64 from the arguments as given."""
    fx, fy, cx, cy, w, h, znear, zfar = (float(v) for v in (fx, fy, cx, cy, W, H, znear, zfar))
    return [[2.0 * fx / w, 0.0, -(w - 2.0 * cx) / w, 0.0], [0.0, 2.0 * fy / h, -(h - 2.0 * cy) / h, 0.0],
            [0.0, 0.0, zfar / (zfar - znear), -(zfar * znear) / (zfar - znear)], [0.0, 0.0, 1.0, 0.0]]


def camera_oracle(pose, fx, fy, cx, cy, W, H, znear=ZNEAR, zfar=ZFAR):
    """pose [B,4,4] (or [4,4]) float32 -> dict of float64 arrays view [B,4,4], proj [B,4,4], campos [B,3] (squeezed for a [4,4] pose)."""
    pose = np.asarray(pose, dtype=np.float32)
    single = pose.ndim == 2
    poses = pose.reshape(-1, 4, 4)
    P = projection(fx, fy, cx, cy, W, H, znear, zfar)
    view, proj, campos = (np.zeros((len(poses), 4, 4)), np.zeros((len(poses), 4, 4)), np.zeros((len(poses), 3)))
    for b, p32 in enumerate(poses):
        p = [[float(p32[i][j]) for j in range(4)] for i in range(4)]
        for i in range(4):
            for j in range(4):
                view[b, i, j] = p[j][i]
                proj[b, i, j] = ((p[0][i] * P[j][0] + p[1][i] * P[j][1]) + p[2][i] * P[j][2]) + p[3][i] * P[j][3]
        adj, det = _adj3(p)
        t = (p[0][3], p[1][3], p[2][3])
        for i in range(3):
            campos[b, i] = -(((adj[i][0] * t[0] + adj[i][1] * t[1]) + adj[i][2] * t[2]) / det)
    out = dict(view=view, proj=proj, campos=campos)
    return {k: v[0] for k, v in out.items()} if single else out


def _affine_inverse(m):
    adj, det = _adj3(m)
    inv = [[adj[i][j] / det for j in range(3)] for i in range(3)]
    out = [[inv[i][0], inv[i][1], inv[i][2], -((inv[i][0] * m[0][3] + inv[i][1] * m[1][3]) + inv[i][2] * m[2][3])] for i in range(3)]
    return out + [[0.0, 0.0, 0.0, 1.0]]


def _affine_mul(x, y):
    out = []
    for i in range(3):
        row = [(x[i][0] * y[0][j] + x[i][1] * y[1][j]) + x[i][2] * y[2][j] for j in range(3)]
        row.append(((x[i][0] * y[0][3] + x[i][1] * y[1][3]) + x[i][2] * y[2][3]) + x[i][3])
        out.append(row)
    return out + [[0.0, 0.0, 0.0, 1.0]]


def _so3_exp_and_v(phi):
    th2 = (phi[0] * phi[0] + phi[1] * phi[1]) + phi[2] * phi[2]
    if th2 < 1e-8:
        a, b, c = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        th = math.sqrt(th2)
        a, b, c = math.sin(th) / th, (1.0 - math.cos(th)) / th2, (th - math.sin(th)) / (th2 * th)
    K = [[0.0, -phi[2], phi[1]], [phi[2], 0.0, -phi[0]], [-phi[1], phi[0], 0.0]]
    K2 = [[(K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j] for j in range(3)] for i in range(3)]
    eye = lambda i, j: 1.0 if i == j else 0.0
    R = [[(eye(i, j) + a * K[i][j]) + b * K2[i][j] for j in range(3)] for i in range(3)]
    V = [[(eye(i, j) + b * K[i][j]) + c * K2[i][j] for j in range(3)] for i in range(3)]
    return R, V


def virtual_view_oracle(pose0, pose1, alpha, base=None):
    """float64 [4,4] of pose0 Exp(alpha Log(pose0^-1 pose1)), and of that times base^-1 (None without a base)."""
    f = lambda m: [[float(v) for v in row] for row in np.asarray(m, dtype=np.float32).reshape(4, 4)]
    p0, p1, alpha = f(pose0), f(pose1), float(alpha)
    rel = _affine_mul(_affine_inverse(p0), p1)
    cosv = min(1.0, max(-1.0, (((rel[0][0] + rel[1][1]) + rel[2][2]) - 1.0) * 0.5))
    th = math.acos(cosv)
    k = 1.0 + th * th / 6.0 if th < 1e-4 else th / math.sin(th)
    phi = [k * ((rel[2][1] - rel[1][2]) * 0.5), k * ((rel[0][2] - rel[2][0]) * 0.5), k * ((rel[1][0] - rel[0][1]) * 0.5)]
    _, V = _so3_exp_and_v(phi)
    adj, det = _adj3(V)
    tau = [((adj[i][0] * rel[0][3] + adj[i][1] * rel[1][3]) + adj[i][2] * rel[2][3]) / det for i in range(3)]
    tau, phi = [alpha * v for v in tau], [alpha * v for v in phi]
    R, V = _so3_exp_and_v(phi)
    E = [[R[i][0], R[i][1], R[i][2], (V[i][0] * tau[0] + V[i][1] * tau[1]) + V[i][2] * tau[2]] for i in range(3)] + [[0.0, 0.0, 0.0, 1.0]]
    out = _affine_mul(p0, E)
    rel_out = None if base is None else np.array(_affine_mul(out, _affine_inverse(f(base))), dtype=np.float64)
    return np.array(out, dtype=np.float64), rel_out


# ---- the bar ----------------------------------------------------------------------------------------------------------------------------
def input_scale(*arrays):
    return max([1.0] + [float(np.abs(np.asarray(a, dtype=np.float64)).max()) for a in arrays if a is not None])


def ulp_distance(got, ref64, scale=1.0):
    """(largest |got - f32(ref)| in units of the bar of this module, index of that entry).  <= 1 passes."""
    got = np.asarray(got)
    assert got.dtype == np.float32, got.dtype
    r32 = np.asarray(ref64, dtype=np.float64).astype(np.float32)
    bar = np.spacing(np.abs(r32)).astype(np.float64) + 64.0 * 2.0 ** -53 * scale
    d = np.abs(got.astype(np.float64) - r32.astype(np.float64)) / bar
    k = int(np.argmax(d))
    return float(d.reshape(-1)[k]), np.unravel_index(k, d.shape)


def assert_one_ulp(got, ref64, scale, what):
    d, at = ulp_distance(got, ref64, scale)
    print(f"{what}: {d:.3f} of the bar at {tuple(int(v) for v in at)}")
    assert d <= 1.0, f"{what}: {d:.3f} x (one float32 ulp + the oracle's float64 error) at {at}"
    return d


def assert_bit_equal(got, ref64, what):
    """got == f32(oracle), every entry (stricter than one float32 ulp; +0 and -0 count as equal)."""
    got = np.asarray(got)
    assert got.dtype == np.float32, got.dtype
    r32 = np.asarray(ref64, dtype=np.float64).astype(np.float32)
    bad = np.argwhere(got != r32)
    print(f"{what}: {'bit-equal with' if bad.size == 0 else 'NOT bit-equal with'} the oracle rounded to float32")
    assert bad.size == 0, f"{what}: {len(bad)} entries differ from the float64 oracle rounded to float32, first at {tuple(bad[0])}: {got[tuple(bad[0])]!r} != {r32[tuple(bad[0])]!r}"


def assert_exact_zeros_and_ones(got, ref64, what):
    """Entries that are exactly 0 or 1 in the float64 oracle are exactly 0 or 1 in the output."""
    got, ref = np.asarray(got), np.asarray(ref64)
    for v in (0.0, 1.0):
        m = ref == v
        assert np.array_equal(got[m], np.full(int(m.sum()), v, dtype=np.float32)), f"{what}: an entry that is exactly {v} in the oracle is not"


# ---- the yardstick: the host float32 route (synthetic.make_camera / Camera(is_co3d=True)) with general intrinsics -------------------------
def host_route(pose, fx, fy, cx, cy, W, H, znear=ZNEAR, zfar=ZFAR):
    """The statements of scene/cameras.py:76-98 in torch float32 on the host, for one [4,4] pose: (view, full, campos) as numpy float32."""
    import torch
    w2c = torch.as_tensor(np.asarray(pose, dtype=np.float32).reshape(4, 4))
    view_T = w2c.t().contiguous()
    proj = torch.tensor(projection(fx, fy, cx, cy, W, H, znear, zfar), dtype=torch.float32)
    full = view_T.unsqueeze(0).bmm(proj.t().unsqueeze(0)).squeeze(0)
    return view_T.numpy(), full.numpy(), view_T.inverse()[3, :3].numpy()


# ---- poses --------------------------------------------------------------------------------------------------------------------------------
def rodrigues(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def make_pose(axis, angle, t, skew=0.0):
    """[4,4] float32 world-to-camera; skew != 0 adds that much of a fixed non-symmetric matrix to the rotation block (off orthonormal)."""
    M = np.eye(4)
    M[:3, :3] = rodrigues(axis, angle) + skew * np.array([[1.0, -2.0, 0.5], [0.25, 1.5, -1.0], [-0.75, 0.5, 2.0]])
    M[:3, 3] = t
    return M.astype(np.float32)


def sequence_pose(f, step_angle=0.006, step_shift=0.02):
    """Frame f of a trajectory like sequence.FrameSequence's: 0.006 rad and 0.02 units per frame."""
    return make_pose((0.1, 1.0, 0.05), step_angle * f, (step_shift * f, 0.2 * step_shift * math.sin(0.7 * f), 0.001 * f))


def batch_poses(B, seed=0):
    """B poses: the identity first, a chained product `rel @ pose` (not orthonormal to the last bit), one 1e-6 off orthonormal, random ones."""
    g = np.random.default_rng(100 + seed)
    out = [np.eye(4, dtype=np.float32)]
    if B > 1:
        chain = np.eye(4, dtype=np.float32)
        for f in range(1, 9):
            chain = (sequence_pose(f) @ np.linalg.inv(sequence_pose(f - 1)).astype(np.float32)) @ chain      # float32 products, as the trainer chains them
        out.append(chain.astype(np.float32))
    if B > 2:
        out.append(make_pose((1.0, -0.4, 0.3), 0.8, (0.3, -1.2, 2.0), skew=1e-6))
    while len(out) < B:
        out.append(make_pose(g.normal(size=3), g.uniform(-3.0, 3.0), g.normal(size=3) * 2.0))
    return np.stack(out[:B]).astype(np.float32)


# (W, H, fx, fy, cx, cy): 64x48 centred, 980x545 with fx != fy and an off-centre principal point, 17x9
INTRINSICS = {"64x48 centred": (64, 48, 42.0, 42.0, 32.0, 24.0),
              "980x545 general": (980, 545, 611.3, 598.7, 501.25, 260.5),
              "17x9": (17, 9, 11.0, 11.0, 8.5, 4.5)}

# the hand-worked cases.  Identity: view = I, campos = 0.  A 90 degree turn about y, R = [[0,0,1],[0,1,0],[-1,0,0]], t = (1,2,3):
# view = pose^T; camera centre = -R^T t = -( (0*1 + 0*2 + -1*3), 2, (1*1 + 0 + 0) ) = (3, -2, -1)
HAND_POSE = np.array([[0, 0, 1, 1], [0, 1, 0, 2], [-1, 0, 0, 3], [0, 0, 0, 1]], dtype=np.float32)
HAND_VIEW = np.array([[0, 0, -1, 0], [0, 1, 0, 0], [1, 0, 0, 0], [1, 2, 3, 1]], dtype=np.float64)
HAND_CAMPOS = np.array([3.0, -2.0, -1.0])
# with W = H = 4, fx = fy = 2, cx = cy = 2, znear = 1, zfar = 3: P = [[1,0,0,0],[0,1,0,0],[0,0,1.5,-1.5],[0,0,1,0]], full = view P^T
HAND_INTR = dict(fx=2.0, fy=2.0, cx=2.0, cy=2.0, W=4, H=4, znear=1.0, zfar=3.0)
HAND_FULL = np.array([[0, 0, -1.5, -1], [0, 1, 0, 0], [1, 0, 0, 0], [1, 2, 3.0, 3]], dtype=np.float64)
