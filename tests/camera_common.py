"""Cameras with real intrinsics for tests/: unequal focal lengths and a principal point off the image centre.

synthetic.make_camera sets fy = fx and (cx, cy) = (W/2, H/2): the two principal-point entries of the projection are then exactly zero
and the two focal lengths, the two frustum limits and the two halves of the projection's Jacobian are interchangeable.  The reference's
data is not like that (COLMAP PINHOLE cameras carry fx != fy; CO3D frames carry a principal point per frame, which its Camera class
builds into the projection as -(w - 2 cx)/w and -(h - 2 cy)/h).  general_camera restates that construction (the co3d branch:
transposed view, OpenGL-style projection from the intrinsics, full = view_T @ proj_T) for any (fx, fy, cx, cy), with
tanfovx = W / (2 fx) and tanfovy = H / (2 fy) -- what the kernels recover the focal lengths from.  tests/golden/camera_general.npz
(tools/make_golden.py gen_camera_general) holds it to the reference's own output."""
import math

import torch

import parity

syn = parity.syn
CAMERA_NAMES = ("aniso", "offcentre", "both", "far", "far-both")


def general_camera(W, H, fx, fy, cx, cy, R=None, t=None, znear=0.01, zfar=100.0):
    """The dict of synthetic.make_camera (plus cx, cy) for a pinhole camera with intrinsics (fx, fy, cx, cy).  R, t = world-to-camera."""
    fx, fy, cx, cy = float(fx), float(fy), float(cx), float(cy)
    w2c = torch.eye(4, dtype=torch.float32)
    if R is not None:
        w2c[:3, :3] = R.float()
    if t is not None:
        w2c[:3, 3] = t.float()
    view_T = w2c.t().contiguous()
    proj = torch.tensor([[2 * fx / W, 0.0, -(W - 2 * cx) / W, 0.0],
                         [0.0, 2 * fy / H, -(H - 2 * cy) / H, 0.0],
                         [0.0, 0.0, zfar / (zfar - znear), -(zfar * znear) / (zfar - znear)],
                         [0.0, 0.0, 1.0, 0.0]], dtype=torch.float32)
    proj_T = proj.t().contiguous()
    full = (view_T.unsqueeze(0).bmm(proj_T.unsqueeze(0))).squeeze(0).contiguous()
    campos = view_T.inverse()[3, :3].contiguous()
    return dict(image_width=W, image_height=H, tanfovx=0.5 * W / fx, tanfovy=0.5 * H / fy, viewmatrix=view_T, projmatrix=full,
                campos=campos, fx=fx, fy=fy, cx=cx, cy=cy)


def intrinsics(name, W, H):
    """(fx, fy, cx, cy) of the named camera; f is make_camera's focal length.  The offsets are no whole pixels.  On "far" and "far-both"
    the frame reaches beyond 1.3 tanfov on one side (x: 0.72 W from the principal point > 0.65 W; y: 0.71 H and 0.7 H > 0.65 H), so the
    frustum clamp of the projection's Jacobian acts on splats that are on screen."""
    f = 0.5 * W / math.tan(0.5 * syn.FOVX_FRANCIS)
    return {"centred": (f, f, W / 2.0, H / 2.0),
            "aniso": (f, 1.37 * f, W / 2.0, H / 2.0),
            "offcentre": (f, f, W / 2.0 + 0.125 * W, H / 2.0 - 0.135 * H),
            "both": (0.85 * f, 1.2 * f, W / 2.0 + 0.125 * W, H / 2.0 - 0.135 * H),
            "far": (f, f, W / 2.0 + 0.22 * W, H / 2.0 - 0.21 * H),
            "far-both": (0.8 * f, 1.3 * f, W / 2.0 - 0.23 * W, H / 2.0 + 0.2 * H)}[name]


def named_camera(name, W, H, R=None, t=None):
    return general_camera(W, H, *intrinsics(name, W, H), R=R, t=t)


def _cam_spec(cam, W, H):
    if isinstance(cam, str):
        return dict(zip(("fx", "fy", "cx", "cy"), intrinsics(cam, W, H)))
    return dict(cam)


def general_scene(N, W, H, deg, seed, cam, posed=False, **scene_kw):
    """synthetic.make_scene(N, W, H, deg, seed, posed=posed) seen through the camera `cam` (a name of the table, or a dict with fx, fy,
    cx, cy and optionally R, t).  The pose is the scene's own (make_scene's rotated and translated camera when posed) unless `cam`
    supplies R, t; the camera replaces projmatrix, tanfovx and tanfovy.  The points are refilled into the ACTUAL frustum: every point
    keeps its view depth z (so the 2 % near or behind the camera stay there, and the scales stay footprint-sized) and its place
    (u, v) in [0, 1]^2 of the overscanned frame, which now spans [-0.05, 1.05] W x [-0.05, 1.05] H of this camera's image:
    x = (u_px - cx) / fx z, y = (v_px - cy) / fy z."""
    sc = syn.make_scene(N, W, H, sh_degree=deg, seed=seed, posed=posed, **scene_kw)
    spec = _cam_spec(cam, W, H)
    w2c0 = sc["viewmatrix"].t().double()
    R = spec.get("R", w2c0[:3, :3])
    t = spec.get("t", w2c0[:3, 3])
    gc = general_camera(W, H, spec["fx"], spec["fy"], spec["cx"], spec["cy"], R=R, t=t)
    pc = sc["means3D"].double() @ w2c0[:3, :3].t() + w2c0[:3, 3][None]             # the cloud in make_scene's camera frame
    z = pc[:, 2]
    zs = torch.where(z.abs() < 1e-6, torch.full_like(z, 1e-6), z)
    u = 0.5 * (pc[:, 0] / (1.05 * sc["tanfovx"] * zs) + 1.0)                       # make_scene's u, v in [0, 1]
    v = 0.5 * (pc[:, 1] / (1.05 * sc["tanfovy"] * zs) + 1.0)
    upx, vpx = (-0.05 + 1.1 * u) * W, (-0.05 + 1.1 * v) * H
    pc = torch.stack(((upx - gc["cx"]) / gc["fx"] * z, (vpx - gc["cy"]) / gc["fy"] * z, z), 1)
    w2c = gc["viewmatrix"].t().double()
    sc["means3D"] = ((pc - w2c[:3, 3][None]) @ w2c[:3, :3]).float().contiguous()  # p_w = R^T (p_c - t)
    sc.update(gc)
    return sc


def pixel_gaussian_scene(W, H, stride, surface, seed=0, cam=None):
    """A stage-A single-image model as the reference initialises it (one Gaussian per strided pixel, un-projected with the frame's
    depth into the frame's own camera, identity rotation, footprint-sized, band 0 of 16 stored SH coefficients:
    /root/reference/trainer/ht3dgs_trainer.py:352-363, :172-212; 3dgs_hierarchical_training_amd/sequence.py pixel_scene) -- built on the
    host from an analytic depth map.  surface = "plane": every Gaussian at EXACTLY the same depth (the whole depth order is the tie
    rule: index order); "waves": a smooth surface (runs of nearly equal depths along its level lines).  cam: a name of the camera table
    (None: synthetic.make_camera's centred camera); the pixels are un-projected through ITS intrinsics:
    x = (xs + 0.5 - cx + jitter) / fx z."""
    cam = syn.make_camera(W, H) if cam is None else named_camera(cam, W, H)
    cx, cy = cam.get("cx", 0.5 * W), cam.get("cy", 0.5 * H)
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(stride // 2, H, stride), torch.arange(stride // 2, W, stride), indexing="ij")
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    u, v = xs.float() / W, ys.float() / H
    if surface == "plane":
        z = torch.full(u.shape, 4.0)
    else:
        z = 3.0 + 0.8 * torch.sin(6.0 * u) * torch.cos(5.0 * v) + 0.5 * u
    n = z.shape[0]
    # (centres a fraction of a pixel off the pixel centres, as after the first iterations of the fit: ON the centres every 3-sigma rect
    #  and every alpha threshold of the grid sits on a binary32 rounding edge at once -- a third of the pixels, measured)
    x = (xs.float() + 0.5 - cx + 0.6 * (torch.rand(n, generator=g) - 0.5)) / cam["fx"] * z
    y = (ys.float() + 0.5 - cy + 0.6 * (torch.rand(n, generator=g) - 0.5)) / cam["fy"] * z
    sc = {k: cam[k] for k in ("image_width", "image_height", "tanfovx", "tanfovy", "viewmatrix", "projmatrix", "campos")}
    sc["sh_degree"] = 0
    sc["means3D"] = torch.stack((x, y, z), 1).float().contiguous()
    # footprint-sized, a little anisotropic and a little turned: a model some iterations into its fit
    sc["scales"] = ((0.7 * stride * z / cam["fx"])[:, None] * (0.8 + 0.4 * torch.rand(n, 3, generator=g))).float().contiguous()
    if cam["fy"] != cam["fx"]:
        # The reference's initial scale is isotropic: the root of the mean squared distance to the three nearest neighbours
        # (scene/gaussian_model_ht.py:212-217, distCUDA2).  On a pixel grid un-projected through fx != fy the spacings are
        # dx = z / fx and dy = z / fy: two neighbours at the smaller spacing, the third at the larger one (while their ratio is below
        # 2), so s = sqrt((2 dmin^2 + dmax^2) / 3) -- which is z / fx when fy = fx, the line above; x 0.817 under "both".
        #
        # THIS RESCALING REMOVES A FAILURE, and the failure is a finding about the suite, not about intrinsics.  With the scales
        # left at z / fx (the centred builder's line, taken literally) the every-pixel "waves" model at 250x188 under "both" -- splats
        # 0.99 px tall on a 1 px grid -- passes the forward (0.34 % edge pixels) and every norm-wise bar (at most 4.0e-5) but misses
        # the ELEMENT-WISE bar already on the host emulation of gsr_math.h: means3D 748 of 141 000 entries (0.53 % against the
        # 0.03 % of parity.ELEM_BAD_MAX), means2D 461, opacities 1 346 of 47 000, scales 111, rotations 417 of 188 000.  The same grid
        # under the CENTRED make_camera with every scale x 1.2 misses it the same way (means3D 607, means2D 403, opacities 1 193,
        # scales 84, rotations 347), and x 1.41 breaks the norm-wise 1e-4 as well (rotations 3.7e-4, means2D 1.3e-4, scales 1.2e-4,
        # opacities 1.1e-4); at x 1 it is 8 opacity and 4 rotation entries, with the rescaled "both" 4 and 13.  The C oracle and the
        # autograd oracle agree to 1e-7 on these cameras and the known answers hold, so it is the binary32 arithmetic of the
        # blend's per-pixel terms: an every-pixel model whose footprints have grown by ~20 % is beyond the suite's element-wise bar,
        # whatever the camera.  No test holds that regime; it is recorded as an open gap in DESIGN.md ("Real intrinsics") and
        # reproduced by tools/stage_a_density_probe.py.
        fmin, fmax = min(cam["fx"], cam["fy"]), max(cam["fx"], cam["fy"])
        assert fmax < 2 * fmin
        sc["scales"] = (sc["scales"] * (cam["fx"] * math.sqrt((2.0 / fmax ** 2 + 1.0 / fmin ** 2) / 3.0))).contiguous()
    rot = torch.zeros(n, 4); rot[:, 0] = 1.0
    rot[:, 1:] = 0.05 * torch.randn(n, 3, generator=g)
    sc["rotations"] = (rot / rot.norm(dim=1, keepdim=True)).contiguous()
    sc["opacities"] = (0.5 + 0.4 * torch.rand(n, 1, generator=g)).contiguous()
    shs = torch.zeros(n, 16, 3)
    col = torch.stack((0.5 + 0.4 * torch.sin(9.0 * u), 0.5 + 0.4 * torch.cos(7.0 * v), 0.5 + 0.3 * torch.sin(5.0 * (u + v))), 1)
    shs[:, 0] = (col - 0.5) / 0.28209479177387814
    sc["shs"] = shs.contiguous()
    return sc
