"""What the depth-loss tests share (tests/test_depth_loss_cpu.py, tests/test_gpu_depth_loss.py): the comparison scene, the float64
reference (train_step.depth_loss, itself pinned to the reference's code by tests/golden/depth_loss.npz), the kink set and the bars.

The bars are the project's own: value |v - ref| <= 2e-6 max(1, |ref|) (tests/test_gpu_loss.py), gradient 1e-4 norm-wise and
1e-4 max|g| element-wise (GRAD_RTOL).  |.| has kinks: one sign decided differently at a pair whose difference is below rounding
moves two entries by a whole stencil weight, so the gradient bars are taken over the pixels OUTSIDE the kink set, which is read off
the float64 reference with tau = 1e-5 and may hold at most 1e-3 of the pixels (a condition on the scene, not a measurement).  On a kink
pixel the value may differ by the summed magnitude of that pixel's kink terms plus the element bar."""
import importlib

import numpy as np
import torch

ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")

VALUE_RTOL = 2e-6
GRAD_RTOL = 1e-4
TAU = 1e-5
KINK_SHARE_MAX = 1e-3
LO, HI, VALID = 0.02, 20.0, 0.02


def scene(H, W, seed=21, invalid=0.10):
    """gt = 2 + 3 yy + 1.5 sin(6 xx) + 0.2 U(0,1) on the unit grid with a random 10 % set to 0 (invalid mono-depth pixels),
    p = 0.6 gt + 0.8 + 0.15 N(0,1), the first four rows of p at 26 and the last four at 0.004 (both sides of the clamp; fewer rows
    on planes lower than twelve), everything rounded to float32.  (tools/make_golden.py depth_scene is the same formula.)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.linspace(0.0, 1.0, H), np.linspace(0.0, 1.0, W), indexing="ij")
    gt = 2.0 + 3.0 * yy + 1.5 * np.sin(6.0 * xx) + 0.2 * rng.random((H, W))
    gt[rng.random((H, W)) < invalid] = 0.0
    p = 0.6 * gt + 0.8 + 0.15 * rng.standard_normal((H, W))
    p[:min(4, H // 3)] = 26.0
    p[H - min(4, H // 3):] = 0.004
    return p.astype(np.float32), gt.astype(np.float32)


def reference(p32, g32, kind, dtype=torch.float64):
    """(value, gradient w.r.t. the unclamped plane, s, t, M) of train_step.depth_loss in `dtype` on the float32 inputs (CPU)."""
    p = torch.from_numpy(np.ascontiguousarray(p32)).to(dtype).requires_grad_(True)
    g = torch.from_numpy(np.ascontiguousarray(g32)).to(dtype)
    v, s, t, M = ts.depth_loss(p, g, kind, return_fit=True)
    v.backward()
    f = lambda x: None if x is None else float(x.detach() if torch.is_tensor(x) else x)
    v = v.detach()
    return float(v), p.grad.double().numpy(), f(s), f(t), f(M)


def kink_set(p32, g32, kind):
    """(mask [H,W] of the kink pixels, allowance [H,W]): read off the float64 reference.  A pixel is in the set when it is in a masked
    pair with |d_b - d_a| <= tau; for 'l1' when |pc - g| <= tau; when p is within tau of a clamp bound or g within tau of 0.02.
    allowance = the summed magnitude of the pixel's kink terms (for an upstream gradient of 1): |s| / M per kink pair (the sign's
    +-1 times the stencil weight 0.5 s / M, flipped), 2 / (H W) for 'l1'; a whole gradient entry (the plane's largest) where the
    clamp's or the mask's own threshold is the kink."""
    p, g = p32.astype(np.float64), g32.astype(np.float64)
    H, W = p.shape
    pc = np.clip(p, LO, HI)
    kink = np.zeros((H, W), bool)
    allow = np.zeros((H, W))
    _, gref, s, t, M = reference(p32, g32, kind)
    edge = (np.abs(p - LO) <= TAU) | (np.abs(p - HI) <= TAU) | (np.abs(g - VALID) <= TAU)
    if kind == "l1":
        k = np.abs(pc - g) <= TAU
        kink |= k
        allow += k * (2.0 / (H * W))
    else:
        m = g > VALID
        d = m * (s * pc + t - g)
        w = abs(s) / max(M, 1.0)
        kx = m[:, 1:] & m[:, :-1] & (np.abs(d[:, 1:] - d[:, :-1]) <= TAU)
        ky = m[1:, :] & m[:-1, :] & (np.abs(d[1:, :] - d[:-1, :]) <= TAU)
        for a, b, k in ((np.s_[:, 1:], np.s_[:, :-1], kx), (np.s_[1:, :], np.s_[:-1, :], ky)):
            kink[a] |= k; kink[b] |= k
            allow[a] += k * w; allow[b] += k * w
    kink |= edge
    allow += edge * np.abs(gref).max()
    return kink, allow


def check(value, grad, p32, g32, kind, upstream=1.0, what=""):
    """Hold (value, grad) -- grad for the given upstream gradient -- to the bars above.  Prints every figure before it asserts."""
    ref_v, ref_g, _, _, _ = reference(p32, g32, kind)
    ref_g = upstream * ref_g
    kink, allow = kink_set(p32, g32, kind)
    share = kink.mean()
    grad = np.asarray(grad, dtype=np.float64).reshape(ref_g.shape)
    off = ~kink
    gmax = np.abs(ref_g).max()
    diff = np.abs(grad - ref_g)
    norm = np.linalg.norm(ref_g[off])
    rel = np.linalg.norm((grad - ref_g)[off]) / norm if norm > 0 else np.linalg.norm((grad - ref_g)[off])
    emax = diff[off].max() if off.any() else 0.0
    over = (diff - (abs(upstream) * allow + GRAD_RTOL * gmax))[kink].max() if kink.any() else 0.0
    print(f"[depth-loss {what} {kind} {ref_g.shape}] value {value!r} ref {ref_v!r} rel {abs(value - ref_v) / max(1.0, abs(ref_v)):.3e}; "
          f"kink share {share:.3e}; norm-wise {rel:.3e}; element max {emax:.3e} (bar {GRAD_RTOL * gmax:.3e}); kink excess {over:.3e}")
    assert share <= KINK_SHARE_MAX, share
    assert abs(value - ref_v) <= VALUE_RTOL * max(1.0, abs(ref_v)), (value, ref_v)
    assert rel <= GRAD_RTOL, rel
    assert emax <= GRAD_RTOL * gmax, (emax, gmax)
    assert over <= 0.0, over
