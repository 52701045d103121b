"""Shared parity machinery for tests/: scene -> kwargs, tolerance rules, host-emulation binding.

Tolerances (BASELINE.json north_star): forward RGB within 1e-5 abs, gradients within 1e-4 rel.
  * forward: every pixel must be within FWD_ATOL of the float64 oracle.  For a pixel with a discrete decision on a
    rounding edge (alpha cut 1/255, power > 0, transmittance stop 1e-4) the oracle enumerates the outcomes of those
    decisions and the implementation must match ONE of them within FWD_ATOL (check_forward / resolve_branches); the
    measured share of such pixels is printed and bounded per case.  Only pixels on a tile-rect rounding edge, or with
    more edge decisions than the enumeration covers, stay "unresolved": bounded by FLIP_ATOL, share <= UNRESOLVED_MAX_FRAC.
  * gradients: upstream grads are kept everywhere except on unresolved pixels (the oracle's backward differentiates
    the branch adopted per pixel); per tensor max|g - g_ref| <= GRAD_RTOL * max|g_ref| (norm-wise) AND element-wise
    |g - g_ref| <= ELEM_RTOL |g_ref| + ELEM_RTOL rms(g_ref).
  * accumulation: the blend backward sums a Gaussian's per-tile parts either with float64 atomics in arrival order (default) or
    in list order ("deterministic_backward").  Both form the same float32 parts, and a float64 sum of float32 parts is exact
    while their exponent span plus log2(count) fits in 29 bits (csrc/blend_common.h), so the two give the SAME BITS apart from
    a rare float32 rounding-boundary flip of an inexact sum: same_accumulation() allows at most FLIP_MAX_ENTRIES such entries
    per tensor, each within FLIP_RTOL of its own magnitude (+ FLIP_RMS_RTOL of the tensor's rms).  A lost or doubled tile
    part moves an entry by a share of itself, far beyond that.
"""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import torch

from oracle import binding

FWD_ATOL = 1e-5
DEPTH_RTOL = 1e-5      # depth feature is O(z): relative to max depth
FLIP_ATOL = 2e-2
AMBIG_MAX_FRAC = 0.05
UNRESOLVED_MAX_FRAC = 2e-4
GRAD_RTOL = 1e-4
ELEM_RTOL = 1e-4
ELEM_BAD_MAX = 3e-4     # share of a tensor's entries allowed outside the element-wise bar (never fewer than 2 entries): about twice
                        # the largest share the GPU parity suite measures under this bound on MI355X, 1.6e-4 (13 of 83 250 opacity
                        # entries of the every-pixel model of test_parity_on_a_single_image_model_of_pixel_gaussians: binary32
                        # arithmetic of a tile's part, the same entries with fixed-order and default accumulation)
FLIP_MAX_ENTRIES = 4    # same_accumulation(): differing entries allowed per tensor (rounding-boundary flips of inexact float64 sums)
FLIP_RTOL = 1e-5
FLIP_RMS_RTOL = 1e-7

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
syn = importlib.import_module("3dgs_hierarchical_training_amd.synthetic")


def scene_kwargs(sc, mode="sh", bg=(0.0, 0.0, 0.0), colors_seed=7):
    """mode: 'sh' (shs + scales/rotations), 'pre' (colors_precomp + cov3D_precomp), 'mixed' (colors + scale/rot)."""
    kw = dict(means3D=sc["means3D"], opacities=sc["opacities"], viewmatrix=sc["viewmatrix"],
              projmatrix=sc["projmatrix"], campos=sc["campos"], bg=torch.tensor(bg, dtype=torch.float32),
              image_height=sc["image_height"], image_width=sc["image_width"], tanfovx=sc["tanfovx"],
              tanfovy=sc["tanfovy"], sh_degree=sc["sh_degree"], scale_modifier=sc.get("scale_modifier", 1.0))
    N = sc["means3D"].shape[0]
    g = torch.Generator().manual_seed(colors_seed)
    if mode == "sh":
        kw.update(shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"])
    elif mode == "mixed":
        kw.update(colors_precomp=torch.rand(N, 3, generator=g), scales=sc["scales"], rotations=sc["rotations"])
    elif mode == "pre":
        cov = torch.from_numpy(binding.cov3d(sc["scales"].numpy(), kw["scale_modifier"], sc["rotations"].numpy())).float()
        kw.update(colors_precomp=torch.rand(N, 3, generator=g), cov3D_precomp=cov)
    else:
        raise ValueError(mode)
    return kw


def upstream_grads(H, W, seed=0, depth_scale=0.1, alpha_scale=0.1):
    rng = np.random.default_rng(seed)
    gc = rng.standard_normal((3, H, W)).astype(np.float32)
    gd = (depth_scale * rng.standard_normal((H, W))).astype(np.float32)
    ga = (alpha_scale * rng.standard_normal((H, W))).astype(np.float32)
    return gc, gd, ga


def check_forward(got, oracle: "binding.OracleRender", what="", ambig_max_frac=None, fwd_atol=None, resolve=True,
                  unresolved_max_frac=None):
    """got = (color[3,H,W], radii[N], depth[1,H,W], alpha[1,H,W]) numpy float32/int32.  fwd_atol overrides FWD_ATOL (only the
    very large image test does: see its docstring).

    Pixels with rounding-edge decisions are RESOLVED, not excused: the oracle enumerates the outcomes of those decisions and
    adopts, per pixel, the branch closest to `got` (binding.resolve_branches); the result must then be within the ordinary
    tolerance there too.  What is left over ("unresolved": a tile-rect rounding edge, or more edge decisions than the
    enumeration covers) is bounded by FLIP_ATOL and its share by UNRESOLVED_MAX_FRAC.  Returns the report, including
    `grad_mask` (pixels whose upstream gradient may be kept: everything but the unresolved ones) -- a later
    oracle.backward() differentiates the adopted branches."""
    FWD_ATOL = globals()["FWD_ATOL"] if fwd_atol is None else fwd_atol
    color, radii, depth, alpha = [np.asarray(x) for x in got]
    amb = oracle.px_ambig != 0
    frac = float(amb.mean())
    lim = AMBIG_MAX_FRAC if ambig_max_frac is None else ambig_max_frac
    print(f"[parity] {what}: {frac:.4%} of pixels have a rounding-edge decision")
    assert frac <= lim, f"{what}: {frac:.3%} of pixels have a rounding-edge decision (bound {lim:.3%})"
    changed = 0
    if resolve and frac > 0:
        changed = oracle.resolve_branches(color, alpha.reshape(oracle.H, oracle.W))["changed"]
    dc = np.abs(color.astype(np.float64) - oracle.color).max(0)
    dd = np.abs(depth.astype(np.float64) - oracle.depth)[0]
    da = np.abs(alpha.astype(np.float64) - oracle.alpha)[0]
    zmax = max(1.0, float(np.abs(oracle.depth).max()))
    dscale = FWD_ATOL / globals()["FWD_ATOL"]   # 1 unless the caller widened the forward tolerance
    dtol = DEPTH_RTOL * zmax * 2 * dscale
    ok = ~amb
    assert dc[ok].max(initial=0) <= FWD_ATOL, f"{what}: colour err {dc[ok].max():.3e} on unambiguous pixels"
    assert da[ok].max(initial=0) <= FWD_ATOL, f"{what}: alpha err {da[ok].max():.3e}"
    assert dd[ok].max(initial=0) <= dtol, f"{what}: depth err {dd[ok].max():.3e}"
    within = (dc <= FWD_ATOL) & (da <= FWD_ATOL) & (dd <= dtol)
    unresolved = amb & ~within
    ufrac = float(unresolved.mean())
    ulim = (UNRESOLVED_MAX_FRAC if resolve else 1.0) if unresolved_max_frac is None else unresolved_max_frac
    assert ufrac <= ulim, f"{what}: {ufrac:.4%} of pixels match none of their branches (bound {ulim:.4%})"
    assert dc.max(initial=0) <= FLIP_ATOL and da.max(initial=0) <= FLIP_ATOL, f"{what}: flip err {dc.max():.3e}"
    gok = oracle.g_ambig == 0
    assert np.array_equal(np.asarray(radii)[gok], oracle.radii[gok]), f"{what}: radii mismatch"
    return dict(ambig_frac=frac, branches_adopted=int(changed), unresolved_frac=ufrac, max_color_err=float(dc[~unresolved].max(initial=0)),
                grad_mask=~unresolved)


def check_grads(got: dict, ref: dict, what="", rtol=GRAD_RTOL, elementwise=True, elem_bad_max=ELEM_BAD_MAX, elem_bad_min_entries=2):
    """Two bars per tensor: norm-wise max|g - g_ref| <= rtol max|g_ref|, and element-wise
    |g - g_ref| <= ELEM_RTOL |g_ref| + ELEM_RTOL rms(g_ref) (rms over the non-zero reference entries) on all but a
    share `elem_bad_max` of the entries (the binary32 arithmetic of a tile's part -- pixels of opposite sign cancelling in the wave
    reduction -- leaves a few entries of a cancelling gradient outside the per-entry bar)."""
    rep = {}
    for k, g in got.items():
        if g is None or k not in ref:
            continue
        r = np.asarray(ref[k], np.float64).reshape(np.asarray(g).shape)
        g = np.asarray(g, np.float64)
        scale = np.abs(r).max()
        err = np.abs(g - r).max() if g.size else 0.0
        rep[k] = err / scale if scale > 0 else err
        assert np.isfinite(g).all(), f"{what}: non-finite grad {k}"
        if scale == 0:
            assert err == 0, f"{what}: grad {k} should be zero"
            continue
        assert err <= rtol * scale, f"{what}: grad {k} rel err {err / scale:.3e} (max|ref|={scale:.3e})"
        if elementwise:
            nz = r != 0
            rms = float(np.sqrt((r[nz] ** 2).mean())) if nz.any() else 0.0
            er = ELEM_RTOL * (rtol / GRAD_RTOL)      # a test that documents a wider norm-wise bound widens this one with it
            bad = np.abs(g - r) > er * np.abs(r) + er * rms
            rep[k + "/elem_bad"] = float(bad.mean())
            if bad.any():
                print(f"[parity] {what}: grad {k}: elem_bad {bad.mean():.3e} ({int(bad.sum())} of {bad.size})")
            assert bad.sum() <= (max(elem_bad_min_entries, elem_bad_max * bad.size) if elem_bad_max > 0 else 0), f"{what}: grad {k}: {bad.mean():.3%} of the entries off element-wise (rms {rms:.3e})"
    return rep


def same_accumulation(got: dict, want: dict, what="", max_entries=None, verbose=True):
    """Gradients of the default accumulation (`got`) against the fixed-order one (`want`), or of two routes that must give the same
    bits: per tensor either equal bits or at most FLIP_MAX_ENTRIES differing entries, each within FLIP_RTOL |want| +
    FLIP_RMS_RTOL rms(want) (rms over the non-zero entries).  Takes numpy arrays or tensors; prints and returns the count of
    differing entries per tensor.  max_entries=0 asks for equal bits (two runs of the fixed-order mode); verbose=False prints only
    counts that are not zero."""
    lim_n = FLIP_MAX_ENTRIES if max_entries is None else max_entries
    counts = {}
    for k, w in want.items():
        if w is None:
            continue
        g = got[k]
        g = g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
        w = w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        diff = g != w
        if np.issubdtype(g.dtype, np.floating):
            diff &= ~(np.isnan(g) & np.isnan(w))
        n = int(diff.sum())
        counts[k] = n
        if n == 0:
            continue
        assert n <= lim_n, f"{what}: {k}: {n} entries differ (at most {lim_n} rounding-boundary flips allowed)"
        w64, g64 = w.astype(np.float64), g.astype(np.float64)
        nz = w64 != 0
        rms = float(np.sqrt((w64[nz] ** 2).mean())) if nz.any() else 0.0
        d = np.abs(g64 - w64)[diff]
        lim = FLIP_RTOL * np.abs(w64)[diff] + FLIP_RMS_RTOL * rms
        assert np.all(d <= lim), f"{what}: {k}: a differing entry is off by {float((d / np.maximum(lim, 1e-300)).max()):.3g} x its allowance"
    if verbose or any(counts.values()):
        print(f"[accumulation] {what}: differing entries {({k: v for k, v in counts.items() if v} or 'none')}")
    return counts


def oracle_case(o: "binding.OracleRender", run, upstream, what="", **fwd_kw):
    """The two-pass comparison every parity test goes through.  run(grads_or_None) -> {'fwd': ..., 'grads': ...} is the
    implementation under test.  Pass 1: its forward alone; the oracle adopts, per rounding-edge pixel, the branch it took
    (check_forward) and every pixel is held to the forward tolerance.  Pass 2: the upstream gradients are kept on every
    pixel except the unresolved ones, the oracle differentiates the adopted branches, the implementation runs forward +
    backward.  Returns (forward report, implementation output, oracle gradients)."""
    o.forward()
    rep = check_forward(run(None)["fwd"], o, what, **fwd_kw)
    keep = rep["grad_mask"]
    gc, gd, ga = upstream
    gc = gc * keep[None]
    gd = None if gd is None else gd * keep
    ga = None if ga is None else ga * keep
    ref = o.backward(gc, gd, ga)
    out = run((gc, gd, ga))
    return rep, out, ref


# ------------------------------------------------------------------ host emulation of csrc/gsr_math.h
_EMU = None


def hostemu_lib():
    global _EMU
    if _EMU is None:
        d = os.path.join(REPO, "tests", "hostemu")
        so, src = os.path.join(d, "libhostemu.so"), os.path.join(d, "hostemu.cpp")
        hdr = os.path.join(REPO, "3dgs_hierarchical_training_amd", "csrc", "gsr_math.h")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src, "-o", so])
        lib = C.CDLL(so)
        lib.hostemu_forward.restype = C.c_void_p
        lib.hostemu_forward.argtypes = [C.POINTER(binding.GsrOracleIn)] + [C.c_void_p] * 4
        lib.hostemu_backward.argtypes = [C.c_void_p] * 13
        lib.hostemu_free.argtypes = [C.c_void_p]
        lib.hostemu_num_rendered.restype = C.c_int64
        lib.hostemu_num_rendered.argtypes = [C.c_void_p]
        _EMU = lib
    return _EMU


def hostemu_run(oracle: "binding.OracleRender", grads=None):
    """Run the binary32 host emulation on the SAME input arrays the oracle object holds."""
    lib = hostemu_lib()
    N, H, W, M = oracle.N, oracle.H, oracle.W, max(oracle.M, 1)
    color = np.zeros((3, H, W), np.float32); depth = np.zeros((1, H, W), np.float32)
    alpha = np.zeros((1, H, W), np.float32); radii = np.zeros(N, np.int32)
    p = binding._ptr
    ctx = lib.hostemu_forward(C.byref(oracle.args), p(color), p(depth), p(alpha), p(radii))
    out = dict(fwd=(color, radii, depth, alpha), num_rendered=int(lib.hostemu_num_rendered(ctx)))
    if grads is not None:
        gc, gd, ga = [np.ascontiguousarray(g, np.float32) if g is not None else None for g in grads]
        g = dict(means3D=np.zeros((N, 3), np.float32), means2D=np.zeros((N, 3), np.float32),
                 opacities=np.zeros((N, 1), np.float32), colors_precomp=np.zeros((N, 3), np.float32),
                 shs=np.zeros((N, M, 3), np.float32), scales=np.zeros((N, 3), np.float32),
                 rotations=np.zeros((N, 4), np.float32), cov3D_precomp=np.zeros((N, 6), np.float32))
        cam = np.zeros(35, np.float32)
        lib.hostemu_backward(ctx, p(gc), p(gd), p(ga), p(g["means3D"]), p(g["means2D"]), p(g["opacities"]),
                             p(g["colors_precomp"]), p(g["shs"]), p(g["scales"]), p(g["rotations"]), p(g["cov3D_precomp"]), p(cam))
        g["viewmatrix"], g["projmatrix"], g["campos"] = cam[:16].reshape(4, 4), cam[16:32].reshape(4, 4), cam[32:]
        out["grads"] = g
    lib.hostemu_free(ctx)
    return out
