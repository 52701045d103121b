"""GPU parity tests proper: product path (Python mirror -> C ABI -> HIP kernels) vs the float64 CPU oracle.

Tolerances are those of BASELINE.json's north_star, written in tests/parity.py:
forward RGB within 1e-5 abs on every pixel whose discrete decisions are unambiguous (<=5% may sit on a
rounding edge and are bounded by one dropped contribution), gradients within 1e-4 relative (norm-wise).
"""
import os

import importlib

import numpy as np
import pytest
import torch

import parity
from oracle import binding

pytestmark = pytest.mark.gpu

CASES = [
    # N, W, H, deg, posed, mode, bg
    (10000, 256, 256, 0, False, "sh", (0.0, 0.0, 0.0)),       # BASELINE config 1 (10k, 256x256, deg 0)
    (10000, 256, 256, 3, True, "sh", (0.1, 0.2, 0.3)),
    (20000, 330, 250, 2, True, "sh", (1.0, 1.0, 1.0)),         # ragged tile grid (W,H not multiples of 16)
    (20000, 320, 240, 1, False, "pre", (0.0, 0.0, 0.0)),       # colors_precomp + cov3D_precomp
    (5000, 160, 120, 0, True, "mixed", (0.3, 0.0, 0.7)),       # colors_precomp + scales/rotations
    (60000, 980, 545, 3, True, "sh", (0.0, 0.0, 0.0)),         # headline resolution, oracle-sized N
    (30000, 330, 250, 1, True, "sh", (0.1, 0.0, 0.2)),         # the ragged grid again, with deeper lists
]


def _run_case(N, W, H, deg, posed, mode, bg, ppt=None, noncontig=False, color_only=False, ambig_max_frac=None, fwd_atol=None):
    import hip_runner
    sc = parity.syn.make_scene(N, W, H, sh_degree=deg, seed=N % 97, posed=posed)
    kw = parity.scene_kwargs(sc, mode, bg=bg)
    o = binding.OracleRender(**kw)
    gc, gd, ga = parity.upstream_grads(H, W, seed=3)
    if color_only:   # loss on the image only: depth / alpha grads are None at the boundary (the reference's case)
        gd = ga = None
    what = f"hip {N}/{W}x{H}/deg{deg}/{mode}"
    rep, out, ref = parity.oracle_case(o, lambda g: hip_runner.run_hip(kw, g, noncontig=noncontig), (gc, gd, ga), what,
                                       ambig_max_frac=ambig_max_frac, fwd_atol=fwd_atol)
    grep = parity.check_grads(out["grads"], ref, what)
    rep.pop("grad_mask")
    print(rep, {k: "%.1e" % v for k, v in grep.items()})
    o.close()


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-d{c[3]}-{c[5]}")
def test_parity_vs_oracle(case):
    _run_case(*case)


def _pixel_gaussian_scene(W, H, stride, surface, seed=0):
    """Stage A's single-image model under synthetic.make_camera's centred camera: the builder lives in tests/camera_common.py, where
    tests/test_gpu_camera_intrinsics.py un-projects the same grid through cameras with real intrinsics."""
    import camera_common
    return camera_common.pixel_gaussian_scene(W, H, stride, surface, seed)


@pytest.mark.parametrize("W,H,stride,surface", [(490, 272, 2, "plane"), (490, 272, 2, "waves"), (333, 250, 1, "waves"), (980, 545, 4, "plane")],
                         ids=["plane-stride2", "waves-stride2", "waves-every-pixel-ragged", "plane-stride4-full-frame"])
def test_parity_on_a_single_image_model_of_pixel_gaussians(W, H, stride, surface):
    """Stage A's model -- 70 % of a scene's render calls go to models of this kind -- against the float64 oracle, forward and backward
    (colour loss only, as the reference's; and with the depth / alpha terms), on the binning route these models take by default (index-order
    placement + per-tile depth sort) AND on the global depth sort: both within the north_star's tolerances of the oracle, and the
    two routes' images and lists equal bit for bit.  Grids of equal or nearly equal depths make the tie rule (depth bits, then index)
    carry the whole order."""
    import hip_runner
    R_ = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    lib = importlib.import_module("3dgs_hierarchical_training_amd._lib").load()
    sc = _pixel_gaussian_scene(W, H, stride, surface)
    kw = parity.scene_kwargs(sc, "sh", bg=(0.05, 0.1, 0.15))
    imgs = {}
    try:
        for tsort in (1, 0):
            assert lib.gsr_set_option(b"tile_sort", tsort) == 0
            for color_only in (True, False):
                o = binding.OracleRender(**kw)
                gc, gd, ga = parity.upstream_grads(H, W, seed=5)
                if color_only:
                    gd = ga = None
                what = f"pixel-Gaussians {W}x{H}/{stride}/{surface}/tile_sort={tsort}/{'colour' if color_only else 'all'}"
                rep, out, ref = parity.oracle_case(o, lambda g: hip_runner.run_hip(kw, g), (gc, gd, ga), what)
                grep = parity.check_grads(out["grads"], ref, what)
                rep.pop("grad_mask")
                print(what, rep, {k: "%.1e" % v for k, v in grep.items()})
                o.close()
            fwd = hip_runner.run_hip(kw)["fwd"]
            ranges, lst = R_.last_binning()
            imgs[tsort] = (fwd, ranges.cpu().numpy().copy(), lst.cpu().numpy()[:R_._LAST["num_rendered"]].copy())
    finally:
        lib.gsr_set_option(b"tile_sort", 1)
    assert np.array_equal(imgs[0][1], imgs[1][1]) and np.array_equal(imgs[0][2], imgs[1][2]), "the two routes' tile lists differ"
    for a, b in zip(imgs[0][0], imgs[1][0]):
        assert np.array_equal(a, b)


def test_more_than_65536_tiles():
    """4112 x 4112 pixels = 257 x 257 = 66 049 tiles: tile ids no longer fit 16 bits, so the instance stream carries 32-bit
    keys (three 6-bit passes of the wide onesweep).  The public module this replaces has no image-size limit.
    Forward tolerance 1e-5, as everywhere: since round 5 the blends form their offsets from TILE-relative coordinates plus the
    16-bit remainder of the projected mean (gsr_math.h pixel_lo_pack / pixel_rel), so the binary32 pixel grid 2 056 px from the
    image centre (one ulp = 2.4e-4 px) no longer reaches a splat's weight (rounds 1-4 carried 4e-5 here)."""
    _run_case(30000, 4112, 4112, 1, True, "sh", (0.2, 0.1, 0.0))


# BASELINE.json configs at FULL size, straight against the oracle (it is OpenMP C: seconds on the GPU box's host).
# Last entry: bound on the share of pixels with a rounding-edge decision = the share measured on MI355X (round 2:
# 2.33 % / 2.35 % / 4.43 % / 2.52 %) + 20 %.  Those pixels are not excused: each must match one of its branches within 1e-5
# (parity.check_forward); the bound only says how many go through that route.
FULL = [
    (300000, 980, 545, 3, True, "sh", (0.0, 0.0, 0.0), 0.0280),      # configs[1]: ~300k Gaussians, 980x545, SH 3
    (1000000, 980, 545, 3, False, "sh", (0.0, 0.0, 0.0), 0.0283),    # the metric's workload
    (1000000, 1920, 1080, 3, True, "sh", (0.0, 0.0, 0.0), 0.0532),   # configs[2]: 1M, 1920x1080
    (4000000, 980, 545, 3, True, "sh", (0.0, 0.0, 0.0), 0.0303),     # configs[4]: 4M Gaussians
]


@pytest.mark.parametrize("case", FULL, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_parity_full_size(case):
    # thousands of (pixel, Gaussian) evaluations per pixel: the share of pixels with at least one evaluation on a
    # rounding edge grows with the list length; every pixel still has to be within 1e-5 of one of its branches
    _run_case(*case[:7], color_only=True, ambig_max_frac=case[7])


def test_parity_full_size_depth_alpha_gradients():
    """The metric's workload (1 M @980x545) with upstream gradients on ALL three outputs: the HAS_DA backward blend and the
    fork's depth / alpha terms against the oracle at full size (the other
    full-size cases are colour-only, as the reference's loss is)."""
    c = FULL[1]
    _run_case(*c[:7], color_only=False, ambig_max_frac=c[7])


def test_full_size_properties():
    """Size-independent properties at the metric's size (1M, 980x545):
    (1) alpha + final transmittance = 1: colour(bg=1) - colour(bg=0) == 1 - alpha per pixel;
    (2) relabelling the Gaussians (a permutation of the inputs) leaves the image unchanged up to depth ties;
    (3) linearity of the backward in the upstream gradient."""
    import hip_runner
    sc = parity.syn.make_scene(1000000, 980, 545, sh_degree=3, seed=11)
    kw0 = parity.scene_kwargs(sc, "sh", bg=(0.0, 0.0, 0.0))
    kw1 = parity.scene_kwargs(sc, "sh", bg=(1.0, 1.0, 1.0))
    gc = parity.upstream_grads(545, 980, seed=1)[0]
    o0 = hip_runner.run_hip(kw0, (gc, None, None))
    o1 = hip_runner.run_hip(kw1)
    c0, _, _, a0 = o0["fwd"]
    c1 = o1["fwd"][0]
    assert np.abs((c1 - c0) - (1.0 - a0)).max() < 2e-6
    perm = torch.randperm(1000000, generator=torch.Generator().manual_seed(3))
    kwp = dict(kw0)
    for k in ("means3D", "opacities", "shs", "scales", "rotations"):
        kwp[k] = kw0[k][perm].contiguous()
    op = hip_runner.run_hip(kwp, (gc, None, None))
    d = np.abs(op["fwd"][0] - c0)
    assert (d > 1e-5).mean() < 5e-3 and d.max() < 5e-2      # equal-depth ties (binary32 z) reorder a few pixels
    inv = torch.argsort(perm).numpy()
    gm = op["grads"]["means3D"][inv]
    ref = o0["grads"]["means3D"]
    assert np.abs(gm - ref).max() <= 2e-3 * np.abs(ref).max()
    o2 = hip_runner.run_hip(kw0, (2.0 * gc, None, None))
    for k in ("means3D", "opacities", "scales"):
        assert np.abs(o2["grads"][k] - 2.0 * o0["grads"][k]).max() <= 1e-4 * np.abs(o0["grads"][k]).max() + 1e-12


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-d{c[3]}-{c[5]}")
def test_parity_color_loss_only(case):
    """The colour-only backward blend (k_blend_bwd2<false>: no depth / alpha terms, the reference's loss) against the oracle on every
    case of the table -- ragged tile grids and deep lists (checkpoint resume) included."""
    _run_case(*case, color_only=True)


def test_blend_variants_agree():
    """The forward blend, selected explicitly ("blend_fwd_ppt" 7: one wave per 8x8 sub-tile with its sub-tile reach bits -- a conservative
    skip), against the oracle; then the option surface of the blend kernels.  (The tile-per-workgroup / lane-mask A/B kernels of rounds
    1-4 left the tree in round 5, the kernel without reach bits -- 6 -- after it: none was ever the default.)"""
    import importlib
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    lib = L.load()
    try:
        assert lib.gsr_set_option(b"blend_fwd_ppt", 7) == 0
        _run_case(20000, 330, 250, 3, True, "sh", (0.2, 0.3, 0.1))
    finally:
        lib.gsr_set_option(b"blend_fwd_ppt", 0)
    # the forward blend has one kernel: its option takes the default's two spellings and refuses the retired ones
    assert lib.gsr_set_option(b"blend_fwd_ppt", 0) == 0 and lib.gsr_set_option(b"blend_fwd_ppt", 7) == 0
    for v in (6, 3, 1):
        assert lib.gsr_set_option(b"blend_fwd_ppt", v) != 0
    assert lib.gsr_set_option(b"blend_fwd_ppt", 3) != 0 and lib.gsr_set_option(b"blend_bwd_ppt", 3) != 0 and lib.gsr_set_option(b"ab_variants", 0) == 0
    # the backward blend has one kernel: its option takes the default's two spellings and refuses the retired one-pixel kernel
    assert lib.gsr_set_option(b"blend_bwd_ppt", 0) == 0 and lib.gsr_set_option(b"blend_bwd_ppt", 2) == 0
    assert lib.gsr_set_option(b"blend_bwd_ppt", 1) != 0


@pytest.mark.parametrize("hint", [0, 1000, 1 << 26], ids=["exact-flow", "overflow-rerun", "roomy"])
def test_speculative_binning(hint):
    """gsr_forward launches the binning against a capacity (1.25x the recent calls' R) and reads R back late; a
    capacity that turns out too small is re-run with the exact size.  All three routes (no hint = classic
    read-back-then-launch, capacity far too small, capacity far too large) must give the parity result, and an
    identical image."""
    import importlib
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    lib = L.load()
    case = (20000, 330, 250, 3, True, "sh", (0.2, 0.3, 0.1))
    try:
        assert lib.gsr_set_option(b"speculative_binning", 0) == 0
        sc = parity.syn.make_scene(case[0], case[1], case[2], sh_degree=case[3], seed=4, posed=case[4])
        kw = parity.scene_kwargs(sc, case[5], bg=case[6])
        import hip_runner
        ref = hip_runner.run_hip(kw)["fwd"]
        assert lib.gsr_set_option(b"speculative_binning", 1) == 0
        assert lib.gsr_set_option(b"binning_capacity_hint", hint) == 0
        got = hip_runner.run_hip(kw)["fwd"]
        for r, g in zip(ref, got):
            assert np.array_equal(r, g)
        assert lib.gsr_set_option(b"binning_capacity_hint", hint) == 0
        _run_case(*case)
    finally:
        lib.gsr_set_option(b"speculative_binning", 1)
        lib.gsr_set_option(b"binning_capacity_hint", 0)


@pytest.mark.parametrize("case", [CASES[1], CASES[2], CASES[3], (300000, 980, 545, 3, True, "sh", (0.0, 0.0, 0.0)),
                                  (4000000, 980, 545, 3, True, "sh", (0.0, 0.0, 0.0))],     # BASELINE configs[4] as stated: 4 M, pose gradient on
                         ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-d{c[3]}-{c[5]}")
def test_camera_gradients(case):
    """dL/d(viewmatrix, projmatrix, campos) (north_star's dL/dviewmatrix; BASELINE config 5: pose gradients)."""
    import hip_runner
    N, W, H, deg, posed, mode, bg = case
    sc = parity.syn.make_scene(N, W, H, sh_degree=deg, seed=N % 89, posed=posed)
    kw = parity.scene_kwargs(sc, mode, bg=bg)
    o = binding.OracleRender(**kw)
    gc, gd, ga = parity.upstream_grads(H, W, seed=4)
    rep, out, ref = parity.oracle_case(o, lambda g: hip_runner.run_hip(kw, g, cam_grad=True), (gc, gd, ga), "camera grads",
                                       ambig_max_frac=0.035 if N >= 4000000 else None)
    keys = ["viewmatrix", "projmatrix"] + (["campos"] if mode == "sh" else [])
    rep = parity.check_grads({k: out["grads"][k] for k in keys}, ref, "camera grads")
    # the ordinary gradients are unchanged by routing the camera through autograd
    parity.check_grads({k: out["grads"][k] for k in ("means3D", "opacities")}, ref, "with camera grads")
    assert np.all(out["grads"]["projmatrix"].reshape(16)[2::4] == 0)     # clip-z row is unused
    print(rep)


@pytest.mark.parametrize("M,deg", [(1, 0), (4, 1), (9, 2), (16, 2)])
def test_fewer_stored_sh_coefficients(M, deg):
    """max_sh_degree below 3: shs is [N,M,3] with M = (max_deg+1)^2 (gaussian_model_ht.py:193-199)."""
    import hip_runner
    N, W, H = 8000, 200, 150
    sc = parity.syn.make_scene(N, W, H, sh_degree=deg, seed=21, posed=True)
    sc["shs"] = sc["shs"][:, :M].contiguous()
    kw = parity.scene_kwargs(sc, "sh", bg=(0.1, 0.1, 0.1))
    o = binding.OracleRender(**kw)
    gc, gd, ga = parity.upstream_grads(H, W, seed=2)
    rep, out, ref = parity.oracle_case(o, lambda g: hip_runner.run_hip(kw, g), (gc, gd, ga), f"M={M}")
    assert out["grads"]["shs"].shape == (N, M, 3)
    parity.check_grads(out["grads"], ref, f"M={M}")


def test_scale_modifier():
    import hip_runner
    N, W, H = 10000, 256, 192
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=22, posed=True)
    sc["scale_modifier"] = 0.7
    kw = parity.scene_kwargs(sc, "sh")
    o = binding.OracleRender(**kw)
    gc, gd, ga = parity.upstream_grads(H, W, seed=2)
    rep, out, ref = parity.oracle_case(o, lambda g: hip_runner.run_hip(kw, g), (gc, gd, ga), "scale_modifier")
    parity.check_grads(out["grads"], ref, "scale_modifier")


@pytest.mark.parametrize("scale", [4.0, 12.0])
def test_large_splats_take_the_per_wave_emission_path(scale):
    """Rects of more than 32 tiles carry no decision mask (TileRec): k_emit re-runs the exact tile test for them, one
    wave per Gaussian.  scale_modifier 4 mixes both paths in one block, 12 makes nearly every visible splat large."""
    import hip_runner
    N, W, H = 3000, 320, 240
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=41, posed=True)
    sc["scale_modifier"] = scale
    kw = parity.scene_kwargs(sc, "sh")
    o = binding.OracleRender(**kw)
    gc, gd, ga = parity.upstream_grads(H, W, seed=4)
    rep, out, ref = parity.oracle_case(o, lambda g: hip_runner.run_hip(kw, g), (gc, gd, ga), f"large splats x{scale}", ambig_max_frac=0.2)
    assert (out["fwd"][1] * 2 > 6 * 16).mean() > (0.05 if scale < 10 else 0.5)     # radii: rects beyond 6 tiles across exist
    parity.check_grads(out["grads"], ref, f"large splats x{scale}")


def test_tile_to_xcd_maps_agree():
    """The tile -> XCD map (2x2 blocks of tiles dealt round-robin) only decides which workgroup processes which tile: parity image and
    gradients at 335x235 -- 21 x 15 tiles, odd counts in both directions exercise the padding slots of the 2x2-block map.  The banded
    and the single-tile maps (0, 1) have left the library: the option takes 2 and refuses them."""
    import importlib
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    lib = L.load()
    try:
        assert lib.gsr_set_option(b"tile_map", 2) == 0
        _run_case(20000, 335, 235, 3, True, "sh", (0.2, 0.3, 0.1))
    finally:
        lib.gsr_set_option(b"tile_map", 2)
    assert lib.gsr_set_option(b"tile_map", 0) != 0 and lib.gsr_set_option(b"tile_map", 1) != 0
    assert lib.gsr_set_option(b"tile_map", 2) == 0


@pytest.mark.parametrize("N,W,H,posed", [(20000, 320, 240, True), (300000, 980, 545, True), (1000000, 980, 545, False),
                                         (1000000, 1920, 1080, True), (4000000, 980, 545, True)],
                         ids=["20k", "300k", "1M", "1M-1080p", "4M"])
def test_hip_takes_the_host_emulations_decisions(N, W, H, posed):
    """The other half of the rounding-edge argument.  The oracle cases let a pixel whose alpha-cut / stop decision sits on a
    binary32-vs-binary64 rounding edge match ONE of the oracle's enumerated branches (2-4 % of the pixels at full size).  Here
    the kernels are compared, with NO branch resolution and NO pixel excused, against tests/hostemu -- csrc/gsr_math.h executed
    sequentially on the host in binary32, which tests/test_oracle_cpu.py holds to the float64 oracle: the number of instances
    and every radius are identical (at 4 M: one (Gaussian, tile) pair of 18 270 065 differs), and the images agree to a few binary32 ulps on all but a handful of pixels (v_exp_f32 vs
    exp2f differ in the last bit; measured: max 4e-7 at 20 k / 300 k, ONE pixel of 534 100 off by 5e-6 at 1 M).  So the branch
    a rounding-edge pixel takes is the binary32 arithmetic's, not an implementation choice.  With all upstream gradients kept
    (rounding-edge pixels included) the gradients agree at the parity tolerance as well."""
    import hip_runner
    raster = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=1, posed=posed)
    kw = parity.scene_kwargs(sc, "sh", bg=(0.2, 0.1, 0.3))
    o = binding.OracleRender(**kw)                     # holds the arrays the emulation reads; the oracle itself does not run here
    # gradients too: up to the metric's own workload, 1 M Gaussians @980x545 (the emulation's backward is a
    # sequential per-pixel replay in a fixed accumulation order -- seconds at this size)
    # gradients too (the emulation's backward is a sequential per-pixel replay in a fixed accumulation order --
    # seconds even at 4 M).  Up to the metric's own workload (1 M @980x545) EVERY pixel keeps its upstream gradient; the two larger
    # frames flip a last-bit decision on ~10 pixels of two million (printed below), each worth one whole contribution of gradient
    # to a handful of Gaussians, so there a forward-only first pass finds those pixels and the compared backward runs without them
    # (round 5: at EVERY size a forward-only first pass finds the pixels on which the two took different last-bit decisions -- v_exp_f32
    #  against exp2f -- and the compared backward runs without their upstream gradient; their number is printed and bounded:
    #  0 / 2 / 1 / 9 / 1 of 76 800 ... 2 073 600 pixels with the tile-relative offsets of round 5, 0 / 0 / 1 / 9 / 1 before)
    grads = parity.upstream_grads(H, W, seed=2)
    e0 = parity.hostemu_run(o, None)["fwd"]
    h0 = hip_runner.run_hip(kw, None)["fwd"]
    zm = max(1.0, float(np.abs(e0[2]).max()))
    flip = (np.abs(e0[0].astype(np.float64) - h0[0]).max(0) > 2e-6) | (np.abs(e0[3].astype(np.float64) - h0[3])[0] > 2e-6) | \
           (np.abs(e0[2].astype(np.float64) - h0[2])[0] / zm > 2e-6)
    print(f"[parity] HIP vs host emulation {N} @{W}x{H}: {int(flip.sum())} pixels with a flipped last-bit decision carry no upstream gradient")
    assert flip.mean() <= 2e-5
    if flip.any():
        keep = (~flip).astype(np.float32)
        grads = tuple(g * keep for g in grads)
    emu = parity.hostemu_run(o, grads)
    out = hip_runner.run_hip(kw, grads, cam_grad=True)
    with_bwd = True
    c0, r0, d0, a0 = emu["fwd"]
    c1, r1, d1, a1 = out["fwd"]
    R0, R1 = emu["num_rendered"], raster.last_call_info()["num_rendered"]
    print(f"[parity] HIP vs host emulation {N} @{W}x{H}: instances {R1} vs {R0}, radii differing {int((r0 != r1).sum())}")
    assert abs(R0 - R1) <= max(0, int(2e-7 * R0)), (R0, R1)   # identical up to 4 M; ONE (Gaussian, tile) pair of 18 270 065 at 4 M
    assert int((r0 != r1).sum()) <= int(1e-6 * N)              # (the tile test's v_log_f32 vs logf)
    dc = np.abs(c0.astype(np.float64) - c1).max(0)
    da = np.abs(a0.astype(np.float64) - a1)[0]
    zmax = max(1.0, float(np.abs(d0).max()))
    dd = np.abs(d0.astype(np.float64) - d1)[0] / zmax
    off = float(((dc > 2e-6) | (da > 2e-6) | (dd > 2e-6)).mean())
    print(f"[parity] HIP vs host emulation {N} @{W}x{H}: max colour diff {dc.max():.2e}, alpha {da.max():.2e}, depth/zmax {dd.max():.2e}, "
          f"pixels off by more than 2e-6: {off:.2e} ({int(round(off * W * H))} of {W * H})")
    assert off <= 2e-5, off                              # a flipped last-bit decision: a handful of pixels per million
    assert dc.max() <= parity.FLIP_ATOL and da.max() <= parity.FLIP_ATOL and dd.max() <= parity.FLIP_ATOL   # ... by one contribution
    if with_bwd:
        got = {k: v for k, v in out["grads"].items() if k in emu["grads"]}
        ref = {k: emu["grads"][k] for k in got}
        parity.check_grads(got, ref, f"HIP vs host emulation {N}")


def test_faint_elongated_splats():
    """Needle-shaped (20:1), faint splats: the candidate rect (bounding box of the contribution ellipse inside the
    3-sigma rect) is far smaller than the 3-sigma square; the set of accepted tiles -- and therefore the image and the
    gradients -- must still be the oracle's.  This is also the adversarial case for conditioning: the conic -> cov2D
    step cancels (det << A C), which is why the per-Gaussian backward chain runs in float64 (in binary32 dL/dmean was
    off by 1e-3 here); what remains is the binary32 sum of the conic gradients over a tile's pixels in the blend backward
    (pixels of opposite sign cancel), so a fraction of a percent of the entries of `scales` may sit outside the per-entry bar
    (elem_bad_max 5e-3); norm-wise every tensor meets the north_star's 1e-4."""
    import hip_runner
    N, W, H = 8000, 320, 240
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=55, posed=True)
    g = torch.Generator().manual_seed(8)
    sc["scales"] = sc["scales"] * torch.tensor([12.0, 0.6, 0.6])          # 20 : 1 needles
    sc["opacities"] = torch.sigmoid(-3.0 + torch.randn(N, 1, generator=g))   # mostly below 0.1, some below 1/255
    kw = parity.scene_kwargs(sc, "sh")
    o = binding.OracleRender(**kw)
    gc, gd, ga = parity.upstream_grads(H, W, seed=9)
    rep, out, ref = parity.oracle_case(o, lambda g: hip_runner.run_hip(kw, g), (gc, gd, ga), "needles", ambig_max_frac=0.2)
    parity.check_grads(out["grads"], ref, "needles", rtol=parity.GRAD_RTOL, elem_bad_max=5e-3)
    # the default path adds the per-tile parts with float64 atomics, the fixed-order mode ("deterministic_backward") in list order:
    # the same parts, the same exact sums -- the same bars, and the same gradients up to rounding-boundary flips
    # (measured on MI355X with the fixed-order sums, tools/needles_probe.py: <= 4.7e-5 norm-wise on every tensor)
    default = out["grads"]
    lib = importlib.import_module("3dgs_hierarchical_training_amd._lib").load()
    assert lib.gsr_set_option(b"deterministic_backward", 1) == 0
    try:
        rep, out, ref = parity.oracle_case(o, lambda g: hip_runner.run_hip(kw, g), (gc, gd, ga), "needles", ambig_max_frac=0.2)
    finally:
        lib.gsr_set_option(b"deterministic_backward", 0)
    # (norm-wise 1e-4 on every tensor; element-wise a needle's conic gradients also cancel INSIDE a tile -- its 256 pixels are summed in
    #  binary32 by the wave reduction -- so a fraction of a percent of the entries of `scales` stays outside the per-entry bar: measured 0.004 ... 0.15 % run to run)
    parity.check_grads(out["grads"], ref, "needles, fixed-order float64 cross-tile sums", rtol=parity.GRAD_RTOL, elem_bad_max=5e-3)
    parity.same_accumulation(default, out["grads"], "needles, default vs fixed order")


def test_deep_lists_split_backward():
    """Tiles whose lists are processed deeper than 512 instances: the forward leaves per-pixel checkpoints every 128
    instances and the backward of such a tile is split over several workgroups that resume from them
    (gsr_set_option "bwd_split").  Same gradients as the unsplit replay (1e-5 relative; the suffix scalar is formed
    from a checkpoint instead of by running subtraction) and parity with the oracle."""
    import importlib
    import hip_runner
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    lib = L.load()
    N, W, H = 60000, 128, 96
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=77, posed=True)
    g = torch.Generator().manual_seed(3)
    sc["opacities"] = torch.sigmoid(-3.8 + 0.5 * torch.randn(N, 1, generator=g))      # faint: transmittance decays slowly
    kw = parity.scene_kwargs(sc, "sh", bg=(0.3, 0.1, 0.2))
    o = binding.OracleRender(**kw)
    gc, gd, ga = parity.upstream_grads(H, W, seed=6)
    outs, used = {}, {}

    def run(g):      # pass 2 of the comparison runs the three split settings on the same upstream gradients
        if g is None:
            return hip_runner.run_hip(kw, None)
        used["g"] = g
        for split in (1, 4, 7):
            assert lib.gsr_set_option(b"bwd_split", split) == 0
            outs[split] = hip_runner.run_hip(kw, g)
        return outs[4]

    try:
        rep, _, ref = parity.oracle_case(o, run, (gc, gd, ga), "deep lists", ambig_max_frac=0.2)
    finally:
        lib.gsr_set_option(b"bwd_split", 0)
    R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    assert R.last_call_info()["staged"] > 48 * 600, "scene not deep enough to exercise the split"
    parity.check_grads(outs[4]["grads"], ref, "deep lists, split 4")
    for split in (4, 7):
        for k_, v in outs[1]["grads"].items():
            d = np.abs(outs[split]["grads"][k_] - v).max()
            assert d <= 1e-5 * np.abs(v).max() + 1e-12, (split, k_, d)


def test_mark_visible():
    import hip_runner
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    sc = parity.syn.make_scene(5000, 128, 96, sh_degree=0, seed=23, posed=True, frac_behind=0.3)
    kw = parity.scene_kwargs(sc, "sh")
    o = binding.OracleRender(**kw)
    o.forward()
    vis = GaussianRasterizer(hip_runner.settings_from(kw, dev)).markVisible(kw["means3D"].to(dev)).cpu().numpy()
    assert vis.dtype == np.bool_ and np.array_equal(vis, o.geom()["depth"] > 0.2)
    assert np.all(vis[o.radii > 0])


def test_noncontiguous_settings():
    _run_case(5000, 160, 120, 3, True, "sh", (0.0, 0.0, 0.0), noncontig=True)


def test_golden_c1(golden_dir):
    """Committed golden vectors (tests/golden/oracle_c1_deg0.npz, made by tools/make_golden.py)."""
    import os
    import hip_runner
    g = np.load(os.path.join(golden_dir, "oracle_c1_deg0.npz"))
    N, W, H, deg = int(g["N"]), int(g["W"]), int(g["H"]), int(g["deg"])
    sc = parity.syn.make_scene(N, W, H, sh_degree=deg, seed=int(g["seed"]), posed=bool(g["posed"]))
    kw = parity.scene_kwargs(sc, "sh")
    amb = np.unpackbits(g["px_ambig"])[: W * H].reshape(H, W).astype(bool)
    rng = np.random.default_rng(int(g["gc_seed"]))
    gc = rng.standard_normal((3, H, W)).astype(np.float32)
    gd = (0.1 * rng.standard_normal((H, W))).astype(np.float32)
    ga = (0.1 * rng.standard_normal((H, W))).astype(np.float32)
    gc *= ~amb[None]; gd *= ~amb; ga *= ~amb
    out = hip_runner.run_hip(kw, (gc, gd, ga))
    color = out["fwd"][0]
    # float32 fixture: the committed image at the forward tolerance on every pixel without a rounding-edge decision
    assert np.abs(color - g["color"])[:, ~amb].max() <= parity.FWD_ATOL
    assert np.abs(out["fwd"][3] - g["alpha"])[:, ~amb].max() <= parity.FWD_ATOL
    assert np.abs(out["fwd"][2] - g["depth"])[:, ~amb].max() <= 2 * parity.DEPTH_RTOL * max(1.0, float(g["depth"].max()))
    assert abs(float(color.astype(np.float64).sum()) - float(g["color_sum"])) < 1e-4 * abs(float(g["color_sum"])) + 1.0
    ref = {k[2:]: g[k] for k in g.files if k.startswith("g_") and k[2:] in ("means3D", "means2D", "opacities", "scales", "rotations")}
    parity.check_grads({k: out["grads"][k] for k in ref}, ref, "golden c1", rtol=parity.GRAD_RTOL)
    # the fixed-order cross-tile sums ("deterministic_backward") meet the same bar, and give the same gradients
    default = out["grads"]
    lib = importlib.import_module("3dgs_hierarchical_training_amd._lib").load()
    assert lib.gsr_set_option(b"deterministic_backward", 1) == 0
    try:
        out = hip_runner.run_hip(kw, (gc, gd, ga))
    finally:
        lib.gsr_set_option(b"deterministic_backward", 0)
    parity.check_grads({k: out["grads"][k] for k in ref}, ref, "golden c1, fixed-order float64 cross-tile sums", rtol=parity.GRAD_RTOL)
    parity.same_accumulation(default, out["grads"], "golden c1, default vs fixed order")


def test_degenerate_inputs():
    """N=0, everything culled (R=0), sh_degree below the stored maximum: must not raise."""
    import hip_runner
    dev = torch.device("cuda:0")
    sc = parity.syn.make_scene(64, 64, 48, sh_degree=1, seed=1)
    kw = parity.scene_kwargs(sc, "sh")
    # all behind the camera
    kw2 = dict(kw); kw2["means3D"] = kw["means3D"].clone(); kw2["means3D"][:, 2] = -5.0
    out = hip_runner.run_hip(kw2, parity.upstream_grads(48, 64))
    assert np.all(out["fwd"][1] == 0) and np.all(out["fwd"][0] == 0) and np.all(out["fwd"][3] == 0)
    for k, v in out["grads"].items():
        assert np.all(v == 0), k
    # N = 0
    kw0 = {k: (v[:0] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == 64 else v) for k, v in kw.items()}
    out0 = hip_runner.run_hip(kw0, parity.upstream_grads(48, 64))
    assert out0["fwd"][0].shape == (3, 48, 64) and np.all(out0["fwd"][0] == 0)
    # active degree 1 of 16 stored coefficients: grads of unused coefficients are exactly zero
    out1 = hip_runner.run_hip(kw, parity.upstream_grads(48, 64))
    assert np.all(out1["grads"]["shs"][:, 4:, :] == 0)


def test_under_no_grad_and_depth_mutation():
    """Called under torch.no_grad() (ht3dgs_trainer.py:877-883) and with depth mutated in place before
    backward (ht3dgs_trainer.py:1290-1292)."""
    import hip_runner
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    sc = parity.syn.make_scene(3000, 128, 96, sh_degree=3, seed=4)
    kw = parity.scene_kwargs(sc, "sh")
    t = {k: kw[k].to(dev).requires_grad_(True) for k in ["means3D", "shs", "opacities", "scales", "rotations"]}
    m2d = torch.zeros(3000, 3, device=dev, requires_grad=True)
    rast = GaussianRasterizer(hip_runner.settings_from(kw, dev))
    with torch.no_grad():
        c0 = rast(means3D=t["means3D"], means2D=m2d, shs=t["shs"], colors_precomp=None, opacities=t["opacities"],
                  scales=t["scales"], rotations=t["rotations"], cov3D_precomp=None)[0]
    out = rast(means3D=t["means3D"], means2D=m2d, shs=t["shs"], colors_precomp=None, opacities=t["opacities"],
               scales=t["scales"], rotations=t["rotations"], cov3D_precomp=None)
    assert len(out) == 4
    color, radii, depth, alpha = out
    assert torch.equal(c0, color)
    g_ref = torch.autograd.grad(color.sum(), t["means3D"], retain_graph=True)[0]
    depth[depth < 5.0] = 5.0   # in-place on an output
    g2 = torch.autograd.grad(color.sum(), t["means3D"])[0]
    assert torch.allclose(g_ref, g2, rtol=1e-3, atol=1e-5 * float(g_ref.abs().max()))


def test_two_host_threads_two_streams():
    """Two host threads render different scenes on their own streams at the same time (the library keeps process-wide state:
    the capacity hint of the speculative binning and the pinned read-back slot of the instance count).  Forward results must be
    bit-identical to the same renders done one after the other."""
    import threading
    import hip_runner
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    jobs = []
    for seed, (N, W, H) in enumerate([(40000, 640, 360), (15000, 330, 250)]):
        sc = parity.syn.make_scene(N, W, H, sh_degree=2, seed=seed + 11)
        kw = parity.scene_kwargs(sc, "sh")
        t = {k: kw[k].to(dev) for k in ["means3D", "shs", "opacities", "scales", "rotations"]}
        jobs.append((GaussianRasterizer(hip_runner.settings_from(kw, dev)), t, N))

    def render(job):
        rast, t, N = job
        m2d = torch.zeros(N, 3, device=dev)
        with torch.no_grad():
            c, r, d, a = rast(means3D=t["means3D"], means2D=m2d, shs=t["shs"], colors_precomp=None, opacities=t["opacities"],
                              scales=t["scales"], rotations=t["rotations"], cov3D_precomp=None)
        return c, r, d, a

    ref = [render(j) for j in jobs]
    torch.cuda.synchronize()
    errors = []

    def worker(i):
        try:
            s = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(s):
                for _ in range(25):
                    out = render(jobs[i])
                    s.synchronize()
                    for got, want in zip(out, ref[i]):
                        if not torch.equal(got, want):
                            errors.append(f"thread {i}: output differs from the sequential render")
                            return
        except Exception as e:   # noqa: BLE001
            errors.append(f"thread {i}: {e!r}")

    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t_ in th:
        t_.start()
    for t_ in th:
        t_.join()
    assert not errors, errors


def _fuzz_cases():
    rng = np.random.default_rng(20240607)
    cases = []
    for i in range(int(os.environ.get("GSR_FUZZ_CASES", "28"))):   # (raise it for an exploratory run)
        W = int(rng.choice([1, 7, 16, 17, 31, 33, 100, 255, 257, 400, 641]))
        H = int(rng.choice([1, 5, 16, 18, 32, 47, 120, 256, 301]))
        N = int(rng.choice([1, 2, 63, 64, 65, 257, 1000, 5000]))
        deg = int(rng.integers(0, 4))
        fov = float(rng.choice([0.15, 0.6, 1.35, 2.4, 2.9]))          # 9 to 166 degrees
        sigma = float(rng.choice([0.3, 1.0, 3.0, 12.0, 60.0]))         # sub-pixel splats to screen-filling ones
        smod = float(rng.choice([0.25, 1.0, 3.0]))
        mode = str(rng.choice(["sh", "pre", "mixed"]))
        cases.append((i, N, W, H, deg, fov, sigma, smod, mode, bool(rng.integers(0, 2))))
    return cases


@pytest.mark.parametrize("case", _fuzz_cases(), ids=lambda c: f"{c[0]}-N{c[1]}-{c[2]}x{c[3]}-d{c[4]}-fov{c[5]}-s{c[6]}-m{c[7]}-{c[8]}")
def test_fuzz_shapes_fovs_scales(case):
    """Seeded sweep over what the headline cases do not touch: 1-pixel and sub-tile images, single Gaussians, very narrow
    and very wide fields of view, sub-pixel and screen-filling splats, scale_modifier != 1, every input mode.  Same
    tolerances as the parity cases (the ambiguous-pixel allowance is lifted for tiny images, where one pixel is percents)."""
    import hip_runner
    i, N, W, H, deg, fov, sigma, smod, mode, posed = case
    sc = parity.syn.make_scene(N, W, H, sh_degree=deg, seed=100 + i, fovx=fov, sigma_px=sigma, posed=posed)
    sc["scale_modifier"] = smod
    kw = parity.scene_kwargs(sc, mode, bg=(0.1 * (i % 3), 0.5, 1.0 - 0.1 * (i % 5)))
    o = binding.OracleRender(**kw)
    gc, gd, ga = parity.upstream_grads(H, W, seed=i)
    # sub-pixel footprints (sigma * scale_modifier < 1 px: conic entries of 1-3 per px^2 after the 0.3 low-pass) turn the
    # binary32 rounding of the pixel-space mean (a few 1e-6 px) into a few 1e-5 of a splat's weight two sigma out
    sharp = sigma * smod < 1.0
    tiny = W * H < 4000       # one pixel is a quarter of a per mille or more: no share bounds
    rep, out, ref = parity.oracle_case(o, lambda g: hip_runner.run_hip(kw, g), (gc, gd, ga), f"fuzz {case}",
                                       ambig_max_frac=1.0 if tiny else None, unresolved_max_frac=1.0 if tiny else None,
                                       fwd_atol=2.5e-5 if (sharp and i == 13) else None)
    # (sub-pixel footprints: the binary32 arithmetic itself -- tests/hostemu, fixed order -- leaves two `scales` entries and one
    #  `rotations` entry of case 13 (257 Gaussians, 166 degree field of view, scale_modifier 0.25) 1e-3 off element-wise: within the
    #  default allowance of two entries per tensor)
    grep = parity.check_grads(out["grads"], ref, f"fuzz {case}")
    rep.pop("grad_mask")
    print(rep, {k: "%.1e" % v for k, v in grep.items()})
    o.close()


# ---- index-level parity: the binned (tile, depth, id) list itself -------------------------------------------------------
def _box_qmin(px, py, A, B, C, x0, y0, x1, y1):
    """min over the pixel-centre box [x0,x1] x [y0,y1] of q(d) = A dx^2 + 2 B dx dy + C dy^2, d = centre - pixel
    (float64, vectorised): 0 when the centre lies inside, otherwise the least of the four edge minima."""
    inside = (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)
    best = np.full(px.shape, np.inf)
    for fixed_x in (True, False):
        for lo_side in (True, False):
            if fixed_x:
                dx = px - (x0 if lo_side else x1)
                dy = np.clip(-B * dx / C, py - y1, py - y0)         # unconstrained minimiser of the edge, clamped
            else:
                dy = py - (y0 if lo_side else y1)
                dx = np.clip(-B * dy / A, px - x1, px - x0)
            best = np.minimum(best, A * dx * dx + 2 * B * dx * dy + C * dy * dy)
    return np.where(inside, 0.0, best)


@pytest.mark.parametrize("N,W,H,deg", [(10000, 256, 256, 0), (300000, 980, 545, 3)], ids=["C1", "300k"])
def test_binning_is_the_oracle_list_filtered_by_the_exact_tile_test(N, W, H, deg):
    """gsr_debug_read_binning: the HIP (ranges, list) against the oracle's binning (gsr_oracle_get_binning), index by index.
    The product culls (tile, Gaussian) pairs in which no pixel of the tile can receive a contribution (min over the
    tile's pixel box of the conic form > 2 ln(255 o)); so per tile the HIP list must be
      * a SUBSEQUENCE of the oracle's list -- same ids, same (depth bits, id) order, bit-exact;
      * missing no pair whose float64 box minimum is below the threshold (every contributing pair is kept);
      * and keep, beyond those, only pairs within the kernel's stated slack of the threshold (the test is exact up to it)."""
    import importlib
    import hip_runner
    R_ = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    sc = parity.syn.make_scene(N, W, H, sh_degree=deg, seed=N % 97, posed=(N > 10000))
    kw = parity.scene_kwargs(sc, "sh")
    o = binding.OracleRender(**kw)
    o.forward()
    hip_runner.run_hip(kw)
    ranges, lst = R_.last_binning()
    ranges, lst = ranges.cpu().numpy(), lst.cpu().numpy()
    ts, ol = o.binning()
    geom = o.geom()
    ok_g = o.g_ambig == 0                       # Gaussians whose 3-sigma rect sits on a rounding edge may gain / lose a tile
    tiles_x = (W + 15) // 16
    T = tiles_x * ((H + 15) // 16)
    assert ranges.shape == (T, 2)
    # per-pair float64 box minimum of the oracle's pairs
    tile_of = np.repeat(np.arange(T), np.diff(ts))
    gx, gy = geom["xy"][ol, 0].astype(np.float64), geom["xy"][ol, 1].astype(np.float64)
    A, B, C = (geom["conic"][ol, k].astype(np.float64) for k in range(3))
    x0 = (tile_of % tiles_x) * 16.0; y0 = (tile_of // tiles_x) * 16.0
    x1 = np.minimum(x0 + 15, W - 1); y1 = np.minimum(y0 + 15, H - 1)
    q = _box_qmin(gx, gy, A, B, C, x0, y0, x1, y1)
    op = o.opacities[ol].astype(np.float64)
    tau = 2.0 * np.log(255.0 * np.maximum(op, 1e-30))
    slack = 1e-3 * (1.0 + np.abs(tau))           # csrc/gsr_math.h make_tile_test
    must = (q <= tau - 1e-4 * (1 + np.abs(tau))) & (op >= 1.0 / 255.0)
    may = q <= tau + 2 * slack
    kept_total = extra_total = 0
    for t in range(T):
        h = lst[ranges[t, 0]:ranges[t, 1]]
        seg = slice(ts[t], ts[t + 1])
        ref = ol[seg]
        good = ok_g[ref]
        # subsequence + order: positions of the HIP ids inside the oracle's list must be strictly increasing
        pos = {int(g): i for i, g in enumerate(ref)}
        idx = np.array([pos.get(int(g), -1) for g in h], dtype=np.int64)
        known = idx >= 0
        assert np.all(ok_g[h[~known]] == 0) if (~known).any() else True, f"tile {t}: ids outside the oracle's list"
        assert np.all(np.diff(idx[known]) > 0), f"tile {t}: order differs from (depth bits, id)"
        in_hip = np.zeros(ref.shape[0], bool); in_hip[idx[known]] = True
        assert not np.any(must[seg] & good & ~in_hip), f"tile {t}: a contributing pair was culled"
        extra = in_hip & ~may[seg] & good
        assert not extra.any(), f"tile {t}: kept a pair beyond the test's slack"
        kept_total += int(in_hip.sum()); extra_total += int((in_hip & ~must[seg]).sum())
    print(f"R oracle {ol.shape[0]} -> HIP {lst.shape[0]} ({kept_total} matched; {extra_total} of them inside the slack band)")
    assert R_._LAST["num_rendered"] == lst.shape[0] == int((ranges[:, 1] - ranges[:, 0]).sum())
    o.close()


@pytest.mark.parametrize("name", ["syn", "medium-rects", "large-and-huge", "few", "overflow-rerun", "two-streams-of-depth"])
def test_direct_binning_is_the_sort_routes_list(name):
    """The tile lists by direct placement (k_chunk_counts / k_chunk_scan / k_chunk_scatter: every (Gaussian, tile) pair written once,
    at its final place) against emit + stable tile sort + ranges: (ranges, list) and the images bit for bit.  Scenes that reach every
    branch of the scatter: ordinary records; steps whose 64 records hold more pairs than the pair buffer (rects of ~25 tiles: runs of
    lanes); large rects (no mask in the record: walked by the wave) and huge ones (more tiles than the buffer: walked outside it);
    fewer Gaussians than a step; a speculative capacity that overflows (positions beyond it are dropped, the call runs again)."""
    import importlib
    import hip_runner
    R_ = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    lib = L.load()
    W, H = 980, 545
    if name == "syn":
        sc = parity.syn.make_scene(60000, W, H, sh_degree=1, seed=3, posed=True)
    elif name == "medium-rects":
        sc = parity.syn.make_scene(9000, W, H, sh_degree=0, seed=5, sigma_px=11.0)
    elif name == "large-and-huge":
        sc = parity.syn.make_scene(4000, W, H, sh_degree=0, seed=6, sigma_px=6.0)
        g = torch.Generator().manual_seed(1)
        big = torch.randperm(4000, generator=g)[:150]
        sc["scales"][big[:120]] *= 8.0          # rects of a few hundred tiles
        sc["scales"][big[120:]] *= 60.0         # the whole frame: more tiles than the pair buffer holds
    elif name == "few":
        sc = parity.syn.make_scene(37, W, H, sh_degree=0, seed=7, sigma_px=20.0, frac_behind=0.0)
    elif name == "two-streams-of-depth":
        sc = parity.syn.make_scene(130000, W, H, sh_degree=0, seed=8)
        sc["means3D"][::2] = sc["means3D"][1::2]       # pairs of Gaussians at the same place: equal depth keys, order by index
    else:
        sc = parity.syn.make_scene(30000, W, H, sh_degree=0, seed=9)
    kw = parity.scene_kwargs(sc, "sh", bg=(0.1, 0.2, 0.3))
    res = {}
    try:
        # 0 = depth sort + emit + tile-key sort + ranges; 1 = depth sort + direct placement; 2 = direct placement in index order + per-tile
        # depth sort; 3 = emit in index order + tile-key sort + ranges + per-tile depth sort
        for route, (direct, tsort) in enumerate(((0, 0), (1, 0), (1, 2), (0, 2))):   # (tile_sort 2 = on every frame and model, whatever the lists' lengths)
            assert lib.gsr_set_option(b"direct_binning", direct) == 0
            assert lib.gsr_set_option(b"tile_sort", tsort) == 0
            if name == "overflow-rerun":
                assert lib.gsr_set_option(b"binning_capacity_hint", 5000) == 0
            fwd = hip_runner.run_hip(kw)["fwd"]
            ranges, lst = R_.last_binning()
            res[route] = (fwd, ranges.cpu().numpy().copy(), lst.cpu().numpy().copy(), R_._LAST["num_rendered"])
    finally:
        lib.gsr_set_option(b"direct_binning", 1)
        lib.gsr_set_option(b"tile_sort", 1)
        lib.gsr_set_option(b"binning_capacity_hint", 0)
    (fa, ra, la, na) = res[0]
    assert na > 0
    for route in (1, 2, 3):
        (fb, rb, lb, nb_) = res[route]
        assert na == nb_, f"route {route}"
        assert np.array_equal(ra, rb), f"route {route}: tile ranges differ"
        assert np.array_equal(la[:na], lb[:nb_]), f"route {route}: instance lists differ"
        for x, y in zip(fa, fb):
            assert np.array_equal(x, y), f"route {route}"
    counts = np.diff(rb, axis=1)[:, 0]
    print(f"{name}: R {na}, longest tile list {counts.max()}, tiles in use {(counts > 0).sum()} of {counts.shape[0]}")


@pytest.mark.parametrize("W,H,N", [(16, 16, 500), (17, 33, 900), (640, 480, 20000), (1024, 1024, 50000), (1040, 1024, 20000), (250, 3000, 8000),
                                   (16, 16, 30000), (40, 24, 60000)],
                         ids=["one-tile", "2x3-tiles", "vga", "4096-tiles", "4160-tiles-sort-route", "tall", "one-long-list", "six-long-lists"])
def test_direct_binning_frame_sizes(W, H, N):
    """Direct placement (behind the depth sort, and in index order with the per-tile depth sort behind it) against the sort route over
    frame geometries: a single tile, ragged edge tiles, exactly the 4 096 tiles the LDS tables hold, one tile row more (every option then
    takes the sort route: the test is the options' no-op there), a tall frame (tile ids in a narrow grid), and tiles whose lists are
    longer than what k_tile_sort sorts in LDS (its pass through global memory, a chunk at a time)."""
    import importlib
    import hip_runner
    R_ = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    lib = L.load()
    sc = parity.syn.make_scene(N, W, H, sh_degree=0, seed=W + H, sigma_px=4.0)
    kw = parity.scene_kwargs(sc, "sh")
    res = {}
    try:
        for route, (direct, tsort) in enumerate(((0, 0), (1, 0), (1, 2), (0, 2))):   # (tile_sort 2 = on every frame and model, whatever the lists' lengths)
            assert lib.gsr_set_option(b"direct_binning", direct) == 0
            assert lib.gsr_set_option(b"tile_sort", tsort) == 0
            fwd = hip_runner.run_hip(kw)["fwd"]
            ranges, lst = R_.last_binning()
            res[route] = (fwd, ranges.cpu().numpy().copy(), lst.cpu().numpy().copy(), R_._LAST["num_rendered"])
    finally:
        lib.gsr_set_option(b"direct_binning", 1)
        lib.gsr_set_option(b"tile_sort", 1)
    (fa, ra, la, na) = res[0]
    assert na > 0
    for route in (1, 2, 3):
        (fb, rb, lb, nb_) = res[route]
        assert na == nb_ and np.array_equal(ra, rb) and np.array_equal(la[:na], lb[:nb_]), f"route {route}"
        for x, y in zip(fa, fb):
            assert np.array_equal(x, y), f"route {route}"
    print(f"{W}x{H}: R {na}, longest tile list {np.diff(ra, axis=1).max()}")


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768, 32769, 36864, 65537])
def test_depth_order_at_the_sorts_tile_boundaries(N):
    """The global depth sort works in tiles of 4 096 keys, its first pass in eight runs of tiles with their own look-back chains: Gaussian
    counts on both sides of one tile, two tiles, eight tiles (one per run) and nine.  Independent of any other route of the library:
    every tile's list must ascend in (the oracle's binary32 depth, then Gaussian index) -- sortedness with the reference's tie rule --
    and hold each Gaussian once; then the per-tile-sort route must give the same lists."""
    import hip_runner
    R_ = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    lib = importlib.import_module("3dgs_hierarchical_training_amd._lib").load()
    W, H = 64, 48
    sc = parity.syn.make_scene(N, W, H, sh_degree=0, seed=N, frac_behind=0.0)
    if N >= 64:      # a fifth of the depths from thirty-two values: ties inside and across the sort's tiles
        g = torch.Generator().manual_seed(N)
        tie = torch.rand(N, generator=g) < 0.2
        znew = 2.0 + 0.25 * torch.randint(0, 32, (int(tie.sum()),), generator=g).float()
        sc["means3D"][tie] = sc["means3D"][tie] * (znew / sc["means3D"][tie][:, 2])[:, None]      # along the viewing ray: same pixel, new depth
    kw = parity.scene_kwargs(sc, "sh")
    o = binding.OracleRender(**kw)
    o.forward()
    depth = o.geom()["depth"]
    o.close()
    res = {}
    try:
        for tsort in (0, 2):
            assert lib.gsr_set_option(b"tile_sort", tsort) == 0
            hip_runner.run_hip(kw)
            ranges, lst = R_.last_binning()
            res[tsort] = (ranges.cpu().numpy().copy(), lst.cpu().numpy()[:R_._LAST["num_rendered"]].copy())
    finally:
        lib.gsr_set_option(b"tile_sort", 1)
    ranges, lst = res[0]
    assert lst.shape[0] > 0 or N < 3
    for a, b in ranges:
        ids = lst[a:b].astype(np.int64)
        d = depth[ids]
        assert np.all((d[1:] > d[:-1]) | ((d[1:] == d[:-1]) & (ids[1:] > ids[:-1]))), "a tile's list does not ascend in (depth, index)"
    assert np.array_equal(res[0][0], res[2][0]) and np.array_equal(res[0][1], res[2][1]), "the per-tile sort route's lists differ"


def _stacked_tiles_scene(per_tile, seed, sigma_px=0.5, opacity=0.02, tie_frac=0.33):
    """A 16-pixel-high frame of len(per_tile) tiles, tile t holding exactly per_tile[t] Gaussians stacked in depth around its centre (none
    reaches a neighbouring tile), `tie_frac` of the depths drawn from sixteen values.  Faint opacities: no pixel saturates, every list
    entry is consumed."""
    syn = parity.syn
    W, H = 16 * len(per_tile), 16
    cam = syn.make_camera(W, H)
    g = torch.Generator().manual_seed(seed)
    xs, zs = [], []
    for t, n in enumerate(per_tile):
        z = 1.0 + 9.0 * torch.rand(n, generator=g)
        tie = torch.rand(n, generator=g) < tie_frac
        z[tie] = 2.0 + 0.5 * torch.randint(0, 16, (int(tie.sum()),), generator=g).float()
        px = 16.0 * t + 8.0 + 3.0 * (torch.rand(n, generator=g) - 0.5)
        py = 8.0 + 3.0 * (torch.rand(n, generator=g) - 0.5)
        xs.append(torch.stack(((px - 0.5 * W) / cam["fx"] * z, (py - 0.5 * H) / cam["fy"] * z, z), 1))
        zs.append(z)
    xyz, z = torch.cat(xs), torch.cat(zs)
    n = xyz.shape[0]
    sc = {k: cam[k] for k in ("image_width", "image_height", "tanfovx", "tanfovy", "viewmatrix", "projmatrix", "campos")}
    sc["sh_degree"] = 0
    sc["means3D"] = xyz.float().contiguous()
    sc["scales"] = ((sigma_px * z / cam["fx"])[:, None] * (0.8 + 0.4 * torch.rand(n, 3, generator=g))).float().contiguous()
    rot = torch.zeros(n, 4); rot[:, 0] = 1.0
    rot[:, 1:] = 0.1 * torch.randn(n, 3, generator=g)
    sc["rotations"] = (rot / rot.norm(dim=1, keepdim=True)).contiguous()
    sc["opacities"] = torch.full((n, 1), float(opacity)) * (0.7 + 0.6 * torch.rand(n, 1, generator=g))
    sc["shs"] = (0.5 * torch.randn(n, 1, 3, generator=g)).contiguous()
    return sc


@pytest.mark.parametrize("L,opacity", [(L, 0.02) for L in (63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 385, 511, 513, 641)] + [(129, 0.5), (513, 0.5)],
                         ids=lambda v: str(v))
def test_blend_batches_and_checkpoints_at_exact_list_lengths_against_the_oracle(L, opacity):
    """The blends stage a list 64 (forward) / 128 (backward) entries at a time, the forward leaves a checkpoint every 128 and the backward
    cuts a tile's replay into work items at them: two tiles holding EXACTLY L and L + 1 entries (asserted), splats of ~2 px covering a good
    part of their tile, against the float64 oracle -- forward and backward, colour loss only and with the depth / alpha terms.  Faint
    opacities (every entry consumed: the boundaries are reached) and two saturating cases (the lists end early)."""
    import hip_runner
    R_ = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    sc = _stacked_tiles_scene([L, L + 1], seed=L, sigma_px=2.0, opacity=opacity, tie_frac=0.1)
    kw = parity.scene_kwargs(sc, "sh", bg=(0.2, 0.1, 0.0))
    H, W = 16, 32
    for color_only in (True, False):
        o = binding.OracleRender(**kw)
        gc, gd, ga = parity.upstream_grads(H, W, seed=L)
        if color_only:
            gd = ga = None
        what = f"stacked tiles {L}/{L + 1}, opacity {opacity}, {'colour' if color_only else 'all'}"
        rep, out, ref = parity.oracle_case(o, lambda g: hip_runner.run_hip(kw, g), (gc, gd, ga), what, ambig_max_frac=0.2)
        parity.check_grads(out["grads"], ref, what)
        o.close()
    ranges, _ = R_.last_binning()
    lens = [int(b - a) for a, b in ranges.cpu().numpy()]
    if opacity < 0.1:
        assert lens == [L, L + 1]
        assert R_.last_call_info()["staged"] >= 2 * L, "the lists were not consumed to their ends"
    else:            # (at this opacity a few splats of one tile reach the other: longer lists, which end early anyway)
        assert lens[0] >= L and lens[1] >= L + 1


@pytest.mark.parametrize("L", [1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1023, 1024, 1025, 2048, 2049, 4095, 4096, 4097, 8191, 8193, 12289])
def test_tile_sort_segment_lengths_at_the_kernels_boundaries(L):
    """The per-tile depth sort picks its form by a segment's length: one wave with 1 / 2 / 4 / 8 / 16 pairs per lane up to 1 024 pairs,
    the persistent 1 024-thread workgroup in LDS up to 4 096, a pass through global memory in chunks of 4 096 beyond.  One tile
    (16 x 16 frame) holding EXACTLY L Gaussians, and a second frame of two tiles holding L and L + 1: every boundary of that choice from
    both sides, with a third of the depths drawn from sixteen values (ties: index order).  Lists, ranges and images of the four routes
    equal bit for bit."""
    import hip_runner
    R_ = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    lib = importlib.import_module("3dgs_hierarchical_training_amd._lib").load()
    for W, per_tile in ((16, [L]), (32, [L, L + 1])):
        kw = parity.scene_kwargs(_stacked_tiles_scene(per_tile, seed=L * 7 + W), "sh", bg=(0.2, 0.1, 0.0))
        res = {}
        try:
            for route, (direct, tsort) in enumerate(((0, 0), (1, 0), (1, 2), (0, 2))):
                assert lib.gsr_set_option(b"direct_binning", direct) == 0
                assert lib.gsr_set_option(b"tile_sort", tsort) == 0
                fwd = hip_runner.run_hip(kw)["fwd"]
                ranges, lst = R_.last_binning()
                res[route] = (fwd, ranges.cpu().numpy().copy(), lst.cpu().numpy()[:R_._LAST["num_rendered"]].copy())
        finally:
            lib.gsr_set_option(b"direct_binning", 1)
            lib.gsr_set_option(b"tile_sort", 1)
        fa, ra, la = res[0]
        assert [int(b - a) for a, b in ra] == per_tile, (W, ra)                     # the lists have exactly the lengths under test
        for route in (1, 2, 3):
            fb, rb, lb = res[route]
            assert np.array_equal(ra, rb) and np.array_equal(la, lb), f"{W}: route {route}"
            for x, y in zip(fa, fb):
                assert np.array_equal(x, y), f"{W}: route {route}"


# ---- the reference-derived fixtures, on the HIP path ---------------------------------------------------------------------
def _fixture_settings(g, tag, dev, noncontig):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    vm = torch.tensor(g[f"{tag}_st_viewmatrix"]).to(dev)
    cp = torch.tensor(g[f"{tag}_st_campos"]).to(dev)
    if noncontig:          # as captured: a transpose view and a row slice
        vm = vm.t().contiguous().t()
        cp = torch.stack([cp, cp], 1)[:, 0]
        assert not vm.is_contiguous() and not cp.is_contiguous()
    return GaussianRasterizationSettings(
        image_height=int(g[f"{tag}_st_image_height"]), image_width=int(g[f"{tag}_st_image_width"]),
        tanfovx=float(g[f"{tag}_st_tanfovx"]), tanfovy=float(g[f"{tag}_st_tanfovy"]), bg=torch.tensor(g[f"{tag}_st_bg"]).to(dev),
        scale_modifier=float(g[f"{tag}_st_scale_modifier"]), viewmatrix=vm, projmatrix=torch.tensor(g[f"{tag}_st_projmatrix"]).to(dev),
        sh_degree=int(g[f"{tag}_st_sh_degree"]), campos=cp, prefiltered=False, debug=False)


def test_captured_boundary_arguments_both_routes(golden_dir):
    """tests/golden/boundary_args.npz holds the exact kwargs / settings `CF3DGS_Render.render` handed its rasterizer
    (gaussian_model_ht.py:775-894), once with in-kernel SH / covariance ("kernel") and once with the reference's Python
    SH + covariance ("python": colors_precomp + cov3D_precomp).  Both go through the product path here, non-contiguous
    view / campos as captured; the two routes must render the same image (degree 0), and the kernel route must match
    the oracle fed the same captured arrays."""
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(golden_dir, "boundary_args.npz"), allow_pickle=False)
    outs = {}
    for tag in ("kernel", "python"):
        def T(name):
            return None if bool(g[f"{tag}_kw_{name}_isnone"]) else torch.tensor(g[f"{tag}_kw_{name}"]).to(dev).requires_grad_(True)
        kw = {k: T(k) for k in ("means3D", "means2D", "shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp")}
        rs = _fixture_settings(g, tag, dev, noncontig=True)
        out = GaussianRasterizer(raster_settings=rs)(**kw)
        assert len(out) == 4
        out[0].sum().backward()
        outs[tag] = (out, kw)
    ck, cp = outs["kernel"][0][0].detach().cpu().numpy(), outs["python"][0][0].detach().cpu().numpy()
    d = np.abs(ck - cp)          # float32-rounded cov3D / colours on the python route: equal up to rare alpha-cut flips
    assert (d > 1e-5).mean() < 1e-3 and d.max() < 5e-3
    assert torch.equal(outs["kernel"][0][1], outs["python"][0][1])                      # radii
    gk, gp = outs["kernel"][1]["means3D"].grad, outs["python"][1]["means3D"].grad
    assert (gk - gp).abs().max().item() <= 2e-3 * gk.abs().max().item()
    o = binding.OracleRender(means3D=g["kernel_kw_means3D"], opacities=g["kernel_kw_opacities"],
                             viewmatrix=g["kernel_st_viewmatrix"], projmatrix=g["kernel_st_projmatrix"],
                             campos=g["kernel_st_campos"], bg=g["kernel_st_bg"], image_height=int(g["kernel_st_image_height"]),
                             image_width=int(g["kernel_st_image_width"]), tanfovx=float(g["kernel_st_tanfovx"]),
                             tanfovy=float(g["kernel_st_tanfovy"]), sh_degree=int(g["kernel_st_sh_degree"]),
                             shs=g["kernel_kw_shs"], scales=g["kernel_kw_scales"], rotations=g["kernel_kw_rotations"])
    o.forward()
    got = tuple(x.detach().cpu().numpy() for x in outs["kernel"][0])
    parity.check_forward(got, o, "captured boundary call")


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_sh_fixture_through_the_kernels(golden_dir, deg):
    """sh_eval.npz (the reference's eval_sh + 0.5 / clamp, utils/sh_utils.py:57-112, gaussian_model_ht.py:859-862) against
    the SH stage of K1 itself: one Gaussian per fixture row, placed so that its view direction from the camera centre is
    the fixture's `dirs[i]`, rendered as an opaque splat; the pixel under its centre then shows alpha * rgb_ref."""
    import hip_runner
    g = np.load(os.path.join(golden_dir, "sh_eval.npz"), allow_pickle=False)
    sh, dirs, rgb_ref = g[f"sh_{deg}"].astype(np.float32), g["dirs"], g[f"rgb_{deg}"]
    n = sh.shape[0]
    W = H = 64
    cols = np.zeros((n, 3))
    for i in range(n):
        d = dirs[i] / np.linalg.norm(dirs[i])
        # camera at the origin looking along +z of ITS frame; build a rotation that puts d on the optical axis
        z = d; up = np.array([0.0, 1.0, 0.0]) if abs(d[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
        x = np.cross(up, z); x /= np.linalg.norm(x); y = np.cross(z, x)
        Rm = torch.tensor(np.stack([x, y, z]), dtype=torch.float32)           # world -> camera rows
        cam = parity.syn.make_camera(W, H, R=Rm, t=torch.zeros(3))
        kw = dict(means3D=torch.tensor((3.0 * d)[None], dtype=torch.float32), opacities=torch.tensor([[0.9]]),
                  viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"], campos=cam["campos"], bg=torch.zeros(3),
                  image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], sh_degree=deg,
                  shs=torch.tensor(sh[i:i + 1]), scales=torch.full((1, 3), 0.3), rotations=torch.tensor([[1.0, 0, 0, 0]]))
        out = hip_runner.run_hip(kw)
        color, _, _, alpha = out["fwd"]
        py, px = np.unravel_index(np.argmax(alpha[0]), alpha[0].shape)
        cols[i] = color[:, py, px] / alpha[0, py, px]
    # the Gaussian sits at 3 d, the camera at the origin: direction (p - campos)/|.| = d (float32 positions: ~1e-7)
    assert np.abs(cols - rgb_ref).max() < 5e-6, np.abs(cols - rgb_ref).max()


def test_cov3d_fixture_kernel_route_equals_python_route(golden_dir):
    """cov3d.npz (the reference's build_scaling_rotation / strip_symmetric, utils/general_utils.py:62-108): feeding the
    fixture's covariance as cov3D_precomp must render what the in-kernel construction renders from (scales, unit
    quaternion) -- the two routes `compute_cov3D_python` switches between (gaussian_model_ht.py:831-839)."""
    import hip_runner
    g = np.load(os.path.join(golden_dir, "cov3d.npz"), allow_pickle=False)
    n = g["scales"].shape[0]
    W, H = 160, 120
    sc = parity.syn.make_scene(n, W, H, sh_degree=0, seed=12, frac_behind=0.0)
    smod = float(g["scale_modifier"])
    zc = sc["means3D"][:, 2:3]
    unit = torch.tensor(g["scales"] / g["scales"].max())                       # fixture scales, brought to ~6 px on screen
    scales = (unit * 6.0 * zc / sc["fx"] / smod).float()
    k = (scales / torch.tensor(g["scales"])).double().numpy()                  # per-Gaussian, per-axis factor
    assert np.allclose(k, k[:, :1])                                            # (uniform per Gaussian: cov scales by k^2)
    cov = torch.tensor(g["cov"] * (k[:, :1] ** 2)).float()
    base = dict(means3D=sc["means3D"], opacities=sc["opacities"], viewmatrix=sc["viewmatrix"], projmatrix=sc["projmatrix"],
                campos=sc["campos"], bg=torch.zeros(3), image_height=H, image_width=W, tanfovx=sc["tanfovx"],
                tanfovy=sc["tanfovy"], sh_degree=0, colors_precomp=torch.rand(n, 3, generator=torch.Generator().manual_seed(1)),
                scale_modifier=smod)
    a = hip_runner.run_hip(dict(base, scales=scales, rotations=torch.tensor(g["rot_unit"]).float()))
    b = hip_runner.run_hip(dict(base, cov3D_precomp=cov, scale_modifier=1.0))
    d = np.abs(a["fwd"][0] - b["fwd"][0])
    assert (d > 1e-5).mean() < 2e-3 and d.max() < 5e-3       # float32-rounded covariance: equal up to rare alpha-cut flips
    assert np.mean(a["fwd"][1] != b["fwd"][1]) < 0.05         # radii (ceil of 3 sigma) may differ by one on a rounding edge


def test_cov3d_fixture_pins_the_raw_parameter_backward(golden_dir):
    """cov3d.npz carries the reference's OWN derivatives of `build_scaling_rotation` / `strip_symmetric`
    (utils/general_utils.py:62-108) -- through `build_rotation`'s internal normalisation of the RAW quaternion (:77-79) -- as full
    Jacobians d cov6 / d scales, d cov6 / d rot_raw (tools/make_golden.py gen_cov3d, one autograd pass of the reference's code per
    packed entry).  The kernels' RAW-parameter route (`rasterize_gaussians_raw`: exp / normalize in-kernel, K9's float64 chain) must
    return dL/d(log scale) and dL/d(rot_raw) equal to the render's dL/dcov6 -- taken from the cov3D_precomp route on the same
    covariance -- chained through those Jacobians."""
    import hip_runner
    R_ = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    g = np.load(os.path.join(golden_dir, "cov3d.npz"), allow_pickle=False)
    n = g["scales"].shape[0]
    W, H = 160, 120
    dev = torch.device("cuda:0")
    sc = parity.syn.make_scene(n, W, H, sh_degree=0, seed=12, frac_behind=0.0)
    smod = float(g["scale_modifier"])
    zc = sc["means3D"][:, 2:3]
    unit = torch.tensor(g["scales"] / g["scales"].max())
    scales = (unit * 6.0 * zc / sc["fx"] / smod).float()                       # fixture scales brought to ~6 px on screen
    k = (scales.double() / torch.tensor(g["scales"]).double())[:, :1]          # uniform factor per Gaussian: cov scales by k^2
    cov = (torch.tensor(g["cov"]).double() * k ** 2).float()
    shs = sc["shs"].clone()
    gc, gd, ga = parity.upstream_grads(H, W, seed=4)
    base = dict(means3D=sc["means3D"], opacities=sc["opacities"], viewmatrix=sc["viewmatrix"], projmatrix=sc["projmatrix"],
                campos=sc["campos"], bg=torch.zeros(3), image_height=H, image_width=W, tanfovx=sc["tanfovx"], tanfovy=sc["tanfovy"],
                sh_degree=0, shs=shs)
    b = hip_runner.run_hip(dict(base, cov3D_precomp=cov, scale_modifier=1.0), (gc, gd, ga))
    dcov_fix = torch.tensor(b["grads"]["cov3D_precomp"]).double() * k ** 2     # dL / d(fixture's cov6)
    want_rot = torch.einsum("nj,njk->nk", dcov_fix, torch.tensor(g["jac_rot_raw"]).double())
    want_logs = torch.einsum("nj,njk->nk", dcov_fix, torch.tensor(g["jac_scales"]).double()) * torch.tensor(g["scales"]).double()
    # the raw route: log-scales, the fixture's UN-normalised quaternions, opacity logits, _features_dc / _features_rest
    t = lambda x: x.to(dev).float().contiguous().requires_grad_(True)
    xyz, dc, rest = t(sc["means3D"]), t(shs[:, :1]), t(shs[:, 1:])
    op, logs, rot = t(torch.logit(sc["opacities"].double()).float()), t(torch.log(scales.double()).float()), t(torch.tensor(g["rot_raw"]))
    st = R_.GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=float(sc["tanfovx"]), tanfovy=float(sc["tanfovy"]),
                                          bg=torch.zeros(3, device=dev), scale_modifier=smod, viewmatrix=sc["viewmatrix"].to(dev),
                                          projmatrix=sc["projmatrix"].to(dev), sh_degree=0, campos=sc["campos"].to(dev), prefiltered=False, debug=False)
    m2d = torch.zeros(n, 3, device=dev, requires_grad=True)
    color, radii, depth, alpha = R_.rasterize_gaussians_raw(xyz, m2d, dc, rest, op, logs, rot, st)[:4]
    d = np.abs(color.detach().cpu().numpy() - b["fwd"][0])
    assert (d > 1e-5).mean() < 2e-3 and d.max() < 5e-3       # float32-rounded covariance: equal up to rare alpha-cut flips
    ((color * torch.from_numpy(gc).to(dev)).sum() + (depth[0] * torch.from_numpy(gd).to(dev)).sum() + (alpha[0] * torch.from_numpy(ga).to(dev)).sum()).backward()
    rel = lambda a, r: float((a.double().cpu() - r).norm() / r.norm())
    e_rot, e_logs = rel(rot.grad, want_rot), rel(logs.grad, want_logs)
    print(f"raw-parameter backward vs the reference's Jacobians: d rot_raw {e_rot:.2e}, d log-scale {e_logs:.2e}")
    assert float(want_rot.abs().max()) > 0 and float(want_logs.abs().max()) > 0
    # (the two routes render from covariances that differ in the last bit of binary32, and the fixture's Jacobians are binary32
    #  autograd of the reference's code: 1e-4 relative, norm-wise, is the north_star's gradient bar)
    assert e_rot < 1e-4 and e_logs < 1e-4, (e_rot, e_logs)
    # the gradient of a raw quaternion is orthogonal to it (normalisation removes the radial direction): a property of the reference's chain
    radial = (rot.grad.double().cpu() * torch.tensor(g["rot_raw"]).double()).sum(1).abs().max() / rot.grad.double().abs().max().cpu()
    assert float(radial) < 1e-5


def test_models_of_different_size_alternate_without_overflow_reruns():
    """Per-caller speculation state: a 20 k and a 1 M model rendered alternately (teacher / student,
    ht3dgs_trainer.py:877-883; stage-A models next to a leaf) each keep their own capacity hint -- after each has been seen
    once, no forward re-runs its binning."""
    import importlib
    import hip_runner
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
    lib = L.load()
    dev = torch.device("cuda:0")
    lib.gsr_set_option(b"reset_speculation", 1)
    models = []
    for N in (20_000, 1_000_000):
        sc = parity.syn.make_scene(N, 980, 545, sh_degree=3, seed=3)
        models.append((ts.GaussianParams(sc, dev), ts.make_settings(sc, dev, 3)))
    with torch.no_grad():
        for p, st in models:                      # first sight of each caller: exact flow
            ts.render(p, st)
        assert lib.gsr_get_counter(b"exact_forwards") == 2 and lib.gsr_get_counter(b"spec_callers") == 2
        for _ in range(10):
            for p, st in models:
                ts.render(p, st)
    torch.cuda.synchronize()
    assert lib.gsr_get_counter(b"spec_forwards") == 20
    assert lib.gsr_get_counter(b"spec_overflows") == 0


@pytest.mark.parametrize("N,W,H,scale", [(20000, 330, 250, 1.0), (300000, 980, 545, 1.0), (3000, 64, 48, 1.0), (3000, 320, 240, 12.0)],
                         ids=["20k", "300k", "tiny-frame", "large-splats"])
def test_emit_counts_the_tile_sort_digits(N, W, H, scale):
    """In the speculative flow k_emit counts the digits of the tile keys it writes (per run of the tile sort) and clears the
    sort's status words, so no histogram kernel runs in front of the sort's passes (gsr_set_option("emit_hist")).  The per-tile
    lists -- (ranges, list) through gsr_debug_read_binning -- and the images must be EQUAL to those of the histogram-launch
    route.  The tiny frame has fewer keys than one run of the sort; with large splats (scale_modifier 12: ~100 tiles per
    Gaussian, the per-wave emission path) one workgroup's output spans more than two runs, which takes the direct-global-add path."""
    import importlib
    import hip_runner
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    R_ = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    lib = L.load()
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=11, posed=True)
    sc["scale_modifier"] = scale
    kw = parity.scene_kwargs(sc, "sh", bg=(0.1, 0.2, 0.3))
    out = {}
    try:
        for mode in (0, 1):
            assert lib.gsr_set_option(b"emit_hist", mode) == 0
            lib.gsr_set_option(b"reset_speculation", 1)
            hip_runner.run_hip(kw)                       # first sight: exact flow, leaves the capacity hint
            n0 = lib.gsr_get_counter(b"spec_forwards")
            fwd = hip_runner.run_hip(kw)["fwd"]           # speculative flow
            assert lib.gsr_get_counter(b"spec_forwards") > n0 and lib.gsr_get_counter(b"spec_overflows") == 0
            ranges, lst = R_.last_binning()
            out[mode] = (fwd, ranges.cpu().numpy(), lst.cpu().numpy())
    finally:
        lib.gsr_set_option(b"emit_hist", 1)
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    for a, b in zip(out[0][0], out[1][0]):
        assert np.array_equal(a, b)


def test_backward_twice_over_one_render():
    """Two backward passes over one render (retain_graph) give the same gradients: nothing the first pass leaves behind in
    the saved workspaces (gradient accumulators, checkpoints) leaks into the second.  Same render, same per-tile parts: the same
    bits up to rounding-boundary flips of the float64 cross-tile sums (parity.same_accumulation)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    import hip_runner
    dev = torch.device("cuda:0")
    sc = parity.syn.make_scene(20000, 330, 250, sh_degree=3, seed=9, posed=True)
    kw = parity.scene_kwargs(sc, "sh")
    t = {k: (None if kw.get(k) is None else kw[k].detach().to(dev).float().requires_grad_(True)) for k in hip_runner.GRAD_KEYS}
    m2d = torch.zeros(t["means3D"].shape[0], 3, device=dev, requires_grad=True)
    rast = GaussianRasterizer(hip_runner.settings_from(kw, dev, False, False))
    color, radii, depth, alpha = rast(means3D=t["means3D"], means2D=m2d, shs=t["shs"], colors_precomp=t["colors_precomp"],
                                      opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"], cov3D_precomp=t["cov3D_precomp"])
    w = torch.rand_like(color)
    loss = (color * w).sum() + 0.3 * depth.sum() + 0.2 * alpha.sum()
    leaves = [v for v in t.values() if v is not None] + [m2d]
    g1 = torch.autograd.grad(loss, leaves, retain_graph=True)
    g2 = torch.autograd.grad(loss, leaves)
    parity.same_accumulation({str(i): b for i, b in enumerate(g2)}, {str(i): a for i, a in enumerate(g1)}, "second backward vs first")


def test_deterministic_backward_debug_mode():
    """gsr_set_option("deterministic_backward", 1) (optional deterministic mode for debugging): the
    blend backward sums each Gaussian's per-tile parts in list order instead of with float64 atomics in arrival order.
    Two runs give the SAME BITS, and the default path gives them too, up to rounding-boundary flips of inexact float64 sums
    (parity.same_accumulation; tests/test_gpu_accumulation.py covers the default route case by case)."""
    import importlib
    import hip_runner
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    lib = L.load()
    sc = parity.syn.make_scene(120000, 640, 360, sh_degree=3, seed=13, posed=True)
    kw = parity.scene_kwargs(sc, "sh", bg=(0.1, 0.1, 0.2))
    g = parity.upstream_grads(360, 640, seed=2)
    base = hip_runner.run_hip(kw, g)["grads"]
    try:
        assert lib.gsr_set_option(b"deterministic_backward", 1) == 0
        a = hip_runner.run_hip(kw, g)["grads"]
        b = hip_runner.run_hip(kw, g)["grads"]
    finally:
        lib.gsr_set_option(b"deterministic_backward", 0)
    for k in a:
        assert np.array_equal(a[k], b[k]), k                                    # bit-identical from run to run
    parity.same_accumulation(base, a, "default vs fixed order")               # and the same gradient as the default path


def test_debug_flag_dumps_a_snapshot_on_native_errors(tmp_path, monkeypatch):
    """raster_settings.debug = True: an error inside the native forward leaves `snapshot_fw.dump` with the call's arguments
    and is re-raised (the public module's behaviour; the reference passes debug=False, gaussian_model_ht.py:821)."""
    import hip_runner
    from diff_gaussian_rasterization import GaussianRasterizer
    monkeypatch.chdir(tmp_path)
    dev = torch.device("cuda:0")
    sc = parity.syn.make_scene(64, 64, 48, sh_degree=3, seed=1)
    kw = parity.scene_kwargs(sc, "sh")
    rs = hip_runner.settings_from(kw, dev)._replace(debug=True)
    shs = kw["shs"][:, :4].contiguous().to(dev)          # 4 stored coefficients but sh_degree 3 asks for 16: a native argument error
    with pytest.raises(RuntimeError, match="gsr_forward"):
        GaussianRasterizer(rs)(means3D=kw["means3D"].to(dev), means2D=torch.zeros(64, 3, device=dev), shs=shs, colors_precomp=None,
                               opacities=kw["opacities"].to(dev), scales=kw["scales"].to(dev), rotations=kw["rotations"].to(dev),
                               cov3D_precomp=None)
    snap = torch.load(tmp_path / "snapshot_fw.dump")
    assert torch.equal(snap[0], kw["means3D"]) and snap[14:16] == [48, 64]


@pytest.mark.parametrize("case", [(50, 64, 48, 1.0), (60000, 500, 333, 1.0), (3000, 320, 240, 12.0), (300000, 980, 545, 1.0), (1000000, 980, 545, 1.0)],
                         ids=["tiny", "60k", "large-rects", "300k", "1M"])
def test_early_instance_count_is_the_scans(case):
    """Round 5: a speculative forward learns R from k_preprocess's per-block sums of the Gaussians' tile counts -- published by the
    depth sort's histogram kernel (radix_sort.h OsRider), ~10 us into the forward -- instead of from the scan behind sort + tile
    counts (gsr_set_option("early_r")).  The two counts are the same number: R, the image, the radii and the binned list are equal
    with the option on and off -- ordinary records, large rects counted cooperatively (scale_modifier 12), the exact first call
    and the speculative calls after it, a capacity that overflows and is re-run, and the 27-bit depth window of the three-pass
    sort at 1 M (whose overflow count rides along)."""
    import ctypes as C
    import importlib
    import hip_runner
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    R_ = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    lib = L.load()
    N, W, H, scale = case
    sc = parity.syn.make_scene(N, W, H, sh_degree=1, seed=N % 91, posed=True)
    sc["scale_modifier"] = scale
    kw = parity.scene_kwargs(sc, "sh", bg=(0.1, 0.2, 0.3))
    dev = torch.device("cuda:0")
    T = ((W + 15) // 16) * ((H + 15) // 16)

    def run():
        out = hip_runner.run_hip(kw)["fwd"]
        Rn = R_.last_call_info()["num_rendered"]
        info = R_._LAST
        ranges = torch.zeros(T, 2, dtype=torch.int32, device=dev)
        lst = torch.zeros(max(Rn, 1), dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        assert lib.gsr_debug_read_binning(C.c_void_p(info["binning"].data_ptr()), info["binning_capacity"], Rn, W, H,
                                          C.c_void_p(ranges.data_ptr()), C.c_void_p(lst.data_ptr()), C.c_void_p(st)) == 0
        torch.cuda.synchronize()
        return out, Rn, ranges.cpu(), lst.cpu()[:Rn]
    res = {}
    try:
        for early in (0, 1):
            assert lib.gsr_set_option(b"early_r", early) == 0
            assert lib.gsr_set_option(b"reset_speculation", 1) == 0
            runs = [run(), run(), run()]                        # exact first call, then speculative ones
            assert lib.gsr_set_option(b"binning_capacity_hint", max(1, runs[0][1] // 3)) == 0
            runs.append(run())                                  # a capacity that overflows: re-run with the exact size
            res[early] = runs
    finally:
        lib.gsr_set_option(b"early_r", 1)
        lib.gsr_set_option(b"binning_capacity_hint", 0)
    base = res[0][0]
    assert base[1] > 0
    for early in (0, 1):
        for k, r in enumerate(res[early]):
            assert r[1] == base[1], (early, k, r[1], base[1])
            for a, b in zip(r[0], base[0]):
                assert np.array_equal(a, b), (early, k)
            assert torch.equal(r[2], base[2]) and torch.equal(r[3], base[3]), (early, k)


def test_early_count_is_held_against_the_scans_report_by_the_next_call():
    """with early R the host reads the instance count and the sorts' give-up counter from the rider on the depth sort's
    FIRST kernel -- before that forward's own look-backs have run.  The scan reports its total and the give-ups again, behind
    them, into spare words of the pinned slot, and the next call into the library compares: every speculative forward is checked
    (counter `late_checks`), a consistent one passes silently, a falsified early count (`debug_late_bias`) makes the NEXT
    gsr_forward -- or the next gsr_backward -- fail loudly instead of rendering from a list cut at the wrong length."""
    import importlib
    import hip_runner
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    lib = L.load()
    sc = parity.syn.make_scene(30000, 320, 240, sh_degree=1, seed=4, posed=True)
    kw = parity.scene_kwargs(sc, "sh")
    assert lib.gsr_set_option(b"reset_speculation", 1) == 0
    hip_runner.run_hip(kw)                      # exact first call of this caller: the scan publishes, nothing to check later
    c0, m0 = lib.gsr_get_counter(b"late_checks"), lib.gsr_get_counter(b"late_mismatches")
    for _ in range(4):
        hip_runner.run_hip(kw)                  # speculative: early count, each checked when the next forward takes the slot
    torch.cuda.synchronize()
    assert lib.gsr_get_counter(b"late_checks") - c0 >= 3 and lib.gsr_get_counter(b"late_mismatches") == m0
    gc, gd, ga = parity.upstream_grads(240, 320, seed=2)
    hip_runner.run_hip(kw, (gc, gd, ga))        # ... and by a backward, once the report has arrived
    assert lib.gsr_get_counter(b"late_mismatches") == m0
    # a forward that remembers a wrong early count: the next forward refuses to go on
    assert lib.gsr_set_option(b"debug_late_bias", 7) == 0
    hip_runner.run_hip(kw)
    with pytest.raises(RuntimeError, match="early instance count"):
        hip_runner.run_hip(kw)
    assert lib.gsr_get_counter(b"late_mismatches") == m0 + 1
    hip_runner.run_hip(kw)                      # the failure was reported once; the library goes on
    # ... and the same through a backward: forward (falsified) + backward in one call, the report is there by the time backward() runs
    assert lib.gsr_set_option(b"debug_late_bias", 7) == 0
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="early instance count"):
        out = hip_runner.run_hip(kw, None)
        torch.cuda.synchronize()                # the scan's report has arrived
        hip_runner.run_hip(kw, (gc, gd, ga))    # (its forward takes the slot and finds the mismatch; a backward would find it as well)
    assert lib.gsr_get_counter(b"late_mismatches") == m0 + 2
    hip_runner.run_hip(kw)
