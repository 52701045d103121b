"""GPU: fused L1+SSIM loss kernels vs the torch restatement of the reference's formula
(train_step.ssim, itself pinned to the reference's SSIM_V2 by tests/golden/loss.npz).  Floating point:
value within 1e-6 abs, gradient within 1e-4 relative (norm-wise).  Those two figures are what float32 reaches on white noise (the
first test's input); the tests of the second half hold the kernels to float64 on smooth training-like images too, every case at twice
the error the float32 arithmetic of the reference's own formula shows on its scene (tests/photometric_loss_common.py)."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
loss_mod = importlib.import_module("3dgs_hierarchical_training_amd.loss")


@pytest.mark.parametrize("H,W", [(40, 56), (545, 980), (33, 17), (16, 16), (1, 1), (3, 50), (11, 5), (17, 1), (129, 257)])
@pytest.mark.parametrize("lam", [0.2, 1.0, 0.0])
def test_fused_loss_matches_torch(H, W, lam):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(H * W)
    gt = torch.rand(3, H, W, generator=g).to(dev)
    raw = (gt.cpu() + 0.3 * torch.randn(3, H, W, generator=g)).to(dev)      # exercises the clamp on both sides
    raw_ref = raw.double().requires_grad_(True)
    ref = ts.photometric_loss(raw_ref.clamp(0, 1), gt.double(), lam)
    ref.backward()
    raw_f = raw.clone().requires_grad_(True)
    out = loss_mod.fused_photometric_loss(raw_f, gt, lam, clamp=True)
    (out * 1.5).backward()
    assert abs(float(out) - float(ref)) < 2e-6
    gref = 1.5 * raw_ref.grad
    err = (raw_f.grad.double() - gref).abs().max().item()
    assert err <= 1e-4 * gref.abs().max().item(), (err, gref.abs().max().item())


def test_fused_loss_golden(golden_dir):
    import os
    g = np.load(os.path.join(golden_dir, "loss.npz"))
    dev = torch.device("cuda:0")
    a, b = torch.tensor(g["img_a"]).to(dev), torch.tensor(g["img_b"]).to(dev)
    lam = float(g["lambda_dssim"])
    ref = (1 - lam) * float(g["l1"]) + lam * (1 - float(g["ssim"]))
    out = loss_mod.fused_photometric_loss(a, b, lam, clamp=False)
    assert abs(float(out) - ref) < 1e-5


@pytest.mark.parametrize("lam", [0.2, 0.0])
def test_loss_report_is_the_reference_dict_from_one_forward(lam):
    """Round 5: `photometric_loss_terms` returns the differentiable loss and the six-float vector {loss, mean SSIM, mean L1,
    loss_rgb = (1 - lambda) mean L1, loss_dssim = 1 - mean SSIM, loss_depth = 0} written by the same finishing kernel -- every entry
    of the dict `Loss.forward` returns (/root/reference/trainer/losses.py:128-136) without a torch kernel per term; only `loss`
    carries a gradient, and it is the gradient of `fused_photometric_loss`."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(11)
    H, W = 97, 131
    gt = torch.rand(3, H, W, generator=g).to(dev)
    raw = (gt.cpu() + 0.3 * torch.randn(3, H, W, generator=g)).to(dev)
    a = raw.clone().requires_grad_(True)
    b = raw.clone().requires_grad_(True)
    loss, terms = loss_mod.fused_photometric_loss_report(a, gt, lam, clamp=True)
    ref, ssim_v, l1_v = loss_mod.fused_photometric_loss_terms(b, gt, lam, clamp=True)
    assert tuple(terms.shape) == (6,) and loss.dim() == 0 and loss.requires_grad and not terms.requires_grad
    assert float(loss) == float(ref) == float(terms[0])
    assert float(terms[1]) == float(ssim_v) and float(terms[2]) == float(l1_v)
    assert abs(float(terms[3]) - (1.0 - lam) * float(l1_v)) < 1e-7 and abs(float(terms[4]) - (1.0 - float(ssim_v))) < 1e-7 and float(terms[5]) == 0.0
    (loss * 0.75).backward()
    (ref * 0.75).backward()
    assert torch.equal(a.grad, b.grad)
    with torch.no_grad():
        l2, t2 = loss_mod.fused_photometric_loss_report(raw, gt, lam, clamp=True)
    assert float(l2) == float(loss) and torch.equal(t2, terms)


# ---- the kernels against float64 on training-like images and on every route ------------------------------------------------------------
# Scenes, reference, yardstick and bars: tests/photometric_loss_common.py (conditions checked by tests/test_photometric_loss_cpu.py).
import photometric_loss_common as P      # noqa: E402

TILING_SHAPES = [(1, 1), (5, 5), (1, 50), (17, 1), (16, 32), (17, 33), (32, 64), (64, 64), (64, 96), (129, 257)]
CASE_SEED = 7


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _run(raw32, gt32, lam, clamp, upstream=1.5, fn=None):
    """(value, gradient as float64 numpy for the given upstream gradient, loss tensor, gradient tensor) of the fused loss."""
    x = _t(raw32).requires_grad_(True)
    out = (fn or loss_mod.fused_photometric_loss)(x, _t(gt32), lam, clamp)
    out = out[0] if isinstance(out, tuple) else out
    (out * upstream).backward()
    assert out.dim() == 0 and x.grad.shape == x.shape
    return float(out.detach()), x.grad.detach().double().cpu().numpy(), out.detach(), x.grad.detach()


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("lam", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("H,W", TILING_SHAPES)
@pytest.mark.parametrize("scene", ["smooth", "noise"])
def test_kernels_match_float64_at_the_yardstick(scene, H, W, lam, clamp):
    """A single 32x16 tile, one pixel past a tile in each direction, planes inside the 5-pixel halo, tile counts 3, 24 and 243 (below 8,
    a multiple of 8, neither: the three branches of loss_tile()'s XCD map)."""
    raw, gt = P.SCENES[scene](3, H, W, CASE_SEED)
    v, g, _, _ = _run(raw, gt, lam, clamp)
    P.check(v, g, raw, gt, lam, clamp, P.yardstick(scene, 3, H, W, lam, clamp), upstream=1.5, what=f"kernels {scene}",
            ref=P.scene_reference(scene, 3, H, W, CASE_SEED, lam, clamp))
    b = P.blocks(H, W) if scene == "smooth" else None
    if b is not None and clamp:          # strictly outside the clamp: exactly zero
        assert not g[(slice(None),) + b["above"]].any() and not g[(slice(None),) + b["below"]].any()
    if b is not None and lam == 0.0:     # ties: the sign-0 branch alone
        assert not g[(slice(None),) + b["tie"]].any()


def test_kernels_match_float64_at_the_training_frame():
    """545 x 980 (the benchmark's frame), smooth, lambda 0.2, clamp=True.  (The scene is the yardstick's first seed, so its float64
    reference -- seconds of 11x11 float64 convolutions on the CPU -- is computed once.)"""
    H, W, lam = 545, 980, 0.2
    raw, gt = P.smooth(3, H, W, P.YARD_SEEDS[0])
    v, g, _, _ = _run(raw, gt, lam, True)
    P.check(v, g, raw, gt, lam, True, P.yardstick("smooth", 3, H, W, lam, True), upstream=1.5, what="kernels smooth",
            ref=P.scene_reference("smooth", 3, H, W, P.YARD_SEEDS[0], lam, True))


@pytest.mark.parametrize("lam", [0.0, 0.2])
def test_clamp_blocks_and_bounds(lam):
    """The raw = 1.2 and raw = -0.1 blocks: exactly zero gradient under clamp=True, the reference's gradient under clamp=False.  Rows at
    exactly 0.0, 1.0 and -0.0 pass their gradient; rows at nextafter(1, 2) and nextafter(0, -1) do not."""
    H, W = 64, 96
    raw, gt = P.smooth(3, H, W, CASE_SEED)
    b = P.blocks(H, W)
    above, below = (slice(None),) + b["above"], (slice(None),) + b["below"]
    Y = {c: P.yardstick("smooth", 3, H, W, lam, c) for c in (True, False)}
    v, g, _, _ = _run(raw, gt, lam, True)
    assert not g[above].any() and not g[below].any()
    v, g, _, _ = _run(raw, gt, lam, False)
    ref = P.scene_reference("smooth", 3, H, W, CASE_SEED, lam, False)
    P.check(v, g, raw, gt, lam, False, Y[False], upstream=1.5, what="kernels smooth, blocks unclamped", ref=ref)
    gmax = 1.5 * np.abs(ref[3]).max()
    for blk in (above, below):
        assert g[blk].all() and np.abs(g[blk] - 1.5 * ref[3][blk]).max() <= P.bar(Y[False], "ee") * gmax
    rb = raw.copy()
    one, zero = np.float32(1.0), np.float32(0.0)
    rb[:, 20] = zero; rb[:, 21] = one; rb[:, 22] = np.float32(-0.0)
    rb[:, 23] = np.nextafter(one, np.float32(2.0)); rb[:, 24] = np.nextafter(zero, np.float32(-1.0))
    assert np.signbit(rb[:, 22]).all() and (rb[:, 23] > 1).all() and (rb[:, 24] < 0).all()
    v, g, _, _ = _run(rb, gt, lam, True)
    P.check(v, g, rb, gt, lam, True, Y[True], upstream=1.5, what="kernels smooth, rows on the bounds")
    assert g[:, 20:23, 30:70].all()                                   # (columns clear of the blocks: gt > 0 there, so sign != 0)
    assert not g[:, 23:25].any()


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("lam", [0.2, 1.0])
def test_ties_receive_the_ssim_gradient_alone(lam, clamp):
    """Render and target exactly equal (black on black): with lambda > 0 the tie block's gradient is the reference's, which has no L1
    term there, at the case's bar.  (lambda = 0: exactly zero, asserted with the tiling cases.)"""
    H, W = 64, 96
    raw, gt = P.smooth(3, H, W, CASE_SEED)
    tie = (slice(None),) + P.blocks(H, W)["tie"]
    v, g, _, _ = _run(raw, gt, lam, clamp)
    ref = P.scene_reference("smooth", 3, H, W, CASE_SEED, lam, clamp)
    Y = P.yardstick("smooth", 3, H, W, lam, clamp)
    ssim_only = P.scene_reference("smooth", 3, H, W, CASE_SEED, 1.0, clamp)[3][tie]
    assert ref[3][tie].any() and np.abs(ref[3][tie] - lam * ssim_only).max() <= 1e-14 * np.abs(ref[3]).max()      # no L1 term in the block
    err = np.abs(g[tie] - 1.5 * ref[3][tie]).max()
    print(f"[photo-loss ties lam {lam} clamp {int(clamp)}] block max err {err:.3e}, bar {P.bar(Y, 'ee') * 1.5 * np.abs(ref[3]).max():.3e}")
    assert g[tie].any() and err <= P.bar(Y, "ee") * 1.5 * np.abs(ref[3]).max()


@pytest.mark.parametrize("H,W", [(5, 5), (64, 96), (129, 257)])
@pytest.mark.parametrize("clamp", [True, False])
def test_identical_images(H, W, clamp):
    img = P.smooth(3, H, W, CASE_SEED)[1]
    v, g, _, _ = _run(img, img, 0.2, clamp)
    P.check_identical(v, g, img, 0.2, clamp, upstream=1.5, what="kernels")
    v, g, _, _ = _run(img, img, 0.0, clamp)
    assert v == 0.0 and not g.any()


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("scene", ["smooth", "noise"])
@pytest.mark.parametrize("H,W", [(16, 32), (64, 96)])
@pytest.mark.parametrize("C", [1, 4])
def test_other_channel_counts(C, H, W, scene, clamp):
    raw, gt = P.SCENES[scene](C, H, W, CASE_SEED)
    v, g, _, _ = _run(raw, gt, 0.2, clamp)
    P.check(v, g, raw, gt, 0.2, clamp, P.yardstick(scene, C, H, W, 0.2, clamp), upstream=1.5, what=f"kernels {scene} C={C}")


def _stack(B, H, W):
    imgs = [P.smooth(3, H, W, 20 + i) if i % 2 == 0 else P.noise(3, H, W, 20 + i) for i in range(B)]
    return np.stack([i[0] for i in imgs]), np.stack([i[1] for i in imgs])


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("B", [1, 2, 5])
def test_stacks(B, clamp):
    """[B,C,H,W] called directly: the value is the SUM of the float64 per-image losses, out[1] / out[2] the means over images, and every
    image's gradient is its own image's reference gradient (its own 1 / (C H W)).  Bars: every image at its scene's yardstick; the
    sums at the sum (the means at the mean) of the images' bars.  B = 1 as a stack is bit-identical with the [C,H,W] call."""
    H, W, lam = 17, 33, 0.2
    raw, gt = _stack(B, H, W)
    Ys = [P.yardstick("smooth" if i % 2 == 0 else "noise", 3, H, W, lam, clamp) for i in range(B)]
    per = [P.reference(r, t, lam, clamp) for r, t in zip(raw, gt)]
    ref_v, ref_s, ref_l, _ = P.reference_stack(raw, gt, lam, clamp)
    x, y = _t(raw), _t(gt)
    out, ws = torch.ops.gsr.photometric_loss_forward(x, y, lam, clamp)
    d = torch.ops.gsr.photometric_loss_backward(x, y, ws, torch.full((), 1.5, device=_dev()), lam, clamp)
    v, g, vt, gt_ = _run(raw, gt, lam, clamp)
    assert tuple(out.shape) == (3,) and d.shape == x.shape
    assert torch.equal(out[0], vt) and torch.equal(d, gt_)                      # both entries: the same launches
    o = out.double().cpu().numpy()
    print(f"[photo-loss stack B={B} clamp {int(clamp)}] value {o[0]!r} ref {ref_v!r}; ssim {o[1]!r} ref {ref_s!r}; l1 {o[2]!r} ref {ref_l!r}")
    assert abs(o[0] - ref_v) <= sum(P.bar(Y, "dv") for Y in Ys)
    assert abs(o[1] - ref_s) <= sum(P.bar(Y, "ds") for Y in Ys) / B and abs(o[2] - ref_l) <= sum(P.bar(Y, "dl") for Y in Ys) / B
    for i in range(B):
        f = P.figures(per[i][0], g[i], per[i], upstream=1.5)
        print(f"[photo-loss stack B={B} clamp {int(clamp)} image {i}] en {f['en']:.3e} (Y {Ys[i]['en']:.3e}) ee {f['ee']:.3e} (Y {Ys[i]['ee']:.3e})")
        assert f["en"] <= P.bar(Ys[i], "en") and f["ee"] <= P.bar(Ys[i], "ee"), (i, f)
    if B == 1:
        v1, _, vt1, g1 = _run(raw[0], gt[0], lam, clamp)
        assert torch.equal(vt1, vt) and torch.equal(g1, gt_[0])


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("lam", [0.2, 0.0])
@pytest.mark.parametrize("scene", ["smooth", "noise"])
def test_terms_match_float64(scene, lam, clamp):
    """All six entries of fused_photometric_loss_report -- loss, mean SSIM, mean L1, (1 - lambda) mean L1, 1 - mean SSIM, 0 -- and the
    three of fused_photometric_loss_terms against float64.  The derived entries are one more binary32 rounding of a float64
    expression of the sums: their bar is the underlying entry's plus 2^-24 of the value."""
    H, W = 64, 96
    raw, gt = P.SCENES[scene](3, H, W, CASE_SEED)
    Y = P.yardstick(scene, 3, H, W, lam, clamp)
    ref = P.scene_reference(scene, 3, H, W, CASE_SEED, lam, clamp)
    x = _t(raw).requires_grad_(True)
    loss, terms = loss_mod.fused_photometric_loss_report(x, _t(gt), lam, clamp)
    (loss * 1.5).backward()
    t = terms.double().cpu().numpy()
    assert float(loss) == t[0]
    P.check(t[0], x.grad.double().cpu().numpy(), raw, gt, lam, clamp, Y, upstream=1.5, ssim=t[1], l1=t[2], what=f"report {scene}", ref=ref)
    eps = 2.0 ** -24
    assert abs(t[3] - (1.0 - lam) * ref[2]) <= (1.0 - lam) * P.bar(Y, "dl") + eps * abs(t[3])
    assert abs(t[4] - (1.0 - ref[1])) <= P.bar(Y, "ds") + eps * abs(t[4])
    assert t[5] == 0.0
    x2 = _t(raw).requires_grad_(True)
    l2, s2, a2 = loss_mod.fused_photometric_loss_terms(x2, _t(gt), lam, clamp)
    (l2 * 1.5).backward()
    P.check(float(l2), x2.grad.double().cpu().numpy(), raw, gt, lam, clamp, Y, upstream=1.5, ssim=float(s2), l1=float(a2), what=f"terms {scene}", ref=ref)


@pytest.mark.parametrize("clamp", [True, False])
def test_upstream_gradient(clamp):
    """A device scalar of 0 gives an all-zero gradient; -2 gives -2 times the gradient for 1 (the kernel multiplies once, by a power of
    two: bit for bit)."""
    raw, gt = P.smooth(3, 64, 96, CASE_SEED)
    x, y = _t(raw), _t(gt)
    grads = {}
    for up in (1.0, 0.0, -2.0):
        a = x.clone().requires_grad_(True)
        loss_mod.fused_photometric_loss(a, y, 0.2, clamp).backward(torch.full((), up, device=_dev()))
        grads[up] = a.grad
    assert grads[1.0].any() and not grads[0.0].any()
    assert torch.equal(grads[-2.0], -2.0 * grads[1.0])


def test_value_and_gradient_repeat_bit_for_bit():
    """Fixed-order partials, no atomics: three runs at 545 x 980 give the same bits."""
    raw, gt = P.smooth(3, 545, 980, P.YARD_SEEDS[0])
    runs = [_run(raw, gt, 0.2, True)[2:] for _ in range(3)]
    for v, g in runs[1:]:
        assert torch.equal(v, runs[0][0]) and torch.equal(g, runs[0][1])


@pytest.mark.parametrize("clamp", [True, False])
def test_ctypes_binding_route_serves_the_same_kernels(clamp, monkeypatch):
    raw, gt = P.smooth(3, 64, 96, CASE_SEED)
    a = _run(raw, gt, 0.2, clamp)
    monkeypatch.setenv("GSR_BINDING", "ctypes")
    b = _run(raw, gt, 0.2, clamp)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def test_each_node_owns_its_workspace():
    """Two forwards, then their two backwards in reverse order: each returns its own gradient."""
    cases = [P.smooth(3, 64, 96, CASE_SEED), P.noise(3, 64, 96, CASE_SEED)]
    alone = [_run(r, t, 0.2, True, upstream=1.0)[3] for r, t in cases]
    xs = [_t(r).requires_grad_(True) for r, _ in cases]
    outs = [loss_mod.fused_photometric_loss(x, _t(t), 0.2, True) for x, (_, t) in zip(xs, cases)]
    outs[1].backward()
    outs[0].backward()
    assert torch.equal(xs[0].grad, alone[0]) and torch.equal(xs[1].grad, alone[1]) and not torch.equal(alone[0], alone[1])


@pytest.mark.parametrize("clamp", [True, False])
def test_nan_render_gives_a_non_finite_loss(clamp):
    """One NaN pixel: loss, mean SSIM and mean L1 are non-finite under both clamp settings, as the reference's statements
    (rendered_image.clamp(0, 1), then the torch loss) are -- a diverged model must not train on silently."""
    raw, gt = P.smooth(3, 64, 96, CASE_SEED)
    raw[1, 40, 50] = np.nan
    pred = torch.from_numpy(raw).double()
    assert not torch.isfinite(P.ts.photometric_loss(pred.clamp(0, 1) if clamp else pred, torch.from_numpy(gt).double(), 0.2))
    out, _ws = torch.ops.gsr.photometric_loss_forward(_t(raw), _t(gt), 0.2, clamp)
    assert not torch.isfinite(out).any(), out
    loss, terms = loss_mod.fused_photometric_loss_report(_t(raw), _t(gt), 0.2, clamp)
    assert not torch.isfinite(loss) and not torch.isfinite(terms[:5]).any()


def test_inf_render_under_the_clamp_is_a_pixel_at_one():
    """+Inf under clamp=True: the three results of a pixel at 1.0, bit for bit; the pixel itself (strictly above the bound) gets no
    gradient, every other pixel the same one."""
    raw, gt = P.smooth(3, 64, 96, CASE_SEED)
    a, b = raw.copy(), raw.copy()
    a[1, 40, 50] = np.inf
    b[1, 40, 50] = 1.0
    oa, _ = torch.ops.gsr.photometric_loss_forward(_t(a), _t(gt), 0.2, True)
    ob, _ = torch.ops.gsr.photometric_loss_forward(_t(b), _t(gt), 0.2, True)
    assert torch.isfinite(oa).all() and torch.equal(oa, ob)
    ga, gb = _run(a, gt, 0.2, True)[3], _run(b, gt, 0.2, True)[3].clone()
    assert float(ga[1, 40, 50]) == 0.0 and float(gb[1, 40, 50]) != 0.0
    gb[1, 40, 50] = 0.0
    assert torch.equal(ga, gb)
