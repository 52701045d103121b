"""CPU: the conditions the GPU tests of the fused L1+SSIM loss rest on (tests/test_gpu_loss.py), from the float64 reference and the
float32 yardstick of tests/photometric_loss_common.py alone -- no kernel runs here.

Y_floor is the float32 level on the inputs of test_fused_loss_matches_torch (white noise, seed H W, clamp=True, lambda 0.2 / 1 / 0) from
33x17 to 129x257.  The issue that set it (value 1.5e-7, gradient figures 1.2e-6) measured value 5e-10 .. 1.5e-7, element 0.6e-6 ..
1.2e-6, norm-wise 2e-7 .. 7e-7 there; test_float32_meets_the_floor_on_white_noise re-measures it where it runs -- on the machine
this file was written on: value <= 1.45e-7 (1.26e-7 with one or two threads: the float32 mean's order), element <= 1.16e-6,
norm-wise <= 6.7e-7.  (It is a level, not a bound of float32: with clamp=False or other seeds single cases read up to 1.6e-7 / 1.5e-6.)"""
import numpy as np
import pytest
import torch

import photometric_loss_common as P


@pytest.mark.parametrize("lam", [0.2, 1.0, 0.0])
@pytest.mark.parametrize("H,W", [(33, 17), (40, 56), (129, 257)])
def test_float32_meets_the_floor_on_white_noise(H, W, lam):
    """Both float32 orders agree with float64 to within Y_floor on the white-noise inputs the floor was measured on."""
    raw, gt = P.noise(3, H, W, H * W)
    ref = P.reference(raw, gt, lam, True)
    for order in ("2d", "separable"):
        v, _, _, g = P.evaluate(raw, gt, lam, True, torch.float32, order)
        f = P.figures(v, g, ref)
        print(f"[floor noise {H}x{W} lam {lam} {order}] " + " ".join(f"{k} {x:.3e}" for k, x in f.items()))
        assert f["dv"] <= P.FLOOR_VALUE and f["en"] <= P.FLOOR_GRAD and f["ee"] <= P.FLOOR_GRAD, f


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("H,W", [(64, 96), (129, 257)])
def test_smooth_is_the_hard_regime(H, W, clamp):
    """The element-wise yardstick on `smooth` is at least 10x the one on `noise` (measured: about 100x): the scene reaches the
    cancellation the white-noise test cannot."""
    a, b = P.yardstick("smooth", 3, H, W, 0.2, clamp)["ee"], P.yardstick("noise", 3, H, W, 0.2, clamp)["ee"]
    print(f"[regime {H}x{W} clamp {int(clamp)}] ee smooth {a:.3e} noise {b:.3e} ratio {a / b:.1f}")
    assert a >= 10.0 * b, (a, b)


def test_smooth_blocks_exist_and_are_exact():
    for H, W in [(8, 8), (17, 33), (64, 96)]:
        raw, gt = P.smooth(3, H, W, 5)
        b = P.blocks(H, W)
        tie = (slice(None),) + b["tie"]
        assert raw[tie].size > 0 and not raw[tie].any() and not gt[tie].any()                       # raw = gt = 0 exactly
        assert (raw[(slice(None),) + b["above"]] == np.float32(1.2)).all() and (raw[(slice(None),) + b["below"]] == np.float32(-0.1)).all()
        assert raw.dtype == np.float32 and gt.dtype == np.float32 and gt.min() >= 0.0 and gt.max() <= 1.0
        # lambda = 0: the float64 gradient is exactly zero in the tie block and under the clamp, and nowhere else
        g = P.reference(raw, gt, 0.0, True)[3]
        assert not g[tie].any() and not g[(slice(None),) + b["above"]].any() and not g[(slice(None),) + b["below"]].any()
        assert np.count_nonzero(g) == np.count_nonzero((raw != gt) & (raw >= 0) & (raw <= 1))
    assert P.blocks(5, 50) is None and P.blocks(17, 1) is None
    raw, gt = P.smooth(3, 5, 5, 5)                     # no blocks on small planes: the gradient does not vanish
    assert P.reference(raw, gt, 0.2, True)[3].any()


@pytest.mark.parametrize("scene", ["noise", "smooth"])
@pytest.mark.parametrize("H,W", [(5, 5), (17, 33), (64, 96)])
def test_the_window_factorises(scene, H, W):
    """In float64 the separable restatement (row pass, column pass) equals the 2-D convolution with the outer product of the 1-D window
    to 1e-12.  train_step's own 2-D window holds the float32 roundings of those 121 products (the reference builds it in float32): one
    rounding of the kind float32 arithmetic makes throughout, so its distance from the separable statement is held below the
    float32 yardstick."""
    raw, gt = P.SCENES[scene](3, H, W, 5)
    for clamp in (True, False):
        sep = P.evaluate(raw, gt, 0.2, clamp, torch.float64, "separable")
        out = P.evaluate(raw, gt, 0.2, clamp, torch.float64, "outer")
        f = P.figures(sep[0], sep[3], out, sep[1], sep[2])
        assert max(f.values()) <= 1e-12, f
        f = P.figures(sep[0], sep[3], P.reference(raw, gt, 0.2, clamp), sep[1], sep[2])
        Y = P.yardstick(scene, 3, H, W, 0.2, clamp)
        print(f"[window {scene} {H}x{W} clamp {int(clamp)}] separable vs train_step's window in float64: " + " ".join(f"{k} {v:.3e}" for k, v in f.items()))
        for k, v in f.items():
            assert v <= max(Y[k], P.FLOORS[k]), (k, v, Y[k])


def test_stack_reference_is_the_per_image_references():
    imgs = [P.smooth(3, 17, 33, s) for s in (1, 2)] + [P.noise(3, 17, 33, 3)]
    raw, gt = np.stack([i[0] for i in imgs]), np.stack([i[1] for i in imgs])
    for clamp in (True, False):
        v, s, l1, g = P.reference_stack(raw, gt, 0.2, clamp)
        per = [P.reference(r, t, 0.2, clamp) for r, t in zip(raw, gt)]
        assert v == sum(p[0] for p in per) and s == sum(p[1] for p in per) / 3 and l1 == sum(p[2] for p in per) / 3
        assert g.shape == raw.shape and all(np.array_equal(g[i], per[i][3]) for i in range(3))
        # and it is the gradient of the SUM of the images' losses, each normalised by its own C H W
        x = torch.from_numpy(raw).double().requires_grad_(True)
        tot = sum(P.ts.photometric_loss(x[i].clamp(0, 1) if clamp else x[i], torch.from_numpy(gt[i]).double(), 0.2) for i in range(3))
        tot.backward()
        assert abs(float(tot.detach()) - v) <= 1e-15 and np.abs(x.grad.numpy() - g).max() <= 1e-15 * np.abs(g).max()


@pytest.mark.parametrize("H,W", [(5, 5), (64, 96), (129, 257)])
def test_float32_on_identical_images(H, W):
    """raw = gt: the float32 restatements stay below the bars check_identical holds the kernels to (measured: below 1.7e-5 of the scale)."""
    img = P.smooth(3, H, W, 5)[1]
    for clamp in (True, False):
        for order in ("2d", "separable"):
            v, _, _, g = P.evaluate(img, img, 0.2, clamp, torch.float32, order)
            P.check_identical(v, g, img, 0.2, clamp, what=f"float32 {order}")
    assert not P.reference(img, img, 0.0, True)[3].any()
