"""gsr_autopatch on the GPU: the redirected optimizer and loss give what the stock torch pieces give."""
import importlib
import os

import pytest
import torch

import parity

pytestmark = pytest.mark.gpu
ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
optim = importlib.import_module("3dgs_hierarchical_training_amd.optim")


def test_reference_optimizer_construction_returns_fused_adam_and_matches_torch():
    import gsr_autopatch
    dev = torch.device("cuda:0")
    W, H, N = 256, 192, 8000
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=2)
    st = ts.make_settings(sc, dev, 3)
    gt = parity.syn.target_image(W, H, seed=1).to(dev)
    gsr_autopatch.apply()
    try:
        pa = ts.GaussianParams(sc, dev, optimizer="torch")       # torch.optim.Adam(groups, lr=0.0, eps=1e-15), as the reference builds it
    finally:
        gsr_autopatch.remove()
    pb = ts.GaussianParams(sc, dev, optimizer="torch")
    assert isinstance(pa.optimizer, optim.FusedAdam) and type(pb.optimizer) is torch.optim.Adam
    assert [g["name"] for g in pa.optimizer.param_groups] == [g["name"] for g in pb.optimizer.param_groups]
    assert pa.optimizer.eps == 1e-15

    class _L:
        class cfg:
            lambda_dssim, lambda_depth = 0.2, 0.0
    for it in range(3):
        # patched route: the trainer's own calls (torch activations, GaussianRasterizer, clamp, Loss.forward, backward, step)
        pkg = ts.render(pa, st, clamp=True, fused_activations=False)
        d = gsr_autopatch.loss_forward(_L(), pkg["image"], gt)
        d["loss"].backward()
        pa.optimizer.step(); pa.optimizer.zero_grad(set_to_none=True)
        # stock route
        pkg_b = ts.render(pb, st, clamp=True, fused_activations=False)
        loss_b = ts.photometric_loss(pkg_b["image"], gt, 0.2)
        if it == 0:
            l1 = (pkg_b["image"] - gt).abs().mean()
            assert abs(float(d["loss"]) - float(loss_b)) <= 2e-6
            assert abs(float(d["loss_rgb"]) - 0.8 * float(l1)) <= 2e-6
            assert abs(float(d["loss_dssim"]) - (1.0 - float(ts.ssim(pkg_b["image"], gt)))) <= 2e-5
            assert float(d["loss_depth"]) == 0.0
        loss_b.backward()
        pb.optimizer.step(); pb.optimizer.zero_grad(set_to_none=True)
    lrs = {g["name"]: g["lr"] for g in pa.optimizer.param_groups}
    for name, k in ts.GaussianParams._GROUP_ATTR.items():
        a, b = getattr(pa, k).detach(), getattr(pb, k).detach()
        bad = ((a - b).abs() > 0.05 * lrs[name] + 5e-7 * b.abs()).float().mean().item()
        assert bad < 2e-3, (k, bad)
    # the surgery protocol of the model file works on the redirected optimizer (prune, then a step)
    mask = torch.zeros(pa.num_points, dtype=torch.bool, device=dev)
    mask[::3] = True
    pa.prune_points(mask)
    pkg = ts.render(pa, st, clamp=True, fused_activations=False)
    gsr_autopatch.loss_forward(_L(), pkg["image"], gt)["loss"].backward()
    pa.optimizer.step()
    assert pa.optimizer.step_count == 4


refstub = importlib.import_module("3dgs_hierarchical_training_amd.refstub")
RAW = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-20))


@pytest.mark.parametrize("deg", [0, 3])
def test_patched_render_equals_the_unpatched_route(deg):
    """`gsr_autopatch.render_fused` (raw tensors -> in-kernel activations) against the wrapper's own sequence
    (torch exp / sigmoid / normalize / cat -> GaussianRasterizer -> clamp) on the same model and camera: same dict, same image,
    radii and visibility, same gradients on the six raw tensors and on `viewspace_points`."""
    import gsr_autopatch
    dev = torch.device("cuda:0")
    W, H, N = 320, 200, 20000
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=4, posed=True)
    sc["sh_degree"] = deg
    pa, pb = ts.GaussianParams(sc, dev, optimizer="torch"), ts.GaussianParams(sc, dev, optimizer="torch")
    ra, rb = refstub.StubRender(pa, bg=(0.2, 0.1, 0.3)), refstub.StubRender(pb, bg=(0.2, 0.1, 0.3))
    cam = refstub.StubCamera.from_scene(sc, dev)
    g = torch.Generator().manual_seed(5)
    wc, wd, wa = torch.randn(3, H, W, generator=g).to(dev), 0.1 * torch.randn(1, H, W, generator=g).to(dev), 0.1 * torch.randn(1, H, W, generator=g).to(dev)
    a = gsr_autopatch.render_fused(ra, cam)
    b = rb.render(cam)
    assert sorted(a.keys()) == sorted(b.keys())
    assert torch.equal(a["radii"], b["radii"]) and torch.equal(a["visibility_filter"], b["visibility_filter"])
    for k in ("image", "depth", "alpha"):
        assert float((a[k] - b[k]).abs().max()) <= 2e-6, k
    assert float(a["image"].max()) <= 1.0 and float(a["image"].min()) >= 0.0
    for pk in (a, b):
        ((pk["image"] * wc).sum() + (pk["depth"] * wd).sum() + (pk["alpha"] * wa).sum()).backward()
    assert _rel(a["viewspace_points"].grad, b["viewspace_points"].grad) < 1e-5
    for k in RAW:
        ga, gb = getattr(pa, k).grad, getattr(pb, k).grad
        if k == "_features_rest" and deg == 0:
            assert float(ga.abs().max()) == 0.0 and float(gb.abs().max()) == 0.0
            continue
        assert _rel(ga, gb) < 1e-4, (k, _rel(ga, gb))


def test_patched_pose_render_equals_get_xyz_route():
    """A pose render (`rotate_seq`: get_xyz = P[idx].retr().act(_xyz), gaussian_model_ht.py:135-148): the fused route passes the
    pose matrix as the in-kernel points_transform; image and the gradients on the pose parameter and on `_xyz` agree with
    transforming the means in torch."""
    import gsr_autopatch
    dev = torch.device("cuda:0")
    W, H, N = 256, 192, 8000
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=6, posed=False)

    class _T:
        def __init__(self, M):
            self.M = M

        def matrix(self):
            return self.M[None]

        def act(self, x):
            return x @ self.M[:3, :3].t() + self.M[:3, 3]

    class _P:
        def __init__(self):
            self.w = torch.tensor([0.02, -0.01, 0.015, 0.03, -0.02, 0.01], device=dev, requires_grad=True)

        def retr(self):
            w = self.w
            z = torch.zeros((), device=dev)
            K = torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])
            Rm = torch.linalg.matrix_exp(K)
            top = torch.cat([Rm, w[3:, None]], 1)
            return _T(torch.cat([top, torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=dev)], 0))
    outs = []
    for patched in (True, False):
        p = ts.GaussianParams(sc, dev, optimizer="torch")
        r = refstub.StubRender(p)
        r.gaussians.P = [_P(), _P()]
        r.gaussians.rotate_seq, r.gaussians.seq_idx = True, 1
        cam = refstub.StubCamera.from_scene(sc, dev)
        pkg = gsr_autopatch.render_fused(r, cam) if patched else r.render(cam)
        w = torch.randn(3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
        (pkg["image"] * w).sum().backward()
        outs.append((pkg["image"].detach(), r.gaussians.P[1].w.grad.clone(), p._xyz.grad.clone(), r.gaussians.P[0].w.grad))
    (ia, wa, xa, w0a), (ib, wb, xb, w0b) = outs
    # the means differ in the last bit between the two routes (torch's matmul vs the kernel's fma chain), so a rounding-edge decision
    # (a tile rect, the 1/255 threshold) may flip on isolated pixels: everything else agrees to a few ulps
    diff = (ia - ib).abs()
    assert float(diff.mean()) <= 1e-6 and float((diff > 5e-6).float().mean()) <= 2e-4, (float(diff.mean()), float((diff > 5e-6).float().mean()))
    assert w0a is None and w0b is None
    assert _rel(wa, wb) < 2e-4, _rel(wa, wb)
    assert _rel(xa, xb) < 1e-4


def test_unmodified_trainer_sequence_on_the_patched_render(monkeypatch):
    """The trainer's own iteration (ht3dgs_trainer.py:102-166) on the three patched pieces -- render_fused, Loss.forward,
    torch.optim.Adam -> FusedAdam -- against the stock pieces: same parameters after three iterations (Adam's first steps move
    every entry by ~lr whatever the gradient's size, so agreement is measured in units of lr), densification statistics included;
    then the reference's order on a densify iteration: statistics, surgery, THEN optimizer.step() on parameters whose .grad the
    surgery dropped (a no-op step, as in the reference)."""
    import gsr_autopatch
    dev = torch.device("cuda:0")
    W, H, N = 256, 192, 8000
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=2)
    gt = parity.syn.target_image(W, H, seed=1).to(dev)
    gsr_autopatch.apply()
    try:
        pa = ts.GaussianParams(sc, dev, optimizer="torch")
    finally:
        gsr_autopatch.remove()
    pb = ts.GaussianParams(sc, dev, optimizer="torch")
    assert isinstance(pa.optimizer, optim.FusedAdam)
    monkeypatch.setenv("GSR_AUTOPATCH_DEFERRED_MIN_N", "0")    # (exercise the deferred optimizer step on this small model too)
    ra, rb = refstub.StubRender(pa), refstub.StubRender(pb)
    cam = refstub.StubCamera.from_scene(sc, dev, original_image=gt)

    class _L:
        class cfg:
            lambda_dssim, lambda_depth = 0.2, 0.0
    for it in range(3):
        pkg = gsr_autopatch.render_fused(ra, cam)
        d = gsr_autopatch.loss_forward(_L(), pkg["image"], gt)
        d["loss"].backward()
        with torch.no_grad():
            vis, radii = pkg["visibility_filter"], pkg["radii"]
            ra.gaussians.max_radii2D[vis] = torch.max(ra.gaussians.max_radii2D[vis], radii[vis])
            gsr_autopatch.add_densification_stats_fused(ra.gaussians, pkg["viewspace_points"], vis)
            pa.optimizer.step(); pa.optimizer.zero_grad(set_to_none=True)
        pkg_b = rb.render(cam)
        loss_b = ts.photometric_loss(pkg_b["image"], gt, 0.2)
        if it == 0:
            assert abs(float(d["loss"]) - float(loss_b)) <= 2e-6
        loss_b.backward()
        with torch.no_grad():
            vis, radii = pkg_b["visibility_filter"], pkg_b["radii"]
            rb.gaussians.max_radii2D[vis] = torch.max(rb.gaussians.max_radii2D[vis], radii[vis])
            rb.gaussians.add_densification_stats(pkg_b["viewspace_points"], vis)
            pb.optimizer.step(); pb.optimizer.zero_grad(set_to_none=True)
    lrs = {g["name"]: g["lr"] for g in pa.optimizer.param_groups}
    for name, k in ts.GaussianParams._GROUP_ATTR.items():
        a, b = getattr(pa, k).detach(), getattr(pb, k).detach()
        bad = ((a - b).abs() > 0.05 * lrs[name] + 5e-7 * b.abs()).float().mean().item()
        assert bad < 2e-3, (k, bad)
    assert torch.equal(ra.gaussians.denom, rb.gaussians.denom)
    # the trainer's boolean-mask statement ran on the patched render's LazyMask (no nonzero / host synchronisation): same maxima
    assert isinstance(pkg["visibility_filter"], gsr_autopatch.LazyMask) and type(pkg_b["visibility_filter"]) is torch.Tensor
    assert torch.equal(ra.gaussians.max_radii2D, rb.gaussians.max_radii2D) and float(ra.gaussians.max_radii2D.max()) > 0
    assert _rel(ra.gaussians.xyz_gradient_accum, rb.gaussians.xyz_gradient_accum) < 1e-3
    assert pa.optimizer.step_count == 3
    # a densify iteration: the surgery replaces every parameter by a fresh leaf (grad None) before the step
    before = pa._xyz.detach().clone()
    pkg = gsr_autopatch.render_fused(ra, cam)
    gsr_autopatch.loss_forward(_L(), pkg["image"], gt)["loss"].backward()
    mask = torch.zeros(pa.num_points, dtype=torch.bool, device=dev)
    mask[::4] = True
    pa.prune_points(mask)
    pa.optimizer.step(); pa.optimizer.zero_grad(set_to_none=True)
    assert torch.equal(pa._xyz.detach(), before[~mask]) and pa.optimizer.step_count == 3      # that iteration's update is dropped
    pkg = gsr_autopatch.render_fused(ra, cam)                                                # ... and training goes on
    gsr_autopatch.loss_forward(_L(), pkg["image"], gt)["loss"].backward()
    pa.optimizer.step()
    assert pa.optimizer.step_count == 4 and not torch.equal(pa._xyz.detach(), before[~mask])


def _autopatched_model(sc, dev):
    import gsr_autopatch
    gsr_autopatch.apply()
    try:
        p = ts.GaussianParams(sc, dev, optimizer="torch")       # torch.optim.Adam(six groups) -> FusedAdam
    finally:
        gsr_autopatch.remove()
    assert isinstance(p.optimizer, optim.FusedAdam)
    return p, refstub.StubRender(p)


class _LossCfg:
    class cfg:
        lambda_dssim, lambda_depth = 0.2, 0.0


def _iteration(r, cam, gt, step=True, zero=True):
    import gsr_autopatch
    pkg = gsr_autopatch.render_fused(r, cam)
    gsr_autopatch.loss_forward(_LossCfg(), pkg["image"], gt)["loss"].backward()
    if step:
        r.gaussians.optimizer.step()
    if zero:
        r.gaussians.optimizer.zero_grad(set_to_none=True)
    return pkg


def test_deferred_adam_under_the_unmodified_trainer_equals_the_separate_step(monkeypatch):
    """Round 4: under gsr_autopatch the backward kernel computes the Adam update into shadow buffers and `optimizer.step()` adopts
    it by swapping storages.  Against the same trainer calls with GSR_AUTOPATCH_DEFERRED=0 (gradients to .grad, one-launch
    FusedAdam.step()) every situation the trainer can create between backward() and step() must end in the same model:
    plain iterations; a step that never comes (zero_grad only); gradients left to accumulate over two backwards; a learning rate
    changed after the render; one group's tensor replaced (opacity reset) -- that group's update dropped, the other five stepped;
    all tensors replaced (densification) -- the whole update dropped."""
    dev = torch.device("cuda:0")
    W, H, N = 256, 192, 6000
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=12)
    gt = parity.syn.target_image(W, H, seed=3).to(dev)
    cam = refstub.StubCamera.from_scene(sc, dev, original_image=gt)

    monkeypatch.setenv("GSR_AUTOPATCH_DEFERRED_MIN_N", "0")      # (the route is meant for large models; the scenarios run on a small one)

    def scenario(deferred):
        monkeypatch.setenv("GSR_AUTOPATCH_DEFERRED", "1" if deferred else "0")
        p, r = _autopatched_model(sc, dev)
        o = p.optimizer
        snaps = []
        snap = lambda: snaps.append({k: getattr(p, k).detach().clone() for k in RAW})
        for _ in range(2):
            _iteration(r, cam, gt)
        snap()                                                        # 0: two plain iterations
        assert (o._pending is None) and (bool(o._shadow) == deferred)
        _iteration(r, cam, gt, step=False)                            # the step never comes: zero_grad drops it
        snap()                                                        # 1: unchanged
        _iteration(r, cam, gt, step=False, zero=False)                # gradients accumulate over two backwards ...
        _iteration(r, cam, gt)                                        # ... and are stepped once
        snap()                                                        # 2
        import gsr_autopatch
        pkg = gsr_autopatch.render_fused(r, cam)
        gsr_autopatch.loss_forward(_LossCfg(), pkg["image"], gt)["loss"].backward()
        for g in o.param_groups:                                      # a learning rate changed between render and step
            g["lr"] = g["lr"] * 0.5
        o.step(); o.zero_grad(set_to_none=True)
        snap()                                                        # 3
        pkg = gsr_autopatch.render_fused(r, cam)
        gsr_autopatch.loss_forward(_LossCfg(), pkg["image"], gt)["loss"].backward()
        p.reset_opacity()                                             # the opacity tensor replaced between backward and step
        o.step(); o.zero_grad(set_to_none=True)
        snap()                                                        # 4
        pkg = gsr_autopatch.render_fused(r, cam)
        gsr_autopatch.loss_forward(_LossCfg(), pkg["image"], gt)["loss"].backward()
        mask = torch.zeros(p.num_points, dtype=torch.bool, device=dev)
        mask[::5] = True
        p.prune_points(mask)                                          # every tensor replaced: the update is dropped
        o.step(); o.zero_grad(set_to_none=True)
        snap()                                                        # 5
        _iteration(r, cam, gt)
        snap()                                                        # 6: training goes on on the new tensors
        steps = {g["name"]: int(o.state[g["params"][0]]["step"]) for g in o.param_groups}
        return snaps, steps
    sa, steps_a = scenario(True)
    sb, steps_b = scenario(False)
    lrs = {"_xyz": 0.00016, "_features_dc": 0.0025, "_features_rest": 0.0025 / 20.0, "_opacity": 0.05, "_scaling": 0.005, "_rotation": 0.001}
    assert steps_a == steps_b, (steps_a, steps_b)
    assert steps_a["xyz"] == 6 and steps_a["opacity"] == 5
    for i, (a, b) in enumerate(zip(sa, sb)):
        for k in RAW:
            assert a[k].shape == b[k].shape, (i, k)
        if i <= 1:
            # plain iterations and a dropped step: the same Adam arithmetic (adam_one, adam_math.h) on the same gradients, whose
            # float64 cross-tile sums repeat their bits -- equal, up to rounding-boundary flips of inexact sums
            parity.same_accumulation(a, b, f"deferred vs separate step, snapshot {i}")
            continue
        for k in RAW:
            # from snapshot 2 on the two routes' arithmetic differs: the accumulated / lr-changed cases recover the gradient from
            # the shadow first moment, (m' - b1 m) / (1 - b1) -- a few ulps of m, not the .grad sum the separate step reads -- and
            # Adam's first steps move an entry by ~lr whatever the gradient's size: agreement is measured in units of lr
            bad = ((a[k] - b[k]).abs() > 0.05 * lrs[k] + 5e-7 * b[k].abs()).float().mean().item()
            assert bad < 3e-3, (i, k, bad)
    for k in RAW:      # the dropped step left the model bit for bit alone
        assert torch.equal(sa[1][k], sa[0][k])


def test_two_renders_feeding_one_backward_sum_their_gradients_on_the_deferred_route(monkeypatch):
    """loss = f(render A) + f(render B) of the same model, one backward, one step.  Plain torch sums the two
    gradients; the deferred route used to let the second render replace the first one's plan, both autograd nodes then wrote the
    same shadows and step() adopted whichever ran last.  Now the first render keeps its plan, the second takes the plain gradient
    route, and step() -- a .grad beside committed shadows -- recovers the first gradient and adds it: the model after the step
    matches the separate-step route (GSR_AUTOPATCH_DEFERRED=0), and differs from a step on either render alone."""
    import gsr_autopatch
    dev = torch.device("cuda:0")
    W, H, N = 256, 192, 6000
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=12)
    sc2 = dict(sc, **{k: parity.syn.make_scene(8, W, H, sh_degree=3, seed=5, posed=True)[k] for k in ("viewmatrix", "projmatrix", "campos")})
    gt, gt2 = parity.syn.target_image(W, H, seed=3).to(dev), parity.syn.target_image(W, H, seed=4).to(dev)
    cam, cam2 = refstub.StubCamera.from_scene(sc, dev, original_image=gt, uid=0), refstub.StubCamera.from_scene(sc2, dev, original_image=gt2, uid=1)
    monkeypatch.setenv("GSR_AUTOPATCH_DEFERRED_MIN_N", "0")

    def run(deferred, both=True):
        monkeypatch.setenv("GSR_AUTOPATCH_DEFERRED", "1" if deferred else "0")
        p, r = _autopatched_model(sc, dev)
        o = p.optimizer
        _iteration(r, cam, gt)                                         # moments leave zero first
        a = gsr_autopatch.render_fused(r, cam)
        loss = gsr_autopatch.loss_forward(_LossCfg(), a["image"], gt)["loss"]
        if both:
            b = gsr_autopatch.render_fused(r, cam2)
            if deferred:
                assert o._pending is not None                          # render A's plan survived render B
            loss = loss + gsr_autopatch.loss_forward(_LossCfg(), b["image"], gt2)["loss"]
        loss.backward()
        o.step(); o.zero_grad(set_to_none=True)
        assert o._pending is None
        _iteration(r, cam, gt)                                         # and training goes on (deferred again)
        return {k: getattr(p, k).detach().clone() for k in RAW}, {g["name"]: int(o.state[g["params"][0]]["step"]) for g in o.param_groups}
    (da, sa), (db, sb), (dc, _) = run(True), run(False), run(True, both=False)
    assert sa == sb and sa["xyz"] == 3, (sa, sb)
    lrs = {"_xyz": 0.00016, "_features_dc": 0.0025, "_features_rest": 0.0025 / 20.0, "_opacity": 0.05, "_scaling": 0.005, "_rotation": 0.001}
    for k in RAW:
        bad = ((da[k] - db[k]).abs() > 0.05 * lrs[k] + 5e-7 * db[k].abs()).float().mean().item()
        assert bad < 3e-3, (k, bad)
    # ... and the second render's gradient is really in it: a step on render A alone ends somewhere else
    off = ((da["_xyz"] - dc["_xyz"]).abs() > 0.05 * lrs["_xyz"]).float().mean().item()
    assert off > 0.05, off


def test_deferred_adam_at_sh_degree_zero_skips_the_rest_group_like_the_separate_step(monkeypatch):
    """The reference starts every model at active SH degree 0 (gaussian_model_ht.py:68; all of stage A stays there): f_rest then has
    an identically zero gradient and, while its moments are zero, the in-kernel update leaves the group out (no shadow to adopt).
    The deferred route must keep the six step counts and the parameters in line with the separate-step route through the first
    iterations at degree 0 and across the step up to degree 1."""
    dev = torch.device("cuda:0")
    W, H, N = 256, 192, 5000
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=14)
    sc["sh_degree"] = 0
    gt = parity.syn.target_image(W, H, seed=5).to(dev)
    cam = refstub.StubCamera.from_scene(sc, dev, original_image=gt)
    out = {}
    monkeypatch.setenv("GSR_AUTOPATCH_DEFERRED_MIN_N", "0")
    for deferred in (True, False):
        monkeypatch.setenv("GSR_AUTOPATCH_DEFERRED", "1" if deferred else "0")
        p, r = _autopatched_model(sc, dev)
        rest0 = p._features_rest.detach().clone()
        for _ in range(3):
            _iteration(r, cam, gt)
        assert torch.equal(p._features_rest.detach(), rest0)          # degree 0: the bands above it never move
        p.oneup_sh_degree()
        for _ in range(2):
            _iteration(r, cam, gt)
        assert not torch.equal(p._features_rest.detach(), rest0)
        o = p.optimizer
        out[deferred] = ({k: getattr(p, k).detach().clone() for k in RAW},
                         {g["name"]: int(o.state[g["params"][0]]["step"]) for g in o.param_groups})
    assert out[True][1] == out[False][1] and set(out[True][1].values()) == {5}, (out[True][1], out[False][1])
    lrs = {"_xyz": 0.00016, "_features_dc": 0.0025, "_features_rest": 0.0025 / 20.0, "_opacity": 0.05, "_scaling": 0.005, "_rotation": 0.001}
    for k in RAW:
        a, b = out[True][0][k], out[False][0][k]
        bad = ((a - b).abs() > 0.05 * lrs[k] + 5e-7 * b.abs()).float().mean().item()
        assert bad < 3e-3, (k, bad)


def test_bookkeeping_kernels_equal_the_trainers_torch_statements():
    """gsr_masked_max / gsr_densify_stats_add / gsr_psnr against the statements they replace (ht3dgs_trainer.py:138,143-144,
    gaussian_model_ht.py:718-721, utils/image_utils.py:16-18), through the patched entry points."""
    import gsr_autopatch
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(5)
    for N in (1, 63, 257, 100_003):
        radii = torch.randint(0, 40, (N,), generator=g, dtype=torch.int32).to(dev)
        radii[::3] = 0
        maxr = (torch.rand(N, generator=g) * 30).to(dev)
        grad = torch.randn(N, 3, generator=g).to(dev)
        accum, denom = torch.rand(N, 1, generator=g).to(dev), torch.randint(0, 5, (N, 1), generator=g).float().to(dev)
        vis = radii > 0
        # the reference's statements on a plain bool mask
        maxr_ref, accum_ref, denom_ref = maxr.clone(), accum.clone(), denom.clone()
        maxr_ref[vis] = torch.max(maxr_ref[vis], radii[vis])
        accum_ref[vis] += torch.norm(grad[vis, :2], dim=-1, keepdim=True)
        denom_ref[vis] += 1
        # the same statement on the patched render's mask + the patched method
        lazy = gsr_autopatch.LazyMask(vis)
        maxr[lazy] = torch.max(maxr[lazy], radii[lazy])
        assert torch.equal(maxr, maxr_ref)

        class _G:
            pass
        gg = _G()
        gg.xyz_gradient_accum, gg.denom = accum, denom
        vp = torch.zeros(N, 3, device=dev, requires_grad=True)
        vp.grad = grad
        with torch.no_grad():
            gsr_autopatch.add_densification_stats_fused(gg, vp, lazy)
        assert gg.xyz_gradient_accum is accum and torch.equal(denom, denom_ref)
        assert torch.allclose(accum, accum_ref, rtol=2e-6, atol=1e-7)
    for shape in ((3, 545, 980), (3, 7, 5), (1, 64, 64), (4, 1, 1)):
        a, b = torch.rand(shape, generator=g).to(dev), torch.rand(shape, generator=g).to(dev)
        mse = ((a - b) ** 2).view(a.shape[0], -1).mean(1, keepdim=True)
        want = 20 * torch.log10(1.0 / torch.sqrt(mse))
        got = gsr_autopatch.psnr_fused(a, b)
        assert got.shape == want.shape and torch.allclose(got, want, rtol=0, atol=2e-4), (shape, got, want)
        a.requires_grad_(True)                                   # outside no_grad with a differentiable input: the original statement
        assert gsr_autopatch.psnr_fused(a, b).requires_grad
        with torch.no_grad():
            assert torch.allclose(gsr_autopatch.psnr_fused(a, b), want, rtol=0, atol=2e-4)
    same = torch.rand(3, 8, 8, device=dev)
    assert torch.isinf(gsr_autopatch.psnr_fused(same, same.clone())).all()       # mse 0 -> +inf, like the reference's expression


def test_clamped_image_and_visibility_come_out_of_the_kernels():
    """Round 5: `rasterize_gaussians_raw(..., extras=3)` also returns clamp(color, 0, 1) -- written by the forward blend's epilogue --
    and the bytes radii > 0 -- written by the preprocess -- i.e. the two torch launches of the reference's wrapper
    (gaussian_model_ht.py:883, :905).  Same values as torch's; a gradient put on the clamped image alone, on the raw image alone, or
    on both reaches the parameters exactly as through `image_raw.clamp(0, 1)`."""
    R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    dev = torch.device("cuda:0")
    W, H, N = 300, 200, 15000
    sc = parity.syn.make_scene(N, W, H, sh_degree=2, seed=8, posed=True)
    st = ts.make_settings(sc, dev, 2, bg=torch.tensor([0.9, -0.2, 1.3]))         # a background outside [0, 1]: the clamp bites
    g = torch.Generator().manual_seed(2)
    w_raw, w_cl = torch.randn(3, H, W, generator=g).to(dev), torch.randn(3, H, W, generator=g).to(dev)
    res = []
    for fused in (True, False):
        p = ts.GaussianParams(sc, dev, optimizer="torch")
        with torch.no_grad():
            p._features_dc.mul_(3.0)                                             # colours beyond 1 as well
        m2d = torch.zeros(N, 3, device=dev, requires_grad=True)
        if fused:
            raw, radii, depth, alpha, clamped, vis8 = R.rasterize_gaussians_raw(p._xyz, m2d, p._features_dc, p._features_rest, p._opacity, p._scaling,
                                                                               p._rotation, st, extras=3)
            assert vis8.dtype == torch.uint8 and torch.equal(vis8.view(torch.bool), radii > 0)
            assert torch.equal(clamped, raw.detach().clamp(0, 1)) and float(clamped.max()) == 1.0 and bool((raw > 1).any())
        else:
            raw, radii, depth, alpha = R.rasterize_gaussians_raw(p._xyz, m2d, p._features_dc, p._features_rest, p._opacity, p._scaling, p._rotation, st)
            clamped = raw.clamp(0, 1)
        ((clamped * w_cl).sum() + (raw * w_raw).sum()).backward()
        res.append({k: getattr(p, k).grad.clone() for k in RAW} | {"m2d": m2d.grad.clone(), "raw": raw.detach().clone()})
    assert torch.equal(res[0]["raw"], res[1]["raw"])
    for k in list(RAW) + ["m2d"]:
        assert _rel(res[0][k], res[1][k]) < 1e-5, (k, _rel(res[0][k], res[1][k]))


# ---- round 6: the frame poses of the unmodified trainer (lietorch LieGroupParameter + its Adam) on the kernels -----------------------
def _lie(dev, pose7=None, delta=None):
    p = refstub.LieGroupParameter(refstub.SE3(torch.tensor([pose7 if pose7 is not None else [0.0, 0, 0, 0, 0, 0, 1]], device=dev)))
    if delta is not None:
        with torch.no_grad():
            p.copy_(torch.tensor([delta], device=dev))
    return p


@pytest.mark.parametrize("with_base", [False, True], ids=["identity-base", "posed-base"])
def test_pose_matrix_node_equals_the_lietorch_statement_and_its_autograd(with_base):
    """`torch.ops.gsr.pose_matrix` (what stands for `P[k].retr()` on the patched render): the [3,4] matrix of Exp(delta) * group
    against the float64 torch statement to float32 rounding, its backward (gsr_pose_grad) against autograd through that statement
    -- at delta = 0 (the series branch, every pose's first render) and away from it; `.grad` lands on the parameter in ITS shape."""
    import gsr_autopatch
    pose = importlib.import_module("3dgs_hierarchical_training_amd.pose")
    pose_opt = importlib.import_module("3dgs_hierarchical_training_amd.pose_opt")
    dev = torch.device("cuda:0")
    ops = gsr_autopatch._ops()
    pose7 = [0.3, -0.2, 0.5, 0.1, -0.2, 0.3, 0.9] if with_base else None
    Wt = torch.randn(3, 4, generator=torch.Generator().manual_seed(5)).to(dev)
    for delta in (None, [0.02, -0.01, 0.03, 0.015, -0.02, 0.01], [0.3, -0.2, 0.1, 0.4, 0.5, -0.3]):
        p = _lie(dev, pose7, delta)
        M = pose_opt.pose_matrix(p, ops)
        d64 = p.detach().double().reshape(6).requires_grad_(True)
        q = p.group.data.double().reshape(7)
        q = torch.cat((q[:3], q[3:] / q[3:].norm()))
        ref = pose.retr_matrix(d64, q)[:3]
        assert tuple(M.shape) == (3, 4) and float((M.detach().double() - ref.detach()).abs().max()) < 1e-6
        (M * Wt).sum().backward()
        (ref * Wt.double()).sum().backward()
        assert tuple(p.grad.shape) == (1, 6)
        assert _rel(p.grad.reshape(6).double(), d64.grad) < 2e-6, (delta, p.grad, d64.grad)
        with torch.no_grad():                                   # no graph: the same matrix, nothing recorded
            assert torch.equal(pose_opt.pose_matrix(p, ops), M.detach())


def test_fused_pose_adam_is_torch_adam_over_the_pose_node():
    """The optimizer `torch.optim.Adam([{'params': [P[k]], 'lr': ..., 'name': 'R'}], lr=0.0, eps=1e-15)` returns while the patch is
    applied (gaussian_model_ht.py:296-311), stepping a lietorch parameter through the pose node, against the stock class stepping the
    same parameter through lietorch's own chain (refstub's torch statement of it): same trajectory of the six numbers over 40 steps,
    same state, with the learning-rate statement of `update_learning_rate_camera` in between."""
    import gsr_autopatch
    pose_opt = importlib.import_module("3dgs_hierarchical_training_amd.pose_opt")
    dev = torch.device("cuda:0")
    pose7 = [0.1, 0.05, -0.2, 0.05, -0.1, 0.02, 0.99]
    Wt = torch.randn(3, 4, generator=torch.Generator().manual_seed(9)).to(dev)
    gsr_autopatch.apply()
    try:
        pa = _lie(dev, pose7)
        oa = torch.optim.Adam([{'params': [pa], 'lr': 1e-3, "name": "R"}], lr=0.0, eps=1e-15)
    finally:
        gsr_autopatch.remove()
    assert isinstance(oa, pose_opt.FusedPoseAdam)
    pb = _lie(dev, pose7)
    ob = torch.optim.Adam([{'params': [pb], 'lr': 1e-3, "name": "R"}], lr=0.0, eps=1e-15)
    assert type(ob) is torch.optim.Adam
    ops = gsr_autopatch._ops()
    for it in range(1, 41):
        lr = 1e-3 * (0.98 ** it)
        for o in (oa, ob):
            for g in o.param_groups:
                g["lr"] = lr
        Ma = pose_opt.pose_matrix(pa, ops)
        Mb = pb.retr().matrix().reshape(4, 4)[:3]
        assert torch.allclose(Ma, Mb, atol=2e-6)
        ((Wt * Ma).sum() + 0.5 * (Ma ** 2).sum()).backward()
        ((Wt * Mb).sum() + 0.5 * (Mb ** 2).sum()).backward()
        assert _rel(pa.grad, pb.grad) < 1e-4, it
        oa.step(); ob.step()
        oa.zero_grad(set_to_none=True); ob.zero_grad(set_to_none=True)
        assert pa.grad is None
        assert torch.allclose(pa.detach(), pb.detach(), atol=5e-6, rtol=1e-4), (it, pa, pb)
    assert float(pb.detach().abs().max()) > 0.01
    sa, sb = oa.state[pa], ob.state[pb]
    assert sa["step"] == 40 and float(sb["step"]) == 40.0
    assert torch.allclose(sa["exp_avg"], sb["exp_avg"], rtol=1e-3, atol=1e-8) and torch.allclose(sa["exp_avg_sq"], sb["exp_avg_sq"], rtol=1e-3, atol=1e-12)
    assert torch.equal(pa.group.data, pb.group.data)             # the group element stays; the six tangent numbers carry the update


@pytest.mark.parametrize("mode", ["rotate_seq", "rotate_xyz"])
def test_unmodified_trainers_pose_iteration_fused_equals_its_lietorch_chain(mode, monkeypatch):
    """The reference's pose iteration (ht3dgs_trainer.py:102-166 under `rotate_seq` with `camera_optimizer[fidx]`, and stage A's
    `train_relative_pose` with the pose in `gaussians.optimizer`): render -> loss -> backward -> optimizer.step() on the patched
    pieces, with the pose on the kernels (pose node + FusedPoseAdam) against GSR_AUTOPATCH_POSE_FUSED=0 (lietorch's chain stated in
    torch + the stock Adam).  Same images, same pose trajectory, same model after its own (deferred) Adam steps."""
    import gsr_autopatch
    dev = torch.device("cuda:0")
    W, H, N = 256, 192, 8000
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=6, posed=False)
    gt = parity.syn.target_image(W, H, seed=3).to(dev)
    res = {}
    for fused in (True, False):
        monkeypatch.setenv("GSR_AUTOPATCH_POSE_FUSED", "1" if fused else "0")
        gsr_autopatch.apply()
        try:
            p = ts.GaussianParams(sc, dev, optimizer="torch")
            r = refstub.StubRender(p)
            g = r.gaussians
            cam = refstub.StubCamera.from_scene(sc, dev, uid=1)
            if mode == "rotate_seq":
                g.P = [_lie(dev), _lie(dev, [0.01, -0.02, 0.015, 0.01, 0.0, -0.01, 1.0])]
                g.rotate_seq, g.seq_idx = True, 1
                cam_opt = [torch.optim.Adam([{'params': [q], 'lr': 1e-3, "name": "R"}], lr=0.0, eps=1e-15) for q in g.P]
                live, popt = g.P[1], cam_opt[1]
            else:
                g.P = [_lie(dev)]
                g.rotate_xyz = True
                live = g.P[0]
                popt = torch.optim.Adam([{'params': [live], 'lr': 1e-3, "name": "R"}], lr=0.0, eps=1e-15)      # training_setup_fix_position
            assert type(popt).__name__ == ("FusedPoseAdam" if fused else "Adam")
            imgs, traj = [], []
            for it in range(12):
                pkg = gsr_autopatch.render_fused(r, cam)
                gsr_autopatch.loss_forward(_LossCfg(), pkg["image"], gt)["loss"].backward()
                if it == 0:
                    pg0 = live.grad.clone()
                imgs.append(pkg["image"].detach().clone())
                if mode == "rotate_seq":
                    p.optimizer.step()
                p.optimizer.zero_grad(set_to_none=True)
                popt.step()
                popt.zero_grad(set_to_none=True)
                traj.append(live.detach().clone().reshape(6))
            g0 = {k: getattr(p, k).detach().clone() for k in ("_xyz", "_opacity", "_scaling")}      # the model after its twelve (deferred) Adam steps
            res[fused] = (imgs, torch.stack(traj), g0, pg0, g.P[0].grad if mode == "rotate_seq" else None)
        finally:
            gsr_autopatch.remove()
    (ia, ta, ga, pga, oa), (ib, tb, gb, pgb, ob) = res[True], res[False]
    assert oa is None and ob is None
    d0 = (ia[0] - ib[0]).abs()
    assert float(d0.mean()) <= 1e-6 and float((d0 > 5e-6).float().mean()) <= 2e-4
    assert _rel(pga, pgb) < 2e-4, _rel(pga, pgb)
    for k in ga:      # (twelve sign-like first Adam steps of the model under two pose trajectories -- float64 central differences in the
                      #  kernel against the float32 lietorch chain, see below -- whose gradients drift apart: not the 1e-4 of one gradient)
        assert _rel(ga[k], gb[k]) < 2e-3, k
    assert mode == "rotate_xyz" or not torch.equal(ga["_xyz"], parity.syn.make_scene(N, W, H, sh_degree=3, seed=6, posed=False)["means3D"].to(dev))
    # twelve Adam steps of lr 1e-3 move each number by ~1e-2; the two routes round the pose gradient differently (float64 central
    # differences in the kernel, float32 autograd through the torch chain) and Adam's first steps are sign-like: agreement to a few
    # percent of a step is what two float32 evaluations of the same loop give
    assert float(tb.abs().max()) > 5e-3
    assert float((ta - tb).abs().max()) < 2e-4, float((ta - tb).abs().max())
    dl = (ia[-1] - ib[-1]).abs()
    assert float(dl.mean()) <= 2e-4


def test_stage_a_pose_fit_under_the_unmodified_trainers_statements_recovers_the_pose():
    """compute_relative_pose's second half (ht3dgs_trainer.py:308-333, :367-378) the way the unmodified trainer runs it: a frozen
    model, `init_RT(None)`, `training_setup_fix_position(gaussian_rot=False)` -> Adam over the one LieGroupParameter, render through
    `get_xyz`'s pose, loss, backward, optimizer.step() -- on the patched render + pose node + FusedPoseAdam.  It must recover the
    relative pose as the library's own loop (stage_a.fit_pair, gsr_pose_step) does from the same start."""
    import gsr_autopatch
    sequence = importlib.import_module("3dgs_hierarchical_training_amd.sequence")
    dev = torch.device("cuda:0")
    W, H = 320, 240
    seq = sequence.FrameSequence(3, 60_000, W, H, dev, seed=0)
    T = seq.true_rel_pose(0, 1)
    scene = seq.pixel_scene(0, stride=1, seed=0)      # one Gaussian per pixel of frame 0: explains its image from the start (stage_a.fit_pair)
    tgt1 = seq.target(1)
    ident = ts.with_sh_degree(seq.settings_for_pose(torch.eye(4)), 0)
    gsr_autopatch.apply()
    try:
        p = ts.GaussianParams(scene, dev, optimizer="torch")
        p.active_sh_degree = 0                          # a stage-A model never leaves degree 0 (gaussian_model_ht.py:68)
        r = refstub.StubRender(p, bg=tuple(float(x) for x in ident.bg.cpu()))
        g = r.gaussians
        g.P = [_lie(dev)]
        g.rotate_xyz = True
        opt = torch.optim.Adam([{'params': [g.P[0]], 'lr': 2e-3, "name": "R"}], lr=0.0, eps=1e-15)
        assert type(opt).__name__ == "FusedPoseAdam"
        cam = refstub.StubCamera(W, H, ident.tanfovx, ident.tanfovy, ident.viewmatrix, ident.projmatrix, ident.campos, uid=1)
        losses = []
        for it in range(250):
            pkg = gsr_autopatch.render_fused(r, cam)
            out = gsr_autopatch.loss_forward(_LossCfg(), pkg["image"], tgt1)
            out["loss"].backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
            p.optimizer.zero_grad(set_to_none=True)
            if it % 50 == 0 or it == 249:
                losses.append(float(out["loss"]))
        M = torch.eye(4)
        M[:3] = importlib.import_module("3dgs_hierarchical_training_amd.pose_opt").pose_matrix(g.P[0], gsr_autopatch._ops()).detach().cpu()
    finally:
        gsr_autopatch.remove()
    err0, err = float((torch.eye(4) - T).abs().max()), float((M - T).abs().max())
    assert losses[-1] < losses[0] and err < 0.3 * err0, (losses, err0, err)
