"""GPU: the f-2 extensions against their torch counterparts.
  * raw-parameter rasterization (activations + SH concat in-kernel) == reference-style torch activations
    followed by the activated-parameter path, values and gradients (1e-5 abs / 1e-4 rel);
  * gsr_adam_step == torch.optim.Adam(eps=1e-15) over several steps (fp32: 1e-6 relative)."""
import importlib

import numpy as np
import pytest
import torch

import parity

pytestmark = pytest.mark.gpu
ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
optim = importlib.import_module("3dgs_hierarchical_training_amd.optim")


@pytest.mark.parametrize("deg", [0, 3])
def test_raw_parameter_path_matches_activated_path(deg):
    dev = torch.device("cuda:0")
    sc = parity.syn.make_scene(20000, 320, 240, sh_degree=deg, seed=5, posed=True)
    gt = parity.syn.target_image(320, 240).to(dev)
    settings = ts.make_settings(sc, dev, deg, bg=torch.tensor([0.1, 0.2, 0.3]))
    res = {}
    for fused in (False, True):
        p = ts.GaussianParams(sc, dev, optimizer="torch")
        with torch.no_grad():
            p._rotation.mul_(1.7)          # un-normalised raw quaternions exercise the normalise Jacobian
        pkg = ts.render(p, settings, clamp=False, fused_activations=fused)
        w = torch.linspace(0.5, 1.5, 3 * 240 * 320, device=dev).view(3, 240, 320)
        (pkg["raw_image"] * w).sum().backward()
        res[fused] = dict(img=pkg["raw_image"].detach(), radii=pkg["radii"],
                          grads={k: getattr(p, k).grad.detach() for k in ["_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"]},
                          m2d=pkg["viewspace_points"].grad.detach())
    assert torch.equal(res[False]["radii"], res[True]["radii"])
    # two binary32 routes whose activated inputs differ in the last bit (torch.exp / sigmoid vs expf in-kernel):
    # each is within 1e-5 of the float64 truth, so they are within 2e-5 of each other (plus rounding-edge flips)
    d = (res[False]["img"] - res[True]["img"]).abs()
    assert (d > 2e-5).float().mean().item() < 1e-4 and d.max().item() < 1e-2
    for k, ref in res[False]["grads"].items():
        got = res[True]["grads"][k]
        assert got.shape == ref.shape
        err = (got - ref).abs().max().item()
        assert err <= 1e-4 * ref.abs().max().item() + 1e-12, (k, err, ref.abs().max().item())
    assert (res[True]["m2d"] - res[False]["m2d"]).abs().max().item() <= 1e-4 * res[False]["m2d"].abs().max().item()


def test_fused_adam_matches_torch_adam():
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    shapes = [(1000, 3), (1000, 1, 3), (1000, 15, 3), (1000, 1), (1000, 3), (1000, 4), (7,)]
    lrs = [1.6e-4, 2.5e-3, 1.25e-4, 5e-2, 5e-3, 1e-3, 1e-2]
    a = [torch.randn(s, generator=g).to(dev).requires_grad_(True) for s in shapes]
    b = [t.detach().clone().requires_grad_(True) for t in a]
    oa = optim.FusedAdam([{"params": [t], "lr": lr} for t, lr in zip(a, lrs)], lr=0.0, eps=1e-15)
    ob = torch.optim.Adam([{"params": [t], "lr": lr} for t, lr in zip(b, lrs)], lr=0.0, eps=1e-15)
    for it in range(5):
        for ta, tb in zip(a, b):
            gr = torch.randn(ta.shape, generator=g).to(dev) * (10.0 ** (it - 2))
            ta.grad, tb.grad = gr.clone(), gr.clone()
        oa.step(); ob.step()
        oa.zero_grad(); ob.zero_grad()
    for ta, tb in zip(a, b):
        assert torch.allclose(ta, tb, rtol=2e-6, atol=1e-7), (ta - tb).abs().max()


def test_train_step_variants_agree():
    """Fully fused train step (HIP loss + in-kernel activations + HIP Adam) tracks the reference-style step
    (torch activations / torch loss / torch Adam) over a few iterations."""
    dev = torch.device("cuda:0")
    sc = parity.syn.make_scene(30000, 320, 240, sh_degree=3, seed=6)
    gt = parity.syn.target_image(320, 240).to(dev)
    settings = ts.make_settings(sc, dev, 3)
    pa, pb = ts.GaussianParams(sc, dev, optimizer="hip"), ts.GaussianParams(sc, dev, optimizer="torch")
    la, lb = [], []
    for _ in range(4):
        la.append(float(ts.train_step(pa, settings, gt, fused_loss=True, fused_activations=True)["loss"]))
        lb.append(float(ts.train_step(pb, settings, gt, fused_loss=False, fused_activations=False)["loss"]))
    assert la[-1] < la[0]
    assert np.allclose(la, lb, rtol=2e-4), (la, lb)


@pytest.mark.parametrize("n,deg", [(30000, 3), (30001, 3), (20011, 1), (4099, 0)])
def test_optimizer_in_backward_equals_backward_then_step(n, deg):
    """GsrFusedAdam (Adam applied inside the per-Gaussian backward kernel) == backward() + gsr_adam_step: same
    gradient arithmetic, same update arithmetic (adam_one, adam_math.h), only the HBM round trip of the gradient is gone.
    The blend backward's float64 cross-tile sums repeat their bits from run to run, so parameters, both moments and the
    screen-space gradient are EQUAL, up to rounding-boundary flips of inexact sums (parity.same_accumulation: at most 4
    entries per tensor; Adam with eps = 1e-15 would turn any other difference of a nearly cancelled gradient into a
    visible fraction of an lr step).  Covers the 16-byte streams (n multiple of 128), the ragged last block, and SH bands
    above the active degree (deg < 3 with 16 stored coefficients: zero gradient, moments still decay)."""
    dev = torch.device("cuda:0")
    sc = parity.syn.make_scene(n, 320, 240, sh_degree=3, seed=9)
    sc["sh_degree"] = deg
    gt = parity.syn.target_image(320, 240).to(dev)
    settings = ts.make_settings(sc, dev, deg)
    pa, pb = ts.GaussianParams(sc, dev, optimizer="hip"), ts.GaussianParams(sc, dev, optimizer="hip")
    names = ["_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"]

    for it in range(3):
        ka = ts.train_step(pa, settings, gt, fused_optimizer=True)
        kb = ts.train_step(pb, settings, gt, fused_optimizer=False)
        assert all(getattr(pa, k).grad is None for k in names)
        got, want = {"viewspace_points": ka["viewspace_points"].grad}, {"viewspace_points": kb["viewspace_points"].grad}
        for k in names:
            got[k], want[k] = getattr(pa, k).detach(), getattr(pb, k).detach()
            sa, sb = pa.optimizer.state[getattr(pa, k)], pb.optimizer.state[getattr(pb, k)]
            for mom in ("exp_avg", "exp_avg_sq"):
                got[k + "/" + mom], want[k + "/" + mom] = sa[mom], sb[mom]
        parity.same_accumulation(got, want, f"in-backward vs step, {n}/deg{deg}, step {it}", verbose=False)
    assert pa.optimizer.step_count == pb.optimizer.step_count == 3
    if deg < 3:   # bands above the active degree: no gradient, so both routes must agree exactly (and stay put)
        hi = 3 * ((deg + 1) ** 2 - 1) // 3
        assert torch.equal(pa._features_rest[:, hi:], pb._features_rest[:, hi:])


@pytest.mark.parametrize("fused_optimizer", [False, True], ids=["step", "in-backward"])
def test_fused_adam_through_densification_matches_torch_adam(fused_optimizer):
    """Train, prune, train, append (densify), reset opacity, train -- FusedAdam (stepped normally or inside the
    backward kernel) against torch.optim.Adam with the same optimizer-state surgery (gaussian_model_ht.py:532-629).
    Moments must be sliced / zero-extended with the parameters and the bias correction must keep counting."""
    dev = torch.device("cuda:0")
    sc = parity.syn.make_scene(12000, 256, 192, sh_degree=3, seed=21)
    gt = parity.syn.target_image(256, 192).to(dev)
    settings = ts.make_settings(sc, dev, 3)
    pa, pb = ts.GaussianParams(sc, dev, optimizer="hip"), ts.GaussianParams(sc, dev, optimizer="torch")
    names = ["_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"]
    gen = torch.Generator().manual_seed(5)

    def steps(k):
        for _ in range(k):
            ts.train_step(pa, settings, gt, fused_optimizer=fused_optimizer)
            ts.train_step(pb, settings, gt, fused_loss=True, fused_activations=True, fused_optimizer=False)

    def compare(tag):
        for k in names:
            a, b = getattr(pa, k).detach(), getattr(pb, k).detach()
            lr = next(g["lr"] for g in pa.optimizer.param_groups if g["params"][0] is getattr(pa, k))
            bad = ((a - b).abs() > 0.05 * lr + 5e-7 * b.abs()).float().mean().item()
            assert a.shape == b.shape and bad < 2e-3, (tag, k, bad)
            sa, sb = pa.optimizer.state[getattr(pa, k)], pb.optimizer.state[getattr(pb, k)]
            assert int(sa["step"]) == int(sb["step"]), (tag, k)
            for mom in ("exp_avg", "exp_avg_sq"):
                scale = sb[mom].abs().max().item()
                bad = ((sa[mom] - sb[mom]).abs() > 1e-3 * sb[mom].abs() + 1e-6 * scale).float().mean().item()
                assert bad < 2e-3, (tag, k, mom, bad)

    steps(2)
    compare("start")
    mask = (torch.rand(pa.num_points, generator=gen) < 0.3).to(dev)
    pa.prune_points(mask); pb.prune_points(mask)
    steps(2)
    compare("after prune")
    idx = torch.randperm(pa.num_points, generator=gen)[:1500].to(dev)
    for p in (pa, pb):
        new = {n: getattr(p, a).detach()[idx].clone() for n, a in p._GROUP_ATTR.items()}
        new["xyz"] = new["xyz"] + 0.01
        p.densification_postfix(new)
    assert pa.num_points == pb.num_points
    steps(2)
    compare("after densify")
    pa.reset_opacity(); pb.reset_opacity()
    steps(2)
    compare("after opacity reset")
    assert pa.optimizer.step_count == 8


@pytest.mark.parametrize("fused_optimizer", [True, False], ids=["in-backward", "step"])
def test_densification_statistics_from_the_backward_kernel(fused_optimizer):
    """The per-iteration statistics of the reference's train_step (max_radii2D, xyz_gradient_accum, denom over the visible
    Gaussians: ht3dgs_trainer.py:141-147, gaussian_model_ht.py:718-721) are accumulated by the per-Gaussian backward kernel
    (GsrDensifyStats) and must equal what `Densifier.add_stats` -- the torch statement of the same lines -- makes of the same
    step's radii and means2D.grad; `add_stats` itself no longer runs in the train step."""
    dm = importlib.import_module("3dgs_hierarchical_training_amd.densify")
    dev = torch.device("cuda:0")
    W, H, N = 320, 240, 20011
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=31, posed=True)
    cam2 = parity.syn.make_scene(8, W, H, sh_degree=3, seed=6, posed=True)
    sc2 = dict(sc)
    for k in ("viewmatrix", "projmatrix", "campos"):
        sc2[k] = cam2[k]
    views = [ts.make_settings(sc, dev, 3), ts.make_settings(sc2, dev, 3)]
    gt = parity.syn.target_image(W, H, seed=1).to(dev)
    p = ts.GaussianParams(sc, dev)
    cfg = dm.DensifyConfig(densify_from_iter=10 ** 9, opacity_reset_interval=10 ** 9)
    den, ref = dm.Densifier(p, 5.0, cfg), dm.Densifier(p, 5.0, cfg)
    calls = [0]
    orig = dm.Densifier.add_stats

    def counted(self, *a):
        calls[0] += self is den
        return orig(self, *a)
    dm.Densifier.add_stats = counted
    try:
        for it in range(1, 7):
            pkg = ts.train_step(p, views[it % 2], gt, densifier=den, iteration=it, fused_optimizer=fused_optimizer,
                                next_settings=views[(it + 1) % 2])
            ref.add_stats(pkg["viewspace_points"], pkg["visibility_filter"], pkg["radii"])
    finally:
        dm.Densifier.add_stats = orig
    assert calls[0] == 0                                   # the train step launched no statistics ops of its own
    assert int((ref.denom > 0).sum()) > N // 3
    assert torch.equal(den.denom, ref.denom) and torch.equal(den.max_radii2D, ref.max_radii2D)
    err = (den.xyz_gradient_accum - ref.xyz_gradient_accum).abs().max().item()
    assert err <= 1e-6 * ref.xyz_gradient_accum.abs().max().item(), err
    # past densify_until_iter nothing accumulates (ht3dgs_trainer.py:137)
    den2 = dm.Densifier(p, 5.0, dm.DensifyConfig(densify_until_iter=3, densify_from_iter=10 ** 9, opacity_reset_interval=10 ** 9))
    ts.train_step(p, views[0], gt, densifier=den2, iteration=5)
    assert float(den2.denom.sum()) == 0.0


def test_optimizer_in_backward_refuses_foreign_tensors():
    dev = torch.device("cuda:0")
    sc = parity.syn.make_scene(2000, 128, 96, sh_degree=3, seed=2)
    settings = ts.make_settings(sc, dev, 3)
    pa, pb = ts.GaussianParams(sc, dev, optimizer="hip"), ts.GaussianParams(sc, dev, optimizer="hip")
    with pytest.raises(RuntimeError, match="fused_adam"):      # someone else's optimizer
        pkg = ts.render(pa, settings, clamp=False, fused_activations=True, fused_adam=pb.optimizer)
        pkg["raw_image"].sum().backward()
    assert pb.optimizer.step_count == 0


def test_optimizer_in_backward_guards():
    """(a) a second backward through the same fused render must not apply the step twice; (b) step() must refuse
    to apply a second update when the in-kernel step already ran and the parameters also carry a .grad."""
    dev = torch.device("cuda:0")
    sc = parity.syn.make_scene(2000, 128, 96, sh_degree=3, seed=2)
    settings = ts.make_settings(sc, dev, 3)
    p = ts.GaussianParams(sc, dev, optimizer="hip")
    pkg = ts.render(p, settings, clamp=False, fused_activations=True, fused_adam=p.optimizer)
    loss = pkg["raw_image"].sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="ran twice"):
        loss.backward()
    assert p.optimizer.step_count == 1
    p.optimizer.step()                           # nothing carries a .grad: a no-op, as in train_step
    assert p.optimizer.step_count == 1
    pkg = ts.render(p, settings, clamp=False, fused_activations=True, fused_adam=p.optimizer)
    (pkg["raw_image"].sum() + 1e-3 * p._xyz.sum()).backward()        # a second loss term reaches _xyz directly
    with pytest.raises(RuntimeError, match="already applied inside backward"):
        p.optimizer.step()


def test_ctypes_binding_route_matches_the_extension(monkeypatch):
    """GSR_BINDING=ctypes: the plain-FFI route over the same C ABI (the INTEGRATION.md example) renders and differentiates
    exactly what torch.ops.gsr.rasterize does."""
    import hip_runner
    sc = parity.syn.make_scene(6000, 200, 150, sh_degree=3, seed=8, posed=True)
    kw = parity.scene_kwargs(sc, "sh", bg=(0.2, 0.1, 0.0))
    g = parity.upstream_grads(150, 200, seed=1)
    a = hip_runner.run_hip(kw, g, cam_grad=True)
    monkeypatch.setenv("GSR_BINDING", "ctypes")
    b = hip_runner.run_hip(kw, g, cam_grad=True)
    for x, y in zip(a["fwd"], b["fwd"]):
        assert np.array_equal(x, y)
    for k in a["grads"]:
        assert np.abs(a["grads"][k] - b["grads"][k]).max() <= 2e-5 * np.abs(a["grads"][k]).max() + 1e-12, k


@pytest.mark.parametrize("fail_tag", ["binning", "scratch"])
def test_allocator_that_returns_null_is_an_error_not_a_crash(monkeypatch, fail_tag):
    """The C ABI takes its R-sized buffers from the caller's allocator callback (include/gsr.h GsrAllocFn).  A callback that returns NULL
    -- the caller out of memory -- makes gsr_forward return GSR_ERR_ALLOC with a message, touches nothing, and leaves the library
    usable: the next call with a working allocator renders the image it rendered before."""
    import hip_runner
    R_ = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    L_ = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    sc = parity.syn.make_scene(5000, 160, 120, sh_degree=1, seed=12)
    kw = parity.scene_kwargs(sc, "sh")
    monkeypatch.setenv("GSR_BINDING", "ctypes")
    ref = hip_runner.run_hip(kw)["fwd"]
    good = R_._Workspace._alloc
    calls = {"n": 0}

    def failing(self, nbytes, tag, user):
        is_bin = tag == L_.GSR_ALLOC_BINNING
        if (fail_tag == "binning") == is_bin:
            calls["n"] += 1
            return None
        return good(self, nbytes, tag, user)
    monkeypatch.setattr(R_._Workspace, "_alloc", failing)
    with pytest.raises(RuntimeError) as ei:
        hip_runner.run_hip(kw)
    assert calls["n"] >= 1 and "code -3" in str(ei.value) and "allocation failed" in str(ei.value), str(ei.value)
    monkeypatch.setattr(R_._Workspace, "_alloc", good)
    again = hip_runner.run_hip(kw)["fwd"]
    for x, y in zip(ref, again):
        assert np.array_equal(x, y)


def test_calc_importance_matches_oracle():
    """Merge-time pruning score (ht3dgs_trainer.py:1427-1462): |dL/dSH| with grad_out = 1 through clamp(0,1),
    summed over views, / num_pixels -- against the float64 oracle's backward."""
    from oracle import binding
    hier = importlib.import_module("3dgs_hierarchical_training_amd.hierarchy")
    dev = torch.device("cuda:0")
    N, W, H = 20000, 320, 240
    views, ref = [], np.zeros((N, 16, 3))
    base = parity.syn.make_scene(N, W, H, sh_degree=3, seed=31, posed=False)
    for s in (1, 2):
        cam = parity.syn.make_scene(8, W, H, sh_degree=3, seed=100 + s, posed=True)   # only its camera is used
        sc = dict(base)
        for k in ("viewmatrix", "projmatrix", "campos", "tanfovx", "tanfovy"):
            sc[k] = cam[k]
        views.append(ts.make_settings(sc, dev, 3))
        kw = parity.scene_kwargs(sc, "sh")
        o = binding.OracleRender(**kw)
        color = o.forward()[0]
        g = ((color >= 0) & (color <= 1)).astype(np.float32)        # d clamp(x,0,1).sum() / dx
        ref += np.abs(o.backward(g, None, None)["shs"])
        o.close()
    ref = ref.reshape(N, 48) / (2 * W * H)
    p = ts.GaussianParams(base, dev, optimizer="torch")
    seg = {k: getattr(p, k).detach() for k in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")}
    imp = hier.calc_importance(seg, views).cpu().numpy()
    assert imp.shape == (N, 48)
    # all-ones upstream gradient on every pixel (ambiguous ones included): a rounding-edge flip moves one
    # contribution of one pixel, far below the scale of a sum over all pixels
    assert np.abs(imp - ref).max() <= 1e-3 * ref.max()
    drop = hier.prune_mask(torch.from_numpy(imp), 0.5)
    assert int(drop.sum()) == N // 2
    sc_ref = ref.max(1)
    assert sc_ref[drop.numpy()].mean() < sc_ref[~drop.numpy()].mean()


@pytest.mark.parametrize("fused", [True, False], ids=["optimizer-in-backward", "torch-adam"])
def test_training_recovers_a_perturbed_scene(fused):
    """End to end: targets are renders of a ground-truth cloud from three cameras; training starts from a copy with perturbed
    colours, opacities, positions and scales and cycles through the views like the reference's loop
    (ht3dgs_trainer.py:81-169).  The photometric loss must fall by more than 5x -- gradients, optimizer-in-backward and the
    loss kernels pull in the same, right direction across views (a sign or convention error in any of them does not)."""
    import importlib
    ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
    syn = importlib.import_module("3dgs_hierarchical_training_amd.synthetic")
    dev = torch.device("cuda:0")
    N, W, H = 4000, 256, 192
    gt_scene = syn.make_scene(N, W, H, sh_degree=3, seed=5, sigma_px=4.0, frac_behind=0.0)
    gen = torch.Generator().manual_seed(9)
    cams = [dict(gt_scene)]
    for k in range(2):
        c = syn.make_camera(W, H, R=syn.random_rotation(gen, 0.12), t=0.1 * torch.randn(3, generator=gen))
        s = dict(gt_scene); s.update(c); cams.append(s)
    gt_params = ts.GaussianParams(gt_scene, dev, optimizer="hip" if fused else "torch")
    settings = [ts.make_settings(s, dev, 3) for s in cams]
    with torch.no_grad():
        targets = [ts.render(gt_params, st)["image"].clone() for st in settings]
    start = dict(gt_scene)
    g2 = torch.Generator().manual_seed(1)
    start["shs"] = gt_scene["shs"] + 0.25 * torch.randn(gt_scene["shs"].shape, generator=g2)
    start["opacities"] = (gt_scene["opacities"] * (0.5 + torch.rand(N, 1, generator=g2))).clamp(0.02, 0.98)
    start["means3D"] = gt_scene["means3D"] + 0.01 * torch.randn(N, 3, generator=g2)
    start["scales"] = gt_scene["scales"] * torch.exp(0.2 * torch.randn(N, 3, generator=g2))
    params = ts.GaussianParams(start, dev, optimizer="hip" if fused else "torch")

    def mean_loss():
        with torch.no_grad():
            return sum(float(ts.photometric_loss(ts.render(params, st)["image"], tg)) for st, tg in zip(settings, targets)) / len(settings)

    l0 = mean_loss()
    for it in range(450):
        v = it % len(settings)
        ts.train_step(params, settings[v], targets[v], fused_optimizer=fused)
    l1 = mean_loss()
    print(f"loss {l0:.5f} -> {l1:.5f}")
    assert l1 < 0.2 * l0, (l0, l1)


def test_extension_ops_run_under_torch_compile():
    """The rasterizer and the fused loss are dispatcher ops with fake kernels (_ext.py): a function built from them compiles
    (torch.compile, graph breaks allowed) and gives the eager loss and gradients."""
    R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    Ls = importlib.import_module("3dgs_hierarchical_training_amd.loss")
    dev = torch.device("cuda:0")
    sc = parity.syn.make_scene(5000, 160, 120, sh_degree=3, seed=1)
    p = ts.GaussianParams(sc, dev, optimizer="torch")
    st = ts.make_settings(sc, dev, 3)
    gt = parity.syn.target_image(160, 120).to(dev)

    def f(xyz, dc, rest, op, sca, rot, target):
        color = R.rasterize_gaussians_raw(xyz, torch.zeros_like(xyz), dc, rest, op, sca, rot, st)[0]
        return Ls.fused_photometric_loss(color, target, 0.2, True)

    args = [p._xyz, p._features_dc, p._features_rest, p._opacity, p._scaling, p._rotation]
    l0 = f(*args, gt)
    l0.backward()
    g0 = [a.grad.clone() for a in args]
    for a in args:
        a.grad = None
    # compile in this process: inductor's default pool of compile workers (one per core, up to 32) would inherit this process's open
    # GPU device file, and that many processes holding the GPU is more than a shared machine allows.  (The backward graph compiles
    # inside backward(), so both stay under the setting.)
    import torch._inductor.config as inductor_config
    with inductor_config.patch(compile_threads=1):
        l1 = torch.compile(f)(*args, gt)
        l1.backward()
    assert abs(float(l0.detach()) - float(l1.detach())) < 1e-6
    for a, b in zip(g0, [a.grad for a in args]):
        assert (a - b).abs().max().item() <= 2e-5 * a.abs().max().item() + 1e-12


PREPARE_SHAPES = [(12800, 3), (10007, 3), (4098, 3), (101, 3), (130, 3), (12800, 0), (10007, 0), (4098, 1), (12800, 2), (130, 0),
                  (12800, "up"), (10007, "up")]
PREPARE_IDS = ["whole-blocks", "ragged-odd", "ragged-mod4", "one-ragged-block", "two-blocks-ragged", "deg0-whole", "deg0-ragged-odd",
               "deg1-ragged-mod4", "deg2-whole", "deg0-two-blocks-ragged", "degree-steps-up-whole", "degree-steps-up-ragged"]


@pytest.mark.parametrize("digits_in_backward", [True, False], ids=["digits-counted-in-backward", "histogram-launch"])
@pytest.mark.parametrize("N,deg", PREPARE_SHAPES, ids=PREPARE_IDS)
def test_prepare_in_backward_is_bit_identical(N, deg, digits_in_backward):
    """"Prepare in backward" (GsrNextView): with `next_settings` the backward that applies the Adam step also runs the NEXT
    render's preprocess on the updated parameters, and that render skips k_preprocess.  Two copies of one model trained on
    two alternating cameras, one with and one without the hand-over, must stay EQUAL: images, radii, parameters, moments --
    bit for bit, on whole blocks and on ragged last blocks (N not a multiple of 128 / of 4).  (The blend backward runs in its
    fixed-order mode here, "deterministic_backward"; the default accumulation: the test below.)
    The hand-over buffer also carries the next depth sort's scratch: its counters are cleared by the blend backward, and up
    to 262 144 Gaussians the per-Gaussian kernel counts the sort's digits too (no histogram launch in the forward); both
    sides of that threshold are run here ("prep_hist_max_n").
    deg: the model's ACTIVE SH degree with 16 coefficients stored (gsr_prepare_supported(16, D, 1) for D = 0..3) -- the
    reference's models start at degree 0 and step up once per 1 000 iterations (gaussian_model_ht.py:68,193-195); "up" walks
    0 -> 1 -> 2 -> 3 with an `oneup_sh_degree()` after every second step, announced through `next_sh_degree` so that the
    hand-over survives the change."""
    _prepare_in_backward_test(N, deg, digits_in_backward, fixed_order=True)


@pytest.mark.parametrize("N,deg", [PREPARE_SHAPES[i] for i in (0, 1, 3, 5, 11)], ids=[PREPARE_IDS[i] for i in (0, 1, 3, 5, 11)])
def test_prepare_in_backward_is_bit_identical_on_the_default_accumulation(N, deg):
    """The same on the default backward (float64 atomics across a Gaussian's tiles): equal up to rounding-boundary flips of inexact
    sums (parity.same_accumulation: at most 4 entries per tensor).  A representative subset of the shapes above -- whole blocks,
    ragged blocks, one ragged block, degree 0, the degree steps -- with the digits counted in the backward."""
    _prepare_in_backward_test(N, deg, True, fixed_order=False)


def _prepare_in_backward_test(N, deg, digits_in_backward, fixed_order):
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    lib = L.load()
    assert lib.gsr_set_option(b"deterministic_backward", 1 if fixed_order else 0) == 0
    assert lib.gsr_set_option(b"prep_hist_max_n", 262144 if digits_in_backward else 0) == 0
    for D in range(4):
        assert lib.gsr_prepare_supported(16, D, 1) == 1
    assert lib.gsr_prepare_supported(9, 2, 1) == 0 and lib.gsr_prepare_supported(16, 3, 0) == 0
    try:
        _prepare_in_backward_case(N, deg, fixed_order)
    finally:
        lib.gsr_set_option(b"deterministic_backward", 0)
        lib.gsr_set_option(b"prep_hist_max_n", 262144)


def _prepare_in_backward_case(N, deg=3, fixed_order=True):
    dev = torch.device("cuda:0")
    W, H = 320, 240
    up = deg == "up"
    d0 = 0 if up else deg
    sc = parity.syn.make_scene(N, W, H, sh_degree=d0, seed=17)
    cam2 = parity.syn.make_scene(8, W, H, sh_degree=d0, seed=5, posed=True)
    sc2 = dict(sc)
    for k in ("viewmatrix", "projmatrix", "campos"):
        sc2[k] = cam2[k]
    views = [ts.make_settings(sc, dev, d0), ts.make_settings(sc2, dev, d0)]
    gts = [parity.syn.target_image(W, H, seed=1).to(dev), parity.syn.target_image(W, H, seed=2).to(dev)]
    pa, pb = ts.GaussianParams(sc, dev), ts.GaussianParams(sc, dev)
    assert pa.active_sh_degree == d0 and pa.max_sh_degree == 3
    names = ["_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"]
    used = 0
    steps = 8 if up else 6
    for it in range(steps):
        v = it % 2
        had = getattr(pa, "_prepared", None) is not None
        raise_after = up and it % 2 == 1 and pa.active_sh_degree < 3          # `oneupSHdegree` after this step
        ka = ts.train_step(pa, views[v], gts[v], next_settings=views[(it + 1) % 2],
                           next_sh_degree=pa.active_sh_degree + 1 if raise_after else None)
        kb = ts.train_step(pb, views[v], gts[v])
        if raise_after:
            pa.oneup_sh_degree(); pb.oneup_sh_degree()
        used += int(had)
        got = {k: ka[k] for k in ("raw_image", "radii", "depth", "alpha")}
        want = {k: kb[k] for k in ("raw_image", "radii", "depth", "alpha")}
        got["viewspace_points"], want["viewspace_points"] = ka["viewspace_points"].grad, kb["viewspace_points"].grad
        for k in names:
            got[k], want[k] = getattr(pa, k).detach(), getattr(pb, k).detach()
        # the moments too (bands above the active degree decay with a zero gradient, as dense Adam has it)
        for ga, gb in zip(pa.optimizer.param_groups, pb.optimizer.param_groups):
            sa, sb = pa.optimizer.state[ga["params"][0]], pb.optimizer.state[gb["params"][0]]
            for mom in ("exp_avg", "exp_avg_sq"):
                got[ga["name"] + "/" + mom], want[gb["name"] + "/" + mom] = sa[mom], sb[mom]
        # fixed order: equal bits; default accumulation: equal up to rounding-boundary flips of inexact cross-tile sums
        parity.same_accumulation(got, want, f"prepare in backward, step {it}", max_entries=0 if fixed_order else None, verbose=False)
    assert used == steps - 1              # every step after the first rendered from a hand-over buffer -- across the degree changes too
    if up:
        assert pa.active_sh_degree == 3
    else:
        # bands above the active degree received no gradient: untouched parameters, zero moments
        nact = (d0 + 1) ** 2 - 1
        assert torch.equal(pa._features_rest[:, nact:], sc["shs"][:, 1 + nact:].to(dev))
        st = pa.optimizer.state[pa._features_rest]
        assert float(st["exp_avg"][:, nact:].abs().sum()) == 0.0
    # an un-announced degree change drops the buffer instead of rendering stale colours
    if not up and d0 < 3:
        ts.train_step(pa, views[0], gts[0], next_settings=views[0])
        ts.train_step(pb, views[0], gts[0])
        assert pa._prepared is not None
        pa.oneup_sh_degree(); pb.oneup_sh_degree()
        ka = ts.train_step(pa, views[0], gts[0], next_settings=views[0])
        kb = ts.train_step(pb, views[0], gts[0])
        assert torch.equal(ka["raw_image"], kb["raw_image"])
    # a render with a DIFFERENT camera does not pick the buffer up, and surgery drops it
    ts.train_step(pa, views[0], gts[0], next_settings=views[0])
    assert pa._prepared is not None
    with torch.no_grad():
        ts.render(pa, views[1], fused_activations=True)
    assert pa._prepared is None
    ts.train_step(pa, views[0], gts[0], next_settings=views[0])
    pa.prune_points(torch.zeros(pa.num_points, dtype=torch.bool, device=dev))
    assert pa._prepared is None
    ts.train_step(pa, views[0], gts[0])


def test_a_render_that_never_reaches_backward_leaves_the_optimizer_untouched():
    """the in-kernel Adam step is PLANNED at render time and COUNTED when its backward runs.  A fused render under
    torch.no_grad(), a render whose loss is discarded, and an exception between forward and backward must not advance the bias-
    correction step; afterwards the fused step and a plain backward + step() on a twin model still agree."""
    dev = torch.device("cuda:0")
    W, H, N = 256, 192, 6000
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=3)
    st = ts.make_settings(sc, dev, 3)
    gt = parity.syn.target_image(W, H, seed=1).to(dev)
    pa, pb = ts.GaussianParams(sc, dev), ts.GaussianParams(sc, dev)
    ts.train_step(pa, st, gt); ts.train_step(pb, st, gt, fused_optimizer=False)
    assert pa.optimizer.step_count == 1 and pb.optimizer.step_count == 1
    with torch.no_grad():                                        # a render that cannot have a backward
        ts.render(pa, st, fused_activations=True, fused_adam=pa.optimizer)
    pkg = ts.render(pa, st, fused_activations=True, fused_adam=pa.optimizer)     # a graph that is dropped
    del pkg
    assert pa.optimizer.step_count == 1 and not pa.optimizer._stepped_in_backward
    pa.optimizer.step()                                          # nothing pending: a no-op, no complaint
    for _ in range(2):
        ts.train_step(pa, st, gt); ts.train_step(pb, st, gt, fused_optimizer=False)
    assert pa.optimizer.step_count == 3 and pb.optimizer.step_count == 3
    # (equal, as in test_optimizer_in_backward_equals_backward_then_step, up to rounding-boundary flips of the blend backward's
    #  float64 cross-tile sums; a step count off by one -- a wrong bias correction 1 / (1 - 0.9^t) at t = 2 instead of 3 -- would move
    #  EVERY element by 30 % of a step)
    got, want = {}, {}
    for name, k in ts.GaussianParams._GROUP_ATTR.items():
        got[k], want[k] = getattr(pa, k).detach(), getattr(pb, k).detach()
        sa, sb = pa.optimizer.state[getattr(pa, k)], pb.optimizer.state[getattr(pb, k)]
        for mom in ("exp_avg", "exp_avg_sq"):
            got[k + "/" + mom], want[k + "/" + mom] = sa[mom], sb[mom]
    parity.same_accumulation(got, want, "fused step after renders without a backward vs plain steps")
    # state_dict reports the reconciled count in torch's layout
    sd = pa.optimizer.state_dict()
    assert all(int(v["step"]) == 3 for v in sd["state"].values())


def test_pose_step_between_prepare_and_consume_invalidates_the_hand_over():
    """gsr::pose_step / pose_step_camera write the transform / camera tensors through raw pointers; they now bump the
    tensors' version counters, so the staleness guards of train_step.render (`_same_transform`, `_camera_versions`) fire when a pose
    moves between the backward that prepared a buffer and the forward that would consume it."""
    dev = torch.device("cuda:0")
    W, H, N = 256, 192, 5000
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=9)
    ident = ts.make_settings(sc, dev, 3)
    gt = parity.syn.target_image(W, H, seed=1).to(dev)
    # camera route
    cps = ts.CameraPoseState(ident, torch.eye(4), dev, lr=1e-3)
    v0 = ts._camera_versions(cps.settings)
    pa = ts.GaussianParams(sc, dev)
    ts.train_step(pa, cps.settings, gt, next_settings=cps.settings)          # prepares for the SAME camera tensors (no `pose=`: not stepped here)
    assert pa._prepared is not None and pa._prepared["valid"]
    pkg = ts.render(ts.GaussianParams(sc, dev, optimizer="torch"), cps.settings, fused_activations=True)
    pkg["raw_image"].sum().backward()
    cps.step()                                                               # the pose moves: versions change
    assert ts._camera_versions(cps.settings) != v0
    pb = ts.GaussianParams.from_raw(pa.raw(), dev)
    ka = ts.render(pa, cps.settings, fused_activations=True)                 # must NOT use the stale buffer
    kb = ts.render(pb, cps.settings, fused_activations=True)
    assert pa._prepared is None
    assert torch.equal(ka["raw_image"], kb["raw_image"])
    # transform-of-the-means route
    ps = ts.PoseState(torch.eye(4), dev, lr=1e-3)
    tag = (ps.M.data_ptr(), ps.M._version)
    leaf = ps.leaf()
    pkg = ts.render(ts.GaussianParams(sc, dev, optimizer="torch"), ident, fused_activations=True, points_transform=leaf)
    pkg["raw_image"].sum().backward()
    ps.step()
    assert not ts._same_transform(tag, ps.M)


def test_pose_refinement_in_the_train_step_keeps_the_hand_over_exact():
    """The reference steps the current frame's pose after every render (camera_optimizer, ht3dgs_trainer.py:162-166).  Here the
    pose is the in-kernel transform Exp(delta) * base (train_step.PoseState) and its update is one kernel (gsr_pose_step).  With
    per-frame transforms the "prepare in backward" hand-over must use the NEXT frame's transform (GsrNextView.points_transform) and
    must be dropped when the next render is of the SAME frame (its transform changes in between): two copies of a model trained
    on three alternating frames, one with and one without the hand-over, stay EQUAL -- images, parameters, pose tangents -- and
    the poses, started off their true values, move towards them."""
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    pose_mod = importlib.import_module("3dgs_hierarchical_training_amd.pose")
    lib = L.load()
    dev = torch.device("cuda:0")
    W, H, N = 320, 240, 12800
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=21)
    ident = ts.make_settings(sc, dev, 3)
    true = [pose_mod.se3_exp(torch.tensor(v)) for v in ([0.0] * 6, [0.03, -0.01, 0.02, 0.004, -0.006, 0.003], [-0.02, 0.02, 0.01, -0.005, 0.002, 0.004])]
    off = [pose_mod.se3_exp(torch.tensor(v)) for v in ([0.0] * 6, [0.006, 0.004, -0.005, 0.002, 0.001, -0.002], [-0.005, 0.006, 0.004, -0.001, -0.002, 0.002])]
    gtp = ts.GaussianParams(sc, dev, optimizer="torch")
    with torch.no_grad():
        gts = [ts.render(gtp, ident, fused_activations=True, points_transform=t[:3].to(dev))["image"].clone() for t in true]
    order = [0, 1, 2, 2, 1, 0, 1, 1, 2, 0, 2, 1]          # includes the same frame twice in a row
    assert lib.gsr_set_option(b"deterministic_backward", 1) == 0
    try:
        runs = []
        for hand_over in (True, False):
            p = ts.GaussianParams(sc, dev)
            for g in p.optimizer.param_groups:            # the model is the truth: keep it (almost) still, only the poses move
                g["lr"] = g["lr"] * 1e-3
            ps = [ts.PoseState(off[k] @ true[k], dev, lr=5e-4) for k in range(3)]
            ps[0].frozen = True
            imgs, used = [], 0
            for i, f in enumerate(order):
                nf = order[i + 1] if i + 1 < len(order) else None
                had = getattr(p, "_prepared", None) is not None
                pkg = ts.train_step(p, ident, gts[f], pose=ps[f], next_settings=ident if (hand_over and nf is not None) else None,
                                    next_pose=ps[nf] if (hand_over and nf is not None) else None)
                used += int(had)
                imgs.append(pkg["raw_image"].detach().clone())
            runs.append((p, ps, imgs, used))
        (pa, psa, ia, used_a), (pb, psb, ib, used_b) = runs
        assert used_b == 0 and used_a == sum(1 for i in range(len(order) - 1) if order[i] != order[i + 1])
        for x, y in zip(ia, ib):
            assert torch.equal(x, y)
        for k in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
            assert torch.equal(getattr(pa, k), getattr(pb, k)), k
        for a, b in zip(psa, psb):
            assert torch.equal(a.delta, b.delta) and torch.equal(a.M, b.M)
        assert float(psa[0].delta.abs().max()) == 0.0                       # the gauge frame never moves
        for k in (1, 2):
            e0 = (off[k] @ true[k] - true[k])[:3].abs().max().item()
            e1 = (psa[k].matrix() - true[k])[:3].abs().max().item()
            assert e1 < e0, (k, e0, e1)
    finally:
        lib.gsr_set_option(b"deterministic_backward", 0)


def test_f_rest_group_is_skipped_while_its_moments_are_zero():
    """GsrFusedAdam with no moment buffers for f_rest (exp_avg[2] = exp_avg_sq[2] = NULL): at SH degree 0 the group's gradient is
    identically zero, and while its moments are zero Adam's update of it is the identity -- FusedAdam then plans the step
    without the group (three quarters of the update's traffic; all of stage A and a leaf's first 1 000 iterations run like
    that).  Two copies of one model, one planning with the skip and one that never skips, must stay EQUAL bit for bit --
    images, parameters, moments -- through degree-0 steps with and without the hand-over, through the announced step up to
    degree 1 (where the skip ends for good), and after an in-place change of the moments through torch (version counter:
    re-validated, not skipped).  The library refuses the skip at a degree where the gradient is not zero."""
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    lib = L.load()
    dev = torch.device("cuda:0")
    W, H, N = 320, 240, 12800 + 37
    assert lib.gsr_set_option(b"deterministic_backward", 1) == 0
    try:
        sc = parity.syn.make_scene(N, W, H, sh_degree=0, seed=21)
        cam2 = parity.syn.make_scene(8, W, H, sh_degree=0, seed=5, posed=True)
        sc2 = dict(sc)
        for k in ("viewmatrix", "projmatrix", "campos"):
            sc2[k] = cam2[k]
        views = [ts.make_settings(sc, dev, 0), ts.make_settings(sc2, dev, 0)]
        gts = [parity.syn.target_image(W, H, seed=1).to(dev), parity.syn.target_image(W, H, seed=2).to(dev)]
        names = ["_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"]

        def never(opt):
            opt._rest_moments_zero = lambda m, v: False

        def same(pa, pb, what):
            for k in names:
                assert torch.equal(getattr(pa, k), getattr(pb, k)), (what, k)
            for ga, gb in zip(pa.optimizer.param_groups, pb.optimizer.param_groups):
                sa, sb = pa.optimizer.state[ga["params"][0]], pb.optimizer.state[gb["params"][0]]
                assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), (what, ga["name"])
                assert sa["step"] == sb["step"], (what, ga["name"])

        pa, pb = ts.GaussianParams(sc, dev), ts.GaussianParams(sc, dev)
        never(pb.optimizer)
        rest0 = pa._features_rest.detach().clone()
        for it in range(5):
            v = it % 2
            nxt = views[(it + 1) % 2] if it != 2 else None           # one step without the hand-over
            ka = ts.train_step(pa, views[v], gts[v], next_settings=nxt)
            kb = ts.train_step(pb, views[v], gts[v], next_settings=nxt)
            assert torch.equal(ka["raw_image"], kb["raw_image"]), it
            same(pa, pb, it)
        grp = {"xyz": pa._xyz, "f_dc": pa._features_dc, "f_rest": pa._features_rest, "opacity": pa._opacity, "scaling": pa._scaling,
               "rotation": pa._rotation}
        ms, vs = pa.optimizer.fused_step_plan(grp, 0, 0)[:2]
        assert ms[2].numel() == 0 and vs[2].numel() == 0 and ms[1].numel() > 0       # the plan really leaves the group out ...
        assert pb.optimizer.fused_step_plan({k: getattr(pb, a) for k, a in zip(grp, names)}, 0, 0)[0][2].numel() > 0
        assert pa.optimizer.fused_step_plan(grp, 0, 1)[0][2].numel() > 0             # ... but not in front of a degree-1 view
        assert pa.optimizer._rest_zero_checks == 1                                   # validated once, not every step
        assert torch.equal(pa._features_rest, rest0)
        st = pa.optimizer.state[pa._features_rest]
        assert int(torch.count_nonzero(st["exp_avg"])) == 0 and int(torch.count_nonzero(st["exp_avg_sq"])) == 0
        # the step up to degree 1, announced: the hand-over needs the rows, the skip is off for that step and for good afterwards
        ka = ts.train_step(pa, views[1], gts[1], next_settings=views[0], next_sh_degree=1)
        kb = ts.train_step(pb, views[1], gts[1], next_settings=views[0], next_sh_degree=1)
        pa.oneup_sh_degree(); pb.oneup_sh_degree()
        for it in range(3):
            v = it % 2
            ka = ts.train_step(pa, views[v], gts[v], next_settings=views[(it + 1) % 2])
            kb = ts.train_step(pb, views[v], gts[v], next_settings=views[(it + 1) % 2])
            assert torch.equal(ka["raw_image"], kb["raw_image"]), it
            same(pa, pb, ("deg1", it))
        assert int(torch.count_nonzero(pa.optimizer.state[pa._features_rest]["exp_avg"])) > 0
        assert pa.optimizer._rest_zero[4] is False
        # moments changed in place through torch while at degree 0: seen (version counter), re-validated, not skipped
        pc, pd = ts.GaussianParams(sc, dev), ts.GaussianParams(sc, dev)
        never(pd.optimizer)
        ts.train_step(pc, views[0], gts[0]); ts.train_step(pd, views[0], gts[0])
        for p in (pc, pd):
            p.optimizer.state[p._features_rest]["exp_avg"].add_(0.01)
        ts.train_step(pc, views[1], gts[1]); ts.train_step(pd, views[1], gts[1])
        same(pc, pd, "after an in-place change")
        assert pc.optimizer._rest_zero_checks == 2 and not torch.equal(pc._features_rest, rest0)
        # the library's own guard: no skipping where the gradient is not zero
        pe = ts.GaussianParams(sc, dev)
        pe.oneup_sh_degree()
        e = torch.empty(0, device=dev)
        pe.optimizer._plan_moments = lambda ms, vs, d, nd: (ms[:2] + [e] + ms[3:], vs[:2] + [e] + vs[3:])
        with pytest.raises(RuntimeError, match="sh_degree 0"):
            ts.train_step(pe, ts.with_sh_degree(views[0], 1), gts[0])
    finally:
        lib.gsr_set_option(b"deterministic_backward", 0)


def test_balanced_blend_placement_changes_nothing_but_the_order():
    """Round 4: the forward blend places its sub-tile waves by the visits each took at the previous render of the same view (a
    device-side cache keyed by a hash of the view matrix, csrc/gsr_kernels.hip balance_build).  Whatever the cache holds the
    placement is a permutation: first render of a view (miss: identity), second render (hit: snake order by predicted visits),
    another view in between, the same view after the scene changed -- image, depth, alpha, radii and the gradients of a
    deterministic backward are bit-identical with the option switched off."""
    import importlib
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
    lib = L.load()
    dev = torch.device("cuda:0")
    W, H, N = 500, 333, 60000
    views = []
    for seed, posed in ((3, False), (4, True)):
        sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=3, posed=False)
        if posed:
            cam = parity.syn.make_scene(8, W, H, sh_degree=3, seed=seed, posed=True)
            for k in ("viewmatrix", "projmatrix", "campos"):
                sc[k] = cam[k]
        views.append(sc)
    g = torch.Generator().manual_seed(9)
    wc = torch.randn(3, H, W, generator=g).to(dev)

    def run(sc, scale):
        t = {k: sc[k].to(dev).clone().requires_grad_(True) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
        with torch.no_grad():
            t["scales"] *= scale
        st = ts.make_settings(sc, dev, 3)
        m2d = torch.zeros(N, 3, device=dev, requires_grad=True)
        out = R.GaussianRasterizer(st)(means3D=t["means3D"], means2D=m2d, shs=t["shs"], colors_precomp=None, opacities=t["opacities"],
                                       scales=t["scales"], rotations=t["rotations"], cov3D_precomp=None)
        (out[0] * wc).sum().backward()
        return [o.detach().clone() for o in out] + [t[k].grad.clone() for k in sorted(t)] + [m2d.grad.clone()]
    seq = [(0, 1.0), (0, 1.0), (1, 1.0), (0, 1.3), (1, 1.0), (0, 1.3)]     # (view, scene change)
    assert lib.gsr_set_option(b"deterministic_backward", 1) == 0
    try:
        res = {}
        for bal in (0, 1):
            assert lib.gsr_set_option(b"blend_balance", bal) == 0
            res[bal] = [run(views[v], s) for v, s in seq]
    finally:
        lib.gsr_set_option(b"deterministic_backward", 0)
        lib.gsr_set_option(b"blend_balance", 1)
    for i, (a, b) in enumerate(zip(res[0], res[1])):
        for j, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), (i, j)


def test_densify_and_reset_iterations_drop_that_iterations_update_like_the_reference():
    """VERDICT r3 item 8.  In the reference the adaptive density control sits between backward() and optimizer.step() and replaces
    parameter tensors by fresh nn.Parameters without .grad (ht3dgs_trainer.py:137-160, gaussian_model_ht.py:584-629, :468-474): a
    densification iteration drops the Adam update of all six groups, an opacity-reset iteration that of the opacity group, and the
    step counts stay behind accordingly.  The fused train step (optimizer inside the backward kernel) must do the same -- it runs
    those iterations unfused -- and agree with the reference-order route (separate torch.optim.Adam step) throughout."""
    dm = importlib.import_module("3dgs_hierarchical_training_amd.densify")
    dev = torch.device("cuda:0")
    sc = parity.syn.make_scene(9000, 256, 192, sh_degree=3, seed=23)
    gt = parity.syn.target_image(256, 192).to(dev)
    settings = ts.make_settings(sc, dev, 3)
    names = ["_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"]
    # densify at iterations 3 and 6 (nothing selected: the threshold is out of reach -- the tensors are replaced all the same),
    # opacity reset at iteration 4
    cfg = dm.DensifyConfig(densification_interval=3, densify_from_iter=1, opacity_reset_interval=4, densify_grad_threshold=1e9,
                           min_opacity=0.0, densify_until_iter=100)
    pa, pb = ts.GaussianParams(sc, dev, optimizer="hip"), ts.GaussianParams(sc, dev, optimizer="torch")
    da, db = dm.Densifier(pa, 1e9, cfg), dm.Densifier(pb, 1e9, cfg)      # (an extent that keeps the world-size prune out of the way)
    assert [da.touches_parameters_at(i) for i in range(1, 8)] == [False, False, True, True, False, True, False]
    for it in range(1, 8):
        before = {k: getattr(pa, k).detach().clone() for k in names}
        ts.train_step(pa, settings, gt, densifier=da, iteration=it)                                               # fused everything
        ts.train_step(pb, settings, gt, fused_loss=False, fused_activations=False, fused_optimizer=False, densifier=db, iteration=it)
        if it in (3, 6):      # the whole update of a densification iteration is dropped: bit for bit the parameters of the iteration before
            for k in names:
                assert torch.equal(getattr(pa, k).detach(), before[k]), (it, k)
        elif it == 4:         # opacity reset: the other five groups step, the opacity is min(sigmoid(o), 0.01) of the UN-updated logits
            for k in names:
                if k != "_opacity":
                    assert not torch.equal(getattr(pa, k).detach(), before[k]), k
            want = ts.inverse_sigmoid(torch.min(torch.sigmoid(before["_opacity"]), torch.full_like(before["_opacity"], 0.01)))
            assert torch.allclose(pa._opacity.detach(), want, rtol=0, atol=1e-6)
        else:
            assert not torch.equal(pa._xyz.detach(), before["_xyz"])
    for k in names:
        a, b = getattr(pa, k).detach(), getattr(pb, k).detach()
        lr = next(g["lr"] for g in pa.optimizer.param_groups if g["params"][0] is getattr(pa, k))
        bad = ((a - b).abs() > 0.05 * lr + 5e-7 * b.abs()).float().mean().item()
        assert bad < 2e-3, (k, bad)
        sa, sb = pa.optimizer.state.get(getattr(pa, k), {}), pb.optimizer.state.get(getattr(pb, k), {})
        assert int(sa.get("step", 0)) == int(sb.get("step", 0)), (k, sa.get("step"), sb.get("step"))
    pa.optimizer._reconcile()
    assert int(pa.optimizer.state[pa._xyz]["step"]) == 5 and int(pa.optimizer.state[pa._opacity]["step"]) in (3, 4)


def test_three_pass_depth_sort_and_its_window_overflow():
    """Round 4: models above 262 144 Gaussians sort their depth keys in three 9-bit passes over the 27 bits of (key - bits(0.2)) --
    the window [0.2, 13 107) of view depths.  (i) Inside the window the forward is bit-identical with the four 8-bit passes.
    (ii) A visible Gaussian beyond the window is detected (a counter in the sort's scratch head, read back with the instance
    count), the forward sorts again on all 32 bits from the clamped result and takes the exact flow: bit-identical again, the
    counter "depth_window_resorts" says so, and that caller stays on the four-pass sort (no second resort)."""
    import importlib
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    lib = L.load()
    lib.gsr_get_counter.restype = __import__("ctypes").c_int64
    dev = torch.device("cuda:0")
    W, H, N = 400, 300, 300000
    sc = parity.syn.make_scene(N, W, H, sh_degree=1, seed=17, posed=False)
    st = ts.make_settings(sc, dev, 1)

    def render(means):
        out = R.GaussianRasterizer(st)(means3D=means, means2D=torch.zeros(N, 3, device=dev), shs=sc["shs"].to(dev), colors_precomp=None,
                                       opacities=sc["opacities"].to(dev), scales=scales, rotations=sc["rotations"].to(dev), cov3D_precomp=None)
        return [o.clone() for o in out]
    scales = sc["scales"].to(dev)
    near = sc["means3D"].to(dev)
    # far: the same cloud with a few hundred Gaussians pushed along their viewing rays to depths of 20 000 - 60 000 (still on screen,
    # scaled up with the distance so that they keep covering pixels)
    far = near.clone()
    idx = torch.arange(0, N, 1000, device=dev)
    f = torch.linspace(4000.0, 9000.0, idx.numel(), device=dev)[:, None]
    far[idx] = far[idx] * f
    scales_far = scales.clone()
    scales_far[idx] = scales_far[idx] * f
    try:
        assert lib.gsr_set_option(b"reset_speculation", 1) == 0
        assert lib.gsr_set_option(b"tile_sort", 0) == 0      # the global depth sort is the subject: the per-tile sort route has none
        res = {}
        for mode in (0, 1):
            assert lib.gsr_set_option(b"depth_sort9", mode) == 0
            res[mode, "near"] = render(near)
            c0 = lib.gsr_get_counter(b"depth_window_resorts")
            scales = scales_far
            res[mode, "far"] = render(far)
            c1 = lib.gsr_get_counter(b"depth_window_resorts")
            res[mode, "far2"] = render(far)
            c2 = lib.gsr_get_counter(b"depth_window_resorts")
            scales = sc["scales"].to(dev)
            if mode == 1:
                assert (c1 - c0, c2 - c1) == (1, 0), (c0, c1, c2)
            else:
                assert c0 == c1 == c2
        assert int((res[1, "far"][1][idx] > 0).sum()) > 10          # (far Gaussians are on screen: their keys were sorted, not culled)
        for key in ("near", "far", "far2"):
            for a, b in zip(res[0, key], res[1, key]):
                assert torch.equal(a, b), key
    finally:
        lib.gsr_set_option(b"depth_sort9", 1)
        lib.gsr_set_option(b"tile_sort", 1)
        lib.gsr_set_option(b"reset_speculation", 1)


def test_balanced_blend_placement_survives_more_views_than_the_cache_holds():
    """The per-view visit cache of the forward blend holds 128 views (least recently used out): a walk over 140 cameras, twice --
    every second visit a hit on a live entry or a miss on an evicted one -- renders each view bit-identically with the placement
    switched off."""
    import importlib
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    lib = L.load()
    dev = torch.device("cuda:0")
    W, H, N = 200, 150, 8000
    sc = parity.syn.make_scene(N, W, H, sh_degree=1, seed=3, posed=False)
    t = {k: sc[k].to(dev) for k in ("means3D", "shs", "opacities", "scales", "rotations")}
    sts = []
    for v in range(140):
        cam = parity.syn.make_scene(8, W, H, sh_degree=1, seed=100 + v, posed=True)
        sts.append(ts.make_settings(dict(sc, viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"], campos=cam["campos"]), dev, 1))

    def walk():
        outs = []
        for rep in range(2):
            for st in sts:
                o = R.GaussianRasterizer(st)(means3D=t["means3D"], means2D=torch.zeros(N, 3, device=dev), shs=t["shs"], colors_precomp=None,
                                             opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"], cov3D_precomp=None)
                outs.append([x.clone() for x in o])
        return outs
    try:
        assert lib.gsr_set_option(b"blend_balance", 0) == 0
        a = walk()
        assert lib.gsr_set_option(b"blend_balance", 1) == 0
        b = walk()
    finally:
        lib.gsr_set_option(b"blend_balance", 1)
    for i, (x, y) in enumerate(zip(a, b)):
        for u, v in zip(x, y):
            assert torch.equal(u, v), i


def _view_cache_stats(lib, W, H):
    import ctypes as C
    out = (C.c_int64 * 4)()
    assert lib.gsr_debug_view_cache_stats(W, H, out) == 0
    return {"lookups": out[0], "hits": out[1], "entries": out[2], "caches": out[3]}


@pytest.mark.parametrize("with_id", [False, True])
def test_balanced_blend_placement_recognises_frames_under_the_reference_calling_convention(with_id):
    """VERDICT r4 item 2.  The reference renders every frame through an IDENTITY camera and moves the points
    (/root/reference/trainer/trainer.py:993-995, scene/gaussian_model_ht.py:135-148: `points_transform` here), and steps the frame's
    pose after every render (ht3dgs_trainer.py:162-166).  Eight frames visited in random order, each pose drifting by ~1e-4 per visit:
    with the caller's frame id (what gsr_autopatch fills from `viewpoint_camera.uid`) and without one (frames recognised by their
    pose, view matrix AND points transform, within the tolerance) every visit after a frame's first is a HIT on that frame's own
    entry -- the round-4 key (a hash of the view-matrix bits alone) put all eight frames into one entry -- and the image / radii are
    bit-identical with the placement switched off."""
    import importlib
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    lib = L.load()
    dev = torch.device("cuda:0")
    W, H, N, F = 487 + (1 if with_id else 0), 300, 40000, 8        # (a frame size of its own: a fresh cache, so the counters below are this test's)
    sc = parity.syn.make_scene(N, W, H, sh_degree=1, seed=3, posed=False)
    st = ts.make_settings(sc, dev, 1)                  # identity camera for every frame
    p = ts.GaussianParams(sc, dev, optimizer="torch")
    gen = torch.Generator().manual_seed(5)
    base = []
    for f in range(F):
        M = torch.eye(4)
        M[:3, :3] = parity.syn.random_rotation(gen, 0.05)
        M[:3, 3] = 0.05 * torch.randn(3, generator=gen)
        base.append(M[:3].contiguous())
    order = [int(x) for x in torch.randint(0, F, (48,), generator=gen)]
    drift = [1e-4 * torch.randn(3, 4, generator=gen) for _ in order]

    def walk():
        poses = [b.clone() for b in base]
        outs = []
        with torch.no_grad():
            for f, d in zip(order, drift):
                poses[f] = poses[f] + d                               # the pose step after the previous render of this frame
                o = R.rasterize_gaussians_raw(p._xyz, torch.zeros(N, 3, device=dev), p._features_dc, p._features_rest, p._opacity, p._scaling,
                                              p._rotation, st, points_transform=poses[f].to(dev), view_id=(f + 1) if with_id else 0)
                outs.append([x.clone() for x in o[:4]])
        return outs
    try:
        assert lib.gsr_set_option(b"blend_balance", 0) == 0
        a = walk()
        assert lib.gsr_set_option(b"blend_balance", 1) == 0
        s0 = _view_cache_stats(lib, W, H)
        b = walk()
        s1 = _view_cache_stats(lib, W, H)
    finally:
        lib.gsr_set_option(b"blend_balance", 1)
    for i, (x, y) in enumerate(zip(a, b)):
        for u, v in zip(x, y):
            assert torch.equal(u, v), i
    lookups, hits = s1["lookups"] - s0["lookups"], s1["hits"] - s0["hits"]
    assert lookups == len(order) and hits == len(order) - len(set(order)), (s0, s1)      # every frame misses once, then always hits
    assert s1["entries"] - s0["entries"] == len(set(order)), (s0, s1)                      # ... on an entry of its own


def test_view_cache_keeps_frames_apart_that_are_farther_than_the_tolerance():
    """Without an id two poses share a cache entry only when every matrix entry is within "view_pose_tol_e6" (default 2e-3): a pose
    2e-2 away is another frame (its own entry), one 5e-4 away is the same frame (a hit, and the entry follows it)."""
    import importlib
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    lib = L.load()
    dev = torch.device("cuda:0")
    W, H, N = 491, 300, 20000
    sc = parity.syn.make_scene(N, W, H, sh_degree=1, seed=4, posed=False)
    st = ts.make_settings(sc, dev, 1)
    p = ts.GaussianParams(sc, dev, optimizer="torch")

    def render(tx):
        M = torch.eye(4)[:3].contiguous()
        M[0, 3] = tx
        with torch.no_grad():
            R.rasterize_gaussians_raw(p._xyz, torch.zeros(N, 3, device=dev), p._features_dc, p._features_rest, p._opacity, p._scaling,
                                      p._rotation, st, points_transform=M.to(dev))
    s0 = _view_cache_stats(lib, W, H)
    for tx in (0.0, 5e-4, 1e-3, 1.5e-3, 2e-2, 2.05e-2, 1.9e-3):      # the entry follows its frame: 1.9e-3 is 4e-4 from the last render of frame A
        render(tx)
    s1 = _view_cache_stats(lib, W, H)
    assert s1["lookups"] - s0["lookups"] == 7 and s1["hits"] - s0["hits"] == 5 and s1["entries"] - s0["entries"] == 2, (s0, s1)


def test_training_steps_are_reproducible_bit_for_bit():
    """The same scene, cameras and targets give the same model every run: bench.py's step (fused activations, loss and Adam, the
    next view prepared in the backward, densification statistics) run twice from the same start ends in identical parameters,
    statistics, render and loss.  The blend backward adds a Gaussian's per-tile parts with float64 atomics, so the order the tiles
    arrive in -- which differs from run to run -- reaches a float32 gradient only when a float32 rounding boundary falls between
    two orders' float64 sums (blend_common.h: about 2^-29 relative of an inexact sum).  With the float32 atomics this replaced,
    every Gaussian whose sum took three or more parts could differ in its last bits, and Adam carried that into the model."""
    dev = torch.device("cuda:0")
    dm = importlib.import_module("3dgs_hierarchical_training_amd.densify")
    W, H = 640, 360
    sc = parity.syn.make_scene(200000, W, H, sh_degree=3, seed=12)
    views = [(ts.make_settings(sc, dev, 3), parity.syn.target_image(W, H, seed=1).to(dev))]
    gen = torch.Generator().manual_seed(4)
    for k in (2, 3):
        cam = parity.syn.make_camera(W, H, R=parity.syn.random_rotation(gen, 0.05), t=0.05 * torch.randn(3, generator=gen))
        views.append((ts.make_settings({**sc, **cam}, dev, 3), parity.syn.target_image(W, H, seed=k).to(dev)))
    runs = []
    for _ in range(2):
        p = ts.GaussianParams(sc, dev)
        den = dm.Densifier(p, scene_extent=5.0, cfg=dm.DensifyConfig(densify_from_iter=10 ** 9, opacity_reset_interval=10 ** 9,
                                                                       densify_until_iter=10 ** 9))
        for i in range(12):
            pkg = ts.train_step(p, views[i % 3][0], views[i % 3][1], next_settings=views[(i + 1) % 3][0], densifier=den, iteration=i + 1)
        torch.cuda.synchronize(dev)
        runs.append({**{k: v.clone() for k, v in p.raw().items()}, "loss": pkg["loss"].clone(), "image": pkg["raw_image"].detach().clone(),
                     "xyz_gradient_accum": den.xyz_gradient_accum.clone(), "max_radii2D": den.max_radii2D.clone()})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), (k, (runs[0][k] - runs[1][k]).abs().max().item())
