"""gsr_autopatch's `HTGaussianModel.densify_and_prune` / `prune_points` on the GPU: the patched methods (selections by the model's own torch
statements, rows moved by gsr_resize_plan / gsr_resize_apply) against the unpatched `refstub.StubSurgeryModel` on clones of one state -- every
tensor, moment, step, statistic and the device generator's state bit for bit -- and against the reference's own run (tests/golden)."""
import importlib
import types
import warnings

import pytest
import torch

import autopatch_resize_common as C
import parity

pytestmark = pytest.mark.gpu
refstub = C.refstub
DEV = "cuda:0"


@pytest.fixture
def autopatch(monkeypatch):
    import gsr_autopatch
    monkeypatch.setenv("GSR_AUTOPATCH_RESIZE", "1")
    monkeypatch.delenv("GSR_AUTOPATCH_EMPTY_CACHE", raising=False)
    gsr_autopatch.apply()
    yield gsr_autopatch
    gsr_autopatch.remove()


def _both(cls, state, optimizer, what, label):
    a, b = C.build(cls, state, optimizer), C.build(refstub.StubSurgeryModel, state, optimizer)
    rng_a, before = C.run(a, what)
    rng_b, _ = C.run(b, what)
    C.assert_installed(a, before)
    C.assert_installed(b)
    C.assert_same_model(a, b, label)
    assert torch.equal(rng_a, rng_b), label
    return a


@pytest.mark.parametrize("coeffs", [16, 1], ids=["16-coefficients", "1-coefficient"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_patched_equals_unpatched_in_every_regime(autopatch, n, coeffs):
    """Sizes around the plan's tile edge, a zero-width `_features_rest`, both optimizers, with and without moments, every regime."""
    cls = C.patched_class(autopatch)
    for optimizer in ("adam", "fused"):
        for moments in (True, False):
            for regime in C.REGIMES:
                state = C.make_state(n, coeffs, regime, moments, device=DEV)
                label = f"{regime} N={n} {optimizer} moments={moments}"
                a = _both(cls, state, optimizer, lambda m: m.densify_and_prune(*state["args"]), label)
                if regime == "all_pruned":
                    assert a._xyz.shape[0] == 0, label
                if regime == "nothing":
                    assert a._xyz.shape[0] == n, label
                if regime in ("clones", "splits") and n >= 255:
                    assert a._xyz.shape[0] > n, label
            state = C.make_state(n, coeffs, "mixture", moments, device=DEV)
            masks = {"all false": torch.zeros(n, dtype=torch.bool, device=DEV), "all true": torch.ones(n, dtype=torch.bool, device=DEV),
                     "random": (torch.rand(n, generator=torch.Generator().manual_seed(n)) < 0.5).to(DEV)}
            for kind, mask in masks.items():
                a = _both(cls, state, optimizer, lambda m: m.prune_points(mask), f"prune_points {kind} N={n} {optimizer} moments={moments}")
                assert a._xyz.shape[0] == int((~mask).sum())
                if kind == "all false" and n > 1:
                    assert float(a.max_radii2D.sum()) > 0 and float(a.denom.sum()) > 0             # non-zero statistics went through


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_the_references_own_run(autopatch, case):
    """tests/golden/trainer_resize.npz: what the reference's HTGaussianModel did on these inputs, its samples handed to `torch.normal`."""
    d = C.golden()
    state = C.golden_state(d, case, device=DEV)
    for cls in (C.patched_class(autopatch), refstub.StubSurgeryModel):
        m = C.build(cls, state, "adam")
        with torch.no_grad():
            if case == "d":
                m.prune_points(state["mask"])
            else:
                with C.inject_samples(d[case + "_samples"]) as inj:
                    m.densify_and_prune(*state["args"])
                assert inj.calls == 1
        C.assert_installed(m)
        C.assert_matches_golden(m, d, case)


def test_the_original_prune_and_split_run_over_the_patched_prune_points(autopatch):
    cls = C.patched_class(autopatch)
    state = C.make_state(600, 16, "world_size", moments=True, device=DEV)
    for what in (lambda m: m.prune(*state["args"]),
                 lambda m: m.densify_and_split(m._mean_gradient(), state["args"][0], state["args"][2]),
                 lambda m: m.densify(*state["args"])):
        a = _both(cls, state, "fused", what, "original callers")
        assert a._xyz.shape[0] != 600


def test_forty_iterations_of_the_trainers_sequence_with_the_deferred_step(autopatch, monkeypatch):
    """The unmodified trainer's iteration (render, loss, backward, statistics, densify_and_prune every 10th iteration, optimizer.step(),
    zero_grad) on the patched render and the deferred FusedAdam step: with the patched surgery the trajectory is the unpatched one bit for
    bit, the dropped update of the densification iterations included."""
    monkeypatch.setenv("GSR_AUTOPATCH_DEFERRED", "1")
    monkeypatch.setenv("GSR_AUTOPATCH_DEFERRED_MIN_N", "0")
    W, H, N = 128, 96, 3000
    sc = parity.syn.make_scene(N, W, H, sh_degree=3, seed=2)
    gt = parity.syn.target_image(W, H, seed=1).to(DEV)
    cam = refstub.StubCamera.from_scene(sc, DEV, original_image=gt)
    ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
    raw = {k: v.to(DEV) for k, v in ts.GaussianParams(sc, "cpu", optimizer="torch").raw().items()}
    loss_cfg = types.SimpleNamespace(cfg=types.SimpleNamespace(lambda_dssim=0.2, lambda_depth=0.0))

    def trajectory(cls):
        g = cls(raw, optimizer="fused", percent_dense=0.01)
        r = types.SimpleNamespace(gaussians=g, bg_color=torch.zeros(3, device=DEV))
        sizes, steps = [], []
        torch.manual_seed(3)
        for it in range(1, 41):
            pkg = autopatch.render_fused(r, cam)
            autopatch.loss_forward(loss_cfg, pkg["image"], gt)["loss"].backward()
            with torch.no_grad():
                vis, radii = pkg["visibility_filter"], pkg["radii"]
                g.max_radii2D[vis] = torch.max(g.max_radii2D[vis], radii[vis])
                autopatch.add_densification_stats_fused(g, pkg["viewspace_points"], vis)
                if it % 10 == 0:
                    g.densify_and_prune(1e-6, 0.005, 30.0, 20 if it > 20 else None)
                g.optimizer.step()
                g.optimizer.zero_grad(set_to_none=True)
            sizes.append(g._xyz.shape[0])
            steps.append(int(g.optimizer.state[g._xyz]["step"]) if g._xyz in g.optimizer.state else 0)
        return g, sizes, steps, torch.cuda.get_rng_state(DEV)
    a, sizes_a, steps_a, rng_a = trajectory(C.patched_class(autopatch))
    b, sizes_b, steps_b, rng_b = trajectory(refstub.StubSurgeryModel)
    print("rows per iteration (patched):", sizes_a[9::10], "steps:", steps_a[9::10])
    assert sizes_a == sizes_b and steps_a == steps_b and len(set(sizes_a)) > 1
    assert steps_a[-1] == 36                                                     # four densification iterations dropped their update
    C.assert_same_model(a, b, "trajectory")
    assert torch.equal(rng_a, rng_b)


def _sync_warnings(f):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            f()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() for w in seen)


def test_host_waits_per_call(autopatch, monkeypatch):
    """A patched call waits for the device as often as one `.cpu()` read and one `torch.cuda.empty_cache()` do; without the latter
    (GSR_AUTOPATCH_EMPTY_CACHE=0), exactly once.  The unpatched arm's count is printed beside it."""
    cls = C.patched_class(autopatch)
    state = C.make_state(1000, 16, "mixture_screen_20", moments=True, device=DEV)
    mask = (torch.rand(1000, generator=torch.Generator().manual_seed(1)) < 0.5).to(DEV)
    probe = torch.arange(5, device=DEV)

    def count(klass, call):
        C.run(C.build(klass, state, "fused"), call)               # (a first call pays one-time initialisations)
        m = C.build(klass, state, "fused")
        return _sync_warnings(lambda: C.run(m, call))
    dp = lambda m: m.densify_and_prune(*state["args"])
    pp = lambda m: m.prune_points(mask)
    one_read = _sync_warnings(lambda: probe.cpu())
    one_read_and_empty_cache = _sync_warnings(lambda: (probe.cpu(), torch.cuda.empty_cache()))
    assert one_read == 1
    patched_dp, unpatched_dp = count(cls, dp), count(refstub.StubSurgeryModel, dp)
    patched_pp, unpatched_pp = count(cls, pp), count(refstub.StubSurgeryModel, pp)
    monkeypatch.setenv("GSR_AUTOPATCH_EMPTY_CACHE", "0")
    patched_dp_lean = count(cls, dp)
    print(f"synchronisation warnings per call: densify_and_prune patched {patched_dp} (without empty_cache {patched_dp_lean}), unpatched {unpatched_dp}; "
          f"prune_points patched {patched_pp}, unpatched {unpatched_pp}; one .cpu() read {one_read}, with empty_cache {one_read_and_empty_cache}")
    assert patched_dp == one_read_and_empty_cache
    assert patched_dp_lean == 1
    assert patched_pp == 1
    assert unpatched_dp > patched_dp and unpatched_pp > patched_pp
