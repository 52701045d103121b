"""gsr_autopatch's `HTGaussianModel.densify_and_prune` / `prune_points` on the CPU: the installation, every fallback to the original method, and
the flag derivation and install logic with the two resize calls replaced by the numpy oracles of tests/resize_common.py.

(The kernels behind the two calls are checked in tests/test_gpu_resize.py; the patched methods on them in tests/test_gpu_autopatch_resize.py.)"""
import sys
import types

import pytest
import torch

import autopatch_resize_common as C

refstub = C.refstub


@pytest.fixture
def autopatch(monkeypatch):
    import gsr_autopatch
    monkeypatch.setenv("GSR_AUTOPATCH_RESIZE", "1")
    gsr_autopatch.apply()
    yield gsr_autopatch
    gsr_autopatch._REQUIRE_CUDA = True
    gsr_autopatch.remove()


@pytest.fixture
def seam(autopatch, monkeypatch):
    """CPU tensors are taken and resize.py is the oracle stand-in."""
    fake = C.OracleResize()
    monkeypatch.setattr(autopatch, "_REQUIRE_CUDA", False)
    monkeypatch.setattr(autopatch, "_resize", lambda: fake)
    return fake


# ---- installation -----------------------------------------------------------------------------------------------------------------------------
def _stand_in_module(with_methods=True):
    mod = types.ModuleType("scene.gaussian_model_ht")

    class HTGaussianModel:
        if with_methods:
            def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size):
                return "original densify_and_prune"

            def prune_points(self, mask):
                return "original prune_points"
    mod.HTGaussianModel = HTGaussianModel
    return mod


@pytest.mark.parametrize("order", ["module first", "apply first"])
def test_apply_installs_the_two_methods_and_remove_restores_them(monkeypatch, order):
    import gsr_autopatch
    monkeypatch.setenv("GSR_AUTOPATCH_RESIZE", "1")
    gsr_autopatch.remove()
    mod = _stand_in_module()
    cls = mod.HTGaussianModel
    orig = (cls.densify_and_prune, cls.prune_points)
    try:
        if order == "module first":
            monkeypatch.setitem(sys.modules, "scene.gaussian_model_ht", mod)
            gsr_autopatch.apply()
        else:
            gsr_autopatch.apply()
            gsr_autopatch._patch_render_and_pose_module(mod)            # what the import hook calls once the module has been executed
        assert cls.densify_and_prune is gsr_autopatch.densify_and_prune_fused and cls.prune_points is gsr_autopatch.prune_points_fused
        gsr_autopatch._patch_render_and_pose_module(mod)                # idempotent: the original stays the original
        assert [f for c, a, f in gsr_autopatch._patched_resize_classes if c is cls] == list(orig)
    finally:
        gsr_autopatch.remove()
    assert (cls.densify_and_prune, cls.prune_points) == orig and not gsr_autopatch._patched_resize_classes


def test_the_switch_leaves_the_methods_alone(monkeypatch):
    import gsr_autopatch
    monkeypatch.setenv("GSR_AUTOPATCH_RESIZE", "0")
    gsr_autopatch.remove()
    mod = _stand_in_module()
    orig = (mod.HTGaussianModel.densify_and_prune, mod.HTGaussianModel.prune_points)
    monkeypatch.setitem(sys.modules, "scene.gaussian_model_ht", mod)
    gsr_autopatch.apply()
    try:
        assert (mod.HTGaussianModel.densify_and_prune, mod.HTGaussianModel.prune_points) == orig
    finally:
        gsr_autopatch.remove()


def test_a_class_without_the_methods_is_skipped(autopatch):
    mod = _stand_in_module(with_methods=False)
    autopatch._patch_render_and_pose_module(mod)
    assert not hasattr(mod.HTGaussianModel, "densify_and_prune") and not hasattr(mod.HTGaussianModel, "prune_points")
    assert not any(c is mod.HTGaussianModel for c, _, _ in autopatch._patched_resize_classes)
    autopatch._patch_resize_module(types.ModuleType("scene.gaussian_model_ht"))       # no class at all


def test_the_shipped_default_is_documented():
    """ON or OFF is decided by the measurement in profiles/trainer_resize.txt; the module docstring and the profile name the same default."""
    import os
    import gsr_autopatch
    assert gsr_autopatch._RESIZE_DEFAULT in ("0", "1")
    word = "ON" if gsr_autopatch._RESIZE_DEFAULT == "1" else "OFF"
    assert f"GSR_AUTOPATCH_RESIZE: ships {word}" in gsr_autopatch.__doc__
    with open(os.path.join(C.HERE, "..", "profiles", "trainer_resize.txt")) as f:
        assert f"GSR_AUTOPATCH_RESIZE: ships {word}" in f.read()


# ---- fallbacks: the original runs, and nothing was changed or drawn first ---------------------------------------------------------------------
class _Recorder:
    """Originals that record their call and what they find: the model untouched, the generator where it was."""

    def __init__(self, autopatch):
        self.calls = []
        cls = type("HTGaussianModel", (refstub.StubSurgeryModel,), {"__module__": refstub.__name__})
        rec = self

        def densify_and_prune(m, max_grad, min_opacity, extent, max_screen_size):
            rec.calls.append(("densify_and_prune", rec.fingerprint(m), (max_grad, min_opacity, extent, max_screen_size)))

        def prune_points(m, mask):
            rec.calls.append(("prune_points", rec.fingerprint(m), mask))
        cls.densify_and_prune, cls.prune_points = densify_and_prune, prune_points
        autopatch._patch_resize_module(types.SimpleNamespace(HTGaussianModel=cls))
        assert cls.prune_points is autopatch.prune_points_fused
        self.cls = cls

    @staticmethod
    def fingerprint(m):
        ts = [getattr(m, k) for k in C.RAW + C.STATS]
        return [(id(t), t._version) for t in ts], [id(g["params"][0]) for g in getattr(m.optimizer, "param_groups", ())], torch.get_rng_state().clone()

    def expect_fallback(self, m, call, which):
        before = self.fingerprint(m)
        self.calls.clear()
        call(m)
        assert len(self.calls) == 1 and self.calls[0][0] == which, (which, self.calls)
        seen = self.calls[0][1]
        assert seen[0] == before[0] and seen[1] == before[1] and torch.equal(seen[2], before[2]), which
        after = self.fingerprint(m)
        assert after[0] == before[0] and after[1] == before[1] and torch.equal(after[2], before[2]), which


def _swap_param(m, attr, tensor):
    """Replace one parameter consistently (model attribute and optimizer group) by `tensor`."""
    p = torch.nn.Parameter(tensor)
    name = dict((a, n) for n, a in C.GROUPS)[attr]
    next(g for g in m.optimizer.param_groups if g["name"] == name)["params"][0] = p
    setattr(m, attr, p)


FALLBACKS = {
    "pose group beside rotation": lambda m: m.optimizer.param_groups.append({"params": [torch.nn.Parameter(torch.zeros(1, 6))], "lr": 0.001, "name": "R"}),
    "five groups": lambda m: m.optimizer.param_groups.pop(),
    "a group renamed": lambda m: m.optimizer.param_groups[1].__setitem__("name", "features"),
    "two parameters in a group": lambda m: m.optimizer.param_groups[0]["params"].append(torch.nn.Parameter(torch.zeros(3))),
    "a group's parameter is not the model's": lambda m: setattr(m, "_opacity", torch.nn.Parameter(m._opacity.detach().clone())),
    "float64 parameter": lambda m: _swap_param(m, "_opacity", m._opacity.detach().double()),
    "strided parameter": lambda m: _swap_param(m, "_rotation", torch.randn(4, m._xyz.shape[0]).t()),
    "rows unlike N": lambda m: _swap_param(m, "_features_dc", m._features_dc.detach()[:-1].clone()),
    "statistics unlike N": lambda m: setattr(m, "max_radii2D", m.max_radii2D[:-1].clone()),
    "float64 statistics": lambda m: setattr(m, "denom", m.denom.double()),
    "moment shape unlike its parameter": lambda m: m.optimizer.state[m._scaling].__setitem__("exp_avg", torch.zeros(m._xyz.shape[0], 1)),
    "a moment missing": lambda m: m.optimizer.state[m._scaling].pop("exp_avg_sq"),
    "no optimizer": lambda m: setattr(m, "optimizer", None),
}


@pytest.mark.parametrize("broken", sorted(FALLBACKS))
def test_every_unexpected_layout_runs_the_original_untouched(seam, autopatch, broken):
    rec = _Recorder(autopatch)
    state = C.make_state(40, 16, "mixture", moments=True)
    m = C.build(rec.cls, state, "adam")
    FALLBACKS[broken](m)
    mask = torch.zeros(40, dtype=torch.bool)
    mask[::3] = True
    rec.expect_fallback(m, lambda m: m.densify_and_prune(*state["args"]), "densify_and_prune")
    rec.expect_fallback(m, lambda m: m.prune_points(mask), "prune_points")
    assert seam.plans == 0 and seam.waits == 0


def test_the_other_fallbacks_run_the_original_untouched(seam, autopatch, monkeypatch):
    rec = _Recorder(autopatch)
    state = C.make_state(40, 16, "mixture", moments=True)
    m = C.build(rec.cls, state, "fused")
    mask = torch.zeros(40, dtype=torch.bool)
    dp = lambda *a: (lambda m: m.densify_and_prune(*a))
    # max_grad that is not positive: a cloned row could qualify for a split
    for bad in (0.0, -1.0, float("nan")):
        rec.expect_fallback(m, dp(bad, 0.005, 4.0, 20), "densify_and_prune")
    # a mask that is not a bool tensor [N]
    for bad in (mask.to(torch.uint8), mask[:-1], mask[:, None], mask[0], mask.tolist(), torch.nonzero(mask)[:, 0]):
        rec.expect_fallback(m, lambda m, bad=bad: m.prune_points(bad), "prune_points")
    # a CPU tensor anywhere (the rule itself: _REQUIRE_CUDA as shipped)
    monkeypatch.setattr(autopatch, "_REQUIRE_CUDA", True)
    rec.expect_fallback(m, dp(*state["args"]), "densify_and_prune")
    rec.expect_fallback(m, lambda m: m.prune_points(mask), "prune_points")
    monkeypatch.setattr(autopatch, "_REQUIRE_CUDA", False)
    # the switch, read at the call as well
    monkeypatch.setenv("GSR_AUTOPATCH_RESIZE", "0")
    rec.expect_fallback(m, dp(*state["args"]), "densify_and_prune")
    rec.expect_fallback(m, lambda m: m.prune_points(mask), "prune_points")
    monkeypatch.setenv("GSR_AUTOPATCH_RESIZE", "1")
    # N = 0
    empty = C.build(rec.cls, {**state, "raw": {k: v[:0] for k, v in state["raw"].items()}, "stats": {k: v[:0] for k, v in state["stats"].items()},
                              "moments": None}, "fused")
    rec.expect_fallback(empty, dp(*state["args"]), "densify_and_prune")
    rec.expect_fallback(empty, lambda m: m.prune_points(mask[:0]), "prune_points")
    # a model whose module has no build_rotation
    other = type("HTGaussianModel", (rec.cls,), {"__module__": __name__})
    rec.expect_fallback(C.build(other, state, "fused"), dp(*state["args"]), "densify_and_prune")
    assert seam.plans == 0 and seam.waits == 0
    # ... and a model that is none of these goes through the seam
    m.prune_points(mask)
    assert seam.plans == 1 and not rec.calls[1:]


def test_a_direct_call_without_an_original_is_an_error(seam, autopatch):
    m = C.build(refstub.StubSurgeryModel, C.make_state(8, 16, "mixture", moments=False), "adam")
    m.optimizer.param_groups.pop()
    with pytest.raises(RuntimeError, match="original HTGaussianModel.prune_points"):
        autopatch.prune_points_fused(m, torch.zeros(8, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="original HTGaussianModel.densify_and_prune"):
        autopatch.densify_and_prune_fused(m, 0.0002, 0.005, 4.0, None)


# ---- flag derivation and install logic against the unpatched stand-in --------------------------------------------------------------------------
@pytest.mark.parametrize("optimizer", ["adam", "fused"])
@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no-state"])
@pytest.mark.parametrize("n,coeffs", [(1, 16), (65, 16), (200, 1)])
def test_patched_densify_and_prune_equals_the_unpatched_stand_in(seam, autopatch, n, coeffs, moments, optimizer):
    cls = C.patched_class(autopatch)
    for regime in C.REGIMES:
        state = C.make_state(n, coeffs, regime, moments)
        a, b = C.build(cls, state, optimizer), C.build(refstub.StubSurgeryModel, state, optimizer)
        seam.waits, seam.applies = 0, []
        rng_a, before = C.run(a, lambda m: m.densify_and_prune(*state["args"]))
        rng_b, _ = C.run(b, lambda m: m.densify_and_prune(*state["args"]))
        what = f"{regime} N={n}"
        C.assert_installed(a, before)
        C.assert_installed(b)
        C.assert_same_model(a, b, what)
        assert torch.equal(rng_a, rng_b), what
        assert seam.waits == 1 and len(seam.applies) == 1 and len(seam.applies[0]) == (18 if moments else 6), what
        if regime == "all_pruned":
            assert a._xyz.shape[0] == 0
        if regime == "nothing":
            assert a._xyz.shape[0] == n
        if regime in ("clones", "splits", "mixture", "denom_zero") and n > 1:
            assert a._xyz.shape[0] != n or not torch.equal(a._xyz.detach(), state["raw"]["_xyz"]), what


@pytest.mark.parametrize("optimizer", ["adam", "fused"])
@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no-state"])
def test_patched_prune_points_equals_the_unpatched_stand_in(seam, autopatch, moments, optimizer):
    cls = C.patched_class(autopatch)
    for n, coeffs in ((1, 16), (65, 16), (200, 1)):
        state = C.make_state(n, coeffs, "mixture", moments)
        for kind, mask in (("all false", torch.zeros(n, dtype=torch.bool)), ("all true", torch.ones(n, dtype=torch.bool)),
                           ("random", torch.rand(n, generator=torch.Generator().manual_seed(n)) < 0.5)):
            a, b = C.build(cls, state, optimizer), C.build(refstub.StubSurgeryModel, state, optimizer)
            seam.waits, seam.applies = 0, []
            rng_a, before = C.run(a, lambda m: m.prune_points(mask))
            rng_b, _ = C.run(b, lambda m: m.prune_points(mask))
            C.assert_installed(a, before)
            C.assert_same_model(a, b, f"{kind} N={n}")
            assert torch.equal(rng_a, rng_b)
            assert float(b.max_radii2D.sum()) > 0 or kind == "all true" or n == 1               # non-zero statistics went through
            assert seam.waits == 1 and [len(k) for k in seam.applies] == [18 if moments else 6, 3]


def test_the_original_prune_and_split_run_over_the_patched_prune_points(seam, autopatch):
    cls = C.patched_class(autopatch)
    state = C.make_state(120, 16, "world_size", moments=True)
    for what in (lambda m: m.prune(*state["args"]),
                 lambda m: m.densify_and_split(m._mean_gradient(), state["args"][0], state["args"][2]),
                 lambda m: m.densify(*state["args"])):
        a, b = C.build(cls, state, "adam"), C.build(refstub.StubSurgeryModel, state, "adam")
        seam.plans = 0
        rng_a, before = C.run(a, what)
        rng_b, _ = C.run(b, what)
        C.assert_installed(a, before)
        C.assert_same_model(a, b)
        assert torch.equal(rng_a, rng_b) and seam.plans == 1 and a._xyz.shape[0] != 120


def test_empty_cache_switch_is_read(seam, autopatch, monkeypatch):
    """CPU tensors never reach torch.cuda.empty_cache(); on a device it is the last call unless GSR_AUTOPATCH_EMPTY_CACHE=0 (GPU test)."""
    called = []
    monkeypatch.setattr(torch.cuda, "empty_cache", lambda: called.append(1))
    cls = C.patched_class(autopatch)
    state = C.make_state(30, 16, "mixture", moments=False)
    C.run(C.build(cls, state, "adam"), lambda m: m.densify_and_prune(*state["args"]))
    assert not called


# ---- against the reference's own run ------------------------------------------------------------------------------------------------------------
def _golden_call(m, state, case):
    if case == "d":
        m.prune_points(state["mask"])
    else:
        m.densify_and_prune(*state["args"])


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
@pytest.mark.parametrize("arm", ["patched", "stand-in"])
def test_both_arms_reproduce_the_references_run(seam, autopatch, arm, case):
    """tests/golden/trainer_resize.npz is what the reference's own HTGaussianModel did on these inputs, with the samples it drew handed to
    `torch.normal`: the patched methods AND the stand-in they are compared with everywhere else both land on it."""
    d = C.golden()
    state = C.golden_state(d, case)
    cls = C.patched_class(autopatch) if arm == "patched" else refstub.StubSurgeryModel
    m = C.build(cls, state, "adam")
    with torch.no_grad():
        if case == "d":
            _golden_call(m, state, case)
        else:
            with C.inject_samples(d[case + "_samples"]) as inj:
                _golden_call(m, state, case)
            assert inj.calls == 1
    C.assert_installed(m)
    C.assert_matches_golden(m, d, case)
    assert (seam.plans > 0) == (arm == "patched")
