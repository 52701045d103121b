"""gsr_autopatch's `HTGaussianTrainer.merge_two_3DGS` on the CPU: the installation, every fallback to the original method, the tail on an
importance the kernels do not take, and the flag and count derivation and the install logic with the three device calls replaced by the numpy
oracles of tests/merge_common.py -- against `refstub.StubMergeTrainer`, against the reference's own run (tests/golden/trainer_merge.npz) and,
where scores tie, against `np.argsort(key, kind="stable")[:k]`.

(The kernels behind the calls are checked in tests/test_gpu_merge.py; the patched method on them in tests/test_gpu_autopatch_merge.py.)"""
import os
import sys
import types

import numpy as np
import pytest
import torch

import autopatch_merge_common as C
import merge_common as MC

refstub = C.refstub


@pytest.fixture
def autopatch(monkeypatch):
    import gsr_autopatch
    monkeypatch.setenv("GSR_AUTOPATCH_MERGE", "1")
    gsr_autopatch.apply()
    yield gsr_autopatch
    gsr_autopatch._REQUIRE_CUDA = True
    gsr_autopatch.remove()


@pytest.fixture
def seam(autopatch, monkeypatch):
    """CPU tensors are taken; merge.py and resize.py are the oracle stand-in."""
    fake = C.OracleMerge()
    monkeypatch.setattr(autopatch, "_REQUIRE_CUDA", False)
    monkeypatch.setattr(autopatch, "_merge", lambda: fake)
    monkeypatch.setattr(autopatch, "_resize", lambda: fake)
    return fake


# ---- installation -----------------------------------------------------------------------------------------------------------------------------
def _stand_in_module(with_method=True):
    mod = types.ModuleType("trainer.ht3dgs_trainer")

    class HTGaussianTrainer:
        @staticmethod
        def calc_importance(gs_render, cameras, pipe):
            return "original calc_importance"
        if with_method:
            def merge_two_3DGS(self, gs_render_dst, gs_render_src, transform_matrix, to_visit_frames_dst=None, to_visit_frames_src=None):
                return "original merge_two_3DGS"
    mod.HTGaussianTrainer = HTGaussianTrainer
    return mod


@pytest.mark.parametrize("order", ["module first", "apply first"])
def test_apply_installs_the_method_and_remove_restores_it(monkeypatch, order):
    import gsr_autopatch
    monkeypatch.setenv("GSR_AUTOPATCH_MERGE", "1")
    gsr_autopatch.remove()
    mod = _stand_in_module()
    cls = mod.HTGaussianTrainer
    orig = cls.merge_two_3DGS
    try:
        if order == "module first":
            monkeypatch.setitem(sys.modules, "trainer.ht3dgs_trainer", mod)
            gsr_autopatch.apply()
        else:
            gsr_autopatch.apply()
            gsr_autopatch._patch_trainer_module(mod)                     # what the import hook calls once the module has been executed
        assert cls.merge_two_3DGS is gsr_autopatch.merge_two_3DGS_fused
        assert cls.calc_importance is gsr_autopatch.calc_importance_fused    # the patch beside it, through the same hook
        gsr_autopatch._patch_trainer_module(mod)                         # idempotent: the original stays the original
        assert [f for c, a, f in gsr_autopatch._patched_merge_classes if c is cls] == [orig]
        # whatever the patched body cannot serve reaches the original (here: no models at all)
        assert cls().merge_two_3DGS(None, None, None) == "original merge_two_3DGS"
    finally:
        gsr_autopatch.remove()
    assert cls.merge_two_3DGS is orig and not gsr_autopatch._patched_merge_classes
    assert cls().merge_two_3DGS(None, None, None) == "original merge_two_3DGS"


def test_the_import_hook_patches_the_module_when_it_is_imported_later(tmp_path, monkeypatch):
    """A module with the reference's path, class and method names, imported AFTER apply(): the post-import hook installs the method."""
    import importlib
    import gsr_autopatch
    monkeypatch.setenv("GSR_AUTOPATCH_MERGE", "1")
    gsr_autopatch.remove()
    pkg = tmp_path / "trainer"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    (pkg / "ht3dgs_trainer.py").write_text(
        "class HTGaussianTrainer:\n    @staticmethod\n    def calc_importance(gs_render, cameras, pipe):\n        return 'original'\n"
        "    def merge_two_3DGS(self, a, b, t, fa=None, fb=None):\n        return 'original merge'\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    saved = {m: sys.modules.pop(m, None) for m in ("trainer.ht3dgs_trainer", "trainer")}
    try:
        gsr_autopatch.apply()
        T = importlib.import_module("trainer.ht3dgs_trainer")
        assert T.HTGaussianTrainer.merge_two_3DGS is gsr_autopatch.merge_two_3DGS_fused
        gsr_autopatch.remove()
        assert T.HTGaussianTrainer().merge_two_3DGS(None, None, None) == "original merge"
    finally:
        gsr_autopatch.remove()
        for m in ("trainer.ht3dgs_trainer", "trainer"):
            sys.modules.pop(m, None)
            if saved[m] is not None:
                sys.modules[m] = saved[m]


def test_the_switch_leaves_the_method_alone(monkeypatch):
    import gsr_autopatch
    monkeypatch.setenv("GSR_AUTOPATCH_MERGE", "0")
    gsr_autopatch.remove()
    mod = _stand_in_module()
    orig = mod.HTGaussianTrainer.merge_two_3DGS
    monkeypatch.setitem(sys.modules, "trainer.ht3dgs_trainer", mod)
    gsr_autopatch.apply()
    try:
        assert mod.HTGaussianTrainer.merge_two_3DGS is orig and not gsr_autopatch._patched_merge_classes
        assert mod.HTGaussianTrainer.calc_importance is gsr_autopatch.calc_importance_fused       # its own switch
    finally:
        gsr_autopatch.remove()


def test_a_class_without_the_method_is_skipped(autopatch):
    mod = _stand_in_module(with_method=False)
    autopatch._patch_merge_module(mod)
    assert not hasattr(mod.HTGaussianTrainer, "merge_two_3DGS") and not autopatch._patched_merge_classes
    autopatch._patch_merge_module(types.ModuleType("trainer.ht3dgs_trainer"))          # no class at all


def test_the_shipped_default_is_documented():
    """ON or OFF is decided by the measurement in profiles/trainer_merge.txt; the module docstring and the profile name the same default."""
    import gsr_autopatch
    assert gsr_autopatch._MERGE_DEFAULT in ("0", "1")
    word = "ON" if gsr_autopatch._MERGE_DEFAULT == "1" else "OFF"
    assert f"GSR_AUTOPATCH_MERGE: ships {word}" in gsr_autopatch.__doc__
    with open(os.path.join(C.HERE, "..", "profiles", "trainer_merge.txt")) as f:
        assert f"GSR_AUTOPATCH_MERGE: ships {word}" in f.read()


# ---- fallbacks: the original runs, and nothing was loaded, scored or changed first -------------------------------------------------------------
class _Recorder:
    """A trainer class whose original `merge_two_3DGS` records its call and what it finds; its `load_viewpoint_cam` and `calc_importance`
    count their calls."""

    def __init__(self, autopatch):
        self.calls, self.scored = [], []
        rec = self

        def merge_two_3DGS(t, dst, src, T, frames_dst=None, frames_src=None):
            rec.calls.append((rec.fingerprint(dst, src), len(t.cam_calls), len(rec.scored), T, frames_dst, frames_src))

        def calc_importance(gs_render, cameras, pipe):
            rec.scored.append(gs_render)
            return torch.zeros(gs_render.gaussians._xyz.shape[0], 48)
        cls = type("HTGaussianTrainer", (refstub.StubMergeTrainer,), {"__module__": refstub.__name__, "merge_two_3DGS": merge_two_3DGS,
                                                                      "calc_importance": staticmethod(calc_importance)})
        autopatch._patch_merge_module(types.SimpleNamespace(HTGaussianTrainer=cls))
        assert cls.merge_two_3DGS is autopatch.merge_two_3DGS_fused
        self.cls = cls

    @staticmethod
    def fingerprint(dst, src):
        out = []
        for r in (dst, src):
            m = getattr(r, "gaussians", None)
            ts = [getattr(m, k, None) for k in C.RAW + C.STATS]
            out.append(([(id(t), getattr(t, "_version", None)) for t in ts],
                        [id(g["params"][0]) for g in getattr(getattr(m, "optimizer", None), "param_groups", ())]))
        return out

    def expect_fallback(self, dst, src, T, ratio=0.5, what=""):
        t = self.cls(prune_ratio=ratio)
        before = self.fingerprint(dst, src)
        self.calls.clear()
        self.scored.clear()
        t.merge_two_3DGS(dst, src, T, [0, 1], [2])
        assert len(self.calls) == 1, (what, self.calls)
        seen, loads, scored, T_seen, fa, fb = self.calls[0]
        assert seen == before and loads == 0 and scored == 0 and T_seen is T and fa == [0, 1] and fb == [2], what
        assert self.fingerprint(dst, src) == before and not t.cam_calls and not self.scored and not t.logger.lines, what


def _swap_param(m, attr, tensor):
    p = torch.nn.Parameter(tensor)
    name = dict((a, n) for n, a in C.GROUPS)[attr]
    next(g for g in m.optimizer.param_groups if g["name"] == name)["params"][0] = p
    setattr(m, attr, p)


def _wider_rest(m):
    n = m._xyz.shape[0]
    _swap_param(m, "_features_rest", torch.zeros(n, 8, 3))
    m.optimizer.state.pop(m._features_rest, None)


# what breaks a model, and on which side it matters: the destination needs the resize patch's whole layout, the source its six tensors
BROKEN = {
    "pose group beside rotation": (lambda m: m.optimizer.param_groups.append({"params": [torch.nn.Parameter(torch.zeros(1, 6))], "lr": 0.001, "name": "R"}), "dst"),
    "five groups": (lambda m: m.optimizer.param_groups.pop(), "dst"),
    "a group's parameter is not the model's": (lambda m: setattr(m, "_opacity", torch.nn.Parameter(m._opacity.detach().clone())), "dst"),
    "statistics unlike N": (lambda m: setattr(m, "max_radii2D", m.max_radii2D[:-1].clone()), "dst"),
    "a moment missing": (lambda m: m.optimizer.state[m._scaling].pop("exp_avg_sq"), "dst"),
    "no optimizer": (lambda m: setattr(m, "optimizer", None), "dst"),
    "float64 parameter": (lambda m: _swap_param(m, "_opacity", m._opacity.detach().double()), "both"),
    "strided parameter": (lambda m: _swap_param(m, "_rotation", torch.randn(4, m._xyz.shape[0]).t()), "both"),
    "rows unlike N": (lambda m: _swap_param(m, "_features_dc", m._features_dc.detach()[:-1].clone()), "both"),
    "a tensor missing": (lambda m: setattr(m, "_scaling", None), "both"),
    "another number of coefficients": (_wider_rest, "both"),
}


@pytest.mark.parametrize("broken", sorted(BROKEN))
def test_every_unexpected_layout_runs_the_original_untouched(seam, autopatch, broken):
    rec = _Recorder(autopatch)
    fn, sides = BROKEN[broken]
    for side in ("dst", "src"):
        dst = C.RZ.build(refstub.StubSurgeryModel, C.make_state(40, 16, True), "adam")
        src = C.RZ.build(refstub.StubSurgeryModel, C.make_state(30, 16, True, seed=1), "adam")
        fn(dst if side == "dst" else src)
        if side == "src" and sides == "dst":
            # the source's optimizer and statistics are not needed: this merge is served
            t = rec.cls(prune_ratio=0.5)
            rec.calls.clear()
            t.merge_two_3DGS(C.render_of(dst), C.render_of(src), torch.eye(4), [0], [1])
            assert not rec.calls and dst._xyz.shape[0] == 20 + 15, broken
            continue
        rec.expect_fallback(C.render_of(dst), C.render_of(src), torch.eye(4), what=f"{broken} ({side})")
    assert not seam.selects or sides == "dst"


def test_the_other_fallbacks_run_the_original_untouched(seam, autopatch, monkeypatch):
    rec = _Recorder(autopatch)
    build = lambda n, seed=0, coeffs=16, opt="fused": C.RZ.build(refstub.StubSurgeryModel, C.make_state(n, coeffs, True, seed=seed), opt)
    dst, src, eye = C.render_of(build(40)), C.render_of(build(30, 1)), torch.eye(4)
    # the transform: a float32 [4,4] tensor on the models' device
    for bad in (eye.double(), eye[:3], eye[None], eye.numpy(), eye.tolist(), None, torch.eye(4, dtype=torch.float16)):
        rec.expect_fallback(dst, src, bad, what="transform")
    # prune_ratio: a number in [0, 1]
    for bad in (-0.1, 1.5, float("nan"), None, "0.5", torch.tensor(0.5)):
        rec.expect_fallback(dst, src, eye, ratio=bad, what=f"ratio {bad!r}")
    # fewer than two rows on either side; no rows at all
    for n_dst, n_src in ((1, 30), (40, 1)):
        rec.expect_fallback(C.render_of(build(n_dst)), C.render_of(build(n_src, 1)), eye, what="one row")
    # models that differ in their trailing shapes (16 against 1 stored coefficients)
    rec.expect_fallback(dst, C.render_of(build(30, 1, coeffs=1)), eye, what="coefficients")
    # one model merged into itself; render objects without a model
    rec.expect_fallback(dst, dst, eye, what="the same model twice")
    rec.expect_fallback(types.SimpleNamespace(), src, eye, what="no destination model")
    # a CPU tensor anywhere (the rule itself: _REQUIRE_CUDA as shipped)
    monkeypatch.setattr(autopatch, "_REQUIRE_CUDA", True)
    rec.expect_fallback(dst, src, eye, what="CPU tensors")
    monkeypatch.setattr(autopatch, "_REQUIRE_CUDA", False)
    # the switch, read at the call as well
    monkeypatch.setenv("GSR_AUTOPATCH_MERGE", "0")
    rec.expect_fallback(dst, src, eye, what="switch")
    monkeypatch.setenv("GSR_AUTOPATCH_MERGE", "1")
    assert not seam.selects and seam.plans == 0
    # the resize patch's switch is not this patch's
    monkeypatch.setenv("GSR_AUTOPATCH_RESIZE", "0")
    t = rec.cls(prune_ratio=0.5)
    t.merge_two_3DGS(dst, src, eye, [0], [1])
    assert seam.selects == [(40, 48, 20), (30, 48, 15)] and seam.plans == 2 and len(seam.applies) == 1 and not rec.calls[1:]


def test_a_direct_call_without_an_original_is_an_error(seam, autopatch):
    t = refstub.StubMergeTrainer()
    with pytest.raises(RuntimeError, match="original HTGaussianTrainer.merge_two_3DGS"):
        autopatch.merge_two_3DGS_fused(t, types.SimpleNamespace(), types.SimpleNamespace(), torch.eye(4), [0], [1])


# ---- an importance the kernels do not take: the reference's own tail, on that importance -------------------------------------------------------
WRONG = {
    "float64": lambda s: s.double(),
    "three dimensions": lambda s: s.reshape(s.shape[0], -1, 3),
    "one dimension": lambda s: s.amax(-1),
    "wider than the selection takes": lambda s: torch.cat([s, s * 0.5], dim=1),
}


@pytest.mark.parametrize("wrong", sorted(WRONG))
@pytest.mark.parametrize("side", ["dst", "src"])
def test_a_wrong_importance_finishes_with_the_references_tail(seam, autopatch, wrong, side):
    n_dst, n_src, T = 41, 40, C.transform("rigid")
    ds, ss = C.make_state(n_dst, 16, True), C.make_state(n_src, 16, True, seed=1)
    sd, sr = C.distinct_scores(n_dst, 16), C.distinct_scores(n_src, 16, seed=1)
    if wrong == "wider than the selection takes":
        assert WRONG[wrong](sd).shape[1] > seam.L.GSR_SELECT_MAX_COLUMNS
    bad_d, bad_s = (WRONG[wrong](sd), sr) if side == "dst" else (sd, WRONG[wrong](sr))
    if wrong in ("one dimension", "three dimensions"):
        # `amax(-1)` of a vector is a scalar without a `shape[0]`, and of [N,16,3] a matrix whose `topk` cannot give N / 2 of 16 columns: the
        # reference's statements fail on them, in the stand-in and in the tail alike -- after both scores, before anything was changed
        for cls in (C.trainer_class(autopatch), C.trainer_class()):
            with pytest.raises((IndexError, RuntimeError)):
                C.merge(cls, ds, ss, "adam", bad_d, bad_s, T, 0.5)
        assert not seam.selects and seam.plans == 0
        return
    ta, a, src_a, before, calls = C.merge(C.trainer_class(autopatch), ds, ss, "adam", bad_d, bad_s, T, 0.5)
    tb, b, _, _, _ = C.merge(C.trainer_class(), ds, ss, "adam", bad_d, bad_s, T, 0.5)
    assert not seam.selects and seam.plans == 0 and not seam.applies         # no kernel call ...
    assert len(calls) == 2                                                   # ... and no second importance
    C.RZ.assert_installed(a, before)
    C.RZ.assert_same_model(a, b, wrong)
    assert ta.logger.lines == tb.logger.lines and len(ta.cam_calls) == 4


# ---- flag and count derivation and install logic against the unpatched stand-in ---------------------------------------------------------------
@pytest.mark.parametrize("optimizer", ["adam", "fused"])
@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no-state"])
@pytest.mark.parametrize("n_dst,n_src,coeffs", [(2, 2, 16), (65, 40, 16), (33, 200, 1)])
def test_patched_merge_equals_the_unpatched_stand_in(seam, autopatch, n_dst, n_src, coeffs, moments, optimizer):
    ds, ss = C.make_state(n_dst, coeffs, moments), C.make_state(n_src, coeffs, moments, seed=1)
    sd, sr = C.distinct_scores(n_dst, coeffs), C.distinct_scores(n_src, coeffs, seed=1)
    for ratio in (0.0, 0.25, 0.5, 0.999, 1.0):
        for kind in ("identity", "rigid", "projective"):
            T = C.transform(kind)
            seam.selects, seam.plans, seam.waits, seam.applies = [], 0, 0, []
            ta, a, src_a, before, calls_a = C.merge(C.trainer_class(autopatch), ds, ss, optimizer, sd, sr, T, ratio)
            tb, b, _, _, calls_b = C.merge(C.trainer_class(), ds, ss, optimizer, sd, sr, T, ratio)
            what = f"{n_dst}+{n_src} ratio {ratio} {kind}"
            k_dst, k_src = int(n_dst * ratio), int(n_src * ratio)
            C.RZ.assert_installed(a, before)
            C.RZ.assert_installed(b)
            C.RZ.assert_same_model(a, b, what)
            assert a._xyz.shape[0] == n_dst - k_dst + n_src - k_src, what
            C.assert_arm_ran(ta, n_dst, n_src, a._xyz.shape[0], calls_a)
            C.assert_arm_ran(tb, n_dst, n_src, a._xyz.shape[0], calls_b)
            assert seam.selects == [(n_dst, 3 * coeffs, k_dst), (n_src, 3 * coeffs, k_src)], what
            assert seam.plans == 2 and seam.waits <= 1 and len(seam.applies) == 1, what
            assert seam.applies[0] == ([MC.PARAM, MC.MOMENT, MC.MOMENT] * 6 if moments else [MC.PARAM] * 6), what
            # the statistics are fresh zeros, the step counts stay
            assert not a.xyz_gradient_accum.any() and not a.denom.any() and not a.max_radii2D.any()
            if moments:
                assert all(float(a.optimizer.state[getattr(a, k)]["step"]) == 3 for k in C.RAW)


def test_the_source_model_is_not_written(seam, autopatch):
    """Not its tensors, its optimizer, its statistics, nor the .grad an importance call left on it."""
    ds, ss = C.make_state(50, 16, True), C.make_state(60, 16, True, seed=1)
    sd, sr = C.distinct_scores(50, 16), C.distinct_scores(60, 16, seed=1)
    cls = C.trainer_class(autopatch)
    dst = C.RZ.build(refstub.StubSurgeryModel, ds, "adam")
    src = C.RZ.build(refstub.StubSurgeryModel, ss, "fused")
    src._features_dc.grad, src._features_rest.grad = torch.ones_like(src._features_dc), torch.ones_like(src._features_rest)
    C.inject(cls, {id(dst): sd, id(src): sr})
    snap = C.snapshot(src)
    cls(prune_ratio=0.5).merge_two_3DGS(C.render_of(dst), C.render_of(src), C.transform("projective"), [0, 1], [2, 3])
    assert dst._xyz.shape[0] == 25 + 30
    C.assert_untouched(src, snap, "source")


def test_calc_importance_is_looked_up_on_the_class_at_the_call(seam, autopatch):
    """A `calc_importance` installed on the class AFTER the patch (a user's own, or another patch) is the one the merge uses."""
    ds, ss = C.make_state(20, 16, False), C.make_state(20, 16, False, seed=1)
    cls = C.trainer_class(autopatch)
    first = C.inject(cls, {})
    dst, src = (C.RZ.build(refstub.StubSurgeryModel, s, "adam") for s in (ds, ss))
    second = C.inject(cls, {id(dst): C.distinct_scores(20, 16), id(src): C.distinct_scores(20, 16, seed=1)})
    cls(prune_ratio=0.5).merge_two_3DGS(C.render_of(dst), C.render_of(src), torch.eye(4), [0], [1])
    assert not first and len(second) == 2 and dst._xyz.shape[0] == 20


# ---- against the reference's own run -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
@pytest.mark.parametrize("arm", ["patched", "stand-in"])
def test_both_arms_reproduce_the_references_run(seam, autopatch, arm, case):
    """tests/golden/trainer_merge.npz is what the reference's own merge_two_3DGS did on these inputs (distinct scores): the patched method
    AND the stand-in it is compared with everywhere else both land on it, every tensor with `torch.equal`."""
    d = C.golden()
    ds, ss, sd, sr, T, ratio = C.golden_case(d, case)
    cls = C.trainer_class(autopatch if arm == "patched" else None)
    t, m, src, before, _ = C.merge(cls, ds, ss, "adam", sd, sr, T, ratio)
    C.RZ.assert_installed(m, before)
    C.assert_matches_golden(m, d, case)
    assert t.logger.lines == [str(s) for s in d[case + "_log"]]
    assert (seam.plans > 0) == (arm == "patched")


# ---- the tie rule ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["zeros_30", "zeros_99", "all_equal", "nan_rows", "inf", "signed_zeros"])
def test_ties_at_the_threshold_go_by_row_number(seam, autopatch, pattern):
    """Among rows whose score equals the k-th smallest the lowest row numbers go: the merged model is the stand-in's with its selection
    replaced by `np.argsort(key, kind="stable")[:k]`; the number of rows dropped is the reference's, every row strictly below the threshold
    is dropped, and the tied rows that stay are the highest-numbered."""
    n_dst, n_src, coeffs, ratio = 120, 90, 16, 0.5
    ds, ss = C.make_state(n_dst, coeffs, True), C.make_state(n_src, coeffs, True, seed=1)
    ds["raw"]["_opacity"] = torch.arange(n_dst, dtype=torch.float32)[:, None]                   # the raw opacity of a row is its row number
    rng = np.random.default_rng(5)
    raw_d, raw_s = MC.score_patterns(n_dst)[pattern][0], MC.score_patterns(n_src, seed=1)[pattern][0]
    sd, sr = (torch.from_numpy(MC.spread(s, 3 * coeffs, rng)) for s in (raw_d, raw_s))
    T = C.transform("rigid")
    _, a, _, before, _ = C.merge(C.trainer_class(autopatch), ds, ss, "adam", sd, sr, T, ratio)
    _, b, _, _, _ = C.merge(C.trainer_class(base=C.OracleSelection), ds, ss, "adam", sd, sr, T, ratio)
    _, c, _, _, _ = C.merge(C.trainer_class(), ds, ss, "adam", sd, sr, T, ratio)              # topk's own choice among the ties
    C.RZ.assert_installed(a, before)
    C.RZ.assert_same_model(a, b, pattern)
    assert a._xyz.shape == c._xyz.shape                                                         # the same number of rows dropped
    key, k = MC.keys_of(sd.numpy()), int(n_dst * ratio)
    came = a._opacity.detach()[:n_dst - k, 0].long().numpy()
    assert np.all(np.diff(came) > 0)                                                            # kept rows in their own order
    kept = np.zeros(n_dst, dtype=bool)
    kept[came] = True
    threshold = np.sort(key, kind="stable")[k - 1]
    assert not kept[key < threshold].any() and kept[key > threshold].all()
    tied = np.flatnonzero(key == threshold)
    gone = tied[~kept[tied]]
    assert np.array_equal(gone, tied[:gone.size])                                               # the lowest-numbered of the tied rows went
