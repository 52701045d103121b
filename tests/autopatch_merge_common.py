"""What the tests of gsr_autopatch's `merge_two_3DGS` share: model states and score patterns, the patched and the unpatched arm over
`refstub.StubMergeTrainer` / `refstub.StubSurgeryModel`, the comparison of two merged models, a stand-in for merge.py and resize.py built on
tests/merge_common.py's numpy oracles (the CPU seam), the stand-in with its selection replaced by that oracle (the arm the tie rule is held
against), and the reading of tests/golden/trainer_merge.npz (the reference's own run)."""
import importlib
import os
import types

import numpy as np
import torch

import autopatch_resize_common as RZ
import merge_common as MC

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "trainer_merge.npz")
refstub = RZ.refstub

RAW, GROUPS, STATS = RZ.RAW, RZ.GROUPS, RZ.STATS
LOG = ("The number of 3D Gaussians in the first 3DGS before merging: {}", "The number of 3D Gaussians in the second 3DGS before merging: {}",
       "The number of 3D Gaussians in the merged 3DGS: {}")


def make_state(n, coeffs, moments, seed=0, device="cpu"):
    """One model state of the resize tests' "mixture" regime (non-zero statistics; twelve moments at step 3 when asked for)."""
    return RZ.make_state(n, coeffs, "mixture", moments, seed=seed, device=device)


def distinct_scores(n, coeffs, seed=0, device="cpu"):
    """[n, 3 coeffs] float32 whose row maxima are all different."""
    rng = np.random.default_rng(31 * seed + n + coeffs)
    top = ((rng.permutation(n) + 1) / np.float32(n + 1)).astype(np.float32)
    assert np.unique(top).size == n
    return torch.from_numpy(MC.spread(top, 3 * coeffs, rng)).to(device)


def transform(kind, device="cpu", seed=3):
    rng = np.random.default_rng(seed)
    T = np.eye(4)
    if kind != "identity":
        Q, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
        Q[:, 0] *= np.sign(np.linalg.det(Q))
        T[:3, :3], T[:3, 3] = Q, rng.uniform(-1, 1, 3)
    if kind == "projective":
        T[:3, :3] *= 1.25
        T[3] = [0.01, -0.02, 0.015, 1.1]
    return torch.from_numpy(T.astype(np.float32)).to(device)


# ---- the two arms ------------------------------------------------------------------------------------------------------------------------------
def trainer_class(autopatch=None, base=None, name="HTGaussianTrainer"):
    """A class that stands for `trainer.ht3dgs_trainer.HTGaussianTrainer`: StubMergeTrainer's methods are its originals; with `autopatch`,
    gsr_autopatch's own installer has replaced `merge_two_3DGS` (`autopatch.remove()` puts it back)."""
    base = refstub.StubMergeTrainer if base is None else base
    cls = type(name, (base,), {"__module__": refstub.__name__, "merge_two_3DGS": base.merge_two_3DGS, "calc_importance": staticmethod(base.calc_importance)})
    if autopatch is not None:
        autopatch._patch_merge_module(types.SimpleNamespace(HTGaussianTrainer=cls))
        assert cls.merge_two_3DGS is autopatch.merge_two_3DGS_fused
    return cls


class OracleSelection(refstub.StubMergeTrainer):
    """The stand-in with its selection (row maximum, `topk`, zero fill, indexed store) replaced by tests/merge_common.py's numpy oracle,
    `np.argsort(key, kind="stable")[:k]`: everything else is the stand-in's own statement sequence."""

    def _lowest_mask(self, gaussians, importance):
        v = importance.detach().cpu().numpy()
        drop = MC.select_oracle(v, int(v.shape[0] * self.pipe_cfg.prune_ratio))["drop"]
        return torch.from_numpy(drop).to(importance.device)[:, None]


def inject(cls, scores):
    """`cls.calc_importance` hands out `scores[id(model)]` (a clone) and counts its calls."""
    calls = []

    def calc_importance(gs_render, cameras, pipe):
        calls.append((gs_render, list(cameras)))
        return scores[id(gs_render.gaussians)].clone()
    cls.calc_importance = staticmethod(calc_importance)
    return calls


def render_of(model):
    return types.SimpleNamespace(gaussians=model, bg_color=torch.zeros(3, device=model._xyz.device))


def merge(cls, dst_state, src_state, optimizer, scores_dst, scores_src, T, ratio, src_optimizer=None):
    """Two models over clones of the states, merged by a trainer of class `cls` with the given scores injected; -> (trainer, dst, src,
    the destination's parameters before the call (kept alive, so that their identities stay taken), calc_importance's calls)."""
    dst = RZ.build(refstub.StubSurgeryModel, dst_state, optimizer)
    src = RZ.build(refstub.StubSurgeryModel, src_state, src_optimizer or optimizer)
    calls = inject(cls, {id(dst): scores_dst, id(src): scores_src})            # (on the class itself, where the merge looks it up; `cls` comes from trainer_class)
    t = cls(prune_ratio=ratio)
    before = [getattr(dst, k) for k in RAW]
    t.merge_two_3DGS(render_of(dst), render_of(src), T, [0, 1], [2, 3])
    return t, dst, src, before, calls


def snapshot(model):
    """Everything of a model that a merge must leave alone when the model is the source: identities, versions, values, gradients, state."""
    ts = [getattr(model, k) for k in RAW + STATS]
    return ([(id(t), t._version) for t in ts], [t.detach().clone() for t in ts], [getattr(model, k).grad for k in RAW],
            [(id(p), {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}) for p, st in model.optimizer.state.items()])


def assert_untouched(model, snap, what=""):
    now = snapshot(model)
    assert now[0] == snap[0], (what, "identity / version")
    assert all(torch.equal(a, b) for a, b in zip(now[1], snap[1])), (what, "values")
    assert all(a is b for a, b in zip(now[2], snap[2])), (what, ".grad")
    assert len(now[3]) == len(snap[3])
    for (pa, sa), (pb, sb) in zip(now[3], snap[3]):
        assert pa == pb and sa.keys() == sb.keys(), what
        assert all(torch.equal(sa[k], sb[k]) if torch.is_tensor(sa[k]) else sa[k] == sb[k] for k in sa), (what, "optimizer state")


def assert_arm_ran(t, n_dst, n_src, n_out, calls):
    """The visible protocol of a merge: three log lines with the reference's texts, four camera loads in order, two scores."""
    assert t.logger.lines == [LOG[0].format(n_dst), LOG[1].format(n_src), LOG[2].format(n_out)], t.logger.lines
    assert [(c[0], c[2]) for c in t.cam_calls] == [(0, True), (1, True), (2, True), (3, True)]
    assert all(torch.is_tensor(c[1]) and c[1].device.type == "cpu" and tuple(c[1].shape) == (4, 4) for c in t.cam_calls)
    assert len(calls) == 2 and len(calls[0][1]) == 2 and len(calls[1][1]) == 2


# ---- the CPU seam: merge.py's and resize.py's calls on the numpy oracles of tests/merge_common.py ----------------------------------------------
class OracleMerge:
    """Stands for the modules `merge` (gsr_autopatch._merge) and `resize` (gsr_autopatch._resize): the selection is the oracle's, a plan is
    the keep mask, the apply is numpy indexing."""
    PARAM, MOMENT = MC.PARAM, MC.MOMENT
    L = types.SimpleNamespace(GSR_SELECT_MAX_COLUMNS=64)
    MAX_TENSORS = 18

    def __init__(self):
        self.selects, self.plans, self.waits, self.applies = [], 0, 0, []

    def select_smallest(self, values, k):
        assert values.dtype == torch.float32 and values.dim() == 2 and values.is_contiguous() and 0 <= k <= values.shape[0]
        sel = MC.select_oracle(values.numpy(), int(k))
        self.selects.append((int(values.shape[0]), int(values.shape[1]), int(k)))
        return torch.from_numpy(sel["drop"]), torch.from_numpy(sel["keep_flags"]), torch.tensor(sel["meta"], dtype=torch.int64)

    def resize_plan(self, flags):
        assert flags.dtype == torch.uint8 and flags.dim() == 1 and flags.is_contiguous()
        self.plans += 1
        keep = flags.numpy() == MC.KEEP
        return keep, torch.tensor([int(keep.sum()), 0, 0, 0, 0, 0, 0, 0], dtype=torch.int64)

    def read_counts_pair(self, meta_a, meta_b):
        self.waits += 1
        return [int(meta_a[0]), int(meta_a[4]), int(meta_b[0]), int(meta_b[4])]

    def merge_apply(self, plan_a, meta, n_a, kept_a, plan_b, n_b, kept_b, src_a, src_b, kinds=None, check=False):
        kinds = [self.PARAM] * len(src_a) if kinds is None else list(kinds)
        assert len(src_a) == len(src_b) == len(kinds) <= self.MAX_TENSORS
        assert plan_a.shape == (n_a,) and plan_b.shape == (n_b,) and kept_a == int(plan_a.sum()) and kept_b == int(plan_b.sum())
        assert all(t.shape[0] == n_a and t.is_contiguous() and t.dtype == torch.float32 and not t.requires_grad for t in src_a)
        assert all((b is None) == (k == self.MOMENT) for b, k in zip(src_b, kinds))
        assert all(b is None or (b.shape[0] == n_b and b.shape[1:] == a.shape[1:] and b.is_contiguous() and not b.requires_grad) for a, b in zip(src_a, src_b))
        self.applies.append(kinds)
        return [torch.from_numpy(MC.merged_oracle(a.numpy(), plan_a, None if b is None else b.numpy(), plan_b, k)) for a, b, k in zip(src_a, src_b, kinds)]


# ---- the reference's own run: tests/golden/trainer_merge.npz -----------------------------------------------------------------------------------
def golden():
    return np.load(GOLDEN)


def golden_case(d, case, device="cpu"):
    """-> (dst state, src state, dst scores, src scores, transform, ratio) of one recorded case."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    out = []
    for side in ("dst", "src"):
        pre = f"{case}_{side}_"
        state = {"raw": {k: t(d[pre + "in" + k]) for k in RAW}, "stats": {k: t(d[pre + "in_" + k]) for k in STATS}, "moments": None, "step": 0,
                 "percent_dense": 0.01}
        if bool(d[case + "_state"]):
            state["moments"] = {k: (t(d[pre + "in_exp_avg" + k]), t(d[pre + "in_exp_avg_sq" + k])) for k in RAW}
            state["step"] = int(d[pre + "in_step_xyz"])
        out.append(state)
    return (out[0], out[1], t(d[case + "_dst_score"]), t(d[case + "_src_score"]), t(d[case + "_transform"]), float(d[case + "_prune_ratio"]))


def moved_points_bar(d, case):
    """How far the moved points of a DEVICE run may lie from the recorded ones (the CPU's): per component, q = (sum of four products) / w
    with w a sum of four products.  A float32 dot product of four terms, in any order and with or without fused multiply-adds, is within
    4 * 2^-24 of its exact value relative to the sum S of the terms' magnitudes; the division adds 2^-24 of the quotient.  Two such
    evaluations (the recorded one and the device's) differ by at most twice that: 2 * 2^-24 * (4 S_num / |w| + 4 |q| S_w / |w| + |q|), which
    3 * 2^-23 * (S_num + |q| S_w) / |w| covers since |q| |w| <= S_num; the bar is that with every term in float64 from the recorded inputs."""
    x = np.concatenate([d[case + "_src_in_xyz"].astype(np.float64), np.ones((d[case + "_src_in_xyz"].shape[0], 1))], axis=1)
    T = d[case + "_transform"].astype(np.float64)
    s_num, s_w = np.abs(x) @ np.abs(T[:3]).T, np.abs(x) @ np.abs(T[3])
    w = x @ T[3]
    q = (x @ T[:3].T) / w[:, None]
    return 3 * 2.0 ** -23 * (s_num + np.abs(q) * s_w[:, None]) / np.abs(w)[:, None]


def assert_matches_golden(m, d, case, exact_points=True):
    """The destination after the case's merge against what the reference's model was after it: every tensor, moment, step and statistic bit
    for bit; with exact_points=False (a device run against the CPU's record) the appended rows of `_xyz` within `moved_points_bar`."""
    pre = case + "_"
    ratio = float(d[pre + "prune_ratio"])
    n_dst, n_src = d[pre + "dst_in_xyz"].shape[0], d[pre + "src_in_xyz"].shape[0]
    kept_dst, kept_src = n_dst - int(n_dst * ratio), n_src - int(n_src * ratio)
    for k in RAW:
        got, ref = getattr(m, k).detach().cpu().numpy(), d[pre + "out" + k]
        assert got.shape == ref.shape and ref.shape[0] == kept_dst + kept_src, (case, k, got.shape, ref.shape)
        rows = slice(0, kept_dst) if (k == "_xyz" and not exact_points) else slice(None)
        np.testing.assert_array_equal(got[rows], ref[rows], err_msg=f"{case} {k}")
        st = m.optimizer.state.get(getattr(m, k))
        assert (st is not None) == bool(d[pre + "state"]), (case, k)
        if st is not None:
            assert float(st["step"]) == float(d[pre + "out_step" + k])
            np.testing.assert_array_equal(st["exp_avg"].cpu().numpy(), d[pre + "out_exp_avg" + k], err_msg=f"{case} exp_avg {k}")
            np.testing.assert_array_equal(st["exp_avg_sq"].cpu().numpy(), d[pre + "out_exp_avg_sq" + k], err_msg=f"{case} exp_avg_sq {k}")
    for k in STATS:
        np.testing.assert_array_equal(getattr(m, k).cpu().numpy(), d[pre + "out_" + k], err_msg=f"{case} {k}")
    if not exact_points:
        keep = MC.select_oracle(d[pre + "src_score"], n_src - kept_src)["keep_flags"] == MC.KEEP
        err = np.abs(m._xyz.detach().cpu().numpy()[kept_dst:].astype(np.float64) - d[pre + "out_xyz"][kept_dst:])
        bar = moved_points_bar(d, case)[keep]
        print(f"{case}: moved points off the CPU's record by at most {float((err / bar).max()):.3f} of the bar")
        assert np.all(err <= bar), (case, "moved points", float((err / bar).max()))
