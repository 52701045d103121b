#!/usr/bin/env python3
"""The unmodified trainer's `merge_two_3DGS`, unpatched and under gsr_autopatch, timed in ONE process per size with alternating arms.

  unpatched  refstub.StubMergeTrainer: the reference's statement sequence -- per model `amax`, `topk`, a zero fill and an indexed store;
             `prune_points` on the destination; the moved points; six boolean gathers; `densification_postfix` (six `torch.cat`, twelve
             moment `cat`s)
  patched    the same class with gsr_autopatch's `merge_two_3DGS_fused` installed: gsr_select_smallest per model, the same three statements
             for the moved points, two gsr_resize_plan, one gsr_merge_apply over 18 tensors, the install

Both arms run with every other patch installed: `prune_points` of the unpatched arm is the patched one (gsr_resize_apply), and the importance
of the second leg is `calc_importance_fused` in both.

Per size (two models of N rows each: 1 M / degree 3, 300 k / degree 3, 130 k / degree 0), `prune_ratio` 0.5, 30 % of the scores exactly 0:
  injected scores     the merge with prepared scores handed out by `calc_importance`: selection + transform + move + install
  with importance     the same merge with `calc_importance` over two 256 x 256 views per model
  host waits          synchronisation warnings per call under torch.cuda.set_sync_debug_mode("warn"), per arm, injected scores
  peak allocation     torch.cuda.max_memory_allocated over the call, above what was allocated when it began, injected scores

Every sample merges into a fresh clone of the same destination state (six tensors, twelve non-zero moments, step 1); the source model is
never written and is shared; building the clone is not timed.  After a warm-up the arms alternate for `--rounds` rounds (at least 20).  One
sample is one call under a host clock that ends in a device synchronise.  Per arm: the median, min - max and the spread of the arm against
itself (the difference of the medians of its odd and even rounds).

THE RULE for the shipped default of GSR_AUTOPATCH_MERGE, fixed before the run: ON if and only if, at all three sizes in this one run, the
patched merge with injected scores is faster than the unpatched one by more than the larger same-arm spread AND the merge with importance
is not slower beyond its spread.  The baseline is the stand-in arm of the same process, never an earlier run.  The last lines say so.

Without --case the sizes run one after the other, each in a fresh child process under its own time limit; the first one that fails or runs
out of time ends the probe.

    python tools/trainer_merge_probe.py > profiles/trainer_merge.txt
"""
import argparse
import importlib
import os
import statistics
import subprocess
import sys
import threading
import time
import types
import warnings

CASES = {"1M_deg3": (1_000_000, 3), "300k_deg3": (300_000, 3), "130k_deg0": (130_000, 0)}
CASE_TIME_LIMIT = 300      # seconds per size
RULE_TAG = "rule at "


def driver(args):
    verdicts = []
    for name in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
        proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
        timed_out = []
        watchdog = threading.Timer(CASE_TIME_LIMIT, lambda: (timed_out.append(1), proc.kill()))
        watchdog.start()
        try:
            for line in proc.stdout:
                print(line, end="", flush=True)
                if line.startswith(RULE_TAG):
                    verdicts.append(line.strip())
            rc = proc.wait()
        finally:
            watchdog.cancel()
        if timed_out:
            print(f"trainer_merge_probe: {name} did not finish in {CASE_TIME_LIMIT} s; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"trainer_merge_probe: {name} ended with code {rc}; stopping", flush=True)
            return rc
    on = len(verdicts) == len(CASES) and all(v.endswith("HOLDS") for v in verdicts)
    print("THE RULE: patched merge with injected scores faster than the unpatched stand-in by more than the larger same-arm spread, and the merge "
          "with importance not slower, at all three sizes:")
    for v in verdicts:
        print("  " + v)
    print(f"GSR_AUTOPATCH_MERGE: ships {'ON' if on else 'OFF'} by this run", flush=True)
    return 0


def arm_stats(x):
    return statistics.median(x), min(x), max(x), abs(statistics.median(x[0::2]) - statistics.median(x[1::2]))


def case(name, rounds, warmup):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gsr_autopatch
    refstub = importlib.import_module("3dgs_hierarchical_training_amd.refstub")
    syn = importlib.import_module("3dgs_hierarchical_training_amd.synthetic")
    ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    os.environ["GSR_AUTOPATCH_MERGE"] = "1"
    os.environ["GSR_AUTOPATCH_RESIZE"] = "1"
    os.environ["GSR_AUTOPATCH_IMPORTANCE"] = "1"
    gsr_autopatch.apply()
    n, degree = CASES[name]
    rounds = max(20, rounds)
    dev = torch.device("cuda:0")
    names = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
    gen = torch.Generator().manual_seed(17)
    W = H = 256
    ratio = 0.5

    # ---- the two model states, their scores, the cameras, the transform --------------------------------------------------------------------
    scenes = [syn.make_scene(n, W, H, sh_degree=degree, seed=11 + k) for k in range(2)]
    raws, moments, scores = [], [], []
    for sc in scenes:
        base = ts.GaussianParams(sc, dev)
        raw = {k: getattr(base, k).detach().clone() for k in names}
        del base
        raws.append(raw)
        moments.append({k: (torch.randn(v.shape, generator=gen).to(dev), torch.rand(v.shape, generator=gen).to(dev)) for k, v in raw.items()})
        s = torch.rand(n, 3 * raw["_features_dc"].shape[1] + 3 * raw["_features_rest"].shape[1], generator=gen)
        s[torch.rand(n, generator=gen) < 0.30] = 0.0                       # unseen Gaussians: a score of exactly 0
        scores.append(s.to(dev))
    row_bytes = sum(v[0].numel() * 4 for v in raws[0].values())
    g2 = torch.Generator().manual_seed(4)
    second = syn.make_camera(W, H, R=syn.random_rotation(g2, 0.1), t=0.05 * torch.randn(3, generator=g2))
    gt = syn.target_image(W, H, seed=1).to(dev)
    cams = {uid: refstub.StubCamera.from_scene(scenes[uid // 2] if uid % 2 == 0 else {**scenes[uid // 2], **second}, dev, original_image=gt, uid=uid)
            for uid in range(4)}
    T = torch.eye(4)
    T[:3, :3], T[:3, 3] = syn.random_rotation(g2, 0.2), 0.1 * torch.randn(3, generator=g2)
    T = T.to(dev)

    # ---- the model class with every other patch installed; the two trainer classes -----------------------------------------------------------
    model_cls = type("HTGaussianModel", (refstub.StubSurgeryModel,), {"__module__": refstub.__name__, "prune_points": refstub.StubSurgeryModel.prune_points,
                                                                      "densify_and_prune": refstub.StubSurgeryModel.densify_and_prune})
    gsr_autopatch._patch_resize_module(types.SimpleNamespace(HTGaussianModel=model_cls))
    assert model_cls.prune_points is gsr_autopatch.prune_points_fused

    def trainer_class(patched):
        cls = type("HTGaussianTrainer", (refstub.StubMergeTrainer,), {"__module__": refstub.__name__, "merge_two_3DGS": refstub.StubMergeTrainer.merge_two_3DGS,
                                                                      "calc_importance": staticmethod(gsr_autopatch.calc_importance_fused)})
        if patched:
            gsr_autopatch._patch_merge_module(types.SimpleNamespace(HTGaussianTrainer=cls))
            assert cls.merge_two_3DGS is gsr_autopatch.merge_two_3DGS_fused
        return cls
    CLS = {"unpatched": trainer_class(False), "patched": trainer_class(True)}
    ARMS = list(CLS)

    def model(k):
        m = model_cls(raws[k], optimizer="fused", percent_dense=0.01, active_sh_degree=degree)
        for a in names:
            m.optimizer.state[getattr(m, a)] = {"step": 1, "exp_avg": moments[k][a][0].clone(), "exp_avg_sq": moments[k][a][1].clone()}
        return m
    src = model(1)
    r_src = types.SimpleNamespace(gaussians=src, bg_color=torch.zeros(3, device=dev))
    by_model = {}

    def injected(gs_render, cameras, pipe):
        return by_model[id(gs_render.gaussians)]

    def sample(arm, with_importance, sync_count=False):
        cls = CLS[arm]
        cls.calc_importance = staticmethod(gsr_autopatch.calc_importance_fused if with_importance else injected)
        dst = model(0)
        by_model.clear()
        by_model.update({id(dst): scores[0], id(src): scores[1]})
        t = cls(prune_ratio=ratio, cameras=cams)
        r_dst = types.SimpleNamespace(gaussians=dst, bg_color=torch.zeros(3, device=dev))
        torch.cuda.synchronize(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        held = torch.cuda.memory_allocated(dev)
        if sync_count:
            torch.cuda.set_sync_debug_mode("warn")
            try:
                with warnings.catch_warnings(record=True) as seen:
                    warnings.simplefilter("always")
                    t.merge_two_3DGS(r_dst, r_src, T, [0, 1], [2, 3])
            finally:
                torch.cuda.set_sync_debug_mode("default")
            return sum("synchroniz" in str(w.message).lower() for w in seen), dst
        t0 = time.perf_counter()
        t.merge_two_3DGS(r_dst, r_src, T, [0, 1], [2, 3])
        torch.cuda.synchronize(dev)
        ms = 1e3 * (time.perf_counter() - t0)
        return ms, dst, (torch.cuda.max_memory_allocated(dev) - held) / 2 ** 20

    def same(a, b):
        return a._xyz.shape == b._xyz.shape and all(torch.equal(getattr(a, k).detach(), getattr(b, k).detach()) for k in names) and all(
            torch.equal(a.optimizer.state[getattr(a, k)][s], b.optimizer.state[getattr(b, k)][s]) for k in names for s in ("exp_avg", "exp_avg_sq"))

    def report(title, with_importance):
        for _ in range(warmup):
            for arm in ARMS:
                sample(arm, with_importance)
        _, ma, _ = sample(ARMS[0], with_importance)
        _, mb, _ = sample(ARMS[1], with_importance)
        shapes, n_after = ma._xyz.shape == mb._xyz.shape, mb._xyz.shape[0]
        equal = same(ma, mb) if shapes else False
        del ma, mb
        t, peak = {arm: [] for arm in ARMS}, {arm: 0.0 for arm in ARMS}
        for _ in range(rounds):
            for arm in ARMS:                                     # A, B, A, B, ...
                ms, m, mib = sample(arm, with_importance)
                del m
                t[arm].append(ms)
                peak[arm] = max(peak[arm], mib)
        st = {k: arm_stats(v) for k, v in t.items()}
        print(f"\n{title}: N {n} + {n} -> {n_after}; both arms keep the same number of rows: {shapes}; the same tensors and moments bit for bit "
              f"(the arms may drop different rows among the tied zero scores): {equal}   [ms per call, host clock around a device synchronise]")
        for k in ARMS:
            med_, lo, hi, spread = st[k]
            print(f"  {k:12s} median {med_:8.3f}   min {lo:8.3f}   max {hi:8.3f}   odd/even rounds' medians differ by {spread:.3f}   peak allocation {peak[k]:8.1f} MiB")
        diff, spread = st["patched"][0] - st["unpatched"][0], max(st["patched"][3], st["unpatched"][3])
        verdict = "no difference beyond the spread" if abs(diff) <= spread else ("FASTER" if diff < 0 else "SLOWER")
        print(f"  [patched] - [unpatched] = {diff:+.3f}; same-arm spread {spread:.3f} -> {verdict}" + (f" ({st['unpatched'][0] / st['patched'][0]:.2f}x)" if diff < -spread else ""), flush=True)
        return verdict

    props = torch.cuda.get_device_properties(dev)
    print(f"trainer_merge_probe {name}: {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs, torch {torch.__version__}), two models of N = {n}, SH degree {degree} "
          f"({row_bytes} bytes of parameters per row, twice that in moments), prune_ratio {ratio}, 30 % zero scores, rounds {rounds}, warm-up {warmup}, library version {L.load().gsr_version()}", flush=True)
    injected_verdict = report("merge_two_3DGS with injected scores (selection + transform + move + install)", False)
    print("\nsynchronisation warnings per call with injected scores (torch.cuda.set_sync_debug_mode('warn'); four of them are the `.cpu()` of the four "
          "poses the camera loads ask for, in both arms):")
    print("  " + "   ".join(f"[{arm}] {sample(arm, False, sync_count=True)[0]}" for arm in ARMS), flush=True)
    importance_verdict = report(f"merge_two_3DGS with calc_importance over two {W} x {H} views per model", True)
    holds = injected_verdict == "FASTER" and importance_verdict != "SLOWER"
    print(f"{RULE_TAG}{name}: injected scores {injected_verdict}, with importance {importance_verdict}: {'HOLDS' if holds else 'FAILS'}\n", flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", choices=tuple(CASES), default=None)
    args = ap.parse_args()
    sys.exit(driver(args) if args.case is None else case(args.case, args.rounds, args.warmup))


if __name__ == "__main__":
    main()
