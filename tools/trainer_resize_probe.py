#!/usr/bin/env python3
"""The unmodified trainer's `densify_and_prune` / `prune_points`, unpatched and under gsr_autopatch, timed in ONE process per size with
alternating arms.

  unpatched  refstub.StubSurgeryModel: the reference's statement sequence -- boolean indexing and torch.cat tensor by tensor, three times over
  patched    the same class with gsr_autopatch's two methods installed: the same selections by the same torch statements, one flag byte per
             row, gsr_resize_plan, one read of `meta`, gsr_resize_apply

Per size (1 M / degree 3, 300 k / degree 3, 130 k / degree 0):
  densify_and_prune   about 5 % of the rows cloned, 5 % split, 5 % under the opacity floor; each arm WITH the trailing torch.cuda.empty_cache()
                      (the reference's behaviour; GSR_AUTOPATCH_EMPTY_CACHE=1) and WITHOUT it (=0; StubSurgeryModel.empty_cache = False)
  prune_points        a random half of the rows removed: the merge's case
  100 iterations      the trainer's iteration on the patched render, loss and deferred FusedAdam step, a densify_and_prune at iteration 50
  host waits          synchronisation warnings per call under torch.cuda.set_sync_debug_mode("warn"), per arm

Every sample starts from a fresh clone of the same state (six tensors, twelve non-zero moments, step 1) and the same seed; building the clone
is not timed.  After a warm-up the arms alternate for `--rounds` rounds (at least 20).  One sample is one call under a host clock that ends in
a device synchronise.  Per arm: the median, min - max and the spread of the arm against itself (the difference of the medians of its odd and
even rounds).

THE RULE for the shipped default of GSR_AUTOPATCH_RESIZE: ON if and only if, at all three sizes in this one run, the patched densify_and_prune
with empty_cache() is faster than the unpatched one with empty_cache() by more than the larger same-arm spread.  The last lines say so.

Without --case the sizes run one after the other, each in a fresh child process under its own time limit; the first one that fails or runs
out of time ends the probe.

    python tools/trainer_resize_probe.py > profiles/trainer_resize.txt
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
CASE_TIME_LIMIT = 400      # seconds per size
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
            print(f"trainer_resize_probe: {name} did not finish in {CASE_TIME_LIMIT} s; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"trainer_resize_probe: {name} ended with code {rc}; stopping", flush=True)
            return rc
    on = len(verdicts) == len(CASES) and all(v.endswith("FASTER") for v in verdicts)
    print("THE RULE: patched densify_and_prune faster than unpatched, empty_cache() in both, by more than the larger same-arm spread, at all three sizes:")
    for v in verdicts:
        print("  " + v)
    print(f"GSR_AUTOPATCH_RESIZE: ships {'ON' if on else 'OFF'} by this run", flush=True)
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
    os.environ["GSR_AUTOPATCH_RESIZE"] = "1"
    os.environ["GSR_AUTOPATCH_DEFERRED_MIN_N"] = "0"
    gsr_autopatch.apply()
    n, degree = CASES[name]
    rounds = max(20, rounds)
    dev = torch.device("cuda:0")
    names = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
    gen = torch.Generator().manual_seed(17)
    W = H = 256
    sc = syn.make_scene(n, W, H, sh_degree=degree, seed=11)
    base = ts.GaussianParams(sc, dev)
    with torch.no_grad():
        base._opacity[(torch.rand(n, generator=gen) < 0.05).to(dev)] = -9.0                  # sigmoid(-9) is under the floor of 0.005
    raw = {k: getattr(base, k).detach().clone() for k in names}
    moments = {k: (torch.randn(v.shape, generator=gen).to(dev), torch.rand(v.shape, generator=gen).to(dev)) for k, v in raw.items()}
    hot = (torch.rand(n, 1, generator=gen) < 0.10).float().to(dev)
    med = float(base.get_scaling.detach().max(dim=1).values.median())
    extent = med / 0.01                                                                      # half of the selected rows are "large"
    prune_mask = (torch.rand(n, generator=gen) < 0.5).to(dev)
    row_bytes = sum(v[0].numel() * 4 for v in raw.values()) * 3
    del base
    patched = type("HTGaussianModel", (refstub.StubSurgeryModel,), {"__module__": refstub.__name__, "prune_points": refstub.StubSurgeryModel.prune_points,
                                                                    "densify_and_prune": refstub.StubSurgeryModel.densify_and_prune})
    gsr_autopatch._patch_resize_module(types.SimpleNamespace(HTGaussianModel=patched))
    assert patched.densify_and_prune is gsr_autopatch.densify_and_prune_fused
    ARMS = {"unpatched": (refstub.StubSurgeryModel, True), "patched": (patched, True),
            "unpatched, no empty_cache": (refstub.StubSurgeryModel, False), "patched, no empty_cache": (patched, False)}

    def fresh(arm, with_moments=True):
        cls, empty_cache = ARMS[arm]
        os.environ["GSR_AUTOPATCH_EMPTY_CACHE"] = "1" if empty_cache else "0"
        m = cls(raw, optimizer="fused", percent_dense=0.01, active_sh_degree=degree)
        m.empty_cache = empty_cache
        if with_moments:
            for k in names:
                m.optimizer.state[getattr(m, k)] = {"step": 1, "exp_avg": moments[k][0].clone(), "exp_avg_sq": moments[k][1].clone()}
        m.xyz_gradient_accum, m.denom = hot.clone(), torch.ones_like(hot)
        torch.manual_seed(5)
        return m

    densify = lambda m: m.densify_and_prune(0.5, 0.005, extent, None)
    prune = lambda m: m.prune_points(prune_mask)

    def sample(arm, call):
        m = fresh(arm)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        with torch.no_grad():
            call(m)
        torch.cuda.synchronize(dev)
        return 1e3 * (time.perf_counter() - t0), m

    def same(a, b):
        return a._xyz.shape == b._xyz.shape and all(torch.equal(getattr(a, k).detach(), getattr(b, k).detach()) for k in names) and all(
            torch.equal(a.optimizer.state[getattr(a, k)][s], b.optimizer.state[getattr(b, k)][s]) for k in names for s in ("exp_avg", "exp_avg_sq"))

    def report(title, arms, call, pairs):
        for _ in range(warmup):
            for arm in arms:
                sample(arm, call)
        _, ma = sample(arms[0], call)
        _, mb = sample(arms[1], call)
        equal, n_after = same(ma, mb), mb._xyz.shape[0]
        del ma, mb
        t = {arm: [] for arm in arms}
        for _ in range(rounds):
            for arm in arms:                                     # A, B, (C, D,) A, B, ...
                ms, m = sample(arm, call)
                del m
                t[arm].append(ms)
        st = {k: arm_stats(v) for k, v in t.items()}
        print(f"\n{title}: N {n} -> {n_after}; both arms give the same tensors and moments bit for bit: {equal}   [ms per call, host clock around a device synchronise]")
        for k in arms:
            med_, lo, hi, spread = st[k]
            print(f"  {k:28s} median {med_:8.3f}   min {lo:8.3f}   max {hi:8.3f}   odd/even rounds' medians differ by {spread:.3f}")
        out = {}
        for a, b in pairs:
            diff, spread = st[b][0] - st[a][0], max(st[a][3], st[b][3])
            verdict = "no difference beyond the spread" if abs(diff) <= spread else ("FASTER" if diff < 0 else "SLOWER")
            print(f"  [{b}] - [{a}] = {diff:+.3f}; same-arm spread {spread:.3f} -> {verdict}" + (f" ({st[a][0] / st[b][0]:.2f}x)" if diff < -spread else ""), flush=True)
            out[(a, b)] = verdict
        return st, out

    props = torch.cuda.get_device_properties(dev)
    print(f"trainer_resize_probe {name}: {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs, torch {torch.__version__}), N = {n}, SH degree {degree} ({row_bytes} bytes of parameters and moments "
          f"per row), rounds {rounds}, warm-up {warmup}, library version {L.load().gsr_version()}", flush=True)
    st, verdicts = report("densify_and_prune (5 % cloned, 5 % split, 5 % pruned)", list(ARMS), densify,
                          [("unpatched", "patched"), ("unpatched, no empty_cache", "patched, no empty_cache")])
    print(f"  the trailing empty_cache() costs the unpatched arm {st['unpatched'][0] - st['unpatched, no empty_cache'][0]:+.3f} ms, "
          f"the patched arm {st['patched'][0] - st['patched, no empty_cache'][0]:+.3f} ms (plus the allocations the next iteration makes anew)")
    rule = verdicts[("unpatched", "patched")]
    report("prune_points (50 % removed)", ["unpatched", "patched"], prune, [("unpatched", "patched")])

    # ---- host waits per call ----------------------------------------------------------------------------------------------------------------
    def sync_warnings(arm, call):
        m = fresh(arm)
        torch.cuda.synchronize(dev)
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as seen:
                warnings.simplefilter("always")
                with torch.no_grad():
                    call(m)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        return sum("synchroniz" in str(w.message).lower() for w in seen)
    print("\nsynchronisation warnings per call (torch.cuda.set_sync_debug_mode('warn')):")
    for title, call, arms in (("densify_and_prune", densify, list(ARMS)), ("prune_points", prune, ["unpatched", "patched"])):
        print(f"  {title:18s} " + "   ".join(f"[{arm}] {sync_warnings(arm, call)}" for arm in arms), flush=True)

    # ---- 100 iterations of the trainer's sequence holding one densification -------------------------------------------------------------------
    gt = syn.target_image(W, H, seed=1).to(dev)
    cam = refstub.StubCamera.from_scene(sc, dev, original_image=gt)
    loss_cfg = types.SimpleNamespace(cfg=types.SimpleNamespace(lambda_dssim=0.2, lambda_depth=0.0))

    def hundred(arm):
        g = fresh(arm, with_moments=False)
        r = types.SimpleNamespace(gaussians=g, bg_color=torch.zeros(3, device=dev))
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for it in range(1, 101):
            pkg = gsr_autopatch.render_fused(r, cam)
            gsr_autopatch.loss_forward(loss_cfg, pkg["image"], gt)["loss"].backward()
            with torch.no_grad():
                vis, radii = pkg["visibility_filter"], pkg["radii"]
                g.max_radii2D[vis] = torch.max(g.max_radii2D[vis], radii[vis])
                gsr_autopatch.add_densification_stats_fused(g, pkg["viewspace_points"], vis)
                if it == 50:
                    g.xyz_gradient_accum, g.denom = hot.clone(), torch.ones_like(hot)      # (the selection of the calls above)
                    densify(g)
                g.optimizer.step()
                g.optimizer.zero_grad(set_to_none=True)
        torch.cuda.synchronize(dev)
        return 1e3 * (time.perf_counter() - t0), g._xyz.shape[0]
    arms = ["unpatched", "patched"]
    for arm in arms:
        hundred(arm)
    t = {arm: [] for arm in arms}
    for _ in range(4):
        for arm in arms:
            ms, n_after = hundred(arm)
            t[arm].append(ms)
    print(f"\n100 iterations of the trainer's sequence at {W} x {H}, densify_and_prune at iteration 50 (N {n} -> {n_after}), empty_cache() in both   [ms per 100 iterations, 4 alternating rounds]")
    for arm in arms:
        med_, lo, hi, spread = arm_stats(t[arm])
        print(f"  {arm:28s} median {med_:9.2f}   min {lo:9.2f}   max {hi:9.2f}   odd/even rounds' medians differ by {spread:.2f}")
    print(f"  [patched] - [unpatched] = {statistics.median(t['patched']) - statistics.median(t['unpatched']):+.2f} ms per 100 iterations")
    print(f"{RULE_TAG}{name}: patched densify_and_prune against unpatched, empty_cache() in both: {rule}\n", flush=True)
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
