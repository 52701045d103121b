#!/usr/bin/env python3
"""Resizing the models of a batch on the batched resize kernels, timed in ONE process per case with alternating arms.

(a) One densification of a batch of B = 8 models -- 5 % of every model's rows cloned, 5 % split, 5 % under the opacity floor:
      batched   BatchedDensifier.densify_and_prune: one plan over the store, one read of `meta`, the children drawn model by model, one apply
      split     what a user of the batched store could do without it: take every model and its moments out of the store
                (GaussianParams.from_raw + slices of the optimizer state), run Densifier(route="kernel") on each alone, and rebuild the
                store with torch.cat and padding rows, tensor by tensor and moment by moment
    at 8 x 130 k Gaussians at SH degree 0 and at 8 x 200 k at degree 3 (sixteen coefficients stored in both).  Every sample starts from a fresh clone of the
    same state (six tensors, twelve non-zero moments, step 1) and the same generator seeds; building the clone is not timed.
(b) The leaf phase of `run_segments.py --local --segments 8 --densify --densify-route kernel` with and without `--leaf-batch 8`, as the
    sum of the "leaf" records' `ms` (the leaves of a batch share their batch's time in equal parts).

The arms alternate -- A, B, A, B, ... -- for `--rounds` rounds after a warm-up.  One sample is one call under a host clock that ends in a
device synchronise.  Per arm: the median, min - max, the spread of the arm against itself (the difference of the medians of its odd and
even rounds) and the number of host synchronisations torch warns about in one call (set_sync_debug_mode("warn")).  An arm wins only if the
difference of the medians exceeds the larger same-arm spread.

Without --case the cases run one after the other, each in a fresh child process under its own time limit; the first one that fails or
runs out of time ends the probe.

    python tools/batch_resize_probe.py > profiles/batch_resize.txt
"""
import argparse
import importlib
import os
import statistics
import subprocess
import sys
import time
import warnings

CASES = {"8x130k_deg0": (8, 130_000, 0), "8x200k_deg3": (8, 200_000, 3), "leaf_phase": None}
CASE_TIME_LIMIT = 420      # seconds per case


def driver(args):
    for name in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=CASE_TIME_LIMIT).returncode
        except subprocess.TimeoutExpired:
            print(f"batch_resize_probe: {name} did not finish in {CASE_TIME_LIMIT} s; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"batch_resize_probe: {name} ended with code {rc}; stopping", flush=True)
            return rc
    return 0


def arm_stats(x):
    return statistics.median(x), min(x), max(x), abs(statistics.median(x[0::2]) - statistics.median(x[1::2]))


def sync_warnings(torch, call):
    """The host synchronisations torch warns about during one call."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.cuda.set_sync_debug_mode("warn")          # (its own "prototype feature" warning is not a wait)
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            call()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() for w in rec)


def report(what, arms, t, waits, unit="ms per call"):
    st = {k: arm_stats(v) for k, v in t.items()}
    print(f"\n{what}   [{unit}, host clock around a device synchronise]")
    for k in arms:
        med, lo, hi, spread = st[k]
        print(f"  {k:8s} median {med:9.3f}   min {lo:9.3f}   max {hi:9.3f}   odd/even rounds' medians differ by {spread:.3f}   "
              f"host synchronisations warned about in one call: {waits[k]}")
    a, b = arms
    diff, spread = st[a][0] - st[b][0], max(st[a][3], st[b][3])
    verdict = "no difference beyond the spread" if abs(diff) <= spread else (f"{a} is FASTER" if diff < 0 else f"{a} is SLOWER")
    print(f"  {a} - {b} = {diff:+.3f}; same-arm spread {spread:.3f} -> {verdict}" + (f" ({st[b][0] / st[a][0]:.2f}x)" if diff < -spread else ""), flush=True)


def densify_case(name, rounds, warmup):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
    bt = importlib.import_module("3dgs_hierarchical_training_amd.batched")
    dm = importlib.import_module("3dgs_hierarchical_training_amd.densify")
    syn = importlib.import_module("3dgs_hierarchical_training_amd.synthetic")
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    nb, n, degree = CASES[name]
    rounds = max(20, rounds)
    dev = torch.device("cuda:0")
    names = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
    gen = torch.Generator().manual_seed(17)
    sc = syn.make_scene(n, 256, 256, sh_degree=degree, seed=11)          # (the same cloud in every model: the contents do not matter to the move)
    base = bt.BatchedGaussianParams([sc] * nb, dev)
    rows = base.num_points
    own = torch.zeros(rows, dtype=torch.bool)
    for b in range(nb):
        own[base.model_rows(b)] = True
    with torch.no_grad():
        base._opacity[((torch.rand(rows, generator=gen) < 0.05) & own).to(dev)] = -9.0          # sigmoid(-9) is under the floor of 0.005
    raw = {k: getattr(base, k).detach() for k in names}
    shape1 = lambda v: (-1,) + (1,) * (v.dim() - 1)
    moments = {k: ((torch.randn(v.shape, generator=gen) * own.reshape(shape1(v))).to(dev), (torch.rand(v.shape, generator=gen) * own.reshape(shape1(v))).to(dev))
               for k, v in raw.items()}
    hot = ((torch.rand(rows, 1, generator=gen) < 0.10) & own.unsqueeze(1)).float().to(dev)
    med = float(base.get_scaling.detach()[base.model_rows(0)].max(dim=1).values.median())
    first_block, counts, max_deg = list(base.first_block), list(base.counts), base.max_sh_degree
    cfg = dm.DensifyConfig(percent_dense=0.01)
    extent = med / 0.01
    seeds = list(range(5, 5 + nb))
    row_bytes = sum(v[0].numel() * 4 for v in raw.values()) * 3
    del base

    def fresh():
        p = bt.BatchedGaussianParams.__new__(bt.BatchedGaussianParams)
        p.max_sh_degree, p.active_sh_degree = max_deg, degree
        for k in names:
            setattr(p, k, raw[k].clone().requires_grad_(True))
        p._build_optimizer(1.0, "hip")
        p.first_block, p.counts = list(first_block), list(counts)
        for g in p.optimizer.param_groups:
            m, v = moments[p._GROUP_ATTR[g["name"]]]
            p.optimizer.state[g["params"][0]] = {"step": 1, "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        p._raw_pad_rows()
        return p

    def batched_arm(p):
        d = dm.BatchedDensifier(p, extent, cfg, seeds=seeds)
        d.xyz_gradient_accum, d.denom = hot.clone(), torch.ones_like(hot)
        return lambda: d.densify_and_prune(0.5, 0.005, None)

    def split_arm(p):
        stats = (hot.clone(), torch.ones_like(hot))

        def call():
            models = []
            for b in range(nb):
                r = p.model_rows(b)
                s = ts.GaussianParams.from_raw({k: getattr(p, k).detach()[r] for k in names}, dev, sh_degree=degree)
                for g, gb in zip(s.optimizer.param_groups, p.optimizer.param_groups):
                    st = p.optimizer.state[gb["params"][0]]
                    s.optimizer.state[g["params"][0]] = {"step": st["step"], "exp_avg": st["exp_avg"][r].clone(), "exp_avg_sq": st["exp_avg_sq"][r].clone()}
                d = dm.Densifier(s, extent, cfg, seed=seeds[b], route="kernel")
                d.xyz_gradient_accum, d.denom = stats[0][r].clone(), stats[1][r].clone()
                d.densify_and_prune(0.5, 0.005, None)
                models.append(s)
            pads = p._raw_pad_rows()
            new_counts = [s.num_points for s in models]
            fb = [0]
            for c in new_counts:
                fb.append(fb[-1] + max(1, (c + bt.BLOCK - 1) // bt.BLOCK))
            for gi, g in enumerate(p.optimizer.param_groups):
                attr = p._GROUP_ATTR[g["name"]]
                parts, m_parts, v_parts = [], [], []
                for b, s in enumerate(models):
                    t = s.optimizer.param_groups[gi]["params"][0]
                    st = s.optimizer.state[t]
                    k = bt.BLOCK * (fb[b + 1] - fb[b]) - new_counts[b]
                    zeros = torch.zeros((k,) + tuple(t.shape[1:]), device=dev)
                    parts += [t.detach(), pads[attr].expand((k,) + tuple(t.shape[1:]))]
                    m_parts += [st["exp_avg"], zeros]
                    v_parts += [st["exp_avg_sq"], zeros]
                p._install_group_tensor(g, torch.cat(parts, dim=0), (torch.cat(m_parts, dim=0), torch.cat(v_parts, dim=0)))
            p._screenspace_zero = None
            p.first_block, p.counts = fb, new_counts
        return call

    arms = {"batched": batched_arm, "split": split_arm}

    def sample(arm):
        p = fresh()
        call = arms[arm](p)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize(dev)
        return 1e3 * (time.perf_counter() - t0), p

    print(f"batch_resize_probe {name}: {torch.cuda.get_device_name(dev)}, B = {nb} models of {n} Gaussians ({rows} store rows), SH degree {degree} "
          f"({row_bytes} bytes of parameters and moments per row), rounds {rounds}, warm-up {warmup}, library version {L.load().gsr_version()}", flush=True)
    for _ in range(warmup):
        for arm in arms:
            sample(arm)
    _, pa = sample("batched")
    _, pb = sample("split")
    same = pa.counts == pb.counts and pa.first_block == pb.first_block and all(torch.equal(getattr(pa, k).detach(), getattr(pb, k).detach()) for k in names) \
        and all(torch.equal(pa.optimizer.state[getattr(pa, k)][m], pb.optimizer.state[getattr(pb, k)][m]) for k in names for m in ("exp_avg", "exp_avg_sq"))
    after = list(pa.counts)
    del pa, pb
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for arm in arms:                    # A, B, A, B, ...
            ms, p = sample(arm)
            del p
            t[arm].append(ms)
    waits = {}
    for arm in arms:
        p = fresh()
        call = arms[arm](p)
        torch.cuda.synchronize(dev)
        waits[arm] = sync_warnings(torch, call)
        del p
    report(f"densify_and_prune of the batch (5 % cloned, 5 % split, 5 % pruned): counts {counts[0]} x {nb} -> {after}; both arms leave the same store, "
           f"padding rows and moments included, bit for bit: {same}", ("batched", "split"), t, waits)
    print(flush=True)
    return 0


def leaf_case(rounds, warmup):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    rs = importlib.import_module("3dgs_hierarchical_training_amd.run_segments")
    segments = importlib.import_module("3dgs_hierarchical_training_amd.segments")
    sequence = importlib.import_module("3dgs_hierarchical_training_amd.sequence")
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    rounds = max(20, rounds)
    base = dict(densify=True, densify_route="kernel")
    cfgs = {"batch8": rs.HTConfig(leaf_batch=8, **base), "alone": rs.HTConfig(leaf_batch=0, **base)}
    c = cfgs["alone"]
    seq = sequence.FrameSequence(c.frames, c.gt_gaussians, c.width, c.height, dev, seed=c.seed)

    def leaf_phase(arm):
        recs = []
        runners = [rs.RankRunner(r, 8, segments.LocalTransport(8), seq, cfgs[arm], dev, log=recs.append) for r in range(8)]
        rs.train_leaves_local(runners, cfgs[arm])
        leaf = [r for r in recs if r["phase"] == "leaf"]
        assert len(leaf) == 8
        return sum(r["ms"] for r in leaf), sum(r["steps"] for r in leaf), [r["gaussians"] for r in sorted(leaf, key=lambda r: r["rank"])]

    print(f"batch_resize_probe leaf_phase: {torch.cuda.get_device_name(dev)}, run_segments --local --segments 8 --densify --densify-route kernel "
          f"({c.frames} frames at {c.width}x{c.height}, {c.leaf_gaussians} Gaussians per leaf, {c.leaf_iters_per_frame} steps per frame), leaf phase "
          f"only, rounds {rounds}, warm-up 1, library version {L.load().gsr_version()}", flush=True)
    for _ in range(1):          # (one warm-up round: a leaf phase is a thousand steps)
        for arm in cfgs:
            _, steps, sizes = leaf_phase(arm)
            print(f"  {arm}: {steps} steps over the 8 leaves, Gaussians per leaf at the end {sizes}", flush=True)
    t = {k: [] for k in cfgs}
    for _ in range(rounds):
        for arm in cfgs:
            t[arm].append(leaf_phase(arm)[0])
    waits = {arm: sync_warnings(torch, lambda arm=arm: leaf_phase(arm)) for arm in cfgs}
    report("the leaf phase: the sum of the eight \"leaf\" records' ms", ("batch8", "alone"), t, waits, unit="ms per leaf phase")
    print(flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", choices=tuple(CASES), default=None)
    args = ap.parse_args()
    if args.case is None:
        sys.exit(driver(args))
    sys.exit(leaf_case(args.rounds, args.warmup) if args.case == "leaf_phase" else densify_case(args.case, args.rounds, args.warmup))


if __name__ == "__main__":
    main()
