#!/usr/bin/env python3
"""Resizing the model by the torch route and by the resize kernels, timed in ONE process per size with alternating arms.

  torch    Densifier(route="torch") / prune_points(route="torch"): boolean indexing and torch.cat, tensor by tensor
  kernel   Densifier(route="kernel") / prune_points(route="kernel"): gsr_resize_plan, one read of `meta`, gsr_resize_apply

Two calls per size:
  densify_and_prune   about 5 % of the rows cloned, 5 % split, 5 % under the opacity floor (the mixed selection of bench.py's warm_densify,
                      thinned out): `densify_and_prune(0.5, 0.005, None)` on statistics that select a tenth of the rows, half of them large
  prune_points        a random half of the rows removed: the merge's case

Every sample starts from a fresh clone of the same state (six tensors, twelve non-zero moments, step 1) and the same generator seed; building
the clone is not timed.  After a warm-up that includes the first randn / bmm, the arms alternate -- torch, kernel, torch, kernel, ... -- for
`--rounds` rounds.  One sample is one call under a host clock that ends in a device synchronise.  Per arm: the median, min - max, the spread
of the arm against itself (the difference of the medians of its odd and even rounds) and the peak allocation over the call beyond what was
allocated before it.  A route wins at a size only if the difference of the medians exceeds the larger same-arm spread.

Without --case the sizes run one after the other, each in a fresh child process under its own time limit; the first one that fails or
runs out of time ends the probe.

    python tools/resize_route_probe.py > profiles/resize_route.txt
"""
import argparse
import importlib
import os
import statistics
import subprocess
import sys
import time

CASES = {"1M_deg3": (1_000_000, 3), "300k_deg3": (300_000, 3), "130k_deg0": (130_000, 0)}
CASE_TIME_LIMIT = 420      # seconds per size


def driver(args):
    for name in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=CASE_TIME_LIMIT).returncode
        except subprocess.TimeoutExpired:
            print(f"resize_route_probe: {name} did not finish in {CASE_TIME_LIMIT} s; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"resize_route_probe: {name} ended with code {rc}; stopping", flush=True)
            return rc
    return 0


def arm_stats(x):
    return statistics.median(x), min(x), max(x), abs(statistics.median(x[0::2]) - statistics.median(x[1::2]))


def case(name, rounds, warmup):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
    dm = importlib.import_module("3dgs_hierarchical_training_amd.densify")
    syn = importlib.import_module("3dgs_hierarchical_training_amd.synthetic")
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    n, degree = CASES[name]
    rounds = max(20, rounds)
    dev = torch.device("cuda:0")
    names = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
    gen = torch.Generator().manual_seed(17)
    sc = syn.make_scene(n, 256, 256, sh_degree=degree, seed=11)
    base = ts.GaussianParams(sc, dev)
    with torch.no_grad():
        base._opacity[(torch.rand(n, generator=gen) < 0.05).to(dev)] = -9.0                  # sigmoid(-9) is under the floor of 0.005
    raw = {k: getattr(base, k).detach() for k in names}
    moments = {k: (torch.randn(v.shape, generator=gen).to(dev), torch.rand(v.shape, generator=gen).to(dev)) for k, v in raw.items()}
    hot = (torch.rand(n, 1, generator=gen) < 0.10).float().to(dev)
    med = float(base.get_scaling.detach().max(dim=1).values.median())
    prune_mask = (torch.rand(n, generator=gen) < 0.5).to(dev)
    row_bytes = sum(v[0].numel() * 4 for v in raw.values()) * 3
    del base

    def fresh(route):
        p = ts.GaussianParams.from_raw(raw, dev, sh_degree=degree)
        for g in p.optimizer.param_groups:
            t = g["params"][0]
            m, v = moments[p._GROUP_ATTR[g["name"]]]
            p.optimizer.state[t] = {"step": 1, "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        d = dm.Densifier(p, scene_extent=med / 0.01, cfg=dm.DensifyConfig(percent_dense=0.01), seed=5, route=route)
        d.xyz_gradient_accum, d.denom = hot.clone(), torch.ones_like(hot)
        return p, d

    def densify(route):
        p, d = fresh(route)
        return p, (lambda: d.densify_and_prune(0.5, 0.005, None))

    def prune(route):
        p, d = fresh(route)
        return p, (lambda: p.prune_points(prune_mask, route=route))

    def sample(make, route):
        p, call = make(route)
        torch.cuda.synchronize(dev)
        before = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize(dev)
        ms = 1e3 * (time.perf_counter() - t0)
        return ms, (torch.cuda.max_memory_allocated(dev) - before) / 2 ** 20, p

    print(f"resize_route_probe {name}: {torch.cuda.get_device_name(dev)}, N = {n}, SH degree {degree} ({row_bytes} bytes of parameters and moments "
          f"per row), rounds {rounds}, warm-up {warmup}, library version {L.load().gsr_version()}", flush=True)
    for what, make in (("densify_and_prune (5 % cloned, 5 % split, 5 % pruned)", densify), ("prune_points (50 % removed)", prune)):
        for _ in range(warmup):
            for route in ("torch", "kernel"):
                sample(make, route)
        _, _, pt = sample(make, "torch")
        _, _, pk = sample(make, "kernel")
        same = pt.num_points == pk.num_points and all(torch.equal(getattr(pt, k).detach(), getattr(pk, k).detach()) for k in names) and all(
            torch.equal(pt.optimizer.state[getattr(pt, k)][m], pk.optimizer.state[getattr(pk, k)][m]) for k in names for m in ("exp_avg", "exp_avg_sq"))
        n_after = pk.num_points
        del pt, pk
        t = {"torch": [], "kernel": []}
        peak = {"torch": [], "kernel": []}
        for _ in range(rounds):
            for route in ("torch", "kernel"):                    # A, B, A, B, ...
                ms, mib, p = sample(make, route)
                del p
                t[route].append(ms)
                peak[route].append(mib)
        st = {k: arm_stats(v) for k, v in t.items()}
        print(f"\n{what}: N {n} -> {n_after}; both routes give the same tensors and moments bit for bit: {same}   [ms per call, host clock around a device synchronise]")
        for k in ("torch", "kernel"):
            med_, lo, hi, spread = st[k]
            print(f"  {k:8s} median {med_:8.3f}   min {lo:8.3f}   max {hi:8.3f}   odd/even rounds' medians differ by {spread:.3f}   "
                  f"peak allocation over the call {max(peak[k]):8.1f} MiB")
        diff, spread = st["kernel"][0] - st["torch"][0], max(st["torch"][3], st["kernel"][3])
        verdict = "no difference beyond the spread" if abs(diff) <= spread else ("kernel route is FASTER" if diff < 0 else "kernel route is SLOWER")
        print(f"  kernel - torch = {diff:+.3f}; same-arm spread {spread:.3f} -> {verdict}" + (f" ({st['torch'][0] / st['kernel'][0]:.2f}x)" if diff < -spread else ""), flush=True)
    print(flush=True)
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
