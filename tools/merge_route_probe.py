#!/usr/bin/env python3
"""The merge's selection and append by the torch route and by the kernels, timed in ONE process per size with alternating arms.

  torch    hierarchy.prune_mask(route="torch"): amax, topk, a zero fill, an indexed store;
           segments.merge_segments(route="torch"): twelve boolean gathers and six torch.cat
  kernel   prune_mask(route="kernel"): gsr_select_smallest on the [N, 3 M] tensor;
           merge_segments(route="kernel"): two gsr_resize_plan, one read of both metas, one gsr_merge_apply

Three legs per size:
  select   prune_mask at ratio 0.5 on an importance tensor with 30 % all-zero rows (the Gaussians no view saw)
  append   merge_segments of two N-row segments, a random half of each kept, the source moved by a 4x4
  both     the two masks from two importance tensors, then the append with them: the destination's work at a merge

After a warm-up the arms alternate -- torch, kernel, torch, kernel, ... -- for `--rounds` rounds.  One sample is one call under a host clock
that ends in a device synchronise.  Per arm: the median, min - max, the spread of the arm against itself (the difference of the medians of
its odd and even rounds), torch's synchronisation warnings over one call (set_sync_debug_mode("warn")) and the peak allocation over the
call beyond what was allocated before it.  A route wins at a size only if the difference of the medians exceeds the larger same-arm spread.

Without --case the sizes run one after the other, each in a fresh child process under its own time limit; the first one that fails or
runs out of time ends the probe.

    python tools/merge_route_probe.py > profiles/merge_route.txt
"""
import argparse
import importlib
import os
import statistics
import subprocess
import sys
import time
import warnings

CASES = {"1M_deg3": (1_000_000, 3), "300k_deg3": (300_000, 3), "130k_deg0": (130_000, 0)}
CASE_TIME_LIMIT = 300      # seconds per size


def driver(args):
    for name in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--rounds", str(args.rounds), "--warmup", str(args.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=CASE_TIME_LIMIT).returncode
        except subprocess.TimeoutExpired:
            print(f"merge_route_probe: {name} did not finish in {CASE_TIME_LIMIT} s; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"merge_route_probe: {name} ended with code {rc}; stopping", flush=True)
            return rc
    return 0


def arm_stats(x):
    return statistics.median(x), min(x), max(x), abs(statistics.median(x[0::2]) - statistics.median(x[1::2]))


def case(name, rounds, warmup):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    hier = importlib.import_module("3dgs_hierarchical_training_amd.hierarchy")
    seg_mod = importlib.import_module("3dgs_hierarchical_training_amd.segments")
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    n, degree = CASES[name]
    coeffs = (degree + 1) ** 2
    rounds = max(20, rounds)
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(17)
    shapes = {"_xyz": (3,), "_features_dc": (1, 3), "_features_rest": (coeffs - 1, 3), "_opacity": (1,), "_scaling": (3,), "_rotation": (4,)}
    segs = [{k: torch.randn((n,) + s, generator=gen).to(dev) for k, s in shapes.items()} for _ in range(2)]
    imps = []
    for _ in range(2):
        imp = 0.5 * torch.rand(n, 3 * coeffs, generator=gen)          # distinct row maxima, so that topk's mask is defined and the routes can be compared
        imp[torch.arange(n), torch.randint(0, 3 * coeffs, (n,), generator=gen)] = 0.5 + (torch.randperm(n, generator=gen) + 1).float() / (2 * n + 2)
        imp[torch.rand(n, generator=gen) < 0.3] = 0.0
        imps.append(imp.to(dev))
    keeps = [(torch.rand(n, generator=gen) < 0.5).to(dev) for _ in range(2)]
    T = torch.eye(4)
    T[:3, 3] = torch.tensor([0.3, -1.0, 2.0])
    T[3] = torch.tensor([0.01, -0.02, 0.03, 1.1])
    T = T.to(dev)
    row_bytes = sum(4 * v[0].numel() for v in segs[0].values())

    def select(route):
        return hier.prune_mask(imps[0], 0.5, route=route)

    def append(route):
        return seg_mod.merge_segments(segs[0], segs[1], keeps[0], keeps[1], T, route=route)

    def both(route):
        drop_dst, drop_src = hier.prune_mask(imps[0], 0.5, route=route), hier.prune_mask(imps[1], 0.5, route=route)
        return seg_mod.merge_segments(segs[0], segs[1], ~drop_dst, ~drop_src, T, route=route)

    def sample(call, route):
        torch.cuda.synchronize(dev)
        before = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.perf_counter()
        out = call(route)
        torch.cuda.synchronize(dev)
        ms = 1e3 * (time.perf_counter() - t0)
        return ms, (torch.cuda.max_memory_allocated(dev) - before) / 2 ** 20, out

    def sync_warnings(call, route):
        torch.cuda.synchronize(dev)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                call(route)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        return sum("synchroniz" in str(w.message).lower() for w in rec)

    def same(a, b):
        if isinstance(a, dict):
            return all(torch.equal(a[k], b[k]) for k in a)
        return bool(torch.equal(a, b))

    print(f"merge_route_probe {name}: {torch.cuda.get_device_name(dev)}, N = {n} per side, SH degree {degree} ({row_bytes} bytes of parameters per "
          f"row, {3 * coeffs} importance columns), rounds {rounds}, warm-up {warmup}, library version {L.load().gsr_version()}", flush=True)
    legs = (("select: prune_mask(ratio 0.5), 30 % zero rows", select), ("append: merge_segments, a random half of each side kept", append),
            ("both: two prune_mask calls and the append with their masks", both))
    for what, call in legs:
        for _ in range(warmup):
            for route in ("torch", "kernel"):
                sample(call, route)
        equal = same(sample(call, "torch")[2], sample(call, "kernel")[2])
        waits = {route: sync_warnings(call, route) for route in ("torch", "kernel")}
        t = {"torch": [], "kernel": []}
        peak = {"torch": [], "kernel": []}
        for _ in range(rounds):
            for route in ("torch", "kernel"):                    # A, B, A, B, ...
                ms, mib, out = sample(call, route)
                del out
                t[route].append(ms)
                peak[route].append(mib)
        st = {k: arm_stats(v) for k, v in t.items()}
        print(f"\n{what}: both routes give the same result bit for bit: {equal}   [ms per call, host clock around a device synchronise]")
        for k in ("torch", "kernel"):
            med_, lo, hi, spread = st[k]
            print(f"  {k:8s} median {med_:8.3f}   min {lo:8.3f}   max {hi:8.3f}   odd/even rounds' medians differ by {spread:.3f}   "
                  f"synchronisation warnings {waits[k]:2d}   peak allocation over the call {max(peak[k]):8.1f} MiB")
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
