#!/usr/bin/env python3
"""Render-only forward against today's no-grad path, timed in ONE process on the same inputs (include/gsr.h GsrForwardArgs::render_only).

Two callers, two pairs of arms per size:
  teacher   A = what hierarchy.render_raw ran before: zeros_like means2D, rasterize_gaussians_raw under no_grad, [0].clamp(0, 1)
            B = render_gaussians_raw(clamped=True)[4]
  eval      A = what train_step.render ran under no_grad: rasterize_gaussians_raw under no_grad, depth + alpha kept, color.clamp(0, 1)
            B = render_gaussians_raw(depth_alpha=True, clamped=True)
After a warm-up of every shape the arms alternate call by call -- A, B, A, B, ... -- for at least 200 calls per arm; a host clock around a
device synchronise (CALL time: launches, allocations and the wait for the instance count included).  Per arm: the median, min-max, and
the spread of the arm against itself (medians of its odd and of its even calls).  RULE for switching a caller: B is not slower than A by
more than the same-arm spread (the larger of the two arms') at ANY size.  From passes of their own: the library's "blend_fwd" profile
stage (KERNEL time of the forward blend alone, from the dispatch's own timestamps) and the peak of torch's allocated bytes over one call.

Sizes (seeded synthetic scenes at 980x545): 1m = 1 M Gaussians / degree 3, 300k = 300 k / degree 3, 130k = 130 k / degree 0.

    python tools/render_only_probe.py [1m] [300k] [130k]        # default: all three; writes profiles/render_only.txt
"""
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
syn = importlib.import_module("3dgs_hierarchical_training_amd.synthetic")
R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
L = importlib.import_module("3dgs_hierarchical_training_amd._lib")

W, H = 980, 545
CALLS, WARMUP, STAGE_CALLS = 200, 10, 30
SIZES = {"1m": ("1 M / degree 3", 1_000_000, 3, 0), "300k": ("300 k / degree 3", 300_000, 3, 1), "130k": ("130 k / degree 0", 130_000, 0, 3)}


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return 1e3 * (time.perf_counter() - t0)


def arm_stats(x):
    return statistics.median(x), min(x), max(x), abs(statistics.median(x[0::2]) - statistics.median(x[1::2]))


def stage(lib, name):
    tot, cnt = C.c_double(0), C.c_int64(0)
    lib.gsr_profile_read(name.encode(), C.byref(tot), C.byref(cnt))
    return tot.value, int(cnt.value)


def arms_of(raw, rs):
    x = (raw["_xyz"], raw["_features_dc"], raw["_features_rest"], raw["_opacity"], raw["_scaling"], raw["_rotation"])

    def teacher_a():
        with torch.no_grad():
            m2d = torch.zeros_like(x[0])
            return R.rasterize_gaussians_raw(x[0], m2d, *x[1:], rs)[0].clamp(0, 1)

    def teacher_b():
        return R.render_gaussians_raw(*x, rs, clamped=True)[4]

    def eval_a(m2d=torch.zeros_like(x[0])):
        with torch.no_grad():
            color, radii, depth, alpha = R.rasterize_gaussians_raw(x[0], m2d, *x[1:], rs)
            return color.clamp(0, 1), color, depth, alpha, radii

    def eval_b():
        color, radii, depth, alpha, clamped, _ = R.render_gaussians_raw(*x, rs, depth_alpha=True, clamped=True)
        return clamped, color, depth, alpha, radii
    return {"teacher": (teacher_a, teacher_b), "eval": (eval_a, eval_b)}


def probe(size, dev, lib, say):
    name, n, deg, seed = SIZES[size]
    sc = syn.make_scene(n, W, H, sh_degree=deg, seed=seed)
    raw = ts.GaussianParams(sc, dev, optimizer="torch").raw()
    raw = {k: v.detach() for k, v in raw.items()}
    rs = ts.make_settings(sc, dev, deg)
    verdicts = {}
    for caller, (a, b) in arms_of(raw, rs).items():
        assert torch.equal(a() if caller == "teacher" else a()[0], b() if caller == "teacher" else b()[0]), "the arms render different images"
        for _ in range(WARMUP):
            a(), b()
        t = {"A": [], "B": []}
        for _ in range(CALLS):
            t["A"].append(timed(a, dev))
            t["B"].append(timed(b, dev))
        st = {k: arm_stats(v) for k, v in t.items()}
        say(f"\n{name} @ {W}x{H}, caller {caller}: ms per call (host clock around a device synchronise), {CALLS} calls per arm, alternating")
        for k, what in (("A", "today's no-grad path"), ("B", "render-only")):
            med, lo, hi, spread = st[k]
            say(f"  {k} {what:21s} median {med:7.3f}   min {lo:7.3f}   max {hi:7.3f}   odd/even calls' medians differ by {spread:.3f}")
        spread = max(st["A"][3], st["B"][3])
        diff = st["B"][0] - st["A"][0]
        ok = diff <= spread
        verdicts[caller] = ok
        say(f"  B - A = {diff:+.3f} ms; same-arm spread {spread:.3f} ms -> render-only {'NOT slower' if ok else 'SLOWER'} at this size")
        for k, fn in (("A", a), ("B", b)):             # peak of the allocator over one call
            torch.cuda.synchronize(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            out = fn()
            torch.cuda.synchronize(dev)
            say(f"  {k} peak allocation over the call {(torch.cuda.max_memory_allocated(dev) - before) / 2 ** 20:8.1f} MiB, kept after it "
                f"{(torch.cuda.memory_allocated(dev) - before) / 2 ** 20:8.1f} MiB")
            del out
        lib.gsr_set_option(b"profile", 2)              # the forward blend's own dispatch timestamps; a pass of its own
        try:
            for k, fn in (("A", a), ("B", b)):
                stage(lib, "blend_fwd")
                for _ in range(STAGE_CALLS):
                    fn()
                torch.cuda.synchronize(dev)
                tot, cnt = stage(lib, "blend_fwd")
                say(f"  {k} kernel time, stage blend_fwd {1e3 * tot / max(cnt, 1):8.1f} us per call over {cnt} calls")
        finally:
            lib.gsr_set_option(b"profile", 0)
    return verdicts


def main():
    sizes = [s.lower() for s in sys.argv[1:]] or list(SIZES)
    for s in sizes:
        if s not in SIZES:
            raise SystemExit(f"unknown size {s!r}: one of {sorted(SIZES)}")
    dev = torch.device("cuda:0")
    lib = L.load()
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "render_only.txt"), "w") as fh:
        def say(line):
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()
        say(f"render_only_probe: {torch.cuda.get_device_name(dev)}, library version {lib.gsr_version()}, sizes {sizes}")
        verdicts = {s: probe(s, dev, lib, say) for s in sizes}
        say("")
        for caller in ("teacher", "eval"):
            ok = all(v[caller] for v in verdicts.values())
            say(f"verdict {caller}: render-only is {'NOT slower at every probed size -> the caller takes it' if ok else 'SLOWER at some size -> the caller stays'}")


if __name__ == "__main__":
    main()
