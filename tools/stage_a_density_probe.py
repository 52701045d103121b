#!/usr/bin/env python3
"""CPU probe: how dense may stage A's every-pixel model be before binary32 misses the suite's gradient bars?

The host emulation of csrc/gsr_math.h against the float64 oracle (parity.check_forward, then the element-wise and norm-wise
measures of parity.check_grads, counted instead of asserted) on tests/camera_common.py pixel_gaussian_scene at 250x188, stride 1,
"waves": the centred camera with every scale x 1, x 1.2, x 1.41, and the camera "both" with the reference's neighbour-distance scale
and with z / fx taken literally.  Findings: DESIGN.md, "Real intrinsics", open gap.

Usage:  python tools/stage_a_density_probe.py
"""
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import camera_common as cc  # noqa: E402
import parity  # noqa: E402
from oracle import binding  # noqa: E402

W, H, STRIDE, SURFACE = 250, 188, 1, "waves"


def run(tag, sc):
    kw = parity.scene_kwargs(sc, "sh", bg=(0.05, 0.1, 0.15))
    o = binding.OracleRender(**kw)
    o.forward()
    rep = parity.check_forward(parity.hostemu_run(o)["fwd"], o, tag)
    gc, gd, ga = parity.upstream_grads(H, W, seed=5)
    keep = rep["grad_mask"]
    gc *= keep[None]; gd *= keep; ga *= keep
    ref = o.backward(gc, gd, ga)
    emu = parity.hostemu_run(o, (gc, gd, ga))
    out = []
    for k in ("means3D", "means2D", "opacities", "scales", "rotations"):
        g = np.asarray(emu["grads"][k], np.float64)
        r = np.asarray(ref[k], np.float64).reshape(g.shape)
        rms = np.sqrt((r[r != 0] ** 2).mean())
        bad = np.abs(g - r) > parity.ELEM_RTOL * np.abs(r) + parity.ELEM_RTOL * rms
        out.append(f"{k} {int(bad.sum())}/{bad.size} off, norm-wise {np.abs(g - r).max() / np.abs(r).max():.1e}")
    print(f"{tag}: edge pixels {rep['ambig_frac']:.2%}; " + "; ".join(out))
    o.close()


def main():
    for f in (1.0, 1.2, 1.41):
        sc = cc.pixel_gaussian_scene(W, H, STRIDE, SURFACE)
        sc["scales"] = sc["scales"] * f
        run(f"centred, scales x {f}", sc)
    sc = cc.pixel_gaussian_scene(W, H, STRIDE, SURFACE, cam="both")
    run("both, neighbour-distance scale", sc)
    fx, fy = cc.intrinsics("both", W, H)[:2]
    k = fx * math.sqrt((2.0 / max(fx, fy) ** 2 + 1.0 / min(fx, fy) ** 2) / 3.0)
    sc["scales"] = sc["scales"] / k
    run("both, scales z / fx", sc)


if __name__ == "__main__":
    main()
