"""CPU: the C-ABI library loads and exports every symbol include/gsr.h declares; the product path refuses to
run without a GPU or without the built extension (no fallback)."""
import ctypes as C
import importlib
import os
import re
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_build_and_exports():
    b = importlib.import_module("3dgs_hierarchical_training_amd.build")
    lib_path = b.build()
    assert os.path.exists(lib_path)
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    lib = L.load()
    hdr = open(os.path.join(REPO, "include", "gsr.h")).read()
    declared = set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", hdr)) - {"gsr_alloc_fn"}
    assert declared, "no declarations parsed"
    for sym in declared:
        assert hasattr(lib, sym), f"libgsr_hip.so does not export {sym}"
    assert set(L.EXPORTS) <= declared | {"gsr_forward_scratch_bytes"}
    assert lib.gsr_version() >= 100
    assert lib.gsr_geom_bytes(10) >= 480 and lib.gsr_image_bytes(64, 64) >= 64 * 64 * 28


def test_struct_layout_matches_header():
    """ctypes mirrors of the argument structs have the field order of include/gsr.h."""
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    hdr = open(os.path.join(REPO, "include", "gsr.h")).read()
    for name, cls in [("GsrForwardArgs", L.GsrForwardArgs), ("GsrBackwardArgs", L.GsrBackwardArgs), ("GsrForwardOut", L.GsrForwardOut),
                      ("GsrFusedAdam", L.GsrFusedAdam)]:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for stmt in body.split(";"):
            stmt = stmt.strip()
            if not stmt:
                continue
            for part in stmt.split(","):
                fields.append(re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[\d+\])?$", part.strip())[0])
        assert fields == [f[0] for f in cls._fields_], name


def test_cpu_tensors_are_refused():
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    rs = GaussianRasterizationSettings(image_height=16, image_width=16, tanfovx=0.5, tanfovy=0.5, bg=torch.zeros(3),
                                       scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0,
                                       campos=torch.zeros(3), prefiltered=False, debug=False)
    r = GaussianRasterizer(rs)
    x = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r(means3D=x, means2D=x, shs=None, colors_precomp=torch.zeros(4, 3), opacities=torch.ones(4, 1),
          scales=torch.ones(4, 3), rotations=torch.ones(4, 4), cov3D_precomp=None)
    with pytest.raises(Exception, match="excatly one"):
        r(means3D=x, means2D=x, shs=None, colors_precomp=None, opacities=torch.ones(4, 1), scales=torch.ones(4, 3),
          rotations=torch.ones(4, 4), cov3D_precomp=None)
    with pytest.raises(Exception, match="exactly one"):
        r(means3D=x, means2D=x, shs=None, colors_precomp=x, opacities=torch.ones(4, 1), scales=None, rotations=None,
          cov3D_precomp=None)


def test_missing_library_fails_loudly(monkeypatch):
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L, "LIB_PATH", "/nonexistent/libgsr_hip.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.load()


def test_product_path_does_not_import_oracle():
    """The oracle is test infrastructure: nothing under the package or the drop-in alias may reference it."""
    pkg = os.path.join(REPO, "3dgs_hierarchical_training_amd")
    for root in (pkg, os.path.join(REPO, "diff_gaussian_rasterization"), os.path.join(REPO, "simple_knn")):
        for dp, _, fns in os.walk(root):
            for fn in fns:
                if fn.endswith((".py", ".hip", ".h")):
                    txt = open(os.path.join(dp, fn)).read()
                    assert "import oracle" not in txt and "from oracle" not in txt and "hostemu" not in txt.replace("tests/hostemu", ""), fn


def test_direct_binning_geometry_invariants():
    """Host logic of the direct binning (csrc/gsr_kernels.hip direct_bin_geometry): chunks of whole 64-Gaussian steps that cover N,
    u16 counters that cannot overflow (a chunk, and a group of chunks, below 65 536 Gaussians), at most 64 groups, frames above
    4 096 tiles left to the sort route.  No GPU needed."""
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    lib = L.load()
    out = (C.c_int64 * 7)()
    for N in (1, 63, 64, 65, 1000, 20_000, 130_000, 1_000_000, 4_000_000, 30_000_000):
        for T in (1, 64, 256, 2170, 4096):
            assert lib.gsr_debug_direct_binning_geometry(N, T, out) == 0
            ok, S, NC, G, Cg, Tp, nbytes = (int(v) for v in out)
            if not ok:
                assert N > 4_000_000      # (only a model too large for 16-bit chunk counters is refused at these frame sizes)
                continue
            assert S % 64 == 0 and S >= 128 and S <= 65472
            assert NC * S >= N > (NC - 1) * S
            assert G * Cg >= NC > (G - 1) * Cg and 1 <= G <= 64
            assert Cg * S <= 65535
            assert Tp % 64 == 0 and T <= Tp < T + 64
            assert nbytes >= NC * Tp * 2 + G * Tp * 4 + (T + 1) * 4
    for N, T in ((0, 100), (1000, 0), (1000, 4097), (1000, 8160)):
        assert lib.gsr_debug_direct_binning_geometry(N, T, out) == 0 and out[0] == 0


def test_sort_scratch_bytes_closed_form():
    """Scratch of a sort over n pairs (csrc/radix_sort.h onesweep_scratch_bytes), in 32-bit words over nb = max(1, ceil(n / 4096)) tiles:
    four 8-bit passes -- head of 4 x 32 x 256 digit counts + 128 tickets, then 4 x 256 status words per tile -- or three 9-bit
    passes -- 3 x 32 x 512 + 128, then 3 x 512 per tile -- whichever is larger, rounded up to 256 bytes.  No GPU needed."""
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    lib = L.load()
    for n in (0, 1, 4096, 4097, 1_000_000, 30_000_000):
        nb = max(1, -(-n // 4096))
        want = (4 * max(32896 + 1024 * nb, 49280 + 1536 * nb) + 255) // 256 * 256
        assert lib.gsr_sort_scratch_bytes(n) == want, n


def test_tile_sort_option_values():
    """`tile_sort` takes 0 / 1 / 2 (off / where the lists are short / wherever the direct binning runs) and nothing else; its threshold
    is a non-negative count.  No GPU needed: options are host state."""
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    lib = L.load()
    try:
        for v in (0, 2, 1):
            assert lib.gsr_set_option(b"tile_sort", v) == 0
        assert lib.gsr_set_option(b"tile_sort", 3) != 0 and lib.gsr_set_option(b"tile_sort", -1) != 0
        assert lib.gsr_set_option(b"tile_sort_max_avg", 0) == 0 and lib.gsr_set_option(b"tile_sort_max_avg", 800) == 0
        assert lib.gsr_set_option(b"tile_sort_max_avg", -5) != 0
    finally:
        lib.gsr_set_option(b"tile_sort", 1)
        lib.gsr_set_option(b"tile_sort_max_avg", 700)


INT_MIN, INT_MAX = -2**31, 2**31 - 1
# name: (default, lowest accepted, highest accepted, refused outside).  Outside the range a name that is not refused stores a
# value of its own choice and returns GSR_OK (tests/options_check/options_check.cpp looks at what is stored).
OPTION_TABLE = {
    "bwd_split": (0, 0, 64, True),
    "ckpt_first": (1, 1, 64, True),
    "tile_sort": (1, 0, 2, True),
    "tile_sort_max_avg": (700, 0, INT_MAX, True),
    "view_pose_tol_e6": (2000, 0, INT_MAX, True),
    "small_sort9": (1, 0, INT_MAX, True),
    "list_cut": (1, 0, 2, False),
    "list_cut_min_n": (2000000, 0, INT_MAX, False),
    "list_cut_margin_e3": (50, 0, INT_MAX, False),
    "list_cut_deep": (8, 0, INT_MAX, False),
    "poll_iters": (400000, 0, INT_MAX, False),
    "prep_hist_max_n": (262144, INT_MIN, INT_MAX, False),
    "blend_balance": (1, 0, 1, False),
    "early_r": (1, 0, 1, False),
    "depth_sort9": (1, 0, 1, False),
    "direct_binning": (1, 0, 1, False),
    "speculative_binning": (1, 0, 1, False),
    "emit_hist": (1, 0, 1, False),
    "deterministic_backward": (0, 0, 1, False),
}
RETIRED_OPTIONS = {"blend_fwd_ppt": (0, 7), "tile_map": (2,), "sort_algo": (2,), "blend_bwd_ppt": (0, 2)}


def test_option_table_accepts_and_refuses_as_documented():
    """gsr_set_option over every value option: the boundary values of the accepted range are taken, one value beyond each end is
    refused (GSR_ERR_ARG, -1) or taken, as the table says; the retired names take the values that selected what is now the only
    code path and refuse their neighbours; "ab_variants" returns 0 whatever it is given; an unknown or a null name is refused.
    No GPU needed: options are host state."""
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    lib = L.load()
    try:
        for name, (_, lo, hi, refused_outside) in OPTION_TABLE.items():
            n = name.encode()
            assert lib.gsr_set_option(n, lo) == 0 and lib.gsr_set_option(n, hi) == 0, name
            for beyond in ([lo - 1] if lo > INT_MIN else []) + ([hi + 1] if hi < INT_MAX else []):
                assert lib.gsr_set_option(n, beyond) == (-1 if refused_outside else 0), (name, beyond)
        for name, accepted in RETIRED_OPTIONS.items():
            n = name.encode()
            for v in accepted:
                assert lib.gsr_set_option(n, v) == 0, (name, v)
            for v in sorted({min(accepted) - 1, max(accepted) + 1} | set(range(min(accepted), max(accepted))) - set(accepted)):
                assert lib.gsr_set_option(n, v) == -1, (name, v)
        for v in (INT_MIN, -1, 0, 1, 5, INT_MAX):
            assert lib.gsr_set_option(b"ab_variants", v) == 0
        assert lib.gsr_set_option(b"no_such_option", 1) == -1 and lib.gsr_set_option(b"", 0) == -1
        assert lib.gsr_set_option(b"tile_sort_emit_max_n", 400000) == -1     # (a threshold of the library that no name sets)
        assert lib.gsr_set_option(None, 1) == -1
    finally:
        for name, (default, _, _, _) in OPTION_TABLE.items():
            assert lib.gsr_set_option(name.encode(), default) == 0


def test_options_header_stores_what_the_table_says(tmp_path):
    """csrc/options.h on its own (plain C++17): tests/options_check/options_check.cpp asserts the defaults of Options{}, the value every
    "store the default" / "store 0" / "store value != 0" rule leaves in the snapshot, and that a refused call leaves it unchanged."""
    import subprocess
    exe = str(tmp_path / "options_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread",
                           os.path.join(REPO, "tests", "options_check", "options_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "options_check: ok" in r.stdout, r.stderr[-600:]


def test_options_from_the_environment_at_load():
    """`GSR_OPTS=name=value,...` is applied by _lib.load() (a whole test run or bench under a non-default route of the library); a name or
    value the library refuses is an error at load, not a silently ignored word.  Own processes: the options are process state."""
    import subprocess
    code = ("import importlib, sys; sys.path.insert(0, '.'); L = importlib.import_module('3dgs_hierarchical_training_amd._lib'); "
            "lib = L.load(); print('loaded', lib.gsr_set_option(b'tile_sort', 1))")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ok = subprocess.run([sys.executable, "-c", code], cwd=root, env={**os.environ, "GSR_OPTS": "tile_sort=2, blend_bwd_ppt=2"}, capture_output=True, text=True)
    assert ok.returncode == 0 and "loaded 0" in ok.stdout, ok.stderr[-400:]
    for bad in ("no_such_option=1", "tile_sort=7", "blend_bwd_ppt=1", "sort_algo=0", "blend_fwd_ppt=6", "tile_map=1"):
        r = subprocess.run([sys.executable, "-c", code], cwd=root, env={**os.environ, "GSR_OPTS": bad}, capture_output=True, text=True)
        assert r.returncode != 0 and "GSR_OPTS" in r.stderr, (bad, r.stdout, r.stderr[-400:])


def test_forward_flags_of_a_retired_variant_or_map_are_refused():
    """forward_flags keep their bit layout; the variant field (bits 1..3) holds 7 and the map field (bits 4..5) holds 2, the one forward
    blend and the one tile -> XCD map.  Flags with bit 0 set that carry another value cannot come from this library: gsr_backward and
    gsr_importance_accumulate refuse them before anything is enqueued.  The default's flags and flags 0 (the round-1 caller) pass that
    check and stop at the next one, a missing pointer."""
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    lib = L.load()
    fake = 0x1000          # never dereferenced: every call here is refused by an argument check
    good = 1 | (7 << 1) | (2 << 4) | (1 << 6) | (1 << 13)
    b = L.GsrBackwardArgs()
    b.N, b.M, b.D, b.W, b.H, b.d_means3D = 128, 1, 0, 32, 32, fake
    a = L.GsrForwardArgs()
    a.N, a.M, a.D, a.W, a.H = 128, 16, 3, 32, 32
    a.shs = a.campos = a.geom = a.image = a.out_color = a.means3D = fake
    out = L.GsrForwardOut()
    out.num_rendered, out.binning = 10, fake
    for flags in (good & ~(7 << 1) | (6 << 1), good & ~(7 << 1) | (1 << 1), good & ~(3 << 4) | (1 << 4), good & ~(3 << 4)):
        b.forward_flags = out.forward_flags = flags
        assert lib.gsr_backward(C.byref(b), None) == -1 and "forward_flags do not come from gsr_forward" in lib.gsr_last_error().decode()
        assert lib.gsr_importance_accumulate(C.byref(a), C.byref(out), fake, fake, None) == -1
        assert "forward_flags do not come from gsr_forward" in lib.gsr_last_error().decode()
    for flags in (good, 0):
        b.forward_flags = flags
        assert lib.gsr_backward(C.byref(b), None) == -1 and "missing workspace / gradient pointer" in lib.gsr_last_error().decode()
