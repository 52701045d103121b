"""GPU: V views of ONE model in one launch chain (include/gsr.h gsr_forward_views, gsr_importance_accumulate_views;
rasterizer.forward_views / importance_accumulate_views, hierarchy.calc_importance(views_per_call=...)).

The forward of V views is held to V single-view forwards bit for bit; the importance over views to the float64 oracle at the project's
bar for this quantity (importance_common.RTOL) and to the per-view route at the bar two float-atomic runs are held to (1e-6 of the
maximum).  Scenes and references: tests/views_common.py on tests/importance_common.py."""
import ctypes as C
import importlib
import types
import warnings

import numpy as np
import pytest
import torch

import importance_common as ic
import parity
import views_common as vc
from test_python_sh_cpu import PythonShRender

pytestmark = pytest.mark.gpu
hier = ic.hier
ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
E = importlib.import_module("3dgs_hierarchical_training_amd._ext")
L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
bt = importlib.import_module("3dgs_hierarchical_training_amd.batched")
refstub = importlib.import_module("3dgs_hierarchical_training_amd.refstub")
rs_mod = importlib.import_module("3dgs_hierarchical_training_amd.run_segments")
seg_mod = importlib.import_module("3dgs_hierarchical_training_amd.segments")
sequence = importlib.import_module("3dgs_hierarchical_training_amd.sequence")
DEV = torch.device("cuda:0")
FRAME_A, FRAME_B = ic.SCENE_A[1:3], ic.SCENE_B[1:3]          # 100x75 and 72x40: partial tiles on both edges
# (direct_binning, tile_sort): the list-building routes as tests/test_gpu_render_only.py forces them -- depth sort + emit + tile-key sort;
# depth sort + direct placement; direct placement in index order + per-tile depth sort; emit in index order + tile sort + per-tile sort
ROUTES = ((0, 0), (1, 0), (1, 2), (0, 2))


# ---- the forward ---------------------------------------------------------------------------------------------------------------------
def _cameras(W, H, V, order=None):
    """V per-view scene dicts (their cameras are what is used) in `order`; more than eight views repeat the eight with a small shift."""
    cams = list(vc.scene(8, W, H, 3, vc.MAX_VIEWS)[1])
    out = []
    for v in range(V):
        sc = dict(cams[v % len(cams)])
        if v >= len(cams):                                  # a ninth .. sixteenth camera: the same rotation, moved a little
            w2c = sc["viewmatrix"].t().clone()
            cam = vc.syn.make_camera(W, H, vc.syn.FOVX_FRANCIS, w2c[:3, :3], w2c[:3, 3] + 0.05 * (v // len(cams)))
            sc.update({k: cam[k] for k in ("viewmatrix", "projmatrix", "campos")})
        out.append(sc)
    return out if order is None else [out[i] for i in order]


def _model(N, W, H, kind="raw", seed=5):
    """The eight model tensors of the forward ops, in their order, and the raw flag.  kind: raw (split SH storage, raw parameters),
    act (one SH tensor, activated parameters), pre (colors_precomp + cov3D_precomp), cov (SH + cov3D_precomp), col (colours + scales)."""
    sc = vc.syn.make_scene(N, W, H, sh_degree=3, seed=seed, posed=False, frac_behind=0.0 if N < 100 else 0.02)
    e = torch.empty(0, device=DEV)
    d = lambda t: t.to(DEV).contiguous()
    if kind == "raw":
        p = ts.GaussianParams(sc, DEV, optimizer="torch")
        return (p._xyz.detach(), p._features_dc.detach(), e, p._opacity.detach(), p._scaling.detach(), p._rotation.detach(), e,
                p._features_rest.detach()), True
    kw = parity.scene_kwargs(sc, {"act": "sh", "cov": "pre", "pre": "pre", "col": "mixed"}[kind])
    sh = d(sc["shs"]) if kind in ("act", "cov") else e
    col = d(kw["colors_precomp"]) if kind in ("pre", "col") else e
    cov = d(kw["cov3D_precomp"]) if kind in ("pre", "cov") else e
    sr = (e, e) if kind in ("pre", "cov") else (d(sc["scales"]), d(sc["rotations"]))
    return (d(sc["means3D"]), sh, col, d(sc["opacities"]), sr[0], sr[1], cov, e), False


def _single(model, raw, rs, deg, xf=None, sh_origin=None):
    """One view through torch.ops.gsr.rasterize_forward with both extras: (color, radii, depth, alpha, clamped, visible)."""
    e, eb = torch.empty(0, device=DEV), torch.empty(0, dtype=torch.uint8, device=DEV)
    out = E.load().rasterize_forward(*model, rs.viewmatrix, rs.projmatrix, rs.campos, rs.bg, e if xf is None else xf, int(rs.image_height),
                                     int(rs.image_width), float(rs.tanfovx), float(rs.tanfovy), 1.0, deg, raw, False, False, eb, [], 0, 3,
                                     sh_origin)
    return out[0], out[1], out[2], out[3], out[8], out[9]


def _views(model, raw, settings, deg, xf=None, sh_origin=None):
    means, sh, col, op, sc, rot, cov, rest = model
    none = lambda t: None if t.numel() == 0 else t
    return R.forward_views(means, none(sh), op, none(sc), none(rot), bt.batch_settings(settings, DEV), sh_rest=none(rest), raw_params=raw,
                           cov3Ds_precomp=none(cov), colors_precomp=none(col), points_transform=xf, sh_origin=sh_origin, extras=3)


NAMES = ("color", "radii", "depth", "alpha", "clamped", "visible")


def _assert_views_equal_singles(model, raw, settings, deg, xf=None, sh_origin=None, what=""):
    got = _views(model, raw, settings, deg, xf, sh_origin)
    N, V = model[0].shape[0], len(settings)
    assert tuple(got[1].shape) == (V, N) and tuple(got[5].shape) == (V, N) and got[0].shape[0] == V
    for v, rs in enumerate(settings):
        one = _single(model, raw, rs, deg, None if xf is None else xf[v], None if sh_origin is None else sh_origin[v])
        for name, a, b in zip(NAMES, got, one):
            assert torch.equal(a[v], b), (what, "view", v, name)
    return got


@pytest.mark.parametrize("V", [1, 2, 3, 16])
@pytest.mark.parametrize("N", [1, 127, 128, 129, 1000])
def test_forward_of_views_equals_single_forwards(N, V):
    """Colour, depth, alpha, radii, the clamped colour and the visibility bytes of every view, bit for bit, at the sizes around a
    128-Gaussian block and at 1, 2, 3 and 16 views; raw parameters, split SH storage, degree 3, 100x75."""
    W, H = FRAME_A
    model, raw = _model(N, W, H)
    got = _assert_views_equal_singles(model, raw, vc.settings(_cameras(W, H, V), DEV, 3), 3, what=f"N {N} V {V}")
    if N >= 127:
        assert int(got[5].sum()) > 0          # something is seen


@pytest.mark.parametrize("kind", ["raw", "act"])
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_forward_degrees_and_parameter_forms(deg, kind):
    """SH degrees 0-3 with raw parameters on split SH storage and with activated parameters on one SH tensor; 72x40, three views."""
    W, H = FRAME_B
    model, raw = _model(1000, W, H, kind)
    _assert_views_equal_singles(model, raw, vc.settings(_cameras(W, H, 3), DEV, deg), deg, what=f"deg {deg} {kind}")


@pytest.mark.parametrize("kind", ["pre", "cov", "col"])
def test_forward_precomputed_covariance_and_colour(kind):
    """cov3D_precomp and colors_precomp (together, and each with the other input in its ordinary form)."""
    W, H = FRAME_B
    model, raw = _model(1000, W, H, kind)
    _assert_views_equal_singles(model, raw, vc.settings(_cameras(W, H, 3), DEV, 3), 3, what=kind)


def _transforms(V):
    """A different rigid [3,4] transform per view: small rotations about the z axis and small shifts."""
    out = []
    for v in range(V):
        a = 0.03 * (v + 1)
        out.append(torch.tensor([[np.cos(a), -np.sin(a), 0.0, 0.02 * v], [np.sin(a), np.cos(a), 0.0, -0.01 * v], [0.0, 0.0, 1.0, 0.015 * v]],
                                dtype=torch.float32))
    return torch.stack(out).to(DEV)


def test_forward_per_view_points_transform_and_sh_origin():
    """A points_transform per view, an sh_origin per view, and both: each view sees its own."""
    W, H = FRAME_A
    model, raw = _model(1000, W, H)
    cams = _cameras(W, H, 3)
    settings = vc.settings(cams, DEV, 3)
    xf = _transforms(3)
    origins = torch.stack([sc["campos"] + torch.tensor([0.3, -0.25, 0.2]) * (v + 1) for v, sc in enumerate(cams)]).to(DEV)
    _assert_views_equal_singles(model, raw, settings, 3, xf=xf, what="points_transform")
    _assert_views_equal_singles(model, raw, settings, 3, sh_origin=origins, what="sh_origin")
    _assert_views_equal_singles(model, raw, settings, 3, xf=xf, sh_origin=origins, what="both")
    # ... and the origins matter: the colour of a view differs from the one the module's direction gives
    plain = _views(model, raw, settings, 3)
    moved = _views(model, raw, settings, 3, sh_origin=origins)
    assert not torch.equal(plain[0], moved[0]) and torch.equal(plain[1], moved[1])


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: f"direct{r[0]}-tsort{r[1]}")
def test_forward_on_every_list_building_route(route):
    """Each list-building route forced for the views forward AND the single forwards: the same bits; one view and three."""
    W, H = FRAME_A
    model, raw = _model(1000, W, H)
    lib = L.load()
    try:
        assert lib.gsr_set_option(b"direct_binning", route[0]) == 0 and lib.gsr_set_option(b"tile_sort", route[1]) == 0
        for V in (1, 3):
            _assert_views_equal_singles(model, raw, vc.settings(_cameras(W, H, V), DEV, 3), 3, what=f"route {route} V {V}")
    finally:
        lib.gsr_set_option(b"direct_binning", 1)
        lib.gsr_set_option(b"tile_sort", 1)


def test_forward_with_a_blind_view_between_two_that_see():
    """A camera turned away from the cloud between two that see it: its image is the background, its radii are zero, and the views
    on either side are what they are alone."""
    W, H = FRAME_A
    model, raw = _model(1000, W, H)
    cams = _cameras(W, H, 2)
    cams = [cams[0], vc.away_camera(cams[0]), cams[1]]
    settings = vc.settings(cams, DEV, 3)
    got = _assert_views_equal_singles(model, raw, settings, 3, what="blind view")
    assert int(got[1][1].abs().sum()) == 0 and int(got[5][1].sum()) == 0 and int(got[5][0].sum()) > 0 and int(got[5][2].sum()) > 0
    assert torch.equal(got[0][1], settings[0].bg.reshape(3, 1, 1).expand(3, H, W)) and float(got[3][1].abs().max()) == 0.0


def test_forward_permuted_cameras_and_repeat():
    """Cameras permuted: the views' outputs permute with them; the same call again: the same bits."""
    W, H = FRAME_B
    model, raw = _model(1000, W, H)
    perm = [2, 0, 3, 1]
    a = _views(model, raw, vc.settings(_cameras(W, H, 4), DEV, 3), 3)
    b = _views(model, raw, vc.settings(_cameras(W, H, 4, order=perm), DEV, 3), 3)
    again = _views(model, raw, vc.settings(_cameras(W, H, 4), DEV, 3), 3)
    for name, x, y, z in zip(NAMES, a, b, again):
        assert torch.equal(x[perm], y), name
        assert torch.equal(x, z), name


def test_forward_over_ctypes(monkeypatch):
    """The plain-FFI route over the same C ABI gives the extension's bits, with a transform and an SH origin per view."""
    W, H = FRAME_A
    model, raw = _model(129, W, H)
    settings = vc.settings(_cameras(W, H, 3), DEV, 3)
    xf = _transforms(3)
    origins = torch.stack([rs.campos + 0.2 for rs in settings])
    ext = _views(model, raw, settings, 3, xf=xf, sh_origin=origins)
    monkeypatch.setenv("GSR_BINDING", "ctypes")
    assert E.use_ctypes()
    ct = _views(model, raw, settings, 3, xf=xf, sh_origin=origins)
    monkeypatch.delenv("GSR_BINDING")
    for name, x, y in zip(NAMES, ext, ct):
        assert torch.equal(x, y), name


def test_backward_and_single_view_importance_refuse_the_flags_of_a_views_forward():
    """gsr_backward and gsr_importance_accumulate return GSR_ERR_ARG for forward_flags that carry GSR_FWD_FLAG_VIEWS, before anything
    is enqueued: the accumulator they would have written keeps its bits.  The flags come from a real views forward."""
    W, H = FRAME_B
    model, raw = _model(1000, W, H)
    settings = vc.settings(_cameras(W, H, 2), DEV, 3)
    e = torch.empty(0, device=DEV)
    st = bt.batch_settings(settings, DEV)
    out = E.load().rasterize_forward_views(*model, st.viewmatrix, st.projmatrix, st.campos, st.bg, e, H, W, float(st.tanfovx), float(st.tanfovy),
                                           1.0, 3, raw, 0, None)
    flags = int(out[7][2])
    assert flags & L.GSR_FWD_FLAG_VIEWS and int(out[7][0]) > 0
    lib = L.load()
    acc = torch.full((1000, 16, 3), 7.0, device=DEV)
    a, o = L.GsrForwardArgs(), L.GsrForwardOut()
    a.N, a.M, a.D, a.W, a.H = 1000, 16, 3, W, H
    a.means3D, a.shs, a.shs_rest, a.campos = model[0].data_ptr(), model[1].data_ptr(), model[7].data_ptr(), st.campos.data_ptr()
    a.out_color, a.geom, a.image = out[0].data_ptr(), out[4].data_ptr(), out[5].data_ptr()
    o.num_rendered, o.binning_capacity, o.forward_flags, o.binning = int(out[7][0]), int(out[7][1]), flags, out[6].data_ptr()
    assert lib.gsr_importance_accumulate(C.byref(a), C.byref(o), acc.data_ptr(), acc.data_ptr(), None) == -1
    assert b"gsr_importance_accumulate_views" in lib.gsr_last_error()
    b = L.GsrBackwardArgs()
    b.N, b.M, b.D, b.W, b.H, b.forward_flags = 1000, 16, 3, W, H, flags
    assert lib.gsr_backward(C.byref(b), None) == -1 and b"views forward" in lib.gsr_last_error()
    torch.cuda.synchronize()
    assert float(acc.min()) == 7.0 and float(acc.max()) == 7.0


# ---- importance over views -----------------------------------------------------------------------------------------------------------
def _case(N, W, H, deg, V, dark=False):
    """(segment on the device, settings per view sharing one background tensor, oracle importance [N,48]); the views' conditions first."""
    base, views = vc.scene(N, W, H, deg, V, dark)
    for i, v in enumerate(vc.oracle_views(N, W, H, deg, V, dark)):
        ic.assert_meaningful(ic.conditions(v["color"], v["rgb"], v["radii"]), f"{N}/{W}x{H}/deg{deg}{'/dark' if dark else ''} view {i}", dark)
    return ic.segment(base, DEV), vc.settings(views, DEV, deg), vc.oracle_importance(N, W, H, deg, V, dark)


def _within_bar(imp, ref, what):
    err, top = float(np.abs(np.asarray(imp, np.float64) - ref).max()), float(ref.max())
    print(f"[importance views] {what}: max err {err:.3e} = {err / top:.2e} of the maximum entry")
    assert np.isfinite(np.asarray(imp)).all() and err <= ic.RTOL * top, (what, err, top)


A3, B3 = ic.SCENE_A[:3], ic.SCENE_B
ORACLE = [A3 + (d, 4) for d in (0, 1, 2, 3)] + [B3 + (d, 4) for d in (0, 1, 2, 3)] + [A3 + (3, 8), B3 + (2, 8)] + \
         [A3 + (3, 4, True), B3 + (2, 4, True)]


@pytest.mark.parametrize("case", ORACLE, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-d{c[3]}-V{c[4]}" + ("-dark" if len(c) > 5 else ""))
def test_importance_over_views_matches_the_oracle(case):
    """Scenes A and B at degrees 0-3 under four views, at degree 3 / 2 under eight, and their dark variants: within RTOL of the maximum
    entry of the float64 oracle; coefficients >= (D+1)^2 are exactly 0.0."""
    seg, views, ref = _case(*case)
    V = case[4]
    imp = hier.calc_importance(seg, views, route="kernel", views_per_call=V)
    assert tuple(imp.shape) == (case[0], 48) and imp.dtype == torch.float32 and not imp.requires_grad
    _within_bar(imp.cpu().numpy(), ref, f"views route {case}")
    nc = (case[3] + 1) ** 2
    assert float(imp.view(-1, 16, 3)[:, nc:].abs().max() if nc < 16 else 0.0) == 0.0


@pytest.mark.parametrize("V,per_call", [(2, 2), (3, 3), (8, 8), (4, 3)], ids=["V2", "V3", "V8", "3+1"])
def test_views_route_against_the_per_view_route(V, per_call):
    """calc_importance(views_per_call=V) within 1e-6 of the maximum of views_per_call=1 (the bar two float-atomic runs are held to) at
    two, three and eight views, and on four views that group_views cuts into a group of three and a group of one."""
    N, W, H, deg = ic.SCENE_A
    seg, views, _ = _case(N, W, H, deg, V)
    assert [len(g) for g in hier.group_views(views, per_call, N)] == ([3, 1] if (V, per_call) == (4, 3) else [V])
    want = hier.calc_importance(seg, views, route="kernel", views_per_call=1)
    got = hier.calc_importance(seg, views, route="kernel", views_per_call=per_call)
    assert float(want.max()) > 0 and float((got - want).abs().max()) <= 1e-6 * float(want.max())


@pytest.mark.parametrize("V", [4, 8])
def test_rows_no_view_sees_are_neither_read_nor_written(V):
    """With the accumulator prefilled with 7.0 the rows whose oracle importance is zero under ALL V views hold 7.0 bit for bit -- their
    share, taken from the oracle before the kernel runs, is between 30 and 70 % -- and the others 7.0 + their sum within the bar."""
    N, W, H, deg = ic.SCENE_A
    seg, views, ref = _case(N, W, H, deg, V)
    zero = ref.max(1) == 0
    assert 0.3 < zero.mean() < 0.7
    acc = torch.full((N, 16, 3), 7.0, dtype=torch.float32, device=DEV)
    R.importance_accumulate_views(acc, seg["_xyz"], seg["_features_dc"], seg["_opacity"], seg["_scaling"], seg["_rotation"],
                                  hier.stack_views(views, DEV), sh_rest=seg["_features_rest"], raw_params=True)
    acc = acc.cpu().numpy().reshape(N, 48)
    assert (acc[zero] == np.float32(7.0)).all()
    sums = (acc.astype(np.float64) - 7.0) / (V * W * H)
    err = np.abs(sums - ref)[~zero].max()
    # (7 + x carries an absolute rounding of 2^-22 per entry and view on top of the bar)
    assert err <= ic.RTOL * ref.max() + V * 2.0 ** -22 / (V * W * H), err


@pytest.mark.parametrize("case,ratio", [(ic.SCENE_A + (4,), 0.75), (B3 + (2, 4), 0.6), (ic.SCENE_A + (4, True), 0.75), (B3 + (2, 4, True), 0.6)],
                         ids=["A", "B", "A-dark", "B-dark"])
def test_prune_masks_of_both_routes(case, ratio):
    """The rule of test_kernel_route_against_autograd_route for the per-view and the views route: the masks differ in fewer than 1 % of
    the rows, and only in rows whose oracle score lies within 5e-3 of the threshold; the threshold (from the oracle) is positive."""
    seg, views, ref = _case(*case)
    N, V = case[0], case[4]
    score = ref.max(1)
    thr = np.sort(score)[int(N * ratio) - 1]
    assert thr > 0                                    # the ratio lies above the zero-row share
    one = hier.calc_importance(seg, views, route="kernel", views_per_call=1)
    many = hier.calc_importance(seg, views, route="kernel", views_per_call=V)
    d1, dv = hier.prune_mask(one, ratio).cpu().numpy(), hier.prune_mask(many, ratio).cpu().numpy()
    diff = d1 != dv
    assert diff.mean() < 0.01
    assert (np.abs(score[diff] - thr) <= 5e-3 * max(thr, 1e-30)).all()


def test_the_pass_leaves_the_forwards_outputs_untouched():
    """Colour, radii, depth and alpha of the views forward cloned before the pass equal those after it bit for bit, and the pass on the
    forward's own buffers is what the one-call op computes."""
    N, W, H, deg = ic.SCENE_A
    seg, views, _ = _case(N, W, H, deg, 4)
    st = hier.stack_views(views, DEV)
    e = torch.empty(0, device=DEV)
    model = (seg["_xyz"], seg["_features_dc"], e, seg["_opacity"], seg["_scaling"], seg["_rotation"], e, seg["_features_rest"])
    out = E.load().rasterize_forward_views(*model, st.viewmatrix, st.projmatrix, st.campos, st.bg, e, H, W, float(st.tanfovx), float(st.tanfovy),
                                           1.0, deg, True, 0, None)
    color, radii, depth, alpha, geom, image, binning, meta = out[:8]
    before = [t.clone() for t in (color, radii, depth, alpha, geom)]
    lib = L.load()
    acc = torch.zeros(N, 16, 3, device=DEV)
    a, o = L.GsrForwardArgs(), L.GsrForwardOut()
    a.N, a.M, a.D, a.W, a.H = N, 16, deg, W, H
    a.means3D, a.shs, a.shs_rest, a.campos = model[0].data_ptr(), model[1].data_ptr(), model[7].data_ptr(), st.campos.data_ptr()
    a.out_color, a.geom, a.image = color.data_ptr(), geom.data_ptr(), image.data_ptr()
    o.num_rendered, o.binning_capacity, o.forward_flags, o.binning = int(meta[0]), int(meta[1]), int(meta[2]), binning.data_ptr()
    scratch = torch.empty(lib.gsr_importance_scratch_bytes_views(N, 4), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    assert lib.gsr_importance_accumulate_views(C.byref(a), 4, C.byref(o), acc.data_ptr(), scratch.data_ptr(), C.c_void_p(stream)) == 0, \
        lib.gsr_last_error()
    torch.cuda.synchronize()
    assert float(acc.max()) > 0
    for x, y in zip(before, (color, radii, depth, alpha, geom)):
        assert torch.equal(x, y)
    acc2 = torch.zeros(N, 16, 3, device=DEV)
    R.importance_accumulate_views(acc2, seg["_xyz"], seg["_features_dc"], seg["_opacity"], seg["_scaling"], seg["_rotation"], st,
                                  sh_rest=seg["_features_rest"], raw_params=True)
    assert float((acc2 - acc).abs().max()) <= 1e-6 * float(acc.max())
    # flags without GSR_FWD_FLAG_VIEWS are refused by the views entry, before anything is enqueued
    o.forward_flags = int(meta[2]) & ~L.GSR_FWD_FLAG_VIEWS
    keep = acc.clone()
    assert lib.gsr_importance_accumulate_views(C.byref(a), 4, C.byref(o), acc.data_ptr(), scratch.data_ptr(), C.c_void_p(stream)) == -1
    torch.cuda.synchronize()
    assert torch.equal(acc, keep)


def _sync_warnings(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum(1 for w in rec if "synchroniz" in str(w.message).lower())


def test_host_waits_of_an_eight_view_call():
    """Under torch.cuda.set_sync_debug_mode("warn") an eight-view call raises as many synchronisation warnings as a one-view call, and
    the per-view route over the same eight views eight times as many.  Measured on an MI355X: 0, 0 and 0 -- with the views sharing one
    background tensor torch sees no synchronising operation on either route; the wait it cannot see, the library's own for the
    instance count, is one per forward, so the forwards are counted too: 1 for the eight-view call, 8 for the per-view route."""
    N, W, H, deg = ic.SCENE_A
    seg, views, _ = _case(N, W, H, deg, 8)
    hier.calc_importance(seg, views, route="kernel", views_per_call=8)          # warm: extension loaded, caches filled
    hier.calc_importance(seg, views[:1], route="kernel", views_per_call=1)
    one = _sync_warnings(lambda: hier.calc_importance(seg, views[:1], route="kernel", views_per_call=1))
    eight = _sync_warnings(lambda: hier.calc_importance(seg, views, route="kernel", views_per_call=8))
    per_view = _sync_warnings(lambda: hier.calc_importance(seg, views, route="kernel", views_per_call=1))
    print(f"[importance views] synchronisation warnings: one view {one}, eight views in one call {eight}, eight calls {per_view}")
    assert eight == one and per_view == 8 * one
    lib = L.load()
    c0 = lib.gsr_get_counter(b"forward_calls")
    hier.calc_importance(seg, views, route="kernel", views_per_call=8)
    c1 = lib.gsr_get_counter(b"forward_calls")
    hier.calc_importance(seg, views, route="kernel", views_per_call=1)
    c2 = lib.gsr_get_counter(b"forward_calls")
    assert (c1 - c0, c2 - c1) == (1, 8)       # forwards, each with its one wait for the instance count


# ---- the patched trainer method and the merge ------------------------------------------------------------------------------------------
def _lie(pose7, delta):
    p = refstub.LieGroupParameter(refstub.SE3(torch.tensor([pose7], device=DEV)))
    with torch.no_grad():
        p.copy_(torch.tensor([delta], device=DEV))
    return p


@pytest.mark.parametrize("posed", [False, True], ids=["identity", "frame-pose"])
@pytest.mark.parametrize("python_sh", [False, True], ids=["module-sh", "convert_SHs_python"])
def test_autopatch_views_on_trainer_shaped_objects(posed, python_sh, monkeypatch):
    """The patched `HTGaussianTrainer.calc_importance` on the trainer-shaped stand-ins of tests/test_gpu_importance.py, four cameras:
    with GSR_AUTOPATCH_IMPORTANCE_VIEWS=4 the result is within 1e-6 of the maximum of the default's, through the views entry."""
    import gsr_autopatch
    deg, N, (W, H) = 2, ic.SCENE_B[0], FRAME_B
    base, views = vc.scene(N, W, H, deg, 4)
    p = ts.GaussianParams(base, DEV, optimizer="torch")
    p.active_sh_degree = deg
    r = PythonShRender(p, bg=ic.BG)
    g = r.gaussians
    if posed:
        g.P = [_lie([0.0, 0, 0, 0, 0, 0, 1], [0.0] * 6), _lie([0.02, -0.03, 0.01, 0.01, 0.0, -0.01, 1.0], [0.01, -0.02, 0.015, 0.004, -0.003, 0.002])]
        g.rotate_seq, g.seq_idx = True, 1
    cams = [refstub.StubCamera.from_scene(sc, DEV, uid=1) for sc in views]
    pipe = types.SimpleNamespace(compute_cov3D_python=False, convert_SHs_python=python_sh)
    monkeypatch.delenv("GSR_AUTOPATCH_IMPORTANCE_VIEWS", raising=False)
    want = gsr_autopatch.calc_importance_fused(r, cams, pipe)
    calls = []
    real = R.importance_accumulate_views
    monkeypatch.setattr(R, "importance_accumulate_views", lambda *a, **k: calls.append(a[6].viewmatrix.shape[0]) or real(*a, **k))
    monkeypatch.setenv("GSR_AUTOPATCH_IMPORTANCE_VIEWS", "4")
    p._features_dc.grad = torch.ones_like(p._features_dc)
    got = gsr_autopatch.calc_importance_fused(r, cams, pipe)
    assert calls == [4] and p._features_dc.grad is None and tuple(got.shape) == (N, 48) and not got.requires_grad
    assert float(want.max()) > 0 and float((got - want).abs().max()) <= 1e-6 * float(want.max())
    if not posed and not python_sh:
        _within_bar(got.cpu().numpy(), vc.oracle_importance(N, W, H, deg, 4), "patched calc_importance, four views per call")


def test_one_merge_through_run_segments_with_four_views_per_call(monkeypatch):
    """Two leaves of 2 000 Gaussians trained once, then merged twice from the same state through RankRunner.merge_send / merge_recv: with
    importance_views_per_call 1 and 4.  The drop masks of the two runs differ in fewer than 1 % of the rows, and each merged model is
    its own masks' rows of the two children, bit for bit -- so the merged models are equal wherever the masks are."""
    cfg = rs_mod.HTConfig(frames=10, width=96, height=72, gt_gaussians=4000, leaf_gaussians=2000, leaf_iters_per_frame=2,
                          phase1_iters_per_frame=1, phase2_iters_per_frame=[1, 1, 1], prune_ratio=0.5)
    seq = sequence.FrameSequence(cfg.frames, cfg.gt_gaussians, cfg.width, cfg.height, DEV, seed=4)
    trained = [rs_mod.RankRunner(r, 2, seg_mod.LocalTransport(2), seq, cfg, DEV, log=lambda rec: None) for r in range(2)]
    for rr in trained:
        rr.train_leaf()
    pre = [{k: v.clone() for k, v in rr.seg.params.raw().items()} for rr in trained]
    assert all(len(rr.seg.frames) >= 5 for rr in trained)
    masks, plans = {}, {}
    real_prune, real_views = hier.prune_mask, R.importance_accumulate_views
    merged = {}
    for per_call in (1, 4):
        cfg2 = rs_mod.HTConfig(**{**cfg.__dict__, "importance_views_per_call": per_call})
        tr = seg_mod.LocalTransport(2)
        runners = [rs_mod.RankRunner(r, 2, tr, seq, cfg2, DEV, log=lambda rec: None) for r in range(2)]
        for rr, t in zip(runners, trained):
            s = t.seg
            rr.seg = rs_mod.Segment(s.params, s.frames, s.start_fidx, dict(s.poses), s.global_iteration)
        masks[per_call], plans[per_call] = [], []
        monkeypatch.setattr(hier, "prune_mask", lambda imp, ratio, route="torch", _m=masks[per_call]: _m.append(real_prune(imp, ratio, route=route)) or _m[-1])
        monkeypatch.setattr(hier, "importance_accumulate_views",
                            lambda *a, _p=plans[per_call], **k: _p.append(int(a[6].viewmatrix.shape[0])) or real_views(*a, **k))
        (dst, src), = runners[0].schedule[0]
        runners[src].merge_send(0)
        runners[dst].merge_recv(0)
        merged[per_call] = ({k: v.clone() for k, v in runners[dst].seg.params.raw().items()}, dst, src)
    assert plans[1] == [] and plans[4] and max(plans[4]) == 4          # the views entry ran, with groups of up to four
    for a, b in zip(masks[1], masks[4]):
        assert a.shape == b.shape and float((a != b).float().mean()) < 0.01
    for per_call in (1, 4):
        m, dst, src = merged[per_call]
        drop_src, drop_dst = masks[per_call]                               # the sender scores first, then the receiver
        for key in ("_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
            assert torch.equal(m[key], torch.cat((pre[dst][key][~drop_dst], pre[src][key][~drop_src]))), (per_call, key)
    if all(torch.equal(a, b) for a, b in zip(masks[1], masks[4])):
        for key in merged[1][0]:
            assert torch.equal(merged[1][0][key], merged[4][0][key]), key
