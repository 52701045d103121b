"""The in-place Adam streams leave out the stores that would write back exactly what was loaded (adam_unchanged4 / adam_line_changed,
csrc/adam_math.h: by whole 128-byte lines): rows no view has reached yet (g = m = v = 0), SH bands above the active degree.  Nothing may be able to tell: every case below holds the
in-place update (which skips) to the bits of a route that never skips -- the out-of-place update into the optimizer's shadow buffers
(GsrFusedAdam::param_out; its destination holds something else, so it always stores).

All runs use the fixed-order accumulation ("deterministic_backward"), so the gradients of two runs repeat their bits and "equal" means
equal bit for bit (compared as integers: -0.0 is not +0.0, a NaN equals only its own bits).

Scene: 300 Gaussians (three 128-row blocks of the per-Gaussian backward, the last one ragged) at 64x48; 120 of them behind the camera
(culled: their gradient is zero by geometry), 180 on a 15 x 12 grid of 1-pixel Gaussians 4 pixels apart with opacity >= 0.5 (nobody
occludes anybody)."""
import importlib
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
syn = importlib.import_module("3dgs_hierarchical_training_amd.synthetic")
ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
bt = importlib.import_module("3dgs_hierarchical_training_amd.batched")
R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
E = importlib.import_module("3dgs_hierarchical_training_amd._ext")
loss_mod = importlib.import_module("3dgs_hierarchical_training_amd.loss")

W, H, N, N_BEHIND = 64, 48, 300, 120
GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
ATTR = ts.GaussianParams._GROUP_ATTR


def make_scene(deg, seed=3, behind=N_BEHIND):
    """synthetic.make_scene's cloud with its `behind` rows behind the camera (view depth in [-1, 0.2): the identity camera, so view
    depth = z) and the others moved onto the grid."""
    sc = syn.make_scene(N, W, H, sh_degree=deg, seed=seed, frac_behind=behind / N)
    z = sc["means3D"][:, 2].clone()
    front = z >= 1.0
    nf = int(front.sum())
    assert nf == N - behind and int((z < 0.2).sum()) == behind, (nf, behind)
    if not nf:       # the model nobody sees: half a unit further back, behind the second view's camera as well (second_view moves it <= 0.2)
        sc["means3D"][:, 2] -= 0.5
    if nf:
        assert nf <= 15 * 12
        g = torch.Generator().manual_seed(100 + seed)
        cell = torch.randperm(15 * 12, generator=g)[:nf]
        px, py = (cell % 15 + 0.5) * (W / 15.0), (cell // 15 + 0.5) * (H / 12.0)
        zf = z[front]
        sc["means3D"][front] = torch.stack([(px - W / 2.0) / sc["fx"] * zf, (py - H / 2.0) / sc["fy"] * zf, zf], 1).float()
        sc["scales"][front] = ((1.0 * zf / sc["fx"])[:, None] * torch.exp(0.2 * torch.randn(nf, 3, generator=g))).float()
        sc["opacities"][front] = (0.5 + 0.45 * torch.rand(nf, 1, generator=g)).float()
        assert float(sc["opacities"][front].min()) >= 0.5
    return sc


def second_view(sc, seed=7):
    g = torch.Generator().manual_seed(seed)
    sc2 = dict(sc)
    sc2.update(syn.make_camera(W, H, R=syn.random_rotation(g, 0.05), t=0.05 * torch.randn(3, generator=g)))
    return sc2


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def state_of(p):
    """Clones of the six parameter tensors and their moments, by group name."""
    out = {}
    for g in p.optimizer.param_groups:
        t = g["params"][0]
        st = p.optimizer.state[t]
        out[g["name"]] = (t.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())
    return out


def assert_same_state(a, b, what):
    for name in GROUPS:
        for k, part in enumerate(("param", "exp_avg", "exp_avg_sq")):
            assert same_bits(a[name][k], b[name][k]), (what, name, part, int((bits(a[name][k]) != bits(b[name][k])).sum()))


def assert_same_render(a, b, what):
    for k in ("loss", "raw_image", "radii"):
        x, y = a[k], b[k]
        assert same_bits(x, y) if x.dtype == torch.float32 else torch.equal(x, y), (what, k)


def zero_state(p):
    """The optimizer's state as torch lays it out, created up front (a test seeds moments before the first step)."""
    for g in p.optimizer.param_groups:
        t = g["params"][0]
        p.optimizer.state[t] = {"step": 0, "exp_avg": torch.zeros_like(t), "exp_avg_sq": torch.zeros_like(t)}


def step_in_place(p, view, gt, nxt=None):
    """The fused step: the update is applied in place inside the per-Gaussian backward (stores skipped where nothing changed)."""
    return ts.train_step(p, view, gt, next_settings=nxt)


def step_out_of_place(p, view, gt):
    """The same step through the out-of-place outputs: the backward writes the updated rows into shadow buffers -- every one of them --
    and step() adopts them.  Until then the model itself must be untouched."""
    st = ts.with_sh_degree(view, p.active_sh_degree)
    m2d = torch.zeros_like(p._xyz, requires_grad=True)
    color, radii, _, _ = R.rasterize_gaussians_raw(p._xyz, m2d, p._features_dc, p._features_rest, p._opacity, p._scaling, p._rotation, st,
                                                   fused_adam=p.optimizer, fused_adam_deferred=True)
    loss = loss_mod.fused_photometric_loss(color, gt, 0.2, clamp=True)
    before = state_of(p)
    loss.backward()
    assert_same_state(state_of(p), before, "the deferred backward left the model alone")
    assert p.optimizer._pending is not None
    p.optimizer.step()
    p.optimizer.zero_grad(set_to_none=True)
    return {"loss": loss.detach(), "raw_image": color.detach(), "radii": radii}


def step_separate(p, view, gt):
    """backward() to .grad, then FusedAdam.step(): the one-launch k_adam (csrc/optim_kernels.hip), in place."""
    return ts.train_step(p, view, gt, fused_optimizer=False)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def fixed_order_accumulation():
    lib = L.load()
    assert lib.gsr_set_option(b"deterministic_backward", 1) == 0
    yield
    lib.gsr_set_option(b"deterministic_backward", 0)


def views_and_targets(sc, dev, deg):
    v = [ts.make_settings(sc, dev, deg), ts.make_settings(second_view(sc), dev, deg)]
    gt = [syn.target_image(W, H, seed=11).to(dev), syn.target_image(W, H, seed=12).to(dev)]
    return v, gt


def run_arms(sc, dev, deg, steps=3, seed_state=None, after_first_step=None, check_first_step=None):
    """Three models from the same scene through the same `steps` steps (views alternating): in place with the hand-over of the next
    view's preprocess, in place without it, out of place.  Equal after every step."""
    v, gt = views_and_targets(sc, dev, deg)
    arms = {"in place + next view": ts.GaussianParams(sc, dev), "in place": ts.GaussianParams(sc, dev), "out of place": ts.GaussianParams(sc, dev)}
    for p in arms.values():
        zero_state(p)
        if seed_state is not None:
            seed_state(p)
    for it in range(steps):
        k = it % 2
        out = {"in place + next view": step_in_place(arms["in place + next view"], v[k], gt[k], nxt=v[1 - k]),
               "in place": step_in_place(arms["in place"], v[k], gt[k]),
               "out of place": step_out_of_place(arms["out of place"], v[k], gt[k])}
        if it:
            assert out["in place + next view"] is not None and getattr(arms["in place + next view"], "_prepared", None) is not None
        ref = state_of(arms["out of place"])
        for name in ("in place + next view", "in place"):
            assert_same_state(state_of(arms[name]), ref, (name, "step", it + 1))
            assert_same_render(out[name], out["out of place"], (name, "step", it + 1))
        if it == 0 and check_first_step is not None:
            check_first_step(arms, out)
        if it == 0 and after_first_step is not None:
            for p in arms.values():
                after_first_step(p)
    return arms


def touched_and_untouched_rows(p):
    m = p.optimizer.state[p._xyz]["exp_avg"]
    touched = int((m != 0).any(1).sum())
    zero = torch.ones(N, dtype=torch.bool, device=m.device)
    for g in p.optimizer.param_groups:
        st = p.optimizer.state[g["params"][0]]
        zero &= (st["exp_avg"].reshape(N, -1) == 0).all(1) & (st["exp_avg_sq"].reshape(N, -1) == 0).all(1)
    return touched, int(zero.sum())


def test_in_place_equals_out_of_place_at_degree_3(dev):
    """(a) Three fused steps, all six groups, moments, loss, image and radii, after every step; after the first one at least 100 rows
    carry a gradient's trace and at least 100 are exactly as they were created (the rows whose stores are left out)."""
    sc = make_scene(3)

    def first(arms, out):
        for name, p in arms.items():
            touched, zero = touched_and_untouched_rows(p)
            assert touched >= 100 and zero >= 100, (name, touched, zero)
            assert int((out[name]["radii"] > 0).sum()) >= 100
    run_arms(sc, dev, 3, check_first_step=first)


def test_in_place_equals_out_of_place_at_degree_1_with_16_coefficients_stored(dev):
    """(b) Active degree 1 of 3: 36 of the 45 f_rest floats of a TOUCHED row see no gradient either -- unchanged elements in the middle
    of rows that are stored, with changed and unchanged elements sharing lines."""
    sc = make_scene(1)

    def first(arms, out):
        for name, p in arms.items():
            st = p.optimizer.state[p._features_rest]
            m = st["exp_avg"].reshape(N, 15, 3)
            assert int((m[:, :3] != 0).any(2).any(1).sum()) >= 100, name       # the active band moved ...
            assert int(torch.count_nonzero(m[:, 3:])) == 0 and int(torch.count_nonzero(st["exp_avg_sq"].reshape(N, 15, 3)[:, 3:])) == 0, name
    arms = run_arms(sc, dev, 1, check_first_step=first)
    for p in arms.values():
        assert p.active_sh_degree == 1 and p.max_sh_degree == 3


def test_seeded_edge_states_in_untouched_rows(dev):
    """(c) Moments seeded into culled rows before the first step.  m = -0.0 comes back +0.0 (Adam writes m + (g - m)(1 - b1) = +0.0: a
    changed word, stored); a NaN second moment gives the bits of the out-of-place arm; m != 0 with g = 0 decays and is stored."""
    sc = make_scene(3)
    z = sc["means3D"][:, 2]
    r_negzero, r_nan, r_decay = [int(i) for i in torch.argsort(z)[:3]]       # the three rows deepest behind the camera, in either view
    assert float(z[r_decay]) < 0.0

    def seed(p):
        for g in p.optimizer.param_groups:
            st = p.optimizer.state[g["params"][0]]
            st["exp_avg"][r_negzero] = -0.0
            if g["name"] in ("f_rest", "rotation"):
                st["exp_avg"][r_decay] = 0.25
                st["exp_avg_sq"][r_decay] = 1.0
        p.optimizer.state[p._features_rest]["exp_avg_sq"][r_nan] = float("nan")
        assert int(bits(p.optimizer.state[p._xyz]["exp_avg"][r_negzero])[0]) == -2 ** 31

    def first(arms, out):
        b1 = np.float32(1.0) - np.float32(0.9)
        want = np.float32(np.float64(0.25) + np.float64(-0.25) * np.float64(b1))     # fmaf(g - m, 1 - b1, m): one rounding
        for name, p in arms.items():
            for g in p.optimizer.param_groups:
                st = p.optimizer.state[g["params"][0]]
                assert int(bits(st["exp_avg"][r_negzero]).abs().max()) == 0, (name, g["name"], "-0.0 must read back +0.0")
            for t in (p._features_rest, p._rotation):
                m = p.optimizer.state[t]["exp_avg"][r_decay].reshape(-1).cpu().numpy()
                assert (m == want).all() and want != np.float32(0.25), (name, m[:4], want)
            assert bool(torch.isnan(p.optimizer.state[p._features_rest]["exp_avg_sq"][r_nan]).all()), name
            assert bool(torch.isnan(p._features_rest.detach()[r_nan]).all()), name      # p - step * m / NaN
        for t in ("_features_rest", "_rotation"):
            assert not same_bits(getattr(arms["in place"], t).detach()[r_decay], sc_param[t][r_decay].to(dev)), t
    probe = ts.GaussianParams(sc, dev)
    sc_param = {t: getattr(probe, t).detach().clone() for t in ("_features_rest", "_rotation")}
    run_arms(sc, dev, 3, seed_state=seed, check_first_step=first)


def test_a_group_one_step_behind_the_others(dev):
    """(d) GsrFusedAdam::step_lag: after the first step the opacity group's step count is set one back (what an opacity reset leaves
    behind); its bias corrections then differ from the other groups' on both routes alike."""
    sc = make_scene(3)

    def lag(p):
        assert p.optimizer.step_count == 1
        p.optimizer.state[p._opacity]["step"] = 0
    arms = run_arms(sc, dev, 3, after_first_step=lag)
    for p in arms.values():
        o = p.optimizer
        assert o.step_count == 3 and int(o.state[p._opacity]["step"]) == 2


def test_separate_adam_step_equals_the_out_of_place_update(dev):
    """(e) The unmodified trainer's route: gradients to .grad, then FusedAdam.step() = k_adam, in place over rows of which 120 have
    g = m = v = 0 (skipped).  The same arithmetic (adam_one) on the same gradients (fixed-order accumulation) as the out-of-place
    update inside the backward: the same bits, for three steps; the deferred route's own untouched-until-step() property is asserted
    inside step_out_of_place."""
    sc = make_scene(3)
    v, gt = views_and_targets(sc, dev, 3)
    a, b = ts.GaussianParams(sc, dev), ts.GaussianParams(sc, dev)
    for it in range(3):
        k = it % 2
        oa, ob = step_separate(a, v[k], gt[k]), step_out_of_place(b, v[k], gt[k])
        assert_same_state(state_of(a), state_of(b), ("separate step", it + 1))
        assert_same_render(oa, ob, ("separate step", it + 1))
    touched, zero = touched_and_untouched_rows(a)
    assert touched >= 100 and zero >= 100, (touched, zero)


def test_k_adam_direct_call_vector_and_scalar_paths_agree(dev):
    """(e) gsr_adam_step itself on two chunks and a ragged tail: the 16-byte path (aligned tensors) and the per-float path (the same
    data one float off alignment, where the decision is taken per float) leave the same bits; a -0.0 moment with g = 0 reads back +0.0, a moment with
    g = 0 decays, an element with g = m = v = 0 keeps its bits (NaN parameters included)."""
    ops = E.load()
    n = 2 * 4096 + 37
    g = torch.Generator().manual_seed(5)
    p0, m0 = torch.randn(n, generator=g), 0.01 * torch.randn(n, generator=g)
    v0, gr = (0.01 * torch.randn(n, generator=g)) ** 2, 0.1 * torch.randn(n, generator=g)
    idle = torch.rand(n, generator=g) < 0.6           # elements nobody has reached: g = m = v = 0
    gr[idle] = 0.0; m0[idle] = 0.0; v0[idle] = 0.0
    idle_i = torch.nonzero(idle).reshape(-1)
    i_negzero, i_decay, i_nan = int(idle_i[0]), int(idle_i[1]), int(idle_i[2])
    m0[i_negzero] = -0.0
    m0[i_decay], v0[i_decay] = 0.25, 1.0
    p0[i_nan] = float("nan")
    res = []
    for off in (0, 1):                                 # 0: every tensor 16-byte aligned; 1: none
        t = [torch.zeros(n + 4, device=dev)[off:off + n].copy_(x.to(dev)) for x in (p0, gr, m0, v0)]
        assert all((x.data_ptr() % 16 == 0) == (off == 0) for x in t)
        for step in (1, 2):
            ops.adam_step([t[0]], [t[1]], [t[2]], [t[3]], [0.01], 0.9, 0.999, 1e-15, step)
        res.append([x.clone() for x in (t[0], t[2], t[3])])
    for a, b, what in zip(res[0], res[1], ("param", "exp_avg", "exp_avg_sq")):
        assert same_bits(a, b), what
    p, m, v = res[0]
    keep = idle.clone()
    keep[[i_negzero, i_decay]] = False
    keep = keep.to(dev)
    assert same_bits(p[keep], p0.to(dev)[keep]) and int(bits(m[keep]).abs().max()) == 0 and int(bits(v[keep]).abs().max()) == 0
    assert int(bits(m[i_negzero:i_negzero + 1])[0]) == 0
    assert 0.0 < float(m[i_decay]) < 0.25 and float(p[i_decay]) != float(p0[i_decay])
    moved = (~idle).to(dev)
    assert bool((bits(p[moved]) != bits(p0.to(dev)[moved])).all())


def test_eight_batched_models_equal_training_each_alone(dev):
    """(f) Eight models of 300 in one store, one of them entirely behind its camera (every store of its rows is left out): each is
    bit-identical with training it alone, over three steps with the hand-over."""
    B = 8
    scenes = [make_scene(3, seed=20 + k, behind=N if k == 5 else N_BEHIND) for k in range(B)]
    gts = [syn.target_image(W, H, seed=30 + k).to(dev) for k in range(B)]
    cams = [[ts.make_settings(sc, dev, 3), ts.make_settings(second_view(sc, seed=40 + k), dev, 3)] for k, sc in enumerate(scenes)]
    for view in (scenes[5], second_view(scenes[5], seed=45)):      # model 5 is behind both of its cameras (view depth < 0.2: culled)
        w2c = view["viewmatrix"].t()
        assert float((scenes[5]["means3D"] @ w2c[:3, :3].t() + w2c[:3, 3])[:, 2].max()) < 0.0
    singles = [ts.GaussianParams(sc, dev) for sc in scenes]
    batch = bt.BatchedGaussianParams(scenes, dev)
    bviews = [bt.batch_settings([cams[k][v] for k in range(B)], dev) for v in range(2)]
    gt_stack = torch.stack(gts)
    for it in range(3):
        v = it % 2
        pk = ts.train_step(batch, bviews[v], gt_stack, next_settings=bviews[1 - v])
        for k in range(B):
            ps = ts.train_step(singles[k], cams[k][v], gts[k], next_settings=cams[k][1 - v])
            rows = batch.model_rows(k)
            assert same_bits(pk["raw_image"][k], ps["raw_image"]) and torch.equal(pk["radii"][rows], ps["radii"]), (it, k)
            for gb, gs in zip(batch.optimizer.param_groups, singles[k].optimizer.param_groups):
                tb, t1 = gb["params"][0], gs["params"][0]
                assert same_bits(tb.detach()[rows], t1.detach()), (it, k, gb["name"])
                sb, s1 = batch.optimizer.state[tb], singles[k].optimizer.state[t1]
                for mom in ("exp_avg", "exp_avg_sq"):
                    assert same_bits(sb[mom][rows], s1[mom]), (it, k, gb["name"], mom)
    rows = batch.model_rows(5)
    assert int(pk["radii"][rows].abs().sum()) == 0
    for gb in batch.optimizer.param_groups:
        st = batch.optimizer.state[gb["params"][0]]
        assert int(torch.count_nonzero(st["exp_avg"][rows])) == 0 and int(torch.count_nonzero(st["exp_avg_sq"][rows])) == 0
    assert math.isfinite(float(pk["loss"]))
