"""CPU: the host side of the merge on the device (include/gsr.h version 121: gsr_select_smallest, gsr_select_scratch_bytes,
gsr_merge_apply) -- the library version, the exports and their ctypes signatures, every refusal of the C ABI (all before a device is
touched: NULL or fake device pointers) with the rule named by gsr_last_error(), the op schemas, the `route` keywords of hierarchy /
segments / run_segments, and the numpy oracles of tests/merge_common.py: the selection against torch.topk where topk is defined, the
merged layout against `merge_segments(route="torch")` on CPU tensors."""
import ctypes as C
import importlib
import inspect

import numpy as np
import pytest
import torch

import merge_common as MC

E = importlib.import_module("3dgs_hierarchical_training_amd._ext")
L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
M = importlib.import_module("3dgs_hierarchical_training_amd.merge")
hier = importlib.import_module("3dgs_hierarchical_training_amd.hierarchy")
seg_mod = importlib.import_module("3dgs_hierarchical_training_amd.segments")

FAKE = 0x1000      # a non-NULL, 16-byte aligned "device pointer": the refusals come before any use of it


def _last_error():
    return L.load().gsr_last_error().decode()


def test_library_version_exports_and_signatures():
    lib = L.load()
    assert lib.gsr_version() >= 121
    for name in ("gsr_select_scratch_bytes", "gsr_select_smallest", "gsr_merge_apply"):
        assert name in L.EXPORTS and hasattr(lib, name), name
    assert lib.gsr_struct_bytes(0) == C.sizeof(L.GsrForwardArgs) and lib.gsr_struct_bytes(1) == C.sizeof(L.GsrBackwardArgs)      # no existing struct changed
    assert C.sizeof(L.GsrResizeTensor) == 40
    assert lib.gsr_select_scratch_bytes.restype is C.c_size_t and lib.gsr_select_scratch_bytes.argtypes == [C.c_int64]
    assert lib.gsr_select_smallest.restype is C.c_int
    assert lib.gsr_select_smallest.argtypes == [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_size_t, C.c_void_p]
    assert lib.gsr_merge_apply.restype is C.c_int
    assert lib.gsr_merge_apply.argtypes == [C.c_void_p, C.c_size_t, C.c_int64, C.c_int64] * 2 + [C.POINTER(L.GsrMergeTensor), C.c_int32, C.c_void_p,
                                                                                                 C.c_void_p]
    assert C.sizeof(L.GsrMergeTensor) == 40 and [f[0] for f in L.GsrMergeTensor._fields_] == ["src_a", "src_b", "dst", "row_bytes", "kind", "reserved"]
    assert L.GSR_SELECT_MAX_COLUMNS >= 48 and L.GSR_SELECT_META_WORDS == 8 and L.GSR_RESIZE_KEEP == MC.KEEP
    assert (L.GSR_RESIZE_PARAM, L.GSR_RESIZE_MOMENT) == (MC.PARAM, MC.MOMENT) == (M.PARAM, M.MOMENT)


def test_the_scratch_size_is_a_closed_form():
    fn = L.load().gsr_select_scratch_bytes
    assert [fn(n) for n in (0, -1, -2 ** 40)] == [0, 0, 0]
    sizes = [fn(n) for n in (1, 63, 64, 65, 255, 256, 257, 65_536, 65_537, 1_000_000, 2 ** 31 - 1)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0], sizes
    for n in (1, 257, 65_537, 1_000_000):
        assert fn(n) >= 4 * n + 4 * 4 * 256 + 4 * ((n + 255) // 256)      # the keys, four histograms, a counter per 256 rows
        assert fn(n) == fn(n)


def test_select_argument_rules():
    lib = L.load()
    n = 1000
    sb = lib.gsr_select_scratch_bytes(n)
    ok = dict(values=FAKE, N=n, C=48, k=500, drop=FAKE, keep=FAKE, meta=FAKE, scratch=FAKE, sb=sb)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gsr_select_smallest(a["values"], a["N"], a["C"], a["k"], a["drop"], a["keep"], a["meta"], a["scratch"], a["sb"], None)
    cases = [
        (dict(N=-1, k=0), "N must be"), (dict(N=2 ** 31, sb=2 ** 62), "N must be"),
        (dict(C=0), "C must be"), (dict(C=-3), "C must be"), (dict(C=L.GSR_SELECT_MAX_COLUMNS + 1), "C must be"),
        (dict(k=-1), "k must be"), (dict(k=n + 1), "k must be"), (dict(N=0, k=1), "k must be"),
        (dict(drop=None, keep=None), "both NULL"),
        (dict(meta=None), "meta is NULL"), (dict(meta=FAKE + 4), "not 8-byte aligned"), (dict(N=0, k=0, meta=None), "meta is NULL"),
        (dict(values=None), "values is NULL"), (dict(values=FAKE + 2), "not 4-byte aligned"),
        (dict(scratch=None), "scratch is NULL"), (dict(scratch=FAKE + 1), "not 4-byte aligned"),
        (dict(sb=sb - 1), "scratch is shorter"), (dict(sb=0), "scratch is shorter"),
    ]
    for bad, rule in cases:
        assert call(**bad) == -1, bad
        assert rule in _last_error(), (bad, _last_error())
    assert "gsr_select_smallest" in _last_error()
    for c in (1, 3, 12, 48, L.GSR_SELECT_MAX_COLUMNS):          # (these get past the column rule: the next refusal is another one)
        assert call(C=c, meta=None) == -1 and "meta is NULL" in _last_error()


def _table(*entries):
    t = (L.GsrMergeTensor * max(len(entries), 1))()
    for k, e in enumerate(entries):
        t[k].src_a, t[k].src_b, t[k].dst = e.get("src_a", FAKE), e.get("src_b", FAKE), e.get("dst", FAKE)
        t[k].row_bytes, t[k].kind = e.get("row_bytes", 12), e.get("kind", L.GSR_RESIZE_PARAM)
    return t


def test_merge_apply_argument_rules():
    lib = L.load()
    na, nb = 1000, 700
    pa, pb = lib.gsr_resize_plan_bytes(na), lib.gsr_resize_plan_bytes(nb)
    ok = dict(plan_a=FAKE, pa=pa, Na=na, nA=900, plan_b=FAKE, pb=pb, Nb=nb, nB=50, tensors=_table({}), count=1, meta=FAKE)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.gsr_merge_apply(a["plan_a"], a["pa"], a["Na"], a["nA"], a["plan_b"], a["pb"], a["Nb"], a["nB"], a["tensors"], a["count"],
                                   a["meta"], None)
    cases = [
        (dict(Na=-1), "must be in"), (dict(Nb=-1), "must be in"), (dict(Na=2 ** 31), "must be in"), (dict(Nb=2 ** 31), "must be in"),
        (dict(meta=None), "meta is NULL"), (dict(meta=FAKE + 4), "not 8-byte aligned"),
        (dict(count=19, tensors=_table(*[{}] * 19)), "at most"), (dict(count=-1), "at most"), (dict(tensors=None), "tensors is NULL"),
        (dict(nA=na + 1), "capacity"), (dict(nB=nb + 1), "capacity"), (dict(nA=-1), "capacity"), (dict(nB=-1), "capacity"),
        (dict(plan_a=None), "plan_a is NULL"), (dict(plan_b=None), "plan_b is NULL"),
        (dict(plan_a=FAKE + 2), "plan_a is NULL or not 4-byte aligned"), (dict(plan_b=FAKE + 2), "plan_b is NULL or not 4-byte aligned"),
        (dict(pa=pa - 1), "plan_a is shorter"), (dict(pa=0), "plan_a is shorter"), (dict(pb=pb - 1), "plan_b is shorter"),
        (dict(tensors=_table(dict(row_bytes=6))), "multiple of 4"), (dict(tensors=_table(dict(row_bytes=-4))), "multiple of 4"),
        (dict(tensors=_table(dict(row_bytes=2 ** 31))), "multiple of 4"),
        (dict(tensors=_table(dict(kind=2))), "kind is"), (dict(tensors=_table(dict(kind=-1))), "kind is"),
        (dict(tensors=_table(dict(dst=None))), "dst is NULL"), (dict(tensors=_table(dict(src_a=None))), "src_a is NULL"),
        (dict(tensors=_table(dict(src_b=None))), "src_b is NULL"),
        (dict(tensors=_table(dict(src_a=FAKE + 2))), "4-byte aligned"), (dict(tensors=_table(dict(src_b=FAKE + 1))), "4-byte aligned"),
        (dict(tensors=_table(dict(dst=FAKE + 3))), "4-byte aligned"),
        (dict(count=2, tensors=_table({}, dict(row_bytes=7))), "multiple of 4"),          # every entry is looked at
    ]
    for bad, rule in cases:
        assert call(**bad) == -1, bad
        assert rule in _last_error(), (bad, _last_error())
    # not errors, and nothing is launched: no tensors, nothing kept (then no plan is needed), empty models, only skipped entries
    for fine in (dict(count=0, tensors=None), dict(nA=0, nB=0), dict(nA=0, nB=0, plan_a=None, pa=0, plan_b=None, pb=0),
                 dict(Na=0, nA=0, Nb=0, nB=0, plan_a=None, pa=0, plan_b=None, pb=0),
                 dict(count=2, tensors=_table(dict(src_a=None, src_b=None, dst=None), dict(row_bytes=0)))):
        assert call(**fine) == 0, (fine, _last_error())


def test_op_schemas():
    ops = E.load()
    assert str(ops.select_smallest.default._schema) == "gsr::select_smallest(Tensor values, int k) -> (Tensor drop, Tensor keep_flags, Tensor meta)"
    assert str(ops.merge_apply.default._schema) == \
        ("gsr::merge_apply(Tensor plan_a, Tensor plan_b, Tensor(a!) meta, int Na, int nA, int Nb, int nB, Tensor[] src_a, Tensor[] src_b, "
         "int[] kinds, bool check=False) -> Tensor[]")


def _segment(n, coeffs, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = {"_xyz": (3,), "_features_dc": (1, 3), "_features_rest": (coeffs - 1, 3), "_opacity": (1,), "_scaling": (3,), "_rotation": (4,)}
    return {k: torch.randn((n,) + s, generator=g) for k, s in shapes.items()}


def test_route_keywords_defaults_and_refusals():
    for fn in (hier.prune_mask, hier.merge_send, hier.merge_recv, hier.merge_level, seg_mod.merge_segments):
        assert inspect.signature(fn).parameters["route"].default == "torch", fn
    imp = torch.rand(40, 48)
    a, b = _segment(40, 16, 1), _segment(30, 16, 2)
    ka, kb = torch.rand(40) < 0.5, torch.rand(30) < 0.5
    with pytest.raises(ValueError, match="route"):
        hier.prune_mask(imp, 0.5, route="device")
    with pytest.raises(ValueError, match="route"):
        seg_mod.merge_segments(a, b, ka, kb, route="Kernel")
    with pytest.raises(ValueError, match="route"):
        hier.merge_level(a, [], [], 0.5, route="hip", transport=seg_mod.LocalTransport(2))
    # the kernel routes have no CPU fallback, and say so before a device is touched
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hier.prune_mask(imp, 0.5, route="kernel")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg_mod.merge_segments(a, b, ka, kb, route="kernel")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.select_smallest(imp, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.merge_apply(torch.zeros(320, dtype=torch.int32), torch.zeros(8, dtype=torch.int64), 4, 4, torch.zeros(320, dtype=torch.int32), 4, 4,
                      [torch.zeros(4, 3)], [torch.zeros(4, 3)])
    # the torch routes still take the keyword and are what they were
    assert torch.equal(hier.prune_mask(imp, 0.5, route="torch"), hier.prune_mask(imp, 0.5))
    assert hier.merge_level(a, [], [], 0.5, route="kernel", transport=seg_mod.LocalTransport(2)) is a      # (idle at this level)


def test_run_segments_has_the_flag_and_the_default():
    rs = importlib.import_module("3dgs_hierarchical_training_amd.run_segments")
    assert rs.HTConfig().merge_route == "torch"
    src = inspect.getsource(rs)
    assert '"--merge-route", choices=("torch", "kernel"), default="torch"' in src
    assert "merge_route=a.merge_route" in src and src.count("route=self.cfg.merge_route") == 2      # reaches merge_send and merge_recv


def _torch_mask(values, k):
    """hierarchy.prune_mask's statements at a given k."""
    score = torch.from_numpy(values).amax(-1).reshape(-1)
    mask = torch.zeros_like(score, dtype=torch.bool)
    if k > 0:
        mask[torch.topk(score, k, largest=False).indices] = True
    return mask.numpy()


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000, 65_537])
def test_with_distinct_scores_the_oracle_is_topk(n):
    """Distinct scores, among them a -0 and (from four rows on) a NaN row, a +inf row and a -inf row: torch.topk's mask is defined, and it is
    the oracle's, at C = 1 / 3 / 48 and k = 0 / 1 / N // 2 / N - 1 / N."""
    rng = np.random.default_rng(n)
    score = MC.score_patterns(n)["distinct"][0].copy()
    score[score == 0] = -0.0
    if n >= 4:
        special = rng.choice(np.flatnonzero(score != 0), 3, replace=False)
        score[special] = [np.nan, np.inf, -np.inf]
    for c in (1, 3, 48):
        values = MC.spread(score, c, rng)
        key = MC.keys_of(values)
        assert len(np.unique(key)) == n
        for k in MC.ks_of(n):
            o = MC.select_oracle(values, k, key)
            assert np.array_equal(o["drop"], _torch_mask(values, k)), (c, k)
            assert int(o["drop"].sum()) == k and np.array_equal(o["keep_flags"], (~o["drop"]).astype(np.uint8))
            assert o["meta"][0] == k and o["meta"][4] == (1 if n >= 4 else 0) and o["meta"][5:] == [0, 0, 0]
            if k > 0:
                assert o["meta"][1] == k - 1 and o["meta"][2] == 1
    assert np.array_equal(_torch_mask(values, n // 2), hier.prune_mask(torch.from_numpy(values), 0.5).numpy())


def test_with_ties_the_oracle_takes_topks_values_and_the_first_rows():
    n = 5000
    rng = np.random.default_rng(3)
    score = (rng.permutation(n) + 1).astype(np.float32)
    score[rng.random(n) < 0.6] = 0.0
    zeros = np.flatnonzero(score == 0)
    for c in (1, 48):
        values = MC.spread(score, c, rng)
        for k in (1, len(zeros) // 2, len(zeros) - 1, len(zeros), len(zeros) + 1, n // 2, n - 1):
            o = MC.select_oracle(values, k)
            want = torch.topk(torch.from_numpy(score), k, largest=False).values.numpy()
            assert np.array_equal(np.sort(score[o["drop"]]), np.sort(want)), k
            taken = np.flatnonzero(o["drop"] & (score == 0))
            assert np.array_equal(taken, zeros[:min(k, len(zeros))]), k
            assert o["meta"][:4] == ([k, 0, len(zeros), 0x80000000] if k <= len(zeros) else [k, k - 1, 1, o["meta"][3]])


def test_the_key_orders_like_topk():
    """-inf < negatives < -0 = +0 < denormals < positives < +inf < NaN, and the key is the maximum's key."""
    f = np.array([-np.inf, -3.0, -1e-40, -0.0, 0.0, 1e-40, 2.0, np.inf, np.nan], np.float32)
    key = MC.keys_of(f[:, None])
    assert key[3] == key[4] == 0x80000000 and key[-1] == MC.NAN_KEY and key[0] == 0x007FFFFF
    rest = np.delete(key, 3)
    assert np.all(rest[1:] > rest[:-1])
    assert MC.keys_of(np.array([[1.0, np.nan, 5.0], [-0.0, -1.0, -np.inf]], np.float32)).tolist() == [MC.NAN_KEY, 0x80000000]
    assert MC.select_oracle(np.zeros((0, 3), np.float32), 0)["meta"] == [0] * 8


@pytest.mark.parametrize("with_transform", [False, True])
def test_the_layout_oracle_is_the_torch_route(with_transform):
    a, b = _segment(300, 16, 5), _segment(257, 16, 6)
    T = None
    if with_transform:
        T = torch.eye(4)
        T[:3, :3] = torch.linalg.qr(torch.randn(3, 3, generator=torch.Generator().manual_seed(1)))[0]
        T[:3, 3] = torch.tensor([0.3, -1.0, 2.0])
        T[3] = torch.tensor([0.01, -0.02, 0.03, 1.1])
    for name_a, ka in MC.keep_patterns(300).items():
        for name_b, kb in MC.keep_patterns(257).items():
            out = seg_mod.merge_segments(a, b, torch.from_numpy(ka), torch.from_numpy(kb), T)
            moved = dict(b)
            if T is not None:
                xyz = b["_xyz"]
                moved["_xyz"] = (xyz @ T[:3, :3].t() + T[:3, 3]) / (xyz @ T[3, :3] + T[3, 3]).unsqueeze(1)
            for key in seg_mod.SEGMENT_KEYS:
                want = MC.merged_oracle(a[key].numpy(), ka, moved[key].numpy(), kb)
                assert np.array_equal(out[key].numpy(), want), (name_a, name_b, key)
    m = MC.merged_oracle(a["_xyz"].numpy(), ka, b["_xyz"].numpy(), kb, MC.MOMENT)
    assert np.array_equal(m[:int(ka.sum())], a["_xyz"].numpy()[ka]) and not m[int(ka.sum()):].any() and m.shape[0] == int(ka.sum() + kb.sum())
