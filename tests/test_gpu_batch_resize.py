"""GPU: resizing the models of a batch (include/gsr.h version 122; csrc/resize_kernels.hip, resize.py, batched.py, densify.py) -- the batched
plan and apply against the numpy oracle of tests/batch_resize_common.py, `BatchedGaussianParams.resize_models` / `prune_models` against
every model resized alone, `BatchedDensifier` against one `Densifier` per model, a training trajectory of a batch against its models
trained alone, and the leaf phase of a small local run with and without `leaf_batch`.

The kernels decide a layout with integer scans and copy bytes, and every float of a densification comes from the single-model statements at
the single model's shapes, so everything that is not an image is compared with torch.equal; images follow the rule of
tests/test_gpu_batched.py (equal under `deterministic_backward`, `parity.same_accumulation` on the default accumulation)."""
import contextlib
import ctypes as C
import importlib
import warnings

import numpy as np
import pytest
import torch

import batch_resize_common as BC
import parity
import resize_common as RC

pytestmark = pytest.mark.gpu

L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
R = importlib.import_module("3dgs_hierarchical_training_amd.resize")
dm = importlib.import_module("3dgs_hierarchical_training_amd.densify")
ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
bt = importlib.import_module("3dgs_hierarchical_training_amd.batched")
syn = importlib.import_module("3dgs_hierarchical_training_amd.synthetic")

NAMES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
SEGMENTS = (("rows_a", L.GSR_RESIZE_PLAN_ROWS_A, 0), ("rows_b", L.GSR_RESIZE_PLAN_ROWS_B, 1), ("rows_c", L.GSR_RESIZE_PLAN_ROWS_C, 2),
            ("rank_c", L.GSR_RESIZE_PLAN_RANK_C, 2), ("split_rows", L.GSR_RESIZE_PLAN_SPLIT_ROWS, 3))
PAD = 64      # rows of NaN in front of and behind every source tensor
COUNTS = [(1, 127), (128, 129), (255, 256, 257), (129, 4000, 127, 6000, 2048), tuple(1 + (b * 299) // 15 for b in range(16))]


def _dev():
    return torch.device("cuda:0")


def _shapes(coeffs):
    return {"xyz": (3,), "f_dc": (1, 3), "f_rest": (coeffs - 1, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,)}


def _guarded(n, shape, gen, dev):
    """[n, *shape] of random values as a contiguous view into a buffer whose other rows are NaN: a read outside the rows in use shows."""
    buf = torch.full((n + 2 * PAD,) + shape, float("nan"), device=dev)
    buf[PAD: PAD + n] = torch.randint(-1000, 1000, (n,) + shape, generator=gen).float().to(dev) + 0.5
    return buf[PAD: PAD + n]


def _table(n, coeffs, moments, n_child, seed, dev):
    """(src, kinds, child, pad) of the six groups (+ their twelve moments) over a store of n rows."""
    gen = torch.Generator().manual_seed(seed)
    src, kinds, child, pad = [], [], [], []
    for name, shape in _shapes(coeffs).items():
        sourced = name in ("xyz", "scaling")
        src.append(_guarded(n, shape, gen, dev)); kinds.append(RC.CHILD_SOURCED if sourced else RC.PARAM)
        child.append(_guarded(n_child, shape, gen, dev) if sourced else None)
        pad.append(_guarded(1, shape, gen, dev) if name != "rotation" else None)          # (one group with the NULL pad: zeros)
        if moments:
            for _ in range(2):
                src.append(_guarded(n, shape, gen, dev)); kinds.append(RC.MOMENT); child.append(None); pad.append(None)
    return src, kinds, child, pad


@contextlib.contextmanager
def _sync_warnings():
    """Records torch's warnings about host synchronisations (set_sync_debug_mode("warn")); the mode's own "prototype feature" warning is
    kept out of the record."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            yield rec
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _waits(rec):
    """torch's synchronisation warnings among the recorded ones."""
    return sum("synchroniz" in str(w.message).lower() for w in rec)


def _where(rec):
    return [(w.filename.rsplit("/", 1)[-1], w.lineno) for w in rec if "synchroniz" in str(w.message).lower()]


def _np(t):
    return None if t is None else t.cpu().numpy()


def _check_plan(plan, meta, first_block, bl):
    assert meta.cpu().tolist() == bl["meta"], (meta.cpu().tolist(), bl["meta"])
    n = BC.BLOCK * first_block[-1]
    assert plan.shape == (5 * n,) and R.plan_stride(n) == n
    host = plan.cpu().numpy().astype(np.int64)
    for b, m in enumerate(bl["models"]):
        for key, which, count in SEGMENTS:
            at = which * n + BC.BLOCK * first_block[b]
            assert np.array_equal(host[at: at + m["meta"][count]], m[key]), (b, key)


def _plan_and_apply(per_model_flags, counts, coeffs, moments, seed, dev, padding=0xFF):
    fb = BC.first_block_of(counts)
    f = BC.store_flags(per_model_flags, fb, padding)
    bl = BC.batch_layout_oracle(f, fb, counts)
    plan, meta = R.resize_plan_batched(torch.from_numpy(f).to(dev), fb, counts)
    _check_plan(plan, meta, fb, bl)
    rows = R.read_counts_batched(meta)
    assert [r[:4] for r in rows] == [m["meta"] for m in bl["models"]] and all(r[4] == 0 for r in rows)
    src, kinds, child, pad = _table(BC.BLOCK * fb[-1], coeffs, moments, BC.child_bases(bl)[1], seed, dev)
    out, nfb = R.resize_apply_batched(plan, meta, fb, counts, rows, src, kinds, child, pad, check=True)
    assert nfb == bl["new_first_block"]
    return bl, fb, plan, meta, src, kinds, child, pad, out


def _assert_applied(bl, fb, counts, src, kinds, child, pad, out, what):
    for j, (o, s, k, c, p) in enumerate(zip(out, src, kinds, child, pad)):
        want = BC.batch_apply_oracle(bl, fb, counts, _np(s), k, _np(c), _np(p))
        assert tuple(o.shape) == want.shape and o.dtype == s.dtype and o.is_contiguous(), (what, j)
        assert np.array_equal(_np(o).view(np.int32), want.view(np.int32)), (what, j)


@pytest.mark.parametrize("counts", COUNTS, ids=lambda c: "x".join(str(v) for v in c) if len(c) < 6 else f"{len(c)}models")
def test_plan_and_apply_match_the_oracle(counts):
    """Models that end and start around the 128-row block and the 256-row tile of the single-model plan, models of many blocks beside models
    of one, and sixteen models of 1 to 300 rows.  The eleven flag patterns in every model at once, then rotated over the models, then one
    model with nothing kept beside one that is cloned whole; the flag bytes of padding rows are 0xFF; row widths of 16, 4 and 1 stored
    coefficients, with and without moments (they rotate over the patterns); sources fenced with NaN."""
    dev = _dev()
    pats = [RC.flag_patterns(n, seed=b) for b, n in enumerate(counts)]
    names = list(pats[0])
    assert len(names) == 11
    combos = [(c, m) for c in (16, 4, 1) for m in (True, False)]
    cases = []
    for k, name in enumerate(names):
        cases.append((name, [p[name] for p in pats], combos[k % 6]))
        cases.append((name + " rotated", [p[names[(k + b) % 11]] for b, p in enumerate(pats)], combos[(k + 3) % 6]))
    cases.append(("nothing beside all clone", [p["none" if b % 2 == 0 else "all_clone"] for b, p in enumerate(pats)], combos[0]))
    for k, (what, per_model, (coeffs, moments)) in enumerate(cases):
        bl, fb, plan, meta, src, kinds, child, pad, out = _plan_and_apply(per_model, counts, coeffs, moments, 7 * k + coeffs, dev)
        assert len(out) == len(src) == (18 if moments else 6)
        _assert_applied(bl, fb, counts, src, kinds, child, pad, out, what)
        assert not meta[:, L.GSR_RESIZE_META_STATUS].any()
    bl = BC.batch_layout_oracle(BC.store_flags([p["none"] for p in pats], BC.first_block_of(counts)), BC.first_block_of(counts), counts)
    assert bl["new_first_block"] == list(range(len(counts) + 1)), "a model that loses every row keeps one block"
    print(f"[batch resize {counts if len(counts) < 6 else '16 models'}] {len(cases)} plan + apply cases")


def test_padding_flags_are_ignored_whatever_they_hold():
    dev = _dev()
    counts = (129, 300, 1)
    per_model = [RC.flag_patterns(n, seed=b)["any_byte"] for b, n in enumerate(counts)]
    a = _plan_and_apply(per_model, counts, 4, True, 3, dev, padding=0xFF)
    b = _plan_and_apply(per_model, counts, 4, True, 3, dev, padding=0x00)
    assert torch.equal(a[3], b[3])
    for x, y in zip(a[8], b[8]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_a_repeat_is_bit_identical():
    dev = _dev()
    counts = COUNTS[3]
    per_model = [RC.flag_patterns(n, seed=b)["random_p5"] for b, n in enumerate(counts)]
    a = _plan_and_apply(per_model, counts, 16, True, 3, dev)
    b = _plan_and_apply(per_model, counts, 16, True, 3, dev)
    n = BC.BLOCK * a[1][-1]
    for m, lo in zip(a[0]["models"], a[1]):
        for key, which, count in SEGMENTS:
            at = which * n + BC.BLOCK * lo
            assert torch.equal(a[2][at: at + m["meta"][count]], b[2][at: at + m["meta"][count]]), key
    assert torch.equal(a[3], b[3])
    for x, y in zip(a[8], b[8]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_the_ctypes_route_gives_the_same_bytes(monkeypatch):
    dev = _dev()
    for counts, pattern, coeffs in ((COUNTS[2], "random_p5", 16), (COUNTS[0], "alternating", 1), (COUNTS[4], "long_runs", 4)):
        per_model = [RC.flag_patterns(n, seed=b)[pattern] for b, n in enumerate(counts)]
        monkeypatch.delenv("GSR_BINDING", raising=False)
        ext = _plan_and_apply(per_model, counts, coeffs, True, 11, dev)
        monkeypatch.setenv("GSR_BINDING", "ctypes")
        assert R.E.use_ctypes()
        cty = _plan_and_apply(per_model, counts, coeffs, True, 11, dev)
        monkeypatch.delenv("GSR_BINDING", raising=False)
        assert torch.equal(ext[3], cty[3])
        for x, y in zip(ext[8], cty[8]):
            assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_guard_bytes_around_every_output_stay():
    """The C ABI called directly, with every destination a view into a larger buffer of a guard pattern: the launch writes the rows of the
    new store and nothing around them."""
    dev = _dev()
    lib = L.load()
    counts = COUNTS[3]
    fb = BC.first_block_of(counts)
    per_model = [RC.flag_patterns(n, seed=b)["random_p5"] for b, n in enumerate(counts)]
    f = BC.store_flags(per_model, fb)
    bl = BC.batch_layout_oracle(f, fb, counts)
    plan, meta = R.resize_plan_batched(torch.from_numpy(f).to(dev), fb, counts)
    rows = R.read_counts_batched(meta)
    assert [r[:4] for r in rows] == [m["meta"] for m in bl["models"]]      # (the buffers below are sized by the oracle)
    n_new = BC.BLOCK * bl["new_first_block"][-1]
    src, kinds, child, pad = _table(BC.BLOCK * fb[-1], 4, True, BC.child_bases(bl)[1], 2, dev)
    guard = 0x5A5A5A5A
    bufs, dst = [], []
    for s in src:
        buf = torch.full((n_new + 2 * PAD,) + tuple(s.shape[1:]), 0, dtype=torch.int32, device=dev).fill_(guard)
        bufs.append(buf)
        dst.append(buf[PAD: PAD + n_new])
    table = (L.GsrResizeBatchTensor * len(src))()
    for k, (s, d) in enumerate(zip(src, dst)):
        table[k].src, table[k].dst = s.data_ptr(), d.data_ptr()
        table[k].child = child[k].data_ptr() if child[k] is not None and child[k].numel() else None
        table[k].pad = pad[k].data_ptr() if pad[k] is not None else None
        table[k].row_bytes, table[k].kind = 4 * int(np.prod(s.shape[1:])), kinds[k]
    batch = L.GsrResizeBatch()
    batch.B = len(counts)
    for b, v in enumerate(fb):
        batch.first_block[b] = v
    for b, v in enumerate(counts):
        batch.counts[b] = v
    c4 = (C.c_int64 * (4 * len(counts)))(*[v for r in rows for v in r[:4]])
    nfb = (C.c_int64 * (len(counts) + 1))(*bl["new_first_block"])
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.gsr_resize_apply_batched(plan.data_ptr(), plan.numel() * 4, C.byref(batch), c4, nfb, table, len(src), meta.data_ptr(), C.c_void_p(stream))
    assert rc == 0, lib.gsr_last_error()
    torch.cuda.synchronize()
    for k, (buf, d, s) in enumerate(zip(bufs, dst, src)):
        assert bool((buf[:PAD] == guard).all()) and bool((buf[PAD + n_new:] == guard).all()), k
        want = BC.batch_apply_oracle(bl, fb, counts, _np(s), kinds[k], _np(child[k]), _np(pad[k]))
        assert np.array_equal(_np(d), want.view(np.int32).reshape(d.shape)), k
    assert not meta[:, L.GSR_RESIZE_META_STATUS].any()


def test_a_corrupted_plan_is_a_status_in_its_models_row_not_a_fault():
    """One entry of model 1's lists overwritten from the host -- with a row of ANOTHER model (in range for the store, out of range for the
    model), with -1 and with 2^31 - 1: k_resize_apply_batched compares every row number it reads with the model's own rows before it forms
    an address (the `srow >= row_lo && srow < row_hi` / `rank < nSplit` tests are the only paths to a load), so the row is written as
    zeros, the status word of model 1 alone is raised, and the checked call raises."""
    dev = _dev()
    counts = (300, 1000, 200)
    fb = BC.first_block_of(counts)
    per_model = [RC.flag_patterns(n, seed=b)["random_p5"] for b, n in enumerate(counts)]
    f = BC.store_flags(per_model, fb)
    bl = BC.batch_layout_oracle(f, fb, counts)
    nA, nB, nC, nS = bl["models"][1]["meta"]
    assert nA > 3 and nB > 2 and nC > 2
    n = BC.BLOCK * fb[-1]
    base, new_lo = BC.BLOCK * fb[1], BC.BLOCK * bl["new_first_block"][1]
    spots = {"a row of A": (L.GSR_RESIZE_PLAN_ROWS_A * n + base + 3, 3, 5),                       # row 5 is model 0's
             "a row of B": (L.GSR_RESIZE_PLAN_ROWS_B * n + base + 1, nA + 1, -1),
             "a row of C": (L.GSR_RESIZE_PLAN_ROWS_C * n + base + 2, nA + nB + 2, 2 ** 31 - 1),
             "the row behind the model": (L.GSR_RESIZE_PLAN_ROWS_A * n + base, 0, base + counts[1])}      # a padding row of model 1
    for what, (entry, row, value) in spots.items():
        plan, meta = R.resize_plan_batched(torch.from_numpy(f).to(dev), fb, counts)
        rows = R.read_counts_batched(meta)
        plan[entry] = value
        src, kinds, child, pad = _table(n, 4, True, BC.child_bases(bl)[1], 5, dev)
        kinds = [RC.PARAM if k == RC.CHILD_SOURCED else k for k in kinds]      # (so that segment C reads its rows from the plan)
        out, _ = R.resize_apply_batched(plan, meta, fb, counts, rows, src, kinds, child, pad)
        assert meta[:, L.GSR_RESIZE_META_STATUS].cpu().tolist() == [0, 1, 0], what
        other = torch.ones(BC.BLOCK * bl["new_first_block"][-1], dtype=torch.bool, device=dev)
        other[new_lo + row] = False
        if what == "a row of C":
            other[new_lo + row + nC] = False                                   # copy 1 reads the same entry
        for o, s, k, c, p in zip(out, src, kinds, child, pad):
            want = torch.from_numpy(BC.batch_apply_oracle(bl, fb, counts, _np(s), k, _np(c), _np(p))).to(dev)
            assert torch.equal(o[other], want[other]), what
            if not (k == RC.MOMENT and row >= nA):
                assert not o[new_lo + row].view(torch.int32).any(), what
        with pytest.raises(RuntimeError, match="outside"):
            R.resize_apply_batched(plan, meta, fb, counts, rows, src, kinds, child, pad, check=True)
    # a split rank out of range, for the tensors whose children come from the caller
    plan, meta = R.resize_plan_batched(torch.from_numpy(f).to(dev), fb, counts)
    rows = R.read_counts_batched(meta)
    plan[L.GSR_RESIZE_PLAN_RANK_C * n + base] = nS
    src, kinds, child, pad = _table(n, 4, False, BC.child_bases(bl)[1], 5, dev)
    out, _ = R.resize_apply_batched(plan, meta, fb, counts, rows, src, kinds, child, pad)
    assert meta[:, L.GSR_RESIZE_META_STATUS].cpu().tolist() == [0, 1, 0]
    assert not out[0][new_lo + nA + nB].view(torch.int32).any() and not out[0][new_lo + nA + nB + nC].view(torch.int32).any()
    want = BC.batch_apply_oracle(bl, fb, counts, _np(src[1]), kinds[1], _np(child[1]), _np(pad[1]))
    assert np.array_equal(_np(out[1]), want)


# ---- resize_models / prune_models against every model resized alone ------------------------------------------------------------------

def _scenes(counts, degree=3, seed=41, size=(64, 64)):
    return [syn.make_scene(n, size[0], size[1], sh_degree=degree, seed=seed + b) for b, n in enumerate(counts)]


def _step_random(p, seed, skip=()):
    """One optimizer step on random gradients (non-zero moments, step = 1); the padding rows of a batch get the zero gradient training
    gives them."""
    gen = torch.Generator().manual_seed(seed)
    own = torch.zeros(p.num_points, dtype=torch.bool)
    for b in range(p.num_models):
        own[p.model_rows(b)] = True
    for g in p.optimizer.param_groups:
        if g["name"] not in skip:
            x = g["params"][0]
            x.grad = torch.where(own.reshape((-1,) + (1,) * (x.dim() - 1)), torch.randn(x.shape, generator=gen), torch.zeros(())).to(_dev())
    p.optimizer.step()
    p.optimizer.zero_grad(set_to_none=True)


def _batch_and_singles(counts, optimizer="hip", degree=3, skip=(), seed=41):
    """A stepped batch, and per model a single store that holds the batch's model bit for bit (parameters, moments, step counts)."""
    dev = _dev()
    scenes = _scenes(counts, degree, seed)
    batch = bt.BatchedGaussianParams(scenes, dev, optimizer=optimizer)
    _step_random(batch, seed, skip)
    return batch, _singles_of(batch, scenes, optimizer)


def _singles_of(batch, scenes, optimizer="hip"):
    dev = _dev()
    singles = []
    for b, sc in enumerate(scenes):
        p = ts.GaussianParams.from_raw({k: v.clone() for k, v in batch.model_raw(b).items()}, dev, sh_degree=batch.active_sh_degree,
                                       optimizer=optimizer)
        for g, gb in zip(p.optimizer.param_groups, batch.optimizer.param_groups):
            g["lr"] = gb["lr"]
            st = batch.optimizer.state.get(gb["params"][0])
            if st is not None:
                new = {k: (v[batch.model_rows(b)].clone() if k in ("exp_avg", "exp_avg_sq") else (v.clone() if torch.is_tensor(v) else v))
                       for k, v in st.items()}
                p.optimizer.state[g["params"][0]] = new
        singles.append(p)
    return singles


def _assert_batch_equals_singles(batch, singles, fresh_pad, what):
    assert batch.counts == [p.num_points for p in singles], (what, batch.counts)
    assert batch.first_block == BC.first_block_of([max(1, n) for n in batch.counts]) and batch.num_points == BC.BLOCK * batch.first_block[-1], what
    own = torch.zeros(batch.num_points, dtype=torch.bool, device=_dev())
    for b, p in enumerate(singles):
        r = batch.model_rows(b)
        own[r] = True
        if not p.num_points:          # (a model without rows: every row of its block is padding, checked below)
            continue
        for gb, gs in zip(batch.optimizer.param_groups, p.optimizer.param_groups):
            x, y = gb["params"][0], gs["params"][0]
            name = gb["name"]
            assert x is getattr(batch, batch._GROUP_ATTR[name]) and x.requires_grad and x.is_leaf and x.is_contiguous(), (what, name)
            assert torch.equal(x.detach()[r], y.detach()), (what, b, name)
            sb, ss = batch.optimizer.state.get(x), p.optimizer.state.get(y)
            assert (sb is None) == (ss is None), (what, b, name)
            if sb is not None:
                if p.num_points:          # (a model without rows is not stepped alone: there is nothing to step)
                    assert int(sb["step"]) == int(ss["step"]), (what, b, name)
                for k in ("exp_avg", "exp_avg_sq"):
                    assert sb[k].shape == x.shape and torch.equal(sb[k][r], ss[k]), (what, b, name, k)
    # every other row is padding: the row a freshly built batch has, and zero moments
    for gb in batch.optimizer.param_groups:
        x = gb["params"][0]
        want = fresh_pad[batch._GROUP_ATTR[gb["name"]]]
        assert torch.equal(x.detach()[~own], want.expand((int((~own).sum()),) + tuple(x.shape[1:]))), (what, gb["name"], "padding")
        sb = batch.optimizer.state.get(x)
        if sb is not None:
            assert not sb["exp_avg"][~own].view(torch.int32).any() and not sb["exp_avg_sq"][~own].view(torch.int32).any(), (what, gb["name"])


def _fresh_pad(degree=3):
    """The padding row of a freshly built batch: a one-row model padded to a block, row 1."""
    fresh = bt.BatchedGaussianParams(_scenes((1, 1), degree), _dev())
    return {k: getattr(fresh, k).detach()[1:2].clone() for k in NAMES}


def _flags_for(batch, per_model):
    return torch.from_numpy(BC.store_flags(per_model, batch.first_block)).to(_dev())


@pytest.mark.parametrize("optimizer,skip,degree", [("hip", (), 3), ("torch", ("f_rest",), 3), ("hip", (), 0)])
def test_resize_models_equals_every_model_resized_alone(optimizer, skip, degree):
    """Four models: one grows across a 128-row boundary (120 rows, 20 cloned -> 140), one shrinks across one (130 -> 100), one goes to
    zero rows (it keeps one block of padding), one does not change; then a second resize on the result (the model of zero rows stays)."""
    dev = _dev()
    counts = (120, 130, 77, 256)
    batch, singles = _batch_and_singles(counts, optimizer, degree, skip)
    fresh = _fresh_pad(degree)
    _assert_batch_equals_singles(batch, singles, fresh, "before")
    k = np.full
    rounds = [
        [np.concatenate((k(20, RC.KEEP | RC.CLONE, np.uint8), k(100, RC.KEEP, np.uint8))),
         np.concatenate((k(100, RC.KEEP, np.uint8), k(30, 0, np.uint8))), k(77, 0, np.uint8), k(256, RC.KEEP, np.uint8)],
        None,      # filled below: a mixed pattern on the result of the first round
    ]
    for round_ in range(2):
        if round_ == 1:
            rounds[1] = [RC.flag_patterns(n, seed=b)["random_p5"] if n else np.zeros(0, np.uint8) for b, n in enumerate(batch.counts)]
        per_model = rounds[round_]
        flags = _flags_for(batch, per_model)
        bl = BC.batch_layout_oracle(flags.cpu().numpy(), batch.first_block, batch.counts)
        n_child = BC.child_bases(bl)[1]
        gen = torch.Generator().manual_seed(5 + round_)
        children = None
        if n_child:
            children = {"xyz": torch.randn(n_child, 3, generator=gen).to(dev), "scaling": torch.randn(n_child, 3, generator=gen).to(dev)}
        batch._prepared, batch._screenspace_zero = object(), object()
        steps = [int(batch.optimizer.state[g["params"][0]]["step"]) for g in batch.optimizer.param_groups if g["params"][0] in batch.optimizer.state]
        torch.cuda.synchronize()
        with _sync_warnings() as rec:
            got = batch.resize_models(flags, children=children)
        assert _waits(rec) <= 1, ("one host wait per call", _where(rec))
        assert [list(c) for c in got] == [m["meta"] for m in bl["models"]]
        assert batch._prepared is None and batch._screenspace_zero is None
        assert steps == [int(batch.optimizer.state[g["params"][0]]["step"]) for g in batch.optimizer.param_groups if g["params"][0] in batch.optimizer.state]
        bases, _ = BC.child_bases(bl)
        for b, p in enumerate(singles):
            nS = bl["models"][b]["meta"][3]
            ch = None if children is None else {key: v[bases[b]: bases[b] + 2 * nS] for key, v in children.items()}
            if p.num_points:
                p.resize_by_flags(torch.from_numpy(per_model[b]).to(dev), children=ch)
        _assert_batch_equals_singles(batch, singles, fresh, f"round {round_}")
        if round_ == 0:
            assert batch.counts == [140, 100, 0, 256] and batch.first_block == [0, 2, 3, 4, 6]
    # the resized batch still trains, model by model as alone
    _step_random_rows(batch, singles)
    _assert_batch_equals_singles(batch, singles, fresh, "after a step")


def _step_random_rows(batch, singles):
    """One optimizer step with the same gradient on a model's rows in the batch and alone (zero on padding rows)."""
    gen = torch.Generator().manual_seed(99)
    for gi, gb in enumerate(batch.optimizer.param_groups):
        x = gb["params"][0]
        x.grad = torch.zeros_like(x)
        for b, p in enumerate(singles):
            y = p.optimizer.param_groups[gi]["params"][0]
            g = torch.randn(y.shape, generator=gen).to(_dev())
            y.grad = g
            x.grad[batch.model_rows(b)] = g
    for p in [batch] + [s for s in singles if s.num_points]:
        p.optimizer.step()
        p.optimizer.zero_grad(set_to_none=True)


def test_prune_models_equals_prune_points_per_model():
    dev = _dev()
    counts = (129, 500, 1, 128)
    batch, singles = _batch_and_singles(counts)
    fresh = _fresh_pad()
    gen = torch.Generator().manual_seed(2)
    for round_, p_drop in enumerate((0.5, 0.05, 0.0)):
        mask = (torch.rand(batch.num_points, generator=gen) < p_drop).to(dev)
        if round_ == 0:
            mask[batch.model_rows(2)] = True          # the one-row model loses its row
        rows = [batch.model_rows(b) for b in range(4)]
        torch.cuda.synchronize()
        with _sync_warnings() as rec:
            batch.prune_models(mask)
        assert _waits(rec) <= 1, ("one host wait per call", _where(rec))
        for p, r in zip(singles, rows):
            if p.num_points:
                p.prune_points(mask[r], route="kernel")
        _assert_batch_equals_singles(batch, singles, fresh, f"prune round {round_}")
    assert batch.counts[2] == 0 and batch.first_block[3] - batch.first_block[2] == 1


# ---- BatchedDensifier against one Densifier(route="torch") per model ------------------------------------------------------------------

SEEDS = (13, 14, 15)
DENSIFY_COUNTS = (2000, 1950, 1000)


def _densifier_batch(extent=5.0, hot=0.3, seed=13, **cfg):
    """A stepped batch with its BatchedDensifier, and per model the same model alone with a torch-route Densifier; the same statistics."""
    dev = _dev()
    batch, singles = _batch_and_singles(DENSIFY_COUNTS)
    c = dm.DensifyConfig(**cfg)
    db = dm.BatchedDensifier(batch, extent, c, seeds=SEEDS)
    das = [dm.Densifier(p, extent, c, seed=SEEDS[b]) for b, p in enumerate(singles)]
    gen = torch.Generator().manual_seed(seed)
    n = batch.num_points
    accum = (torch.rand(n, 1, generator=gen) < hot).float() * 2.0
    denom = (torch.rand(n, 1, generator=gen) < 0.9).float()                   # (0 / 0 = NaN -> 0 and 2 / 0 = inf on some rows)
    radii = torch.rand(n, generator=gen) * 50.0
    own = torch.zeros(n, dtype=torch.bool)
    for b in range(batch.num_models):
        own[batch.model_rows(b)] = True
    accum[~own], denom[~own], radii[~own] = 0.0, 0.0, 0.0                     # a padding row is never seen
    db.xyz_gradient_accum, db.denom, db.max_radii2D = accum.to(dev), denom.to(dev), radii.to(dev)
    for b, d in enumerate(das):
        r = batch.model_rows(b)
        d.xyz_gradient_accum, d.denom, d.max_radii2D = accum[r].to(dev), denom[r].to(dev), radii[r].to(dev)
    return batch, singles, db, das


def _assert_same_densifiers(batch, singles, db, das, fresh, what):
    _assert_batch_equals_singles(batch, singles, fresh, what)
    for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
        t = getattr(db, k)
        assert t.shape[0] == batch.num_points and not t.any(), (what, k)
        for d, p in zip(das, singles):
            assert getattr(d, k).shape[0] == p.num_points and not getattr(d, k).any(), (what, k)
    for b, d in enumerate(das):
        assert torch.equal(db.gens[b].get_state(), d.gen.get_state()), (what, b, "generator state")


def _median_scale(p):
    return float(p.get_scaling.detach().max(dim=1).values.median())


def test_batched_densifier_equals_one_densifier_per_model_in_every_regime():
    fresh = _fresh_pad()
    seen = {}

    def run(what, extent, args, expect, hot=0.3, **cfg):
        batch, singles, db, das = _densifier_batch(extent=extent, hot=hot, **cfg)
        n0 = list(batch.counts)
        before = [getattr(batch, k) for k in NAMES]
        gens_before = [g.get_state() for g in db.gens]
        flags, clone, _ = db._resize_flags(*args)
        bl = BC.batch_layout_oracle(flags.cpu().numpy(), batch.first_block, batch.counts)
        n_clone = [int(clone[batch.model_rows(b)].sum()) for b in range(3)]
        for d in das:
            d.densify_and_prune(*args)
        db.densify_and_prune(*args)
        _assert_same_densifiers(batch, singles, db, das, fresh, what)
        metas = [m["meta"] for m in bl["models"]]
        seen[what] = (n0, list(batch.counts), metas, n_clone)
        untouched = [torch.equal(a, g.get_state()) for a, g in zip(gens_before, db.gens)]
        expect(batch, metas, n_clone, before, untouched)

    def nothing(p, metas, n_clone, before, untouched):
        assert all(m == [n, 0, 0, 0] for m, n in zip(metas, DENSIFY_COUNTS)) and all(untouched)
        assert all(getattr(p, k) is b for k, b in zip(NAMES, before)), "no tensor is replaced"
    run("nothing selected", 5.0, (0.5, 0.0, None), nothing, hot=0.0)

    def only_clones(p, metas, n_clone, before, untouched):
        assert all(m[0] == n and m[1] == c > 50 and m[3] == 0 for m, n, c in zip(metas, DENSIFY_COUNTS, n_clone)) and all(untouched)
        assert p.counts == [n + c for n, c in zip(DENSIFY_COUNTS, n_clone)]
    run("only clones", 1e9, (0.5, 0.0, None), only_clones)

    def only_splits(p, metas, n_clone, before, untouched):
        assert n_clone == [0, 0, 0] and all(m[1] == 0 and m[2] == m[3] > 50 for m in metas) and not any(untouched)
        assert p.counts == [n + m[3] for n, m in zip(DENSIFY_COUNTS, metas)]
    run("only splits", 1e-9, (0.5, 0.0, None), only_splits)

    probe = bt.BatchedGaussianParams(_scenes(DENSIFY_COUNTS), _dev())
    smax = torch.cat([probe.get_scaling.detach()[probe.model_rows(b)] for b in range(3)]).max(dim=1).values

    def all_pruned(p, metas, n_clone, before, untouched):
        assert all(m[:3] == [0, 0, 0] and m[3] > 0 for m in metas) and p.counts == [0, 0, 0] and p.first_block == [0, 1, 2, 3] and not any(untouched)
    run("everything pruned", float(smax.median()) / 0.01, (0.5, 2.0, None), all_pruned)

    world = float(smax.quantile(0.6))
    extent = world / 0.1

    def world_size(p, metas, n_clone, before, untouched):
        assert all(m[1] == c > 20 and 0 < m[2] < m[3] and m[0] < n - m[3] for m, n, c in zip(metas, DENSIFY_COUNTS, n_clone))
    run("world-size term", extent, (0.5, 0.0, 20), world_size, percent_dense=float(smax.median()) / extent)

    mixed = dict(percent_dense=float(smax.quantile(0.65)) / 5.0)      # (fewer large rows than small ones)

    def note(p, metas, n_clone, before, untouched):
        assert all(m[1] == c > 20 and 20 < m[3] < c - 1 for m, c in zip(metas, n_clone))
    run("mixed", 5.0, (0.5, 0.0, None), note, **mixed)
    n_clone, n_split = seen["mixed"][3], [m[3] for m in seen["mixed"][2]]

    # the cap is per model: max_points = model 1's rows + clones cancels model 0's clones (2000 + its clones is more), model 1's splits (its
    # clones fit exactly, its splits no more) and nothing of model 2 (1000 rows)
    cap = DENSIFY_COUNTS[1] + n_clone[1]
    assert DENSIFY_COUNTS[0] + n_clone[0] > cap and n_split[1] > 0 and DENSIFY_COUNTS[2] + n_clone[2] + n_split[2] <= cap
    assert DENSIFY_COUNTS[0] + n_split[0] <= cap, "model 0's splits fit once its clones are cancelled"

    def capped(p, metas, n_clone_, before, untouched):
        assert p.counts == [DENSIFY_COUNTS[0] + n_split[0], DENSIFY_COUNTS[1] + n_clone[1], DENSIFY_COUNTS[2] + n_clone[2] + n_split[2]]
        assert untouched == [False, True, False]
    run("max_points cancels model 0's clones and model 1's splits", 5.0, (0.5, 0.0, None), capped, max_points=cap, **mixed)

    def roomy(p, metas, n_clone_, before, untouched):
        assert p.counts == [n + c + s for n, c, s in zip(DENSIFY_COUNTS, n_clone, n_split)]
    run("max_points with room", 5.0, (0.5, 0.0, None), roomy, max_points=DENSIFY_COUNTS[0] + n_clone[0] + n_split[0], **mixed)
    for what, (n0, n1, metas, n_clone_) in seen.items():
        print(f"[batch resize regimes] {what}: counts {n0} -> {n1}, meta {metas}, clones selected {n_clone_}")


def test_batched_densifier_low_opacities_and_host_waits():
    """A fifth of the rows under the opacity floor, so that clones and children leave with it; one host wait for the uncapped call."""
    fresh = _fresh_pad()
    probe = bt.BatchedGaussianParams(_scenes(DENSIFY_COUNTS), _dev())
    pd = float(torch.cat([probe.get_scaling.detach()[probe.model_rows(b)] for b in range(3)]).max(dim=1).values.median()) / 5.0
    batch, singles, db, das = _densifier_batch(percent_dense=pd)
    low = (torch.rand(batch.num_points, generator=torch.Generator().manual_seed(3)) < 0.2).to(_dev())
    with torch.no_grad():
        batch._opacity[low] = -9.0
        for b, p in enumerate(singles):
            p._opacity[low[batch.model_rows(b)]] = -9.0
    flags, clone, _ = db._resize_flags(0.5, 0.005, None)
    bl = BC.batch_layout_oracle(flags.cpu().numpy(), batch.first_block, batch.counts)
    for b, m in enumerate(bl["models"]):
        nA, nB, nC, nS = m["meta"]
        assert 0 < nB < int(clone[batch.model_rows(b)].sum()) and 0 < nC < nS and nA < batch.counts[b] - nS
    for d in das:
        d.densify_and_prune(0.5, 0.005, None)
    torch.cuda.synchronize()
    with _sync_warnings() as rec:
        db.densify_and_prune(0.5, 0.005, None)
    waits = _waits(rec)
    print(f"[batch resize host waits] synchronisation warnings of one BatchedDensifier.densify_and_prune over {DENSIFY_COUNTS}: {waits}")
    assert waits <= 1, _where(rec)
    _assert_same_densifiers(batch, singles, db, das, fresh, "low opacities")
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad"):
            db.densify_and_prune(bad, 0.005, None)


# ---- a training trajectory -----------------------------------------------------------------------------------------------------------

def _same(got, want, what, fixed_order):
    if fixed_order:
        assert got.shape == want.shape and torch.equal(got, want), what
    else:
        parity.same_accumulation({"t": got}, {"t": want}, str(what), verbose=False)


@pytest.mark.parametrize("fixed_order", [True, False], ids=["deterministic_backward", "default-accumulation"])
def test_a_batch_that_densifies_trains_as_its_models_alone(fixed_order):
    """Three models of (3000, 2999, 5000) rows at 330x250, 12 steps with a densification at 4, 8 and 12 and an opacity reset at 8: after
    every step every image, parameter and moment of the batch is what the model trained alone with its own Densifier has."""
    lib = L.load()
    dev = _dev()
    W, H, deg, sizes = 330, 250, 3, (3000, 2999, 5000)
    scenes = [syn.make_scene(n, W, H, sh_degree=deg, seed=40 + k, posed=True) for k, n in enumerate(sizes)]
    gts = [syn.target_image(W, H, seed=10 + k).to(dev) for k in range(3)]
    cams = [ts.make_settings(sc, dev, deg) for sc in scenes]
    bview = bt.batch_settings(cams, dev)
    gt_stack = torch.stack(gts)
    # the threshold: the median mean gradient of a short run of the batch, so that about half of the seen rows are selected; half of the
    # rows are "big" (percent_dense * extent = the median scale): clones and splits both
    pp = bt.BatchedGaussianParams(scenes, dev)
    dp = dm.BatchedDensifier(pp, 5.0, dm.DensifyConfig(densify_from_iter=10 ** 9), seeds=(0, 1, 2))
    for it in range(1, 4):
        ts.train_step(pp, bview, gt_stack, densifier=dp, iteration=it)
    g = (dp.xyz_gradient_accum / dp.denom).squeeze(1)
    thr = float(g[torch.isfinite(g) & (g > 0)].median())
    smax = torch.cat([pp.get_scaling.detach()[pp.model_rows(b)] for b in range(3)]).max(dim=1).values
    cfg = dict(densify_from_iter=2, densification_interval=4, opacity_reset_interval=8, densify_grad_threshold=thr, densify_until_iter=10 ** 6,
               percent_dense=float(smax.median()) / 5.0)
    assert thr > 0
    first = {}
    assert lib.gsr_set_option(b"deterministic_backward", 1 if fixed_order else 0) == 0
    try:
        singles = [ts.GaussianParams(sc, dev) for sc in scenes]
        das = [dm.Densifier(p, 5.0, dm.DensifyConfig(**cfg), seed=21 + b) for b, p in enumerate(singles)]
        batch = bt.BatchedGaussianParams(scenes, dev)
        db = dm.BatchedDensifier(batch, 5.0, dm.DensifyConfig(**cfg), seeds=(21, 22, 23))
        for b, d in enumerate(das):          # what the torch route is about to do at the first densification, from its own flag bytes
            def spy(*args, d=d, b=b, inner=d.densify_and_prune):
                if b not in first:
                    flags, clone, _ = d._resize_flags(*args)
                    f = flags.cpu().numpy()
                    nA, nB, nC, nS = RC.layout_oracle(f)["meta"]
                    first[b] = dict(clones=nB, children=nC, pruned=int(((f & (RC.KEEP | RC.SPLIT)) == 0).sum()))
                return inner(*args)
            d.densify_and_prune = spy
        sizes_seen = []
        for it in range(1, 13):
            pk = ts.train_step(batch, bview, gt_stack, densifier=db, iteration=it, next_settings=bview)
            for k in range(3):
                ps = ts.train_step(singles[k], cams[k], gts[k], densifier=das[k], iteration=it, next_settings=cams[k])
                assert batch.counts[k] == singles[k].num_points, (it, k, batch.counts, singles[k].num_points)
                rows = batch.model_rows(k)
                _same(pk["raw_image"][k], ps["raw_image"], (it, k, "raw_image"), fixed_order)
                for name in NAMES:
                    _same(getattr(batch, name).detach()[rows], getattr(singles[k], name).detach(), (it, k, name), fixed_order)
                for gb, gs in zip(batch.optimizer.param_groups, singles[k].optimizer.param_groups):
                    sb, ss = batch.optimizer.state.get(gb["params"][0]), singles[k].optimizer.state.get(gs["params"][0])
                    assert (sb is None) == (ss is None), (it, k, gb["name"])
                    if sb is not None:
                        for mom in ("exp_avg", "exp_avg_sq"):
                            _same(sb[mom][rows], ss[mom], (it, k, gb["name"], mom), fixed_order)
            if it % 4 == 0:
                batch.optimizer._reconcile()
                for k in range(3):
                    singles[k].optimizer._reconcile()
                    for gb, gs in zip(batch.optimizer.param_groups, singles[k].optimizer.param_groups):
                        sb, ss = batch.optimizer.state.get(gb["params"][0]), singles[k].optimizer.state.get(gs["params"][0])
                        if sb is not None:
                            assert int(sb["step"]) == int(ss["step"]), (it, k, gb["name"])
                    assert torch.equal(db.gens[k].get_state(), das[k].gen.get_state()), (it, k)
                sizes_seen.append(list(batch.counts))
        print(f"[batch resize trajectory] threshold {thr:.3e}, first densification {first}, counts after each densification: {sizes_seen}")
        assert sorted(first) == [0, 1, 2] and all(v["clones"] >= 1 and v["children"] >= 1 and v["pruned"] >= 1 for v in first.values()), first
        assert all(a != b for a, b in zip(sizes_seen[0], sizes)), "every model was resized"
    finally:
        lib.gsr_set_option(b"deterministic_backward", 0)


# ---- the leaf phase of a small local run ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fixed_order", [True, False], ids=["deterministic_backward", "default-accumulation"])
def test_the_leaf_phase_of_a_local_run_with_leaf_batch_equals_the_leaves_alone(fixed_order, monkeypatch):
    """run_segments.run_local over 4 segments (24 frames: leaves of 7, 8, 7 and 8 frames, so leaf_batch=4 trains ranks 0 and 2 in one
    batch and ranks 1 and 3 in another), 3000 Gaussians per leaf at 96x80, 144 and 168 steps per leaf with --densify (a densification at
    iteration 100), against leaf_batch=0: every runner's leaf is the same model, and the merged root follows."""
    rs = importlib.import_module("3dgs_hierarchical_training_amd.run_segments")
    sequence = importlib.import_module("3dgs_hierarchical_training_amd.sequence")
    lib = L.load()
    dev = _dev()
    leaves, arm = {}, [None]
    inner = rs.RankRunner._emit

    def spy(self, rec):
        if rec.get("phase") == "leaf":
            leaves[(arm[0], self.rank)] = ({k: v.clone() for k, v in self.seg.params.raw().items()}, dict(rec), self.seg.global_iteration,
                                           self.seg.params.active_sh_degree, {f: p.clone() for f, p in self.seg.poses.items()})
        return inner(self, rec)
    monkeypatch.setattr(rs.RankRunner, "_emit", spy)
    roots = {}
    assert lib.gsr_set_option(b"deterministic_backward", 1 if fixed_order else 0) == 0
    try:
        for arm[0], leaf_batch in (("alone", 0), ("batch", 4)):
            cfg = rs.HTConfig(frames=24, width=96, height=80, gt_gaussians=4000, leaf_gaussians=3000, leaf_iters_per_frame=24,
                              phase1_iters_per_frame=2, phase2_iters_per_frame=[3, 3, 3], densify=True, densify_route="kernel", sh_up_every=50,
                              leaf_batch=leaf_batch)
            seq = sequence.FrameSequence(cfg.frames, cfg.gt_gaussians, cfg.width, cfg.height, dev, seed=4)
            root, report = rs.run_local(4, seq, cfg, dev, log=lambda rec: None)
            roots[arm[0]] = {k: v.clone() for k, v in root.seg.params.raw().items()}
            recs = [r for r in report if r["phase"] == "leaf"]
            assert len(recs) == 4 and all(("leaf_batch" in r) == (leaf_batch >= 2) for r in recs)
    finally:
        lib.gsr_set_option(b"deterministic_backward", 0)
    sizes = []
    for rank in range(4):
        (ra, reca, ita, dega, posa), (rb, recb, itb, degb, posb) = leaves[("alone", rank)], leaves[("batch", rank)]
        assert (reca["frames"], reca["steps"], reca["gaussians"], ita, dega) == (recb["frames"], recb["steps"], recb["gaussians"], itb, degb), rank
        assert sorted(posa) == sorted(posb) and all(torch.equal(posa[f], posb[f]) for f in posa), rank
        for k in NAMES:
            _same(rb[k], ra[k], ("leaf", rank, k), fixed_order)
        sizes.append(reca["gaussians"])
    print(f"[batch resize leaf phase] Gaussians per leaf: {sizes}")
    assert any(n != 3000 for n in sizes), "the densification at iteration 100 resized a leaf"
    for k in NAMES:
        _same(roots["batch"][k], roots["alone"][k], ("root", k), fixed_order)
