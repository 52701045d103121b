"""What the merge tests share: numpy restatements of what gsr_select_smallest and gsr_merge_apply decide (include/gsr.h, version 121) --
the key of a row, the selection `np.argsort(key, kind="stable")[:k]` with its `meta`, the merged layout
`np.concatenate([a[keep_a], b[keep_b]])` -- and the score patterns and keep patterns the GPU tests run."""
import numpy as np

KEEP = 1
PARAM, MOMENT = 0, 1
NAN_KEY = 0xFFFFFFFF


def keys_of(values):
    """values float32 [N, C] -> uint32 [N]: the row maximum (NaN propagates) as an integer that orders like the float; -0 counts as +0,
    every NaN is the largest key."""
    v = np.asarray(values, dtype=np.float32)
    v = v.reshape(v.shape[0], max(1, int(np.prod(v.shape[1:]))))
    with np.errstate(invalid="ignore"):
        score = v.max(axis=1) if v.shape[0] else np.zeros(0, np.float32)          # np.max propagates NaN, as torch.amax does
    nan = np.isnan(score)
    score = np.where(score == 0, np.float32(0.0), score).astype(np.float32)        # -0 -> +0
    bits = score.view(np.uint32)
    key = np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)
    key[nan] = NAN_KEY
    return key


def select_oracle(values, k, key=None):
    """-> dict(drop bool [N], keep_flags uint8 [N], meta [8]): the k rows with the smallest keys, ties at the threshold by row number."""
    key = keys_of(values) if key is None else key
    n = key.shape[0]
    assert 0 <= k <= n
    order = np.argsort(key, kind="stable")[:k]
    drop = np.zeros(n, dtype=bool)
    drop[order] = True
    meta = [int(k), 0, 0, 0, int((key == NAN_KEY).sum()), 0, 0, 0]
    if k > 0:
        t = key[order[k - 1]]
        meta[1:4] = [int((key < t).sum()), int((key == t).sum()), int(t)]
    if n == 0:
        meta = [0] * 8
    return dict(drop=drop, keep_flags=np.where(drop, 0, KEEP).astype(np.uint8), meta=meta)


def merged_oracle(a, keep_a, b, keep_b, kind=PARAM):
    """The merged array: a's kept rows ascending, then b's (zeros for a MOMENT)."""
    tail = b[keep_b] if kind == PARAM else np.zeros((int(keep_b.sum()),) + a.shape[1:], a.dtype)
    return np.concatenate([a[keep_a], tail])


def spread(score, c, rng):
    """[N, C] float32 whose row maximum is `score`: the score in one random column, and in the others the score again or -inf.  A NaN score
    sits in ONE column beside finite values (for C > 1: a NaN in a column that would not be the maximum)."""
    n = score.shape[0]
    v = np.where(rng.random((n, c)) < 0.5, score[:, None], np.float32(-np.inf)).astype(np.float32)
    nan = np.isnan(score)
    v[nan] = rng.standard_normal((int(nan.sum()), c)).astype(np.float32) + 100.0
    v[np.arange(n), rng.integers(0, c, n)] = score
    return v


def _bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


def score_patterns(n, seed=0):
    """name -> (score float32 [n], extra ks): the patterns of the issue.  Extra ks sit around the counts the pattern is about."""
    rng = np.random.default_rng(1000 * seed + n)
    r = lambda: rng.integers(0, 256, n).astype(np.uint32)
    pats = {}
    pats["distinct"] = ((rng.permutation(n) - n // 2).astype(np.float32), [])
    pats["all_equal"] = (np.full(n, 1.5, np.float32), [])
    pats["all_zero"] = (np.zeros(n, np.float32), [])
    for share in (30, 99):
        s = (rng.permutation(n) + 1).astype(np.float32) / np.float32(n + 1)
        s[rng.random(n) < share / 100.0] = 0.0
        nz = int((s == 0).sum())
        pats[f"zeros_{share}"] = (s, [nz - 1, nz, nz + 1])
    pats["byte0"] = (_bits(np.uint32(0x3F800000) | r()), [])                       # keys that differ in their lowest byte only
    pats["byte1"] = (_bits(np.uint32(0x3F800012) | (r() << np.uint32(8))), [])
    pats["byte2"] = (_bits(np.uint32(0x3F000012) | (r() << np.uint32(16))), [])
    pats["byte3"] = (_bits(np.uint32(0x00400000) | (r() << np.uint32(24))), [])     # ... in their highest byte only (no NaN or inf among them)
    s = np.array([-2.0, -1.0, -0.0, 0.0, 1.0, -0.0, 0.0, -1e-30], np.float32)[rng.integers(0, 8, n)]
    pats["signed_zeros"] = (s, [int((s < 0).sum()), int((s <= 0).sum())])
    s = rng.standard_normal(n).astype(np.float32)
    s[rng.random(n) < 0.2] = np.inf
    s[rng.random(n) < 0.2] = -np.inf
    pats["inf"] = (s, [int((s == -np.inf).sum()), n - int((s == np.inf).sum())])
    u = rng.integers(0, 1 << 23, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << np.uint32(31))
    pats["denormals"] = (_bits(u), [])
    s = rng.standard_normal(n).astype(np.float32)
    s[rng.random(n) < 0.2] = np.nan
    good = n - int(np.isnan(s).sum())
    pats["nan_rows"] = (s, [good - 1, good, good + 1])
    return pats


def ks_of(n, extra=()):
    return sorted({k for k in (0, 1, n // 2, n - 1, n, *extra) if 0 <= k <= n})


def keep_patterns(n, seed=0):
    """name -> bool [n]: the keep patterns of the issue."""
    rng = np.random.default_rng(77 * seed + n)
    i = np.arange(n)
    return {"none": np.zeros(n, bool), "all": np.ones(n, bool), "alternating": i % 2 == 0, "first": i == 0, "last": i == n - 1,
            "random": rng.random(n) < 0.5}
