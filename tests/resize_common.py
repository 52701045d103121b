"""What the resize tests share: a numpy restatement of the layout gsr_resize_plan decides (include/gsr.h, version 120) -- flag bytes -> the
four row lists, the split ranks and `meta` -- plain integer code that serves as the oracle for the plan, the same layout applied to an array
with numpy indexing (the oracle for gsr_resize_apply), and the flag patterns the GPU tests run."""
import numpy as np

KEEP, CLONE, SPLIT, CHILD = 1, 2, 4, 8
PARAM, MOMENT, CHILD_SOURCED = 0, 1, 2


def layout_oracle(flags):
    """flags uint8 [N] -> dict(rows_a, rows_b, rows_c, rank_c, split_rows: int64 arrays; meta: [nA, nB, nC, nSplit])."""
    f = np.asarray(flags, dtype=np.uint8)
    rows = np.arange(f.shape[0], dtype=np.int64)
    is_split = (f & SPLIT) != 0
    is_c = is_split & ((f & CHILD) != 0)
    rank = np.cumsum(is_split) - 1                      # the rank of a split parent among the split parents, in ascending row order
    out = dict(rows_a=rows[(f & KEEP) != 0], rows_b=rows[(f & CLONE) != 0], rows_c=rows[is_c], rank_c=rank[is_c].astype(np.int64),
               split_rows=rows[is_split])
    out["meta"] = [len(out["rows_a"]), len(out["rows_b"]), len(out["rows_c"]), len(out["split_rows"])]
    return out


def source_rows(lay):
    """The source row of every row of the final layout: A, B, C copy 0, C copy 1."""
    return np.concatenate((lay["rows_a"], lay["rows_b"], lay["rows_c"], lay["rows_c"]))


def apply_oracle(lay, src, kind, child=None):
    """The resized array of `src` [N, ...] under the layout, with numpy indexing."""
    nA, nB, nC, nS = lay["meta"]
    out = src[source_rows(lay)].copy()
    if kind == MOMENT:
        out[nA:] = 0
    elif kind == CHILD_SOURCED:
        out[nA + nB: nA + nB + nC] = child[lay["rank_c"]]
        out[nA + nB + nC:] = child[nS + lay["rank_c"]]
    return out


# the hand-worked case: eight rows
#   row   0     1      2            3      4            5           6     7
HAND_FLAGS = np.array([KEEP, 0, KEEP | CLONE, SPLIT, SPLIT | CHILD, KEEP | CLONE, CLONE, SPLIT | CHILD], dtype=np.uint8)
HAND_LAYOUT = dict(rows_a=[0, 2, 5], rows_b=[2, 5, 6], rows_c=[4, 7], rank_c=[1, 2], split_rows=[3, 4, 7], meta=[3, 3, 2, 3])
HAND_SOURCE_ROWS = [0, 2, 5, 2, 5, 6, 4, 7, 4, 7]


def flag_patterns(n, seed=0):
    """name -> flags uint8 [n]: the patterns of the issue."""
    rng = np.random.default_rng(seed + n)
    i = np.arange(n)
    legal = np.array([0, KEEP, KEEP | CLONE, CLONE, SPLIT, SPLIT | CHILD], dtype=np.uint8)      # the combinations a densification produces
    pats = {
        "none": np.zeros(n, np.uint8),
        "all_keep": np.full(n, KEEP, np.uint8),
        "all_clone": np.full(n, CLONE, np.uint8),
        "all_keep_and_clone": np.full(n, KEEP | CLONE, np.uint8),
        "all_split_child": np.full(n, SPLIT | CHILD, np.uint8),
        "split_without_child": np.full(n, SPLIT, np.uint8),
        "alternating": np.where(i % 2 == 0, KEEP | CLONE, SPLIT | CHILD).astype(np.uint8),
        "long_runs": legal[(i // max(1, n // 7)) % len(legal)],          # seven runs: shorter than a tile of the scan, or many tiles long
        "random_p05": np.where(rng.random(n) < 0.05, legal[rng.integers(1, len(legal), n)], KEEP).astype(np.uint8),
        "random_p5": legal[rng.integers(0, len(legal), n)] * (rng.random(n) < 0.5).astype(np.uint8),
        "any_byte": rng.integers(0, 256, n).astype(np.uint8),          # every bit combination, the unused high bits included
    }
    return pats
