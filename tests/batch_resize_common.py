"""What the batched-resize tests share: a numpy restatement of what gsr_resize_plan_batched and gsr_resize_apply_batched decide (include/gsr.h,
version 122), built from the single-model oracle of tests/resize_common.py: every model's layout is `layout_oracle` of its own flag bytes
(row numbers moved to store rows, split ranks left model-local), the new store is `apply_oracle` per model at the model's new first block,
and every row between a model's last row and the end of its last block is the tensor's padding row (zero for a moment)."""
import numpy as np

import resize_common as RC

BLOCK = 128
LISTS = ("rows_a", "rows_b", "rows_c", "rank_c", "split_rows")


def first_block_of(counts):
    """The block offsets of a store that holds models of `counts` rows back to back, each padded to a multiple of 128 rows."""
    fb = [0]
    for n in counts:
        fb.append(fb[-1] + (int(n) + BLOCK - 1) // BLOCK)
    return fb


def store_flags(per_model, first_block, padding=0xFF):
    """One flag array over the store: model b's bytes at its rows, `padding` everywhere else."""
    f = np.full(BLOCK * first_block[-1], padding, np.uint8)
    for b, fm in enumerate(per_model):
        f[BLOCK * first_block[b]: BLOCK * first_block[b] + len(fm)] = fm
    return f


def batch_layout_oracle(flags, first_block, counts):
    """flags uint8 over the store -> dict(models: per model the dict of `layout_oracle` with row numbers as STORE rows and model-local
    ranks; meta: [B][8]; new_counts; new_first_block)."""
    f = np.asarray(flags, dtype=np.uint8)
    models, meta, new_counts, nfb = [], [], [], [0]
    for b, n in enumerate(counts):
        lo = BLOCK * first_block[b]
        lay = RC.layout_oracle(f[lo: lo + n])
        models.append(dict(rows_a=lay["rows_a"] + lo, rows_b=lay["rows_b"] + lo, rows_c=lay["rows_c"] + lo, rank_c=lay["rank_c"],
                           split_rows=lay["split_rows"] + lo, meta=lay["meta"], local=lay))
        nA, nB, nC, nS = lay["meta"]
        meta.append([nA, nB, nC, nS, 0, 0, 0, 0])
        new_counts.append(nA + nB + 2 * nC)
        nfb.append(nfb[-1] + max(1, (new_counts[-1] + BLOCK - 1) // BLOCK))
    return dict(models=models, meta=meta, new_counts=new_counts, new_first_block=nfb)


def child_bases(bl):
    """Row of `child` at which model b's children start: 2 * sum_{j<b} nSplit_j."""
    out, at = [], 0
    for m in bl["models"]:
        out.append(at)
        at += 2 * m["meta"][3]
    return out, at


def batch_apply_oracle(bl, first_block, counts, src, kind, child=None, pad=None):
    """The new store of `src` [128 * first_block[B], ...]: per model `apply_oracle` on the model's own rows, then padding."""
    nfb = bl["new_first_block"]
    out = np.zeros((BLOCK * nfb[-1],) + src.shape[1:], src.dtype)
    if kind != RC.MOMENT and pad is not None:
        out[:] = np.asarray(pad, src.dtype).reshape(src.shape[1:])
    bases, _ = child_bases(bl)
    for b, m in enumerate(bl["models"]):
        lo = BLOCK * first_block[b]
        nS = m["meta"][3]
        ch = None if child is None else child[bases[b]: bases[b] + 2 * nS]
        rows = RC.apply_oracle(m["local"], src[lo: lo + counts[b]], kind, ch)
        out[BLOCK * nfb[b]: BLOCK * nfb[b] + rows.shape[0]] = rows
    return out


# the hand-worked case: two models, 3 and 130 rows -> blocks [0, 1, 3], 384 store rows
#   model 0, store rows 0..2:      KEEP | CLONE, SPLIT | CHILD, 0                       (rows 3..127 are padding)
#   model 1, store rows 128..257:  row 128 SPLIT, row 129 KEEP, rows 130..256 KEEP | CLONE, row 257 SPLIT | CHILD   (rows 258..383 padding)
HAND_COUNTS = [3, 130]
HAND_FIRST_BLOCK = [0, 1, 3]
HAND_FLAGS = [np.array([RC.KEEP | RC.CLONE, RC.SPLIT | RC.CHILD, 0], np.uint8),
              np.array([RC.SPLIT, RC.KEEP] + [RC.KEEP | RC.CLONE] * 127 + [RC.SPLIT | RC.CHILD], np.uint8)]
HAND_META = [[1, 1, 1, 1, 0, 0, 0, 0], [128, 127, 1, 2, 0, 0, 0, 0]]
HAND_NEW_COUNTS = [4, 257]                      # 1 + 1 + 2, 128 + 127 + 2
HAND_NEW_FIRST_BLOCK = [0, 1, 4]                # model 1 grows from two blocks to three
HAND_MODEL0 = dict(rows_a=[0], rows_b=[0], rows_c=[1], rank_c=[0], split_rows=[1])
HAND_MODEL1 = dict(rows_a=list(range(129, 257)), rows_b=list(range(130, 257)), rows_c=[257], rank_c=[1], split_rows=[128, 257])
# the store row every row of the new store came from (-1: padding; the children as (model, copy, rank) below)
HAND_SOURCE_ROWS_MODEL0 = [0, 0, 1, 1]
HAND_SOURCE_ROWS_MODEL1 = list(range(129, 257)) + list(range(130, 257)) + [257, 257]
HAND_CHILD_ROWS = {0: (0, 1), 1: (2 + 1, 2 + 2 + 1)}      # model -> rows of `child` of its one surviving parent's copy 0 and copy 1
