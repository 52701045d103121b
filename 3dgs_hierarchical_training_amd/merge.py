"""The merge on the device: which rows are dropped, and the kept rows of two models appended in one launch.

  select_smallest   gsr_select_smallest   (csrc/select_kernels.hip; semantics in include/gsr.h, version 121)
  read_counts_pair  the route's one host wait: the A-list lengths and status words of BOTH plans in one copy
  merge_apply       gsr_merge_apply       (csrc/resize_kernels.hip)

The kernels decide with integers and copy bytes; they compute no float.  `hierarchy.prune_mask(route="kernel")` and
`segments.merge_segments(route="kernel")` are the callers, and `gsr_autopatch.merge_two_3DGS_fused` under the unmodified trainer.  Both bindings serve it: `torch.ops.gsr.select_smallest` / `merge_apply`, and the
ctypes view of the same C ABI under GSR_BINDING=ctypes.  No CPU fallback: a CPU tensor raises RuntimeError before a device is touched.
"""
import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import torch

from . import _ext as E
from . import _lib as L
from .resize import MOMENT, PARAM, check_route, need_device  # noqa: F401  (re-exported: the kinds and the route check of the resize)


def select_smallest(values: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """values float32 [N, C] (or [N]) -> (drop bool [N], keep_flags uint8 [N], meta int64 [8]) on the device: the k rows with the smallest row
    maximum, ties at the threshold by row number (include/gsr.h).  keep_flags is what resize_plan takes.  Asynchronous."""
    need_device("select_smallest", values=values)
    if values.dtype != torch.float32 or values.dim() not in (1, 2):
        raise ValueError("select_smallest: values is a float32 tensor [N, C] or [N]")
    n, c = int(values.shape[0]), (int(values.shape[1]) if values.dim() == 2 else 1)
    if not 0 <= int(k) <= n:
        raise ValueError(f"select_smallest: k = {k} outside [0, N = {n}]")
    if not 1 <= c <= L.GSR_SELECT_MAX_COLUMNS:
        raise ValueError(f"select_smallest: C = {c} outside [1, {L.GSR_SELECT_MAX_COLUMNS}]")
    if not E.use_ctypes():
        drop, keep, meta = E.load().select_smallest(values.detach(), int(k))
        return drop.view(torch.bool), keep, meta
    lib = L.load()
    values = values.detach().contiguous()
    sb = lib.gsr_select_scratch_bytes(n)
    drop = torch.empty((n,), dtype=torch.uint8, device=values.device)
    keep = torch.empty((n,), dtype=torch.uint8, device=values.device)
    meta = torch.empty((L.GSR_SELECT_META_WORDS,), dtype=torch.int64, device=values.device)
    scratch = torch.empty((sb,), dtype=torch.uint8, device=values.device)
    with torch.cuda.device(values.device):
        stream = torch.cuda.current_stream(values.device).cuda_stream
        L.check(lib.gsr_select_smallest(values.data_ptr() if n else None, n, c, int(k), drop.data_ptr(), keep.data_ptr(), meta.data_ptr(),
                                        scratch.data_ptr() if n else None, sb, C.c_void_p(stream)), "gsr_select_smallest")
    return drop.view(torch.bool), keep, meta


def read_counts_pair(meta_a: torch.Tensor, meta_b: torch.Tensor) -> List[int]:
    """[nA, status_a, nB, status_b]: the A-list length and the status word of two plans' metas, read in ONE copy.
    SYNCHRONISES: the merge's one host wait."""
    v = torch.cat((meta_a, meta_b)).cpu().tolist()          # one launch, one copy of 16 words
    w, st = L.GSR_RESIZE_META_WORDS, L.GSR_RESIZE_META_STATUS
    return [int(v[0]), int(v[st]), int(v[w]), int(v[w + st])]


def merge_apply(plan_a: torch.Tensor, meta: torch.Tensor, n_a: int, kept_a: int, plan_b: torch.Tensor, n_b: int, kept_b: int,
                src_a: Sequence[torch.Tensor], src_b: Sequence[Optional[torch.Tensor]], kinds: Optional[Sequence[int]] = None,
                check: bool = False) -> List[torch.Tensor]:
    """Fresh tensors of kept_a + kept_b rows, one per tensor of src_a ([n_a, ...]; src_b[k] is [n_b, ...] with the same trailing shape): rows
    [0, kept_a) are the rows plan_a's A list names, the rest those of plan_b's.  kinds[k] is PARAM (default) or MOMENT, whose b rows are zero
    and whose src_b[k] may be None.  meta: either plan's meta (a bad plan entry raises its status word); check=True reads it back (a host
    wait) and raises."""
    kinds = [PARAM] * len(src_a) if kinds is None else [int(k) for k in kinds]
    if len(kinds) != len(src_a) or len(src_b) != len(src_a):
        raise ValueError("merge_apply: src_a, src_b and kinds have one entry per tensor")
    if any(b is None and k != MOMENT for b, k in zip(src_b, kinds)):
        raise ValueError("merge_apply: only a MOMENT tensor may come without src_b")
    need_device("merge_apply", plan_a=plan_a, plan_b=plan_b, meta=meta, **{f"src_a[{k}]": t for k, t in enumerate(src_a)},
                **{f"src_b[{k}]": t for k, t in enumerate(src_b)})
    n_a, kept_a, n_b, kept_b = int(n_a), int(kept_a), int(n_b), int(kept_b)
    if not E.use_ctypes():
        absent = plan_a.new_empty((0,), dtype=torch.float32)
        return list(E.load().merge_apply(plan_a, plan_b, meta, n_a, kept_a, n_b, kept_b, [t.detach() for t in src_a],
                                         [absent if t is None else t.detach() for t in src_b], kinds, bool(check)))
    lib = L.load()
    nout = kept_a + kept_b
    src_a = [t.detach().contiguous() for t in src_a]
    src_b = [None if t is None else t.detach().contiguous() for t in src_b]
    dst = [torch.empty((nout,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for t in src_a]
    table = (L.GsrMergeTensor * max(len(src_a), 1))()
    for k, (a, b, d) in enumerate(zip(src_a, src_b, dst)):
        if a.shape[0] != n_a or (b is not None and (b.shape[0] != n_b or b.shape[1:] != a.shape[1:] or b.dtype != a.dtype)):
            raise ValueError(f"merge_apply: src_a[{k}] is [n_a, ...] and src_b[{k}] is [n_b, ...] with the same trailing shape and dtype")
        row_bytes = a.element_size() * math.prod(a.shape[1:])
        moves = row_bytes > 0 and nout > 0
        table[k].src_a = a.data_ptr() if (moves and n_a > 0) else None
        table[k].src_b = b.data_ptr() if (moves and b is not None and n_b > 0) else None
        table[k].dst = d.data_ptr() if moves else None
        table[k].row_bytes, table[k].kind = row_bytes, kinds[k]
    with torch.cuda.device(plan_a.device):
        stream = torch.cuda.current_stream(plan_a.device).cuda_stream
        L.check(lib.gsr_merge_apply(plan_a.data_ptr() if plan_a.numel() else None, plan_a.numel() * 4, n_a, kept_a,
                                    plan_b.data_ptr() if plan_b.numel() else None, plan_b.numel() * 4, n_b, kept_b, table, len(src_a),
                                    meta.data_ptr(), C.c_void_p(stream)), "gsr_merge_apply")
    if check and int(meta[L.GSR_RESIZE_META_STATUS].item()) != 0:
        raise RuntimeError("merge_apply: a plan holds a row number outside its model: the rows it names were written as zeros")
    return dst
