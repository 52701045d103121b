"""Resizing the model on the device: one flag byte per row -> the layout of the resized model -> every row moved in one launch.

  resize_plan    gsr_resize_plan    (csrc/resize_kernels.hip; semantics in include/gsr.h, version 120)
  read_counts    the route's one host wait: the four list lengths (and the status word) of `meta`
  resize_apply   gsr_resize_apply

  resize_plan_batched / read_counts_batched / resize_apply_batched   the same three steps over the B models of a batched store
                 (gsr_resize_plan_batched, gsr_resize_apply_batched, version 122): per-model lists and counts, one read, one launch that
                 writes the new store with its padding rows

The kernels decide a layout and copy bytes; they compute no float.  `GaussianParams.prune_points(route="kernel")` and
`Densifier(route="kernel")` are the callers, `BatchedGaussianParams.resize_models` and `BatchedDensifier` those of the batched entries.
Both bindings serve it: `torch.ops.gsr.resize_plan` / `resize_apply` (`resize_plan_batched` / `resize_apply_batched`), and the ctypes
view of the same C ABI under GSR_BINDING=ctypes.  No CPU fallback: a CPU tensor raises RuntimeError before a device is touched.
"""
import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import torch

from . import _ext as E
from . import _lib as L

KEEP, CLONE, SPLIT, CHILD = L.GSR_RESIZE_KEEP, L.GSR_RESIZE_CLONE, L.GSR_RESIZE_SPLIT, L.GSR_RESIZE_CHILD
PARAM, MOMENT, CHILD_SOURCED = L.GSR_RESIZE_PARAM, L.GSR_RESIZE_MOMENT, L.GSR_RESIZE_CHILD_SOURCED
ROUTES = ("torch", "kernel")


def check_route(route: str, who: str) -> str:
    if route not in ROUTES:
        raise ValueError(f"{who}: route must be 'torch' or 'kernel' (got {route!r})")
    return route


def need_device(who: str, **tensors):
    for k, t in tensors.items():
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise RuntimeError(f"{who}: {k} must be a tensor on a ROCm/HIP device -- there is no CPU fallback")


def plan_stride(n: int) -> int:
    """Entries per segment of a plan for n rows (include/gsr.h: 64 * ceil(n / 64))."""
    return (int(n) + 63) // 64 * 64


def plan_segment(plan: torch.Tensor, n: int, which: int, length: int) -> torch.Tensor:
    """The first `length` entries of segment `which` (L.GSR_RESIZE_PLAN_*) of a plan for n rows: a view."""
    s = plan_stride(n)
    return plan[which * s: which * s + int(length)]


def resize_plan(flags: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """flags uint8 [N] -> (plan int32, meta int64 [8]) on the device.  Asynchronous."""
    need_device("resize_plan", flags=flags)
    if flags.dtype != torch.uint8 or flags.dim() != 1:
        raise ValueError("resize_plan: flags is a uint8 tensor [N]")
    if not E.use_ctypes():
        return E.load().resize_plan(flags)
    lib = L.load()
    flags = flags.contiguous()
    n = int(flags.shape[0])
    pb, sb = lib.gsr_resize_plan_bytes(n), lib.gsr_resize_scratch_bytes(n)
    plan = torch.empty((pb // 4,), dtype=torch.int32, device=flags.device)
    meta = torch.empty((L.GSR_RESIZE_META_WORDS,), dtype=torch.int64, device=flags.device)
    scratch = torch.empty((sb,), dtype=torch.uint8, device=flags.device)
    with torch.cuda.device(flags.device):
        stream = torch.cuda.current_stream(flags.device).cuda_stream
        L.check(lib.gsr_resize_plan(flags.data_ptr() if n else None, n, plan.data_ptr() if n else None, pb, meta.data_ptr(),
                                    scratch.data_ptr() if n else None, sb, C.c_void_p(stream)), "gsr_resize_plan")
    return plan, meta


def read_counts(meta: torch.Tensor, extra: Optional[torch.Tensor] = None) -> List[int]:
    """[nA, nB, nC, nSplit, status] of a plan's meta, then the entries of `extra` (a device int64 tensor read in the same copy).
    SYNCHRONISES: the resize's one host wait."""
    head = meta[:L.GSR_RESIZE_META_STATUS + 1]
    return [int(v) for v in (head if extra is None else torch.cat((head, extra.reshape(-1).to(torch.int64)))).cpu().tolist()]


def resize_apply(plan: torch.Tensor, meta: torch.Tensor, n: int, counts: Sequence[int], src: Sequence[torch.Tensor], kinds: Sequence[int],
                 child: Optional[Sequence[Optional[torch.Tensor]]] = None, check: bool = False) -> List[torch.Tensor]:
    """Fresh tensors of nA + nB + 2 nC rows, one per tensor of `src` ([n, ...], contiguous), filled by one launch.  counts = (nA, nB, nC,
    nSplit) as read from meta; kinds[k] is PARAM, MOMENT or CHILD_SOURCED, and child[k] the [2 nSplit, ...] rows of a CHILD_SOURCED
    tensor.  check=True reads the status word back afterwards (a host wait) and raises when the plan named a row outside [0, n)."""
    nA, nB, nC, nS = (int(c) for c in counts[:4])
    child = [None] * len(src) if child is None else list(child)
    need_device("resize_apply", plan=plan, meta=meta, **{f"src[{k}]": t for k, t in enumerate(src)},
                **{f"child[{k}]": t for k, t in enumerate(child)})
    if len(kinds) != len(src) or len(child) != len(src):
        raise ValueError("resize_apply: src, kinds and child have one entry per tensor")
    if not E.use_ctypes():
        empty = plan.new_empty((0,), dtype=torch.float32)
        return list(E.load().resize_apply(plan, meta, int(n), nA, nB, nC, nS, [t.detach() for t in src], [int(k) for k in kinds],
                                          [empty if c is None else c.detach() for c in child], bool(check)))
    lib = L.load()
    nout = nA + nB + 2 * nC
    src = [t.detach().contiguous() for t in src]
    child = [None if c is None else c.detach().contiguous() for c in child]
    dst = [torch.empty((nout,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for t in src]
    table = (L.GsrResizeTensor * max(len(src), 1))()
    for k, (s, d) in enumerate(zip(src, dst)):
        row_bytes = s.element_size() * math.prod(s.shape[1:])
        moves = row_bytes > 0 and nout > 0 and s.shape[0] > 0
        table[k].src, table[k].dst = (s.data_ptr(), d.data_ptr()) if moves else (None, None)
        table[k].child = child[k].data_ptr() if (int(kinds[k]) == CHILD_SOURCED and child[k] is not None and child[k].numel()) else None
        table[k].row_bytes, table[k].kind = row_bytes, int(kinds[k])
    with torch.cuda.device(plan.device):
        stream = torch.cuda.current_stream(plan.device).cuda_stream
        L.check(lib.gsr_resize_apply(plan.data_ptr() if plan.numel() else None, plan.numel() * 4, int(n), nA, nB, nC, nS, table, len(src),
                                     meta.data_ptr(), C.c_void_p(stream)), "gsr_resize_apply")
    if check and int(meta[L.GSR_RESIZE_META_STATUS].item()) != 0:
        raise RuntimeError("resize_apply: the plan holds a row number outside [0, N): the rows it names were written as zeros")
    return dst


# ---- the models of a batch (include/gsr.h, version 122) ----------------------------------------------------------------------------------
BLOCK = L.GSR_RESIZE_BLOCK


def new_first_block(counts4: Sequence[Sequence[int]]) -> List[int]:
    """The block offsets of the resized store: model b takes max(1, ceil((nA + nB + 2 nC) / 128)) blocks (a model that loses every row keeps
    one block of padding, so model numbers stay what they were)."""
    fb = [0]
    for c in counts4:
        n = int(c[0]) + int(c[1]) + 2 * int(c[2])
        fb.append(fb[-1] + max(1, (n + BLOCK - 1) // BLOCK))
    return fb


def _batch_struct(first_block: Sequence[int], counts: Sequence[int]) -> "L.GsrResizeBatch":
    if not 1 <= len(counts) <= L.GSR_RESIZE_MAX_MODELS or len(first_block) != len(counts) + 1:
        raise ValueError(f"a batch has 1 to {L.GSR_RESIZE_MAX_MODELS} models, first_block one entry more than counts")
    batch = L.GsrResizeBatch()
    batch.B = len(counts)
    for b, v in enumerate(first_block):
        batch.first_block[b] = int(v)
    for b, v in enumerate(counts):
        batch.counts[b] = int(v)
    return batch


def resize_plan_batched(flags: torch.Tensor, first_block: Sequence[int], counts: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """flags uint8 [128 * first_block[B]] over the store of B models -> (plan int32, meta int64 [B, 8]) on the device: per model the lists
    `resize_plan` gives it alone, as store rows, starting at entry 128 * first_block[b] of each segment.  Asynchronous; the number of
    launches does not depend on B."""
    need_device("resize_plan_batched", flags=flags)
    if flags.dtype != torch.uint8 or flags.dim() != 1:
        raise ValueError("resize_plan_batched: flags is a uint8 tensor [N]")
    first_block, counts = [int(v) for v in first_block], [int(v) for v in counts]
    if not E.use_ctypes():
        return E.load().resize_plan_batched(flags, first_block, counts)
    lib = L.load()
    batch = _batch_struct(first_block, counts)
    flags = flags.contiguous()
    n = int(flags.shape[0])
    if n != BLOCK * first_block[-1]:
        raise ValueError("resize_plan_batched: flags has 128 * first_block[B] entries")
    pb, sb = lib.gsr_resize_plan_bytes(n), lib.gsr_resize_scratch_bytes_batched(n)
    plan = torch.empty((pb // 4,), dtype=torch.int32, device=flags.device)
    meta = torch.empty((len(counts), L.GSR_RESIZE_META_WORDS), dtype=torch.int64, device=flags.device)
    scratch = torch.empty((sb,), dtype=torch.uint8, device=flags.device)
    with torch.cuda.device(flags.device):
        stream = torch.cuda.current_stream(flags.device).cuda_stream
        L.check(lib.gsr_resize_plan_batched(flags.data_ptr() if n else None, C.byref(batch), plan.data_ptr() if n else None, pb, meta.data_ptr(),
                                            scratch.data_ptr() if n else None, sb, C.c_void_p(stream)), "gsr_resize_plan_batched")
    return plan, meta


def read_counts_batched(meta: torch.Tensor, extra: Optional[torch.Tensor] = None):
    """meta [B, 8] -> B lists [nA, nB, nC, nSplit, status]; with `extra` (a device int64 tensor read in the same copy) -> (those, its
    entries as a list).  SYNCHRONISES: the batched resize's one host wait."""
    head = meta[:, :L.GSR_RESIZE_META_STATUS + 1].reshape(-1)
    flat = [int(v) for v in (head if extra is None else torch.cat((head, extra.reshape(-1).to(torch.int64)))).cpu().tolist()]
    w, nb = L.GSR_RESIZE_META_STATUS + 1, int(meta.shape[0])
    rows = [flat[b * w:(b + 1) * w] for b in range(nb)]
    return rows if extra is None else (rows, flat[nb * w:])


def resize_apply_batched(plan: torch.Tensor, meta: torch.Tensor, first_block: Sequence[int], counts: Sequence[int],
                         counts4: Sequence[Sequence[int]], src: Sequence[torch.Tensor], kinds: Sequence[int],
                         child: Optional[Sequence[Optional[torch.Tensor]]] = None, pad: Optional[Sequence[Optional[torch.Tensor]]] = None,
                         check: bool = False) -> Tuple[List[torch.Tensor], List[int]]:
    """Fresh tensors of the resized store, one per tensor of `src` ([128 * first_block[B], ...]), filled by one launch, padding rows
    included -> (tensors, the new first_block).  counts4[b] = (nA, nB, nC, nSplit) of model b as read from meta; child[k] holds the models'
    children back to back ([2 sum nSplit_b, ...]) for a CHILD_SOURCED tensor; pad[k] is the tensor's padding row (None: zeros; a MOMENT
    tensor's padding is always zero).  check=True reads the status words back afterwards (a host wait)."""
    first_block, counts = [int(v) for v in first_block], [int(v) for v in counts]
    c4 = [[int(v) for v in c[:4]] for c in counts4]
    child = [None] * len(src) if child is None else list(child)
    pad = [None] * len(src) if pad is None else list(pad)
    need_device("resize_apply_batched", plan=plan, meta=meta, **{f"src[{k}]": t for k, t in enumerate(src)},
                **{f"child[{k}]": t for k, t in enumerate(child)}, **{f"pad[{k}]": t for k, t in enumerate(pad)})
    if len(kinds) != len(src) or len(child) != len(src) or len(pad) != len(src) or len(c4) != len(counts):
        raise ValueError("resize_apply_batched: src, kinds, child and pad have one entry per tensor, counts4 one per model")
    nfb = new_first_block(c4)
    if not E.use_ctypes():
        empty = plan.new_empty((0,), dtype=torch.float32)
        out = E.load().resize_apply_batched(plan, meta, first_block, counts, [v for c in c4 for v in c], nfb, [t.detach() for t in src],
                                            [int(k) for k in kinds], [empty if c is None else c.detach() for c in child],
                                            [empty if p is None else p.detach() for p in pad], bool(check))
        return list(out), nfb
    lib = L.load()
    batch = _batch_struct(first_block, counts)
    nout = BLOCK * nfb[-1]
    src = [t.detach().contiguous() for t in src]
    child = [None if c is None else c.detach().contiguous() for c in child]
    pad = [None if p is None else p.detach().contiguous() for p in pad]
    dst = [torch.empty((nout,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for t in src]
    table = (L.GsrResizeBatchTensor * max(len(src), 1))()
    for k, (s, d) in enumerate(zip(src, dst)):
        row_bytes = s.element_size() * math.prod(s.shape[1:])
        moves = row_bytes > 0 and s.shape[0] > 0
        table[k].src, table[k].dst = (s.data_ptr(), d.data_ptr()) if moves else (None, None)
        table[k].child = child[k].data_ptr() if (int(kinds[k]) == CHILD_SOURCED and child[k] is not None and child[k].numel()) else None
        if table[k].child and (child[k].dtype != s.dtype or child[k].numel() * child[k].element_size() != 2 * sum(c[3] for c in c4) * row_bytes):
            raise ValueError(f"resize_apply_batched: child[{k}] is [2 sum nSplit_b, ...] rows of its tensor")
        if moves and (s.shape[0] != BLOCK * first_block[-1]):
            raise ValueError(f"resize_apply_batched: src[{k}] has 128 * first_block[B] rows")
        table[k].pad = pad[k].data_ptr() if (pad[k] is not None and pad[k].numel()) else None
        if table[k].pad and pad[k].numel() * pad[k].element_size() != row_bytes:
            raise ValueError(f"resize_apply_batched: pad[{k}] is one row of its tensor")
        table[k].row_bytes, table[k].kind = row_bytes, int(kinds[k])
    flat4 = (C.c_int64 * (4 * len(c4)))(*[v for c in c4 for v in c])
    nfb_c = (C.c_int64 * len(nfb))(*nfb)
    with torch.cuda.device(plan.device):
        stream = torch.cuda.current_stream(plan.device).cuda_stream
        L.check(lib.gsr_resize_apply_batched(plan.data_ptr() if plan.numel() else None, plan.numel() * 4, C.byref(batch), flat4, nfb_c, table,
                                             len(src), meta.data_ptr(), C.c_void_p(stream)), "gsr_resize_apply_batched")
    if check and bool(meta[:, L.GSR_RESIZE_META_STATUS].any().item()):
        raise RuntimeError("resize_apply_batched: the plan holds a row number outside its model: the rows it names were written as zeros")
    return dst, nfb
