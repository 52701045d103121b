"""B independent models trained in ONE launch chain (include/gsr.h GsrBatch).

Stage A of the reference -- ~70 % of a scene's render calls -- fits F - 1 single-image models that share nothing
(`for fidx in range(1, seq_len): compute_relative_pose(fidx, fidx - 1)`, /root/reference/trainer/ht3dgs_trainer.py:697-698,
:336-431; the authors note the independence, /root/reference/README.md:131).  One such model (~130 k Gaussians, one 980x545
image) is a chain of ~17 dependent kernels whose sorts, scans and per-Gaussian passes each fill a fraction of an MI355X.  Here B
of them share one parameter store: model b owns the 128-Gaussian blocks [first_block[b], first_block[b + 1]) (each model is
padded to a multiple of 128 with Gaussians that can never be drawn), every kernel of the chain runs once over all of them, and
the B images come back as [B,3,H,W].  Each model's image, radii and parameter updates are bit-identical with training it alone
(tests/test_gpu_batched.py): the B images form one tall tile grid, so a tile's list only ever holds its own model's Gaussians.
"""
from typing import Dict, List, Sequence

import torch

from . import resize as R
from .rasterizer import GaussianRasterizationSettings
from .train_step import GaussianParams

BLOCK = 128


def _pad_rows(t: torch.Tensor, n_pad: int, fill: torch.Tensor) -> torch.Tensor:
    if n_pad == 0:
        return t
    return torch.cat((t, fill.to(device=t.device, dtype=t.dtype).expand((n_pad,) + tuple(t.shape[1:]))), dim=0)     # (scenes built on the device stay there)


def pad_scene_rows(sh_coeffs: int) -> Dict[str, torch.Tensor]:
    """One padding Gaussian as a scene holds it (activated values): far behind every camera, opacity below the 1/255 threshold."""
    return {"means3D": torch.tensor([[0.0, 0.0, -1.0e3]]), "shs": torch.zeros(1, sh_coeffs, 3), "scales": torch.full((1, 3), 1e-3),
            "rotations": torch.tensor([[1.0, 0.0, 0.0, 0.0]]), "opacities": torch.full((1, 1), 1e-4)}


def raw_pad_rows(sh_coeffs: int, device) -> Dict[str, torch.Tensor]:
    """The padding row of each of the six raw tensors on `device`: `pad_scene_rows` through `GaussianParams.raw_from_scene`, the statements a
    freshly built batch's padding rows went through on the same device -- so a padding row written by a resize equals one bit for bit."""
    return GaussianParams.raw_from_scene(pad_scene_rows(sh_coeffs), device)


def concat_scenes(scenes: Sequence[Dict]) -> Dict:
    """One scene dict holding the models back to back, each padded to a multiple of 128 Gaussians.  Padding rows sit far behind
    every camera with an opacity below the 1/255 threshold: culled by the near plane and by the exact tile test alike, they get no
    instance, no gradient, and Adam leaves them where they are (zero gradient, zero moments).  Returns the scene with
    `first_block` (B + 1 block offsets) and `counts` (the models' true sizes)."""
    parts, first_block, counts = {k: [] for k in ("means3D", "shs", "scales", "rotations", "opacities")}, [0], []
    for sc in scenes:
        n = sc["means3D"].shape[0]
        n_pad = (-n) % BLOCK
        pad = pad_scene_rows(sc["shs"].shape[1])
        for k in parts:
            parts[k].append(_pad_rows(sc[k], n_pad, pad[k]))
        counts.append(n)
        first_block.append(first_block[-1] + (n + n_pad) // BLOCK)
    out = dict(scenes[0])
    for k, v in parts.items():
        out[k] = torch.cat(v, dim=0).contiguous()
    out["first_block"], out["counts"] = first_block, counts
    return out


def batch_settings(views: Sequence[GaussianRasterizationSettings], device) -> GaussianRasterizationSettings:
    """One settings tuple for B renders: the cameras stacked ([B,4,4], [B,4,4], [B,3]); image size, field of view, background,
    degree and scale modifier are shared and must agree."""
    v0 = views[0]
    for v in views[1:]:
        if (v.image_height, v.image_width, v.tanfovx, v.tanfovy, v.sh_degree, v.scale_modifier) != \
                (v0.image_height, v0.image_width, v0.tanfovx, v0.tanfovy, v0.sh_degree, v0.scale_modifier):
            raise ValueError("batch_settings: the views of a batch share image size, field of view, SH degree and scale modifier")
    return v0._replace(viewmatrix=torch.stack([v.viewmatrix.to(device).float() for v in views]).contiguous(),
                       projmatrix=torch.stack([v.projmatrix.to(device).float() for v in views]).contiguous(),
                       campos=torch.stack([v.campos.to(device).float() for v in views]).contiguous())


class BatchedGaussianParams(GaussianParams):
    """`GaussianParams` over B models stored back to back (`first_block`, `counts`); one optimizer steps them all (they advance
    in lockstep, as B stage-A fits started together do).  `train_step.render` / `train_step.train_step` recognise the batch by
    `first_block` and return [B,3,H,W] images; targets are [B,3,H,W]."""

    def __init__(self, scenes: Sequence[Dict], device, spatial_lr_scale: float = 1.0, optimizer: str = "hip"):
        sc = concat_scenes(scenes)
        super().__init__(sc, device, spatial_lr_scale=spatial_lr_scale, optimizer=optimizer)
        self.first_block: List[int] = list(sc["first_block"])
        self.counts: List[int] = list(sc["counts"])
        self._raw_pad_rows()

    def _raw_pad_rows(self) -> Dict[str, torch.Tensor]:
        """The six raw padding rows on the store's device, made once (the host-to-device copies behind them are waits a resize need not
        repeat)."""
        pads = getattr(self, "_pad_rows", None)
        if pads is None or pads["_xyz"].device != self._xyz.device:
            pads = self._pad_rows = raw_pad_rows(self._features_rest.shape[1] + 1, self._xyz.device)
        return pads

    @property
    def num_models(self) -> int:
        return len(self.counts)

    # new_retire_table() / retired_sync() (train_step.GaussianParams): one entry per model of the batch.  Models cannot be REMOVED from a
    # batch (prune_points below); a retired one stays in the store, culled from every render and skipped by every update.

    def model_rows(self, b: int) -> slice:
        """Rows of model b's own (un-padded) Gaussians."""
        lo = self.first_block[b] * BLOCK
        return slice(lo, lo + self.counts[b])

    def model_raw(self, b: int) -> Dict[str, torch.Tensor]:
        """Model b's six raw tensors (views of the store, detached): what `capture()` would hold for it."""
        r = self.model_rows(b)
        return {k: getattr(self, k).detach()[r] for k in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")}

    # Resizing one model of a batch moves every later model's blocks, so the single-model calls stay refused: the whole store is resized
    # at once, by the batched resize kernels (resize_models / prune_models; densify.BatchedDensifier is the caller that densifies).
    _REFUSAL = ("BatchedGaussianParams: the models of a batch cannot be resized by the single-model calls "
                "(resize_models / prune_models resize them all at once)")

    def prune_points(self, mask, route="torch"):
        raise RuntimeError(BatchedGaussianParams._REFUSAL)

    def densification_postfix(self, new, route="torch"):
        raise RuntimeError(BatchedGaussianParams._REFUSAL)

    def resize_by_flags(self, flags, planned=None, children=None):
        raise RuntimeError(BatchedGaussianParams._REFUSAL)

    def resize_models(self, flags: torch.Tensor, planned=None, children: Dict[str, torch.Tensor] = None):
        """Every model of the batch resized at once: flags (uint8 over the rows of the store, resize.KEEP | CLONE | SPLIT | CHILD; the bytes
        of padding rows are ignored) -> all six groups and the moments that exist replaced by the tensors of the new store, through one
        gsr_resize_apply_batched launch, padding rows included; `first_block` and `counts` follow.  Model b comes out as
        `GaussianParams.resize_by_flags` leaves it alone, bit for bit, and a padding row as a freshly built batch has it.  planned = (plan,
        meta, rows) when the caller has run `resize.resize_plan_batched` and read meta already; children = {"xyz", "scaling"} -> the
        models' surviving split children back to back ([2 sum nSplit_b, 3]).  One host wait (none with `planned`).  Returns the per-model
        counts [(nA, nB, nC, nSplit)]."""
        R.need_device("BatchedGaussianParams.resize_models", flags=flags, params=self._xyz)
        plan, meta, rows = planned if planned is not None else (None, None, None)
        if plan is None:
            plan, meta = R.resize_plan_batched(flags, self.first_block, self.counts)
            rows = R.read_counts_batched(meta)          # the one host wait
        counts4 = [tuple(int(v) for v in r[:4]) for r in rows]
        pads = self._raw_pad_rows()
        entries, src, kinds, child, pad = [], [], [], [], []
        for g in self.optimizer.param_groups:
            p = g["params"][0]
            st = self.optimizer.state.get(p)
            sourced = children is not None and g["name"] in children
            entries.append((g, st is not None))
            src.append(p.detach()); kinds.append(R.CHILD_SOURCED if sourced else R.PARAM)
            child.append(children[g["name"]] if sourced else None); pad.append(pads[self._GROUP_ATTR[g["name"]]])
            if entries[-1][1]:        # (moments an optimizer has not created yet have nothing to move)
                for k in ("exp_avg", "exp_avg_sq"):
                    src.append(st[k]); kinds.append(R.MOMENT); child.append(None); pad.append(None)
        tensors, new_first_block = R.resize_apply_batched(plan, meta, self.first_block, self.counts, counts4, src, kinds, child, pad)
        out = iter(tensors)
        for g, has_moments in entries:
            new = next(out)
            self._install_group_tensor(g, new, (next(out), next(out)) if has_moments else None)
        self._screenspace_zero = None
        self.first_block = list(new_first_block)
        self.counts = [nA + nB + 2 * nC for nA, nB, nC, _ in counts4]
        return counts4

    def prune_models(self, mask: torch.Tensor):
        """Remove the Gaussians where mask (bool over the rows of the store) is True, in every model at once.  A model that loses every
        row keeps one block of padding."""
        R.need_device("BatchedGaussianParams.prune_models", mask=mask, params=self._xyz)
        return self.resize_models((~mask).to(torch.uint8))          # KEEP = 1
