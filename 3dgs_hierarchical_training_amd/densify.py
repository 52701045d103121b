"""Adaptive density control around the rasterizer: the consumer of `means2D.grad` and `radii`.

Mirrors, without importing the reference, what HTGaussianModel does with the rasterizer's by-products:
  * statistics          /root/reference/scene/gaussian_model_ht.py:718-721 (`add_densification_stats`: norm of the first
                        two components of the screen-space gradient, accumulated per visible Gaussian) and the
                        `max_radii2D` update of /root/reference/trainer/ht3dgs_trainer.py:141-145
  * clone / split       gaussian_model_ht.py:632-676 (threshold on the mean gradient; small ones are cloned in place,
                        large ones replaced by two samples of themselves at scale / 1.6)
  * prune               gaussian_model_ht.py:678-691 (opacity floor, screen-size and world-size ceilings)
  * schedule            ht3dgs_trainer.py:137-155 (every `densification_interval` iterations after `densify_from_iter`,
                        opacity reset every `opacity_reset_interval`)
These are a few torch ops on N-sized tensors once per 100 iterations -- not a kernel.  The optimizer-state surgery is
GaussianParams' (train_step.py), which works on torch.optim.Adam and FusedAdam alike.

Ordering on the iterations that touch the parameters (round 4).  The reference collects the statistics and
densifies BETWEEN backward() and optimizer.step() (ht3dgs_trainer.py:135-160), and its surgery replaces parameter tensors by
fresh `nn.Parameter`s whose .grad is None -- `densify_and_prune` every one of them (`densification_postfix` runs even when nothing
is selected, gaussian_model_ht.py:584-629), `reset_opacity` the opacity tensor (:468-474) -- so the `optimizer.step()` that
follows finds nothing to step for them: THAT ITERATION'S ADAM UPDATE IS DROPPED (all six groups on a densification iteration,
the opacity group on a reset iteration; their step counts do not advance).  An Adam step fused into the backward kernel would
already have been applied by then.  `touches_parameters_at(iteration)` therefore tells `train_step` -- the schedule is known
before the render -- to run such an iteration UNFUSED: gradients to .grad, statistics, surgery, then a real `optimizer.step()`
on whatever still carries a gradient, exactly the reference's sequence.  One iteration in a hundred.
"""
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F

from . import resize as R


@dataclass
class DensifyConfig:
    """Defaults of /root/reference/arguments/__init__.py:133-147."""
    percent_dense: float = 0.01
    densification_interval: int = 100
    opacity_reset_interval: int = 3000
    densify_from_iter: int = 500
    densify_until_iter: int = 15_000
    densify_grad_threshold: float = 0.0002
    min_opacity: float = 0.005
    reset_until_iter: Optional[int] = None
    max_points: Optional[int] = None      # harness-only safety bound (the reference has none)


def _quat_to_rotmat(q: torch.Tensor) -> torch.Tensor:
    """(w,x,y,z), normalised here -> [n,3,3] (the convention of /root/reference/utils/general_utils.py:76-99)."""
    q = F.normalize(q, dim=1)
    w, x, y, z = q.unbind(1)
    return torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), dim=1).reshape(-1, 3, 3)


class Densifier:
    """Per-model statistics + the clone / split / prune surgery, on a `GaussianParams`."""

    def __init__(self, params, scene_extent: float = 1.0, cfg: Optional[DensifyConfig] = None, seed: int = 0, route: str = "torch"):
        """route: how `densify_and_prune` resizes the model.  "torch" (the default): the statement sequence below it, boolean indexing and
        torch.cat per tensor.  "kernel": the same selections, made with the same torch statements, turned into one flag byte per row and
        handed to gsr_resize_plan / gsr_resize_apply (resize.py): one host wait and one launch that moves every row -- the same tensors,
        moments, statistics and generator state to the bit."""
        self.route = R.check_route(route, "Densifier")
        self.params = params
        self.extent = float(scene_extent)
        self.cfg = cfg or DensifyConfig()
        self.gen = torch.Generator(device=params._xyz.device).manual_seed(seed)
        self.reset_stats()

    def reset_stats(self):
        n, dev = self.params.num_points, self.params._xyz.device
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        self.max_radii2D = torch.zeros((n,), device=dev)

    # ---- gaussian_model_ht.py:718-721 + ht3dgs_trainer.py:141-147 -------------------------------------------------
    @torch.no_grad()
    def add_stats(self, viewspace_points: torch.Tensor, visibility_filter: torch.Tensor, radii: torch.Tensor):
        g = viewspace_points.grad
        if g is None:
            return
        vis = visibility_filter
        self.max_radii2D = torch.where(vis, torch.maximum(self.max_radii2D, radii.to(self.max_radii2D.dtype)), self.max_radii2D)
        self.xyz_gradient_accum += (g[:, :2].norm(dim=-1, keepdim=True)) * vis.unsqueeze(1)
        self.denom += vis.unsqueeze(1).to(self.denom.dtype)

    def fused_stats(self, iteration: int):
        """The three statistics tensors for the backward kernel to accumulate into (rasterize_gaussians_raw densify_stats), or
        None when this iteration collects none (iteration >= densify_until_iter, ht3dgs_trainer.py:137)."""
        if iteration >= self.cfg.densify_until_iter:
            return None
        return (self.xyz_gradient_accum, self.denom, self.max_radii2D)

    def touches_parameters_at(self, iteration: int) -> bool:
        """True when `after_backward(iteration, ...)` will replace parameter tensors (densify / prune, opacity reset): the schedule of
        ht3dgs_trainer.py:148-155, known before the render.  train_step keeps the optimizer out of the backward on such iterations
        (module docstring)."""
        c = self.cfg
        if iteration >= c.densify_until_iter:
            return False
        if iteration > c.densify_from_iter and iteration % c.densification_interval == 0:
            return True
        reset_until = c.reset_until_iter if c.reset_until_iter is not None else c.densify_until_iter
        return iteration % c.opacity_reset_interval == 0 and iteration < reset_until

    def _keep_stats(self, keep: torch.Tensor):
        self.xyz_gradient_accum = self.xyz_gradient_accum[keep]
        self.denom = self.denom[keep]
        self.max_radii2D = self.max_radii2D[keep]

    def _append(self, new):
        self.params.densification_postfix(new)
        self.reset_stats()          # gaussian_model_ht.py:621-629: statistics restart after every append

    def _prune(self, mask: torch.Tensor):
        self.params.prune_points(mask)
        self._keep_stats(~mask)

    # ---- gaussian_model_ht.py:632-691 --------------------------------------------------------------------------------
    @torch.no_grad()
    def densify_and_prune(self, max_grad: float, min_opacity: float, max_screen_size: Optional[float]):
        if self.route == "kernel" and self._densify_and_prune_kernel(max_grad, min_opacity, max_screen_size):
            return
        p = self.params
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        big = p.get_scaling.max(dim=1).values > self.cfg.percent_dense * self.extent

        # clone: under-reconstructed, small
        sel = (grads.norm(dim=-1) >= max_grad) & ~big
        if self.cfg.max_points is not None and p.num_points + int(sel.sum()) > self.cfg.max_points:
            sel = torch.zeros_like(sel)
        if bool(sel.any()):
            self._append({name: getattr(p, attr).detach()[sel] for name, attr in p._GROUP_ATTR.items()})
        else:
            self.reset_stats()      # the reference's densification_postfix runs (and zeroes the statistics) even with nothing selected

        # split: over-reconstructed, large (gradients of the Gaussians that were just appended count as zero)
        n = p.num_points
        padded = torch.zeros(n, device=grads.device)
        padded[:grads.shape[0]] = grads.squeeze(1)
        sel = (padded >= max_grad) & (p.get_scaling.max(dim=1).values > self.cfg.percent_dense * self.extent)
        if self.cfg.max_points is not None and n + int(sel.sum()) > self.cfg.max_points:
            sel = torch.zeros_like(sel)
        k = int(sel.sum())
        if k:
            stds = p.get_scaling.detach()[sel].repeat(2, 1)
            samples = torch.randn(stds.shape, generator=self.gen, device=stds.device) * stds
            rots = _quat_to_rotmat(p._rotation.detach()[sel]).repeat(2, 1, 1)
            new = {"xyz": torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + p._xyz.detach()[sel].repeat(2, 1),
                   "scaling": torch.log(p.get_scaling.detach()[sel].repeat(2, 1) / (0.8 * 2)),
                   "rotation": p._rotation.detach()[sel].repeat(2, 1),
                   "f_dc": p._features_dc.detach()[sel].repeat(2, 1, 1),
                   "f_rest": p._features_rest.detach()[sel].repeat(2, 1, 1),
                   "opacity": p._opacity.detach()[sel].repeat(2, 1)}
            self._append(new)
            self._prune(torch.cat((sel, torch.zeros(2 * k, dtype=torch.bool, device=sel.device))))
        else:
            self.reset_stats()      # (gaussian_model_ht.py:621-629 via :676: unconditional, so max_radii2D is always zero at the prune below)

        mask = (p.get_opacity.detach() < min_opacity).squeeze(1)
        if max_screen_size:
            mask = mask | (self.max_radii2D > max_screen_size) | (p.get_scaling.detach().max(dim=1).values > 0.1 * self.extent)
        if bool(mask.any()):
            self._prune(mask)

    @torch.no_grad()
    def _resize_flags(self, max_grad: float, min_opacity: float, max_screen_size: Optional[float]):
        """The flag byte per row that `densify_and_prune` amounts to (resize.KEEP | CLONE | SPLIT | CHILD), from the torch route's own
        statements: elementwise over the N rows, no host wait, any device; max_grad > 0 is the caller's to check.  Returns (flags, the
        clone selection, get_scaling)."""
        clone, split, gone, child_gone, scaling = self._resize_terms(max_grad, min_opacity, max_screen_size)
        return self._flags_of(clone, split, gone, child_gone), clone, scaling

    @torch.no_grad()
    def _resize_terms(self, max_grad: float, min_opacity: float, max_screen_size: Optional[float]):
        """(clone, split, gone, child_gone, get_scaling): the selections of `_resize_flags`, row by row."""
        p, c = self.params, self.cfg
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        scaling = p.get_scaling.detach()
        smax = scaling.max(dim=1).values
        big = smax > c.percent_dense * self.extent
        clone = (grads.norm(dim=-1) >= max_grad) & ~big
        split = (grads.squeeze(1) >= max_grad) & big
        gone = (p.get_opacity.detach() < min_opacity).squeeze(1)            # the final prune's predicate on a row as it stands
        child_gone = gone
        if max_screen_size:
            stats_term = bool(0.0 > max_screen_size)                         # max_radii2D is all zeros at the final prune
            gone = gone | stats_term | (smax > 0.1 * self.extent)
            child_scaling = torch.exp(torch.log(scaling / (0.8 * 2)))
            child_gone = child_gone | stats_term | (child_scaling.max(dim=1).values > 0.1 * self.extent)
        return clone, split, gone, child_gone, scaling

    @staticmethod
    def _flags_of(clone, split, gone, child_gone):
        return ((~split & ~gone).to(torch.uint8) * R.KEEP + (clone & ~gone).to(torch.uint8) * R.CLONE
                + split.to(torch.uint8) * R.SPLIT + (split & ~child_gone).to(torch.uint8) * R.CHILD)

    def _densify_and_prune_kernel(self, max_grad: float, min_opacity: float, max_screen_size: Optional[float]):
        """`densify_and_prune` on the resize kernels.  Every selection below is the torch route's own statement, evaluated on the N rows the
        call starts with; what the torch route decides about an appended row follows from its source row, because an appended row is a copy:
          * a clone carries its parent's parameters, so the final prune removes it iff it removes the parent;
          * a cloned row is never split: its padded gradient is 0 and max_grad > 0 (hence the refusal of max_grad <= 0);
          * a split parent is removed right after its children are appended, whatever the final prune thinks of it;
          * a child has its parent's opacity and the scale exp(log(get_scaling / 1.6)), and the statistics were zeroed before the final
            prune, so its screen-size term is false.
        The kernels then only order rows and copy them; the children's positions and scales are the torch route's statements on
        index_select(split rows), with the same shapes and the same draw from the generator.  Returns True when the call is done, False
        when `cfg.max_points` cancels the clones or the splits: `meta` says so before anything has been changed or drawn, and the capped
        call is left to the torch route."""
        p, c = self.params, self.cfg
        if not max_grad > 0:
            raise ValueError("Densifier(route='kernel'): max_grad must be positive (a cloned row must not qualify for a split)")
        R.need_device("Densifier(route='kernel')", params=p._xyz)
        flags, clone, scaling = self._resize_flags(max_grad, min_opacity, max_screen_size)
        n = p.num_points
        plan, meta = R.resize_plan(flags)
        counts = R.read_counts(meta, clone.sum() if c.max_points is not None else None)      # the call's one host wait
        nA, nB, nC, nS = counts[:4]
        if c.max_points is not None:
            n_clone = counts[5]
            clones_cancelled = n + n_clone > c.max_points
            if clones_cancelled or n + n_clone + nS > c.max_points:
                return False
        children = None
        if nS:
            rows = R.plan_segment(plan, n, R.L.GSR_RESIZE_PLAN_SPLIT_ROWS, nS)
            parent_scaling = scaling.index_select(0, rows)
            parent_rotation = p._rotation.detach().index_select(0, rows)
            stds = parent_scaling.repeat(2, 1)
            samples = torch.randn(stds.shape, generator=self.gen, device=stds.device) * stds
            rots = _quat_to_rotmat(parent_rotation).repeat(2, 1, 1)
            children = {"xyz": torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + p._xyz.detach().index_select(0, rows).repeat(2, 1),
                        "scaling": torch.log(parent_scaling.repeat(2, 1) / (0.8 * 2))}
        if not (nA == n and nB == 0 and nS == 0):       # (nothing moves: no tensor is replaced, as the torch route replaces none)
            p.resize_by_flags(flags, planned=(plan, meta, counts), children=children)
        self.reset_stats()
        return True

    # ---- ht3dgs_trainer.py:137-155 -------------------------------------------------------------------------------------
    @torch.no_grad()
    def after_backward(self, iteration: int, pkg, stats_done: bool = False) -> bool:
        """Call between backward() and optimizer.step() (drop-in order).  Returns True when the model was resized.
        stats_done: the backward kernel already accumulated this iteration's statistics (`fused_stats`)."""
        c = self.cfg
        if iteration >= c.densify_until_iter:
            return False
        if not stats_done:
            self.add_stats(pkg["viewspace_points"], pkg["visibility_filter"], pkg["radii"])
        resized = False
        if iteration > c.densify_from_iter and iteration % c.densification_interval == 0:
            size_threshold = 20 if iteration > c.opacity_reset_interval else None
            self.densify_and_prune(c.densify_grad_threshold, c.min_opacity, size_threshold)
            # the reference's surgery leaves EVERY parameter a fresh nn.Parameter without .grad, selected or not (module docstring):
            # the optimizer.step() that follows must find nothing to apply
            self.params.optimizer.zero_grad(set_to_none=True)
            resized = True
        reset_until = c.reset_until_iter if c.reset_until_iter is not None else c.densify_until_iter
        if iteration % c.opacity_reset_interval == 0 and iteration < reset_until:
            self.params.reset_opacity()
        return resized


class BatchedDensifier(Densifier):
    """`Densifier` over the B models of a `batched.BatchedGaussianParams`: the same interface (`fused_stats`, `touches_parameters_at`,
    `after_backward`, `add_stats`, `reset_stats`), so `train_step(..., densifier=)` takes it unchanged; the statistics run over the rows of
    the store.  `densify_and_prune` resizes every model at once on the batched resize kernels: the flag bytes are `_resize_flags`'
    statements over the whole store, one `resize_plan_batched`, one host read, the children of model b drawn with the model's own
    generator (seeds[b]) at the model's own shape -- the draw `Densifier(seed=seeds[b])` makes for it alone, whatever else is in the batch
    -- and one `resize_models`.  `cfg.max_points` caps each model on its own (max_points=[...]: one cap per model instead)."""

    def __init__(self, params, scene_extent: float = 1.0, cfg: Optional[DensifyConfig] = None, seeds=None, max_points=None):
        if not hasattr(params, "first_block"):
            raise ValueError("BatchedDensifier: params is a batched.BatchedGaussianParams")
        seeds = list(range(params.num_models)) if seeds is None else [int(s) for s in seeds]
        if len(seeds) != params.num_models:
            raise ValueError("BatchedDensifier: one seed per model of the batch")
        super().__init__(params, scene_extent, cfg, seed=seeds[0], route="kernel")
        self.gens = [torch.Generator(device=params._xyz.device).manual_seed(s) for s in seeds]
        self.gen = None          # (every draw is a model's own)
        if max_points is not None and len(max_points) != params.num_models:
            raise ValueError("BatchedDensifier: max_points has one cap per model of the batch")
        self.max_points = None if max_points is None else [int(m) for m in max_points]

    def _caps(self):
        """The cap of every model, or None when nothing is capped."""
        if self.max_points is not None:
            return self.max_points
        return None if self.cfg.max_points is None else [self.cfg.max_points] * self.params.num_models

    @staticmethod
    def cap_decisions(caps, counts, n_clone, n_split):
        """Per model (clones cancelled, splits cancelled) under its cap: the torch route's rule on the model's own numbers."""
        out = []
        for cap, n, nc, ns in zip(caps, counts, n_clone, n_split):
            clones_cancelled = n + nc > cap
            out.append((clones_cancelled, n + (0 if clones_cancelled else nc) + ns > cap))
        return out

    @staticmethod
    def capped_flags(terms, decisions, row_slices):
        """The flag bytes with the capped models' selections cancelled on their rows: cancelled clones clear CLONE; a cancelled split row
        is no split parent any more, so it is KEEP iff the final prune keeps it."""
        clone, split, gone, child_gone = (t.clone() if k < 2 else t for k, t in enumerate(terms[:4]))
        for (clones_cancelled, splits_cancelled), rows in zip(decisions, row_slices):
            if clones_cancelled:
                clone[rows] = False
            if splits_cancelled:
                split[rows] = False
        return Densifier._flags_of(clone, split, gone, child_gone)

    @torch.no_grad()
    def densify_and_prune(self, max_grad: float, min_opacity: float, max_screen_size: Optional[float]):
        p, c = self.params, self.cfg
        if not max_grad > 0:
            raise ValueError("BatchedDensifier: max_grad must be positive (a cloned row must not qualify for a split)")
        R.need_device("BatchedDensifier", params=p._xyz)
        terms = self._resize_terms(max_grad, min_opacity, max_screen_size)
        clone, scaling = terms[0], terms[4]
        flags = self._flags_of(*terms[:4])
        nb = p.num_models
        slices = [p.model_rows(b) for b in range(nb)]
        plan, meta = R.resize_plan_batched(flags, p.first_block, p.counts)
        caps = self._caps()
        if caps is None:
            rows = R.read_counts_batched(meta)                        # the call's one host wait
        else:                                                         # (a padding row is never selected: its gradient is 0 < max_grad)
            rows, n_clone = R.read_counts_batched(meta, torch.stack([clone[s].sum() for s in slices]))
            decisions = self.cap_decisions(caps, p.counts, n_clone, [r[3] for r in rows])
            if any(a or b for a, b in decisions):                     # a capped call: the plan again, and a second wait
                flags = self.capped_flags(terms, decisions, slices)
                plan, meta = R.resize_plan_batched(flags, p.first_block, p.counts)
                rows = R.read_counts_batched(meta)
        children = None
        if any(r[3] for r in rows):
            stride = R.plan_stride(p.num_points)
            xyz, child_scaling = [], []
            for b in range(nb):
                nS = rows[b][3]
                if not nS:
                    continue
                at = R.L.GSR_RESIZE_PLAN_SPLIT_ROWS * stride + R.BLOCK * p.first_block[b]
                parents = plan[at: at + nS]                            # store rows
                parent_scaling = scaling.index_select(0, parents)
                parent_rotation = p._rotation.detach().index_select(0, parents)
                stds = parent_scaling.repeat(2, 1)
                samples = torch.randn(stds.shape, generator=self.gens[b], device=stds.device) * stds
                rots = _quat_to_rotmat(parent_rotation).repeat(2, 1, 1)
                xyz.append(torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + p._xyz.detach().index_select(0, parents).repeat(2, 1))
                child_scaling.append(torch.log(parent_scaling.repeat(2, 1) / (0.8 * 2)))
            children = {"xyz": torch.cat(xyz, dim=0), "scaling": torch.cat(child_scaling, dim=0)}
        if not all(r[0] == n and r[1] == 0 and r[3] == 0 for r, n in zip(rows, p.counts)):      # (nothing moves: no tensor is replaced)
            p.resize_models(flags, planned=(plan, meta, rows), children=children)
        self.reset_stats()
