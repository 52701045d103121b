"""gsr_autopatch -- opt-in fast path for the UNMODIFIED reference trainer.

The reference builds its optimizer and its loss from stock torch pieces:
  * `torch.optim.Adam(l, lr=0.0, eps=1e-15)` over six groups named xyz / f_dc / f_rest / opacity / scaling / rotation
    (/root/reference/scene/gaussian_model_ht.py:275-289) -> foreach Adam: ~1 ms per step at 1 M Gaussians;
  * `Loss.forward` = (1 - l) L1 + l (1 - SSIM) with an 11x11 depthwise `F.conv2d` SSIM
    (/root/reference/trainer/losses.py:98-136, :164-251) -> ~2.7 ms per step at 980x545.
Importing this module BEFORE the trainer swaps both for the HIP kernels of this library without touching a reference file:

    python -m gsr_autopatch run.py --mode train --config arguments/full/Tanks/Francis.yml      # runs run.py under the patches
    # or, at the top of your own launcher:  import gsr_autopatch

  * `torch.optim.Adam(...)` whose parameter groups carry exactly those six names returns a `FusedAdam` (same `param_groups` /
    `state` / `state_dict` protocol, so the model's prune / densify / opacity-reset surgery and capture / restore run on it
    unchanged; one HIP launch per `step()`); every other Adam construction is the stock class;
  * `trainer.losses.Loss.forward` (patched when that module is imported, now or later) evaluates L1 + SSIM forward and backward
    in the fused loss kernels (gsr_loss_forward / gsr_loss_backward) and returns the same dict (`loss`, `loss_rgb`,
    `loss_dssim`, `loss_depth`); the depth term, when enabled, stays the reference's own code.

  * `scene.gaussian_model_ht.CF3DGS_Render.render` (round 4; patched when that module is imported, now or later) hands the model's
    RAW parameter tensors (`_xyz, _features_dc, _features_rest, _opacity, _scaling, _rotation`) to `rasterize_gaussians_raw`: the
    wrapper's torch exp / sigmoid / normalize / cat (and their backward kernels) run inside the preprocess kernels, `get_xyz`'s
    pose action `P[idx].retr().act(xyz)` becomes the in-kernel `points_transform`, and the gradients arrive on the raw tensors
    directly, where `optimizer.step()` picks them up.  With the FusedAdam this module hands out, the backward kernel also computes
    that step's Adam update into SHADOW buffers (the model untouched) and `optimizer.step()` adopts it by swapping storages: the
    trainer's order -- densify / prune / opacity reset BEFORE the step, `update_gaussians=False`, the update dropped when
    `densify_and_prune` replaces every parameter (ht3dgs_trainer.py:137-160) -- is untouched, the separate 1.65 kB-per-Gaussian
    optimizer pass is gone.  (`GSR_AUTOPATCH_DEFERRED=0`: gradients to .grad and a one-launch FusedAdam.step() instead;
    `GSR_AUTOPATCH_DEFERRED_MIN_N`: the same for models below that many Gaussians, default 0.)  The returned dict is the
    reference's (`image` clamped, `depth`, `alpha`, `viewspace_points` whose .grad the backward fills, `visibility_filter`,
    `radii`).  `convert_SHs_python=True` with `view_dependent` (the trainer's default) takes the same route: the SH colour is
    evaluated in the kernels in the reference's direction, normalize(`_xyz` - `get_RT(uid).inverse()[:3, 3]`) of the UNposed means
    (gaussian_model_ht.py:845-865, include/gsr.h GsrForwardArgs::sh_origin); `GSR_AUTOPATCH_PYTHON_SH=0` keeps it on the original
    method.  `override_color`, `compute_cov3D_python`, `convert_SHs_python` without `view_dependent`, CPU tensors or an unexpected
    parameter layout fall back to the ORIGINAL method.  `GSR_AUTOPATCH_RENDER=0` leaves the method alone; `GSR_AUTOPATCH_POSE=0` keeps pose
    renders (rotate_xyz / rotate_seq) on the original method.
  * the frame poses (round 6): a lietorch SE3 `LieGroupParameter` that `get_xyz` reads (`P[k]`, gaussian_model_ht.py:135-148,
    :346-386) reaches the rasterizer through ONE autograd node over its six tangent numbers (`torch.ops.gsr.pose_matrix`: the [3,4]
    `points_transform` from one one-wave kernel, `.grad` of the parameter from another), and the pose optimizers the reference
    builds over such parameters -- `camera_optimizer[k]` (:296-311, stepped after every render: ht3dgs_trainer.py:162-166) and
    stage A's `training_setup_fix_position(gaussian_rot=False)` (:321-333) -- are `FusedPoseAdam` objects: one launch per
    `step()`.  The reference's ~50 small lietorch / torch launches per iteration (exponential map, group product, `matrix()`, their
    backward, Adam on six numbers) become three.  `GSR_AUTOPATCH_POSE_FUSED=0` keeps lietorch's chain and the stock Adam.
  * `HTGaussianModel.add_densification_stats` (same module) accumulates the same two sums without the boolean-mask gathers
    (each of them a `nonzero` + host synchronisation): one masked-add launch over N (gsr_densify_stats_add).
  * the render's `visibility_filter` is a bool-tensor subclass (`LazyMask`) under which the trainer's
    `max_radii2D[vis] = torch.max(max_radii2D[vis], radii[vis])` is one launch (gsr_masked_max) instead of three `nonzero`s;
    `utils.image_utils.psnr` (the training PSNR of every iteration) is two launches (gsr_psnr).  `GSR_AUTOPATCH_LAZY_MASK=0` /
    `GSR_AUTOPATCH_PSNR=0` switch those off.
  * `trainer.ht3dgs_trainer.HTGaussianTrainer.calc_importance` (the colour-importance score of every merge, ht3dgs_trainer.py:1427-1462;
    patched when that module is imported, now or later) runs, per camera, one forward and the importance pass
    (`torch.ops.gsr.importance_accumulate`, include/gsr.h gsr_importance_accumulate) on the raw tensors instead of a render and a full
    backward, and returns the same [N, 48] tensor.  One side effect differs: the reference leaves the summed |grad| in
    `_features_dc.grad` / `_features_rest.grad`, the patched form leaves them None (`merge_two_3DGS` builds new tensors right after
    and reads neither).  `compute_cov3D_python`, an override colour, `convert_SHs_python` without `view_dependent`, an unknown pose
    object, CPU tensors or an unexpected layout run the ORIGINAL method; `GSR_AUTOPATCH_IMPORTANCE=0` leaves the method alone.

  * `trainer.trainer.GaussianTrainer.load_viewpoint_cam` (patched when that module is imported, now or later): the frame loader the trainer
    calls before EVERY iteration (/root/reference/trainer/trainer.py:989-1142) converts the frame's image again and builds a new `Camera`
    (/root/reference/scene/cameras.py:17-101: an upload of the image, a multiply, three small uploads, a `bmm`, an `inverse()` that waits for
    the device) on every call.  Patched, the FIRST call for a frame runs the original and keeps, per trainer and on the device, the
    original's `original_image` tensor itself and the camera's pose-independent fields; later calls return a `Camera` assembled without
    `Camera.__init__` -- identity cameras from cached tensors, posed ones from one launch of gsr_camera_from_pose.  Calls with work the
    cache cannot know (`pose_to_train=True`, `load_depth` / `load_vfi` whose result is not in `mono_depth` / `vfi` yet), a frame whose
    cached image somebody wrote into, and frames beyond `GSR_AUTOPATCH_FRAMES_MB` (default 16384) run the original.
    `HTGaussianModel.get_RT` returns a `DevicePose`, a tensor subclass whose `.cpu()` is itself, so that the trainer's
    `get_RT(fidx).detach().cpu()` no longer waits for the device; `.numpy()`, an operation with a genuine CPU tensor and the original
    loader get the host values at the old cost.  `GSR_AUTOPATCH_FRAMES=0` leaves both methods alone.

  * `scene.gaussian_model_ht.HTGaussianModel.densify_and_prune` and `prune_points` (/root/reference/scene/gaussian_model_ht.py:548-695;
    the trainer's call at ht3dgs_trainer.py:152-153, `merge_two_3DGS`'s at :241; patched when that module is imported, now or later):
    the selections stay torch statements on the model's own properties (`get_scaling`, `get_opacity`, `scaling_inverse_activation`,
    the module's `build_rotation`), become one flag byte per row, and gsr_resize_plan / gsr_resize_apply (resize.py) move every
    parameter and moment in one launch after ONE host wait; the reference's boolean indexing and `torch.cat` per tensor wait 59 times
    per `densify_and_prune` and 21 times per `prune_points`.  Same rows in the same order, fresh `nn.Parameter`s without .grad, state
    dicts re-keyed with `step` kept, statistics zeroed, the same children from the same draw of the default CUDA generator,
    `torch.cuda.empty_cache()` last (`GSR_AUTOPATCH_EMPTY_CACHE=0`: not called; default 1, the reference's behaviour).  A
    `max_grad` that is not positive, an optimizer that is not exactly the six named groups of one parameter each, a CPU, non-float32,
    non-contiguous or wrongly sized tensor, N = 0, moments unlike their parameter or a `mask` that is not a bool tensor [N] run the
    ORIGINAL method.  Measured on one MI355X with `empty_cache()` in both arms (tools/trainer_resize_probe.py,
    profiles/trainer_resize.txt): densify_and_prune 13.27 -> 2.89 ms at 1 M / degree 3, 7.93 -> 1.51 at 300 k / degree 3, 6.82 -> 1.08
    at 130 k / degree 0, beyond the same-arm spread (<= 0.40 ms) at all three sizes -- GSR_AUTOPATCH_RESIZE: ships ON
    (`GSR_AUTOPATCH_RESIZE=0` leaves both methods alone).

  * `trainer.ht3dgs_trainer.HTGaussianTrainer.merge_two_3DGS` (trainer/ht3dgs_trainer.py:214-272; patched where
    `calc_importance` is, through the same hook): the same log lines, the same `load_viewpoint_cam` calls in the same order, both scores
    through `HTGaussianTrainer.calc_importance` as the class holds it at the call (the patched one above, or a user's own); then
    gsr_select_smallest per model on the [N, C] score as it stands instead of `amax`, `topk`, a zero fill and an indexed store; the
    reference's own three torch statements for the moved points on all source rows (the floats are the unpatched trainer's to the bit);
    two gsr_resize_plan and ONE gsr_merge_apply over the destination's six parameters and twelve moments (kept rows copied, appended rows
    zero) instead of `prune_points`, twelve boolean gathers and `densification_postfix`; installed as the resize patch installs, statistics
    zeroed.  The kept counts are N - int(N * prune_ratio) by construction, so from the scores on the call does not wait for the device
    (the stand-in's statements: 29 synchronisation warnings).  Nothing of the source model is written.  THE TIE RULE is the patch's own:
    among rows whose score equals the k-th smallest, the rows with the lowest row numbers go, where `torch.topk` promises nothing; with
    distinct scores at the threshold the result is the unpatched trainer's to the bit; where they tie (unseen Gaussians, score exactly
    0) as many rows go, every row strictly below the threshold goes, and the tied rows that go are the lowest-numbered.  A model outside
    the resize patch's layout (the source: its six tensors), two models of unlike trailing shapes / dtype / device, a `transform_matrix`
    that is not a float32 [4,4] tensor on that device, a `prune_ratio` that is not a number in [0, 1] or a model of fewer than 2 rows
    run the ORIGINAL method, decided before a camera is loaded; an importance of another shape, dtype or device, or wider than
    GSR_SELECT_MAX_COLUMNS, finishes the call with the reference's own statements on that importance.  Measured on one MI355X against
    the stand-in of the same process, every other patch installed in both arms (tools/trainer_merge_probe.py,
    profiles/trainer_merge.txt; two models of N rows, ratio 0.5, 30 % zero scores): 2.42 -> 1.03 ms at 1 M / degree 3, 1.54 -> 0.65 at
    300 k / degree 3, 1.27 -> 0.55 at 130 k / degree 0 with prepared scores, 3.91 -> 2.59, 2.53 -> 1.60, 2.16 -> 1.33 with
    `calc_importance` over two views per model, beyond the same-arm spread (<= 0.02 ms) at all three sizes; the peak allocation of the
    call is higher (767 against 463 MiB at 1 M: all 18 destinations exist before the old tensors are released) --
    GSR_AUTOPATCH_MERGE: ships ON (`GSR_AUTOPATCH_MERGE=0` leaves the method alone).

`apply()` / `remove()` switch the patches on and off (importing the module calls `apply()`); `GSR_AUTOPATCH=0` disables them.
The rasterizer itself needs no patch: `diff_gaussian_rasterization` IS this library's drop-in package.
"""
import importlib
import importlib.abc
import importlib.machinery
import math
import numbers
import os
import sys

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

FUSED_NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
_ORIG_ADAM = torch.optim.Adam
_applied = False
_patched_loss_classes = []          # [(class, original forward)]
LOSS_MODULES = ("trainer.losses",)
RENDER_MODULES = ("scene.gaussian_model_ht",)
TRAINER_MODULES = ("trainer.ht3dgs_trainer",)
FRAME_MODULES = ("trainer.trainer",)
_patched_frame_classes = []         # [(class, attribute, original function)]: GaussianTrainer.load_viewpoint_cam, HTGaussianModel.get_RT
_patched_trainer_classes = []       # [(class, attribute, original attribute as found in the class __dict__)]
_patched_render_classes = []        # [(class, attribute, original function)]
RAW_NAMES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
_REQUIRE_CUDA = True                # (tests drive the dispatch logic with CPU stand-ins and a recording rasterizer)


def _pkg():
    return importlib.import_module("3dgs_hierarchical_training_amd.optim"), importlib.import_module("3dgs_hierarchical_training_amd.loss")


def _ops():
    return importlib.import_module("3dgs_hierarchical_training_amd._ext").load()


def _wants_fused(params, kw) -> bool:
    """The reference's construction: a list of group dicts, one tensor each, named exactly the six groups; no amsgrad, no weight
    decay, parameters on the GPU."""
    try:
        groups = list(params)
    except TypeError:
        return False
    if len(groups) != 6 or not all(isinstance(g, dict) for g in groups):
        return False
    if sorted(g.get("name", "") for g in groups) != sorted(FUSED_NAMES):
        return False
    if kw.get("amsgrad") or kw.get("weight_decay") or kw.get("maximize"):
        return False
    for g in groups:
        ps = list(g["params"]) if not torch.is_tensor(g["params"]) else [g["params"]]
        if len(ps) != 1 or not ps[0].is_cuda or ps[0].dtype != torch.float32:
            return False
    return True


def _wants_pose(params, kw) -> bool:
    """The reference's pose optimizers: `torch.optim.Adam([{'params': [P[k]], 'lr': ..., 'name': 'R'}], lr=0.0, eps=1e-15)` -- one per
    frame (`camera_optimizer[k]`, /root/reference/scene/gaussian_model_ht.py:296-311) or the model's `optimizer` during stage A's pose
    fit (`training_setup_fix_position(gaussian_rot=False)`, :321-333): every parameter a lietorch SE3 `LieGroupParameter` on the GPU."""
    if os.environ.get("GSR_AUTOPATCH_POSE_FUSED", "1") == "0":
        return False
    try:
        groups = list(params)
    except TypeError:
        return False
    if not groups or not all(isinstance(g, dict) for g in groups) or kw.get("amsgrad") or kw.get("weight_decay") or kw.get("maximize"):
        return False
    P = importlib.import_module("3dgs_hierarchical_training_amd.pose_opt")
    for g in groups:
        ps = [g["params"]] if torch.is_tensor(g["params"]) else list(g["params"])
        if not ps or not all(P.is_lie_pose(q) and (q.is_cuda or not _REQUIRE_CUDA) for q in ps):
            return False
    return True


class _AdamMeta(type(_ORIG_ADAM)):
    """`isinstance(opt, torch.optim.Adam)` keeps answering True for everything the patched name constructs (stock Adam objects and
    FusedAdam), as it did before the patch."""

    def __instancecheck__(cls, inst):
        if cls is _AdamDispatch:
            if isinstance(inst, _ORIG_ADAM):
                return True
            optim, pose_opt = sys.modules.get("3dgs_hierarchical_training_amd.optim"), sys.modules.get("3dgs_hierarchical_training_amd.pose_opt")
            return (optim is not None and isinstance(inst, optim.FusedAdam)) or (pose_opt is not None and isinstance(inst, pose_opt.FusedPoseAdam))
        return super().__instancecheck__(inst)


class _AdamDispatch(_ORIG_ADAM, metaclass=_AdamMeta):
    """`torch.optim.Adam` while the patch is applied: constructs FusedAdam for the reference's six-group optimizer, FusedPoseAdam
    for its pose optimizers (groups of lietorch SE3 parameters, `_wants_pose`) and the stock Adam for everything else.  (Returning an object that is not an instance of this class from __new__ skips __init__.)
    A SUBCLASS defined while the patch is applied (`class My(torch.optim.Adam)`) constructs normally: the dispatch only fires for
    the patched name itself."""

    def __new__(cls, params=None, *args, **kw):
        if cls is not _AdamDispatch:
            return super().__new__(cls)
        params = list(params)
        if _wants_fused(params, kw) and not args:
            optim, _ = _pkg()
            groups = [dict(g, params=[g["params"]] if torch.is_tensor(g["params"]) else list(g["params"])) for g in params]
            return optim.FusedAdam(groups, lr=kw.get("lr", 1e-3), betas=kw.get("betas", (0.9, 0.999)), eps=kw.get("eps", 1e-8))
        if _wants_pose(params, kw) and not args:
            P = importlib.import_module("3dgs_hierarchical_training_amd.pose_opt")
            groups = [dict(g, params=[g["params"]] if torch.is_tensor(g["params"]) else list(g["params"])) for g in params]
            return P.FusedPoseAdam(groups, lr=kw.get("lr", 1e-3), betas=kw.get("betas", (0.9, 0.999)), eps=kw.get("eps", 1e-8))
        return _ORIG_ADAM(params, *args, **kw)


def loss_forward(self, rgb_pred, rgb_gt, depth_pred=None, depth_gt=None, rgb_loss_type='l1', **kwargs):
    """Drop-in body of `trainer.losses.Loss.forward` (/root/reference/trainer/losses.py:98-136): same arguments, same returned
    dict; the photometric part is ONE fused forward (+ one fused backward) instead of ~25 torch kernels."""
    _, loss_mod = _pkg()
    lambda_dssim = float(self.cfg.lambda_dssim)
    lambda_depth = float(getattr(self.cfg, "lambda_depth", 0.0))
    rgb_gt = rgb_gt.to(rgb_pred.device)
    if rgb_pred.dim() != 3 or not rgb_pred.is_cuda:       # not the [3,H,W] device image the fused kernels take: the original code
        orig = next((f for c, f in _patched_loss_classes if isinstance(self, c)), None)
        if orig is None:
            raise RuntimeError("gsr_autopatch.loss_forward: needs a [C,H,W] image on the GPU")
        return orig(self, rgb_pred, rgb_gt, depth_pred, depth_gt, rgb_loss_type, **kwargs)
    raw = getattr(rgb_pred, "_gsr_raw", None)      # the patched render's un-clamped colour output (render_fused below), valid while
    fused_clamp = raw is not None and raw[1] == rgb_pred._version and raw[0].shape == rgb_pred.shape     # nobody wrote into the clamped image
    src = raw[0] if fused_clamp else rgb_pred
    want_depth = lambda_depth != 0.0 and depth_pred is not None and depth_gt is not None
    if want_depth and _fused_depth_route(self, rgb_pred, depth_pred, depth_gt):
        # the depth term on the kernels as well (include/gsr.h gsr_depth_loss_*): the reference's two masked assignments are ONE in-place
        # clamp of the caller's plane -- it holds the clamped values afterwards and strictly clamped pixels get zero gradient, as at
        # losses.py:116-117 -- then one dispatcher call writes the whole dict; no host synchronisation (the reference's statements have
        # three: `det.nonzero()` and `if divisor == 0` twice)
        depth_pred.clamp_(0.02, 20.0)
        loss, terms = loss_mod.fused_training_loss_report(src, rgb_gt, depth_pred, depth_gt.to(rgb_pred.device), lambda_dssim, lambda_depth,
                                                          self.depth_loss_type, clamp=fused_clamp)
        return {'loss': loss, 'loss_rgb': terms[3], 'loss_dssim': terms[4], 'loss_depth': terms[5]}
    if _ext_binding() and os.environ.get("GSR_AUTOPATCH_LOSS_REPORT", "1") != "0":
        # one dispatcher call: the finishing kernel wrote every entry of the returned dict (loss_rgb, loss_dssim, a zero loss_depth);
        # the entries are views of its six-float result -- no torch kernel per term, no zero fills in the backward
        loss, terms = loss_mod.fused_photometric_loss_report(src, rgb_gt, lambda_dssim, clamp=fused_clamp)
        rgb_full_loss, dssim_loss, zero_depth = terms[3], terms[4], terms[5]
    else:
        loss, ssim_v, l1_v = loss_mod.fused_photometric_loss_terms(src, rgb_gt, lambda_dssim, clamp=fused_clamp)
        rgb_full_loss = (1.0 - lambda_dssim) * l1_v
        dssim_loss = 1.0 - ssim_v
        zero_depth = None
    if want_depth:      # GSR_AUTOPATCH_DEPTH_LOSS=0, another depth_loss_type, shape or device: the reference's own statements
        depth_gt = depth_gt.to(rgb_pred.device)
        depth_pred[depth_pred < 0.02] = 0.02
        depth_pred[depth_pred > 20.0] = 20.0
        depth_loss = self.get_depth_loss(depth_pred.squeeze(), depth_gt.squeeze())
        loss = loss + lambda_depth * depth_loss
    else:
        depth_loss = zero_depth if zero_depth is not None else torch.zeros((), device=rgb_pred.device)
    return {'loss': loss, 'loss_rgb': rgb_full_loss, 'loss_dssim': dssim_loss, 'loss_depth': depth_loss}


def _fused_depth_route(self, rgb_pred, depth_pred, depth_gt) -> bool:
    """The fused depth term serves the trainer's own call: depth_loss_type 'l1' or 'invariant', depth_pred the [1,H,W] float32 device
    plane of the render and a depth_gt of the same size.  GSR_AUTOPATCH_DEPTH_LOSS=0 keeps the reference's torch statements."""
    if os.environ.get("GSR_AUTOPATCH_DEPTH_LOSS", "1") == "0" or os.environ.get("GSR_AUTOPATCH_LOSS_REPORT", "1") == "0" or not _ext_binding():
        return False
    if getattr(self, "depth_loss_type", None) not in ("l1", "invariant"):
        return False
    if not (torch.is_tensor(depth_pred) and torch.is_tensor(depth_gt)):
        return False
    return (depth_pred.is_cuda and depth_pred.device == rgb_pred.device and depth_pred.dtype == torch.float32 and depth_pred.dim() == 3
            and depth_pred.shape[0] == 1 and tuple(depth_pred.shape[1:]) == tuple(rgb_pred.shape[1:]) and depth_pred.is_contiguous()
            and depth_gt.numel() == depth_pred.numel() and tuple(depth_gt.shape[-2:]) == tuple(depth_pred.shape[1:])
            and depth_gt.dim() in (2, 3) and depth_gt.dtype.is_floating_point)


def _ext_binding() -> bool:
    E = importlib.import_module("3dgs_hierarchical_training_amd._ext")
    return not E.use_ctypes()


# ---- the visibility mask of the patched render: boolean-mask statements without their host synchronisations ------------------------
# The trainer's per-iteration statistics statement (/root/reference/trainer/ht3dgs_trainer.py:143-144),
#     gaussians.max_radii2D[visibility_filter] = torch.max(gaussians.max_radii2D[visibility_filter], radii[visibility_filter])
# is three boolean-mask index operations, each a `nonzero` with a host synchronisation that drains the launch queue -- +0.4 ms per
# iteration at every model size, in stage A as well (the statistics run on every iteration below `densify_until_iter`).  The mask
# this module's render returns is a bool tensor SUBCLASS that recognises exactly that pattern through `__torch_function__`:
# `dense[mask]` becomes a lazy selection (nothing gathered), `torch.max(selection, selection)` the element-wise maximum of the dense
# tensors, `dense[mask] = selection` one `torch.where` written in place -- the same values, no `nonzero`.  Anything else done with the
# mask or a selection (arithmetic, .sum(), printing, indexing other shapes ...) falls back to the plain tensors, gathered for real.
# GSR_AUTOPATCH_LAZY_MASK=0: the render returns a plain bool tensor.
class _LazySelection:
    """`dense[mask]` that has not been gathered.  Tensor-like only as far as the statement above needs; everything else
    materialises."""

    def __init__(self, dense, mask, max_of=None):
        self._dense, self.mask, self.max_of = dense, mask, max_of      # max_of = (a, b): the element-wise maximum, not yet evaluated
        # eager `dense[mask]` would have copied the values NOW: remember the version counters of what stands for them and refuse to
        # be evaluated after an in-place write to any of it -- the trainer's one statement never does that
        self._versions = [(t, t._version) for t in ((dense,) if dense is not None else tuple(max_of)) + (mask,)]

    def _check(self):
        for t, v in self._versions:
            if t._version != v:
                raise RuntimeError("gsr_autopatch: a tensor indexed by the render's visibility_filter was modified in place before the "
                                   "selection was used -- the lazy selection no longer stands for what `dense[mask]` would have copied; "
                                   "set GSR_AUTOPATCH_LAZY_MASK=0 (plain bool mask, eager gathers) for code that keeps such selections")

    @property
    def dense(self):
        self._check()
        if self._dense is None:
            self._dense = torch.maximum(*self.max_of)
            self._versions = [(self.mask, self._versions[-1][1])]
        return self._dense

    @property
    def dense_shape(self):
        return self.max_of[0].shape if self._dense is None else self._dense.shape

    def materialise(self):
        return self.dense[self.mask.as_subclass(torch.Tensor)]

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func is torch.max and len(args) == 2 and not kwargs and isinstance(args[0], _LazySelection) and isinstance(args[1], _LazySelection) \
                and args[0].mask is args[1].mask and args[0].dense_shape == args[1].dense_shape:
            return _LazySelection(None, args[0].mask, max_of=(args[0].dense, args[1].dense))      # (.dense checks the versions)
        unwrap = lambda a: a.materialise() if isinstance(a, _LazySelection) else a
        return func(*[unwrap(a) for a in args], **{k: unwrap(v) for k, v in kwargs.items()})

    def __getattr__(self, name):          # methods / properties of the gathered tensor (.shape, .sum(), .float(), ...)
        return getattr(self.materialise(), name)

    def __repr__(self):
        return repr(self.materialise())


def _lazy_dunder(name):
    def f(self, *a, **k):
        return getattr(self.materialise(), name)(*a, **k)
    return f


for _n in ("add", "radd", "sub", "rsub", "mul", "rmul", "truediv", "rtruediv", "neg", "abs", "lt", "le", "gt", "ge", "eq", "ne", "len",
           "getitem", "iter", "float", "int", "bool", "and", "or", "invert", "pow", "matmul"):
    setattr(_LazySelection, f"__{_n}__", _lazy_dunder(f"__{_n}__"))


class LazyMask(torch.Tensor):
    """The `visibility_filter` of the patched render: a bool tensor that turns `dense[mask]` / `dense[mask] = selection` on a
    1-D tensor of its own length into their synchronisation-free forms (see above) and is an ordinary bool tensor otherwise."""

    @staticmethod
    def __new__(cls, mask):
        return torch.Tensor._make_subclass(cls, mask, False)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func is torch.Tensor.__getitem__ and len(args) == 2 and isinstance(args[1], LazyMask) and type(args[0]) is torch.Tensor \
                and args[0].dim() == 1 and args[0].shape == args[1].shape and not kwargs:
            return _LazySelection(args[0], args[1])
        if func is torch.Tensor.__setitem__ and len(args) == 3 and isinstance(args[1], LazyMask) and isinstance(args[2], _LazySelection) \
                and args[2].mask is args[1] and type(args[0]) is torch.Tensor and args[0].shape == args[1].shape \
                and args[2].dense_shape == args[0].shape and not kwargs:
            dst, m, sel = args[0], args[1].as_subclass(torch.Tensor), args[2]
            sel._check()
            with torch._C.DisableTorchFunctionSubclass():
                pair = getattr(sel, "max_of", None)         # torch.max(dst[mask], radii[mask]): one launch (gsr_masked_max)
                if pair is not None and pair[0] is dst and dst.is_cuda and dst.dtype == torch.float32 and dst.is_contiguous() \
                        and pair[1].dtype == torch.int32 and pair[1].is_contiguous() and m.is_contiguous() and not dst.requires_grad:
                    _ops().masked_max_(dst, pair[1], m)
                else:
                    dst.copy_(torch.where(m, sel.dense.to(dst.dtype), dst))
            return None
        unwrap = lambda a: a.materialise() if isinstance(a, _LazySelection) else a
        with torch._C.DisableTorchFunctionSubclass():
            return func(*[unwrap(a) for a in args], **{k: unwrap(v) for k, v in kwargs.items()})


# ---- CF3DGS_Render.render on the raw-parameter path ------------------------------------------------------------------------------
def _pose_matrix(g):
    """The transform `get_xyz` applies to the means (/root/reference/scene/gaussian_model_ht.py:135-148) as a matrix that keeps its
    autograd link to the pose parameter, or None.  A lietorch SE3 `LieGroupParameter` on the GPU (what `init_RT` / `init_RT_seq` /
    `update_RT_seq` build, :346-386) goes through ONE autograd node over its six tangent numbers (`pose_opt.pose_matrix`: a [3,4]
    tensor, one kernel forward, one backward that leaves `.grad` on the parameter): no `retr()` chain, no matrix exponential in
    torch, nothing N-sized.  Any other pose object -- or `rotate_xyz_inverse`, or GSR_AUTOPATCH_POSE_FUSED=0 -- keeps the original
    statement: lietorch's `matrix()` of `retr()` ([4,4]; `matrix()` is `act` on the basis vectors)."""
    inverse = False
    if getattr(g, "rotate_xyz", False):
        p = g.P[0]
    elif getattr(g, "rotate_xyz_inverse", False):
        p, inverse = g.P[0], True
    elif getattr(g, "rotate_seq", False):
        p = g.P[g.seq_idx]
    else:
        return None
    if not inverse and os.environ.get("GSR_AUTOPATCH_POSE_FUSED", "1") != "0":
        P = importlib.import_module("3dgs_hierarchical_training_amd.pose_opt")
        if P.is_lie_pose(p) and (p.is_cuda or not _REQUIRE_CUDA):
            return P.pose_matrix(p, _ops())
    T = p.retr().inv() if inverse else p.retr()
    return T.matrix().reshape(4, 4)


_ZERO_POINTS = {}


def _view_id(cam, g) -> int:
    """A non-zero number that is the same whenever the same FRAME is rendered: the camera's `uid` (the frame index, or index + 0.5
    for an interpolated frame: /root/reference/trainer/trainer.py:556, :573) together with the pose slot `get_xyz` applies under
    `rotate_seq` (gaussian_model_ht.py:145-146).  The reference trains with an identity camera and moves the points, and steps the
    pose after every render, so neither the camera's matrices nor the pose's bits identify the frame; the id does.  Speed only
    (the forward blend's balanced placement, include/gsr.h GsrForwardArgs::view_id).  0 = unknown (GSR_AUTOPATCH_VIEW_ID=0: off)."""
    if os.environ.get("GSR_AUTOPATCH_VIEW_ID", "1") == "0":
        return 0
    try:
        vid = 1 + int(round(2.0 * float(getattr(cam, "uid"))))
        if getattr(g, "rotate_seq", False):
            vid += 1000003 * (1 + int(g.seq_idx))
        return vid if vid != 0 else 1
    except Exception:
        return 0


def _sh_origin(g, cam, dev):
    """The origin of the SH view direction of the reference's `convert_SHs_python` render (gaussian_model_ht.py:845-865):
    `get_RT(uid).inverse()[:3, 3].detach()` -- the camera centre in the model's own frame -- without a host synchronisation.  `get_RT`
    (:150-165) takes the identity when `P` is None, `P[0]` under `rotate_xyz` and `P[uid]` otherwise (the camera's uid, not seq_idx).
    A lietorch-shaped pose: -R^T t of the detached `pose_opt.pose_matrix` (one kernel, three numbers); any other pose object -- or
    GSR_AUTOPATCH_POSE_FUSED=0 -- the reference's own statement."""
    P = getattr(g, "P", None)
    if P is None:
        return torch.zeros(3, dtype=torch.float32, device=dev)
    uid = getattr(cam, "uid", None)
    p = P[0] if getattr(g, "rotate_xyz", False) else (P[uid] if isinstance(uid, int) else None)
    if p is not None and os.environ.get("GSR_AUTOPATCH_POSE_FUSED", "1") != "0":
        PO = importlib.import_module("3dgs_hierarchical_training_amd.pose_opt")
        if PO.is_lie_pose(p) and (p.is_cuda or not _REQUIRE_CUDA):
            with torch.no_grad():
                M = PO.pose_matrix(p, _ops())
                return -(M[:, :3].t() @ M[:, 3])
    return g.get_RT(uid).inverse()[:3, 3].detach()


def _raw_tensors(g):
    """The six raw parameter tensors when they have the layout the fused path takes, else None."""
    ts = [getattr(g, k, None) for k in RAW_NAMES]
    if any(not torch.is_tensor(t) for t in ts):
        return None
    x = ts[0]
    if (_REQUIRE_CUDA and not x.is_cuda) or x.dim() != 2 or x.shape[0] == 0:
        return None
    N = x.shape[0]
    if any(t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous() or t.shape[0] != N for t in ts):
        return None
    dc, rest, op, sc, rot = ts[1:]
    if tuple(x.shape) != (N, 3) or tuple(dc.shape) != (N, 1, 3) or rest.dim() != 3 or rest.shape[1] < 1 or rest.shape[2] != 3 or \
            tuple(op.shape) != (N, 1) or tuple(sc.shape) != (N, 3) or tuple(rot.shape) != (N, 4):
        return None
    return ts


def render_fused(self, viewpoint_camera, scaling_modifier=1.0, invert_bg_color=False, override_color=None,
                 compute_cov3D_python=False, convert_SHs_python=False):
    """Drop-in body of `CF3DGS_Render.render` (/root/reference/scene/gaussian_model_ht.py:775-908): same arguments, same returned
    dict.  The model's raw tensors go to the kernels as they are (activations of :128-133,176-188 and the SH concat in-kernel,
    `get_xyz`'s pose action as `points_transform`); every configuration the fused path does not cover runs the original method."""
    orig = next((f for c, a, f in _patched_render_classes if a == "render" and isinstance(self, c)), None)
    g = getattr(self, "gaussians", None)
    ts = None
    # convert_SHs_python: served when the colour is the view-dependent SH evaluation (`view_dependent`, arguments/__init__.py:83);
    # the raw-DC colour of view_dependent=False stays on the original method
    # (the origin travels through the PyTorch extension binding only: GSR_BINDING=ctypes keeps these renders on the original method)
    python_sh = bool(convert_SHs_python) and getattr(self, "view_dependent", False) is True and \
        os.environ.get("GSR_AUTOPATCH_PYTHON_SH", "1") != "0" and _ext_binding()
    if override_color is None and not compute_cov3D_python and (python_sh or not convert_SHs_python) and g is not None:
        ts = _raw_tensors(g)
    posed = ts is not None and (getattr(g, "rotate_xyz", False) or getattr(g, "rotate_xyz_inverse", False) or getattr(g, "rotate_seq", False))
    if posed and os.environ.get("GSR_AUTOPATCH_POSE", "1") == "0":
        ts = None
    if ts is None:
        if orig is None:
            raise RuntimeError("gsr_autopatch.render_fused: this configuration needs the original CF3DGS_Render.render")
        return orig(self, viewpoint_camera, scaling_modifier, invert_bg_color, override_color, compute_cov3D_python, convert_SHs_python)
    R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    xyz, f_dc, f_rest, opacity, scaling, rotation = ts
    dev = xyz.device
    # the tensor whose .grad receives the 2D positional gradient (:800-808: `zeros_like(get_xyz, requires_grad=True) + 0` with
    # retain_grad); its values are never read by the rasterizer
    # (one zero buffer per (N, device), a fresh LEAF over it per render -- detach() makes a new tensor object on the same storage, no
    #  fill launch and no allocation; every render's leaf has its own .grad, and a leaf that requires grad cannot be written in place)
    # every render's leaf aliases this storage, so an in-place write under no_grad would reach all later renders -- the
    # buffer's version counter (shared by every detach() of it) must still be the one it was created with, else a fresh one is made
    # (a write through `.data` carries a counter of its own and is NOT seen: the values of `viewspace_points` are never read by the
    # rasterizer, only its .grad is written); and only the two most recent sizes are kept (a model and its frozen teacher), not one N x 12 B buffer per densification size
    zkey = (int(xyz.shape[0]), dev)
    zbuf = _ZERO_POINTS.get(zkey)
    if zbuf is None or zbuf._version != 0:
        while len(_ZERO_POINTS) >= 2:
            _ZERO_POINTS.pop(next(iter(_ZERO_POINTS)))
        _ZERO_POINTS.pop(zkey, None)
        zbuf = _ZERO_POINTS[zkey] = torch.zeros((xyz.shape[0], 3), dtype=torch.float32, device=dev)
    screenspace_points = zbuf.detach().requires_grad_(True)
    bg = self.bg_color if not invert_bg_color else 1 - self.bg_color
    settings = R.GaussianRasterizationSettings(
        image_height=int(viewpoint_camera.image_height), image_width=int(viewpoint_camera.image_width),
        tanfovx=math.tan(viewpoint_camera.FoVx * 0.5), tanfovy=math.tan(viewpoint_camera.FoVy * 0.5), bg=bg,
        scale_modifier=scaling_modifier, viewmatrix=viewpoint_camera.world_view_transform,
        projmatrix=viewpoint_camera.full_proj_transform, sh_degree=g.active_sh_degree, campos=viewpoint_camera.camera_center,
        prefiltered=False, debug=False)
    M = _pose_matrix(g) if posed else None
    sh_origin = _sh_origin(g, viewpoint_camera, dev) if python_sh else None
    # DEFERRED optimizer step: when the model's optimizer is the FusedAdam this module handed out, the backward kernel also computes
    # the Adam update -- into shadow buffers, the model untouched -- and the trainer's `optimizer.step()` adopts it by swapping
    # storages.  Everything the trainer may do in between keeps its meaning (surgery sees the un-updated state and drops the
    # update; a skipped step leaves the model alone; stale .grad = torch's accumulation on the plain route).  GSR_AUTOPATCH_DEFERRED=0: off.
    opt, deferred = getattr(g, "optimizer", None), False
    if opt is not None and hasattr(opt, "deferred_ready") and torch.is_grad_enabled() and os.environ.get("GSR_AUTOPATCH_DEFERRED", "1") != "0":
        opt.flush_pending_as_grads()
        # (GSR_AUTOPATCH_DEFERRED_MIN_N: models below that many Gaussians keep the separate step; default 0 -- measured with the
        #  route's own order bias removed, the deferred step is the faster one at stage A's 130 k Gaussians too: 0.375 against
        #  0.40-0.42 ms per step; 0.90 against 0.98 ms at 1 M)
        if xyz.shape[0] >= int(os.environ.get("GSR_AUTOPATCH_DEFERRED_MIN_N", "0")):
            deferred = opt.deferred_ready({"xyz": xyz, "f_dc": f_dc, "f_rest": f_rest, "opacity": opacity, "scaling": scaling, "rotation": rotation})
    if _ext_binding() and os.environ.get("GSR_AUTOPATCH_EXTRAS", "1") != "0":
        # the clamped image and the visibility bytes come out of the kernels that hold the values (the blend's epilogue, the preprocess):
        # no torch launch for `clamp(0, 1)` / `radii > 0`
        if not torch.is_grad_enabled():
            # a render no backward can follow -- the frozen teacher (trainer/ht3dgs_trainer.py:877-883), eval_nvs (:1050-1061),
            # evaluate_on_training_images, render_nvs, all under torch.no_grad(): the render-only forward, the same six tensors bit for
            # bit and no state, checkpoint or binning buffer behind them
            image_raw, radii, depth, alpha, image, vis8 = R.render_gaussians_raw(
                xyz, f_dc, f_rest, opacity, scaling, rotation, settings, depth_alpha=True, clamped=True, visible=True, points_transform=M,
                view_id=_view_id(viewpoint_camera, g), sh_origin=sh_origin)
        else:
            image_raw, radii, depth, alpha, image, vis8 = R.rasterize_gaussians_raw(
                xyz, screenspace_points, f_dc, f_rest, opacity, scaling, rotation, settings, points_transform=M, fused_adam=opt if deferred else None,
                fused_adam_deferred=deferred, view_id=_view_id(viewpoint_camera, g), extras=3, sh_origin=sh_origin)
        visible = vis8.view(torch.bool) if vis8.numel() == radii.numel() else radii > 0
    else:
        image_raw, radii, depth, alpha = R.rasterize_gaussians_raw(xyz, screenspace_points, f_dc, f_rest, opacity, scaling, rotation,
                                                                   settings, points_transform=M, fused_adam=opt if deferred else None,
                                                                   fused_adam_deferred=deferred, view_id=_view_id(viewpoint_camera, g),
                                                                   sh_origin=sh_origin)
        image = image_raw.clamp(0, 1)
        visible = radii > 0
    image._gsr_raw = (image_raw, image._version)       # lets the patched Loss.forward fuse this clamp into the loss kernels
    if os.environ.get("GSR_AUTOPATCH_LAZY_MASK", "1") != "0":
        visible = LazyMask(visible)            # (the trainer's boolean-mask statistics statement without its host synchronisations)
    return {"image": image, "depth": depth, "alpha": alpha, "viewspace_points": screenspace_points,
            "visibility_filter": visible, "radii": radii}


def calc_importance_fused(gs_render, cameras, pipe, override_color=None):
    """Drop-in body of `HTGaussianTrainer.calc_importance` (/root/reference/trainer/ht3dgs_trainer.py:1427-1462; a staticmethod):
    the same [N, 48] tensor -- sum over the cameras of |d sum(clamped render) / d SH|, over the pixel count -- from one forward and
    the importance pass per camera (hierarchy.py calc_importance's kernel route) instead of a render and a full backward.  Raw
    tensors, pose, SH origin and frame id are taken exactly as render_fused takes them; whatever render_fused would hand to the
    original render hands this call to the original method.  `_features_dc.grad` / `_features_rest.grad` are left None (the
    reference leaves the summed |grad| there; nobody reads it)."""
    orig = next((f for c, a, f in _patched_trainer_classes if a == "calc_importance"), None)
    orig = orig.__func__ if isinstance(orig, staticmethod) else orig
    g = getattr(gs_render, "gaussians", None)
    cov_py, sh_py = bool(getattr(pipe, "compute_cov3D_python", False)), bool(getattr(pipe, "convert_SHs_python", False))
    python_sh = sh_py and getattr(gs_render, "view_dependent", False) is True and \
        os.environ.get("GSR_AUTOPATCH_PYTHON_SH", "1") != "0" and _ext_binding()
    ts = None
    if override_color is None and not cov_py and (python_sh or not sh_py) and g is not None:
        ts = _raw_tensors(g)
    posed = ts is not None and (getattr(g, "rotate_xyz", False) or getattr(g, "rotate_xyz_inverse", False) or getattr(g, "rotate_seq", False))
    if posed and os.environ.get("GSR_AUTOPATCH_POSE", "1") == "0":
        ts = None
    M = None
    if ts is not None and posed:
        try:
            with torch.no_grad():
                M = _pose_matrix(g)
        except Exception:        # a pose object neither pose_opt nor lietorch's retr().matrix() reads: the original's own statement
            ts = None
    if ts is None:
        if orig is None:
            raise RuntimeError("gsr_autopatch.calc_importance_fused: this configuration needs the original HTGaussianTrainer.calc_importance")
        return orig(gs_render, cameras, pipe) if override_color is None else orig(gs_render, cameras, pipe, override_color)
    R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
    xyz, f_dc, f_rest, opacity, scaling, rotation = ts
    dev = xyz.device
    f_dc.grad = None
    f_rest.grad = None
    acc = torch.zeros((xyz.shape[0], f_dc.shape[1] + f_rest.shape[1], 3), dtype=torch.float32, device=dev)
    num_pixels = 0
    make = lambda cam: R.GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5),
        tanfovy=math.tan(cam.FoVy * 0.5), bg=gs_render.bg_color, scale_modifier=1.0, viewmatrix=cam.world_view_transform,
        projmatrix=cam.full_proj_transform, sh_degree=g.active_sh_degree, campos=cam.camera_center, prefiltered=False, debug=False)
    per_call = _importance_views()
    if per_call > 1:
        # runs of cameras that share their frame go through ONE launch chain (hierarchy.group_views; include/gsr.h
        # gsr_importance_accumulate_views): the model's pose and every camera's SH origin stacked per view
        H = importlib.import_module("3dgs_hierarchical_training_amd.hierarchy")
        cameras = list(cameras)
        settings = [make(cam) for cam in cameras]
        for group in H.group_views(settings, per_call, xyz.shape[0]):
            cams = [cameras[i] for i in group]
            if len(group) == 1:
                R.importance_accumulate(acc, xyz, f_dc, opacity, scaling, rotation, settings[group[0]], sh_rest=f_rest, raw_params=True,
                                        points_transform=M, view_id=_view_id(cams[0], g),
                                        sh_origin=_sh_origin(g, cams[0], dev) if python_sh else None)
            else:
                V = len(group)
                R.importance_accumulate_views(
                    acc, xyz, f_dc, opacity, scaling, rotation, H.stack_views([settings[i] for i in group], dev), sh_rest=f_rest,
                    raw_params=True, points_transform=None if M is None else torch.stack([M[:3].to(dev)] * V),
                    sh_origin=torch.stack([_sh_origin(g, c, dev).reshape(3) for c in cams]) if python_sh else None)
            num_pixels += sum(int(c.image_height) * int(c.image_width) for c in cams)
        return (acc.flatten(-2) / num_pixels).detach()
    for cam in cameras:
        settings = make(cam)
        R.importance_accumulate(acc, xyz, f_dc, opacity, scaling, rotation, settings, sh_rest=f_rest, raw_params=True, points_transform=M,
                                view_id=_view_id(cam, g), sh_origin=_sh_origin(g, cam, dev) if python_sh else None)
        num_pixels += int(cam.image_height) * int(cam.image_width)
    return (acc.flatten(-2) / num_pixels).detach()


def _importance_views() -> int:
    """GSR_AUTOPATCH_IMPORTANCE_VIEWS: how many cameras one launch chain of the patched calc_importance takes (1..16; default 1 = a
    forward and a pass per camera, the route as it was -- profiles/importance_views.txt)."""
    v = int(os.environ.get("GSR_AUTOPATCH_IMPORTANCE_VIEWS", "1"))
    if not 1 <= v <= 16:
        raise ValueError(f"GSR_AUTOPATCH_IMPORTANCE_VIEWS={v}: 1..16")
    return v


def _patch_trainer_module(mod):
    """`trainer.ht3dgs_trainer` holds `HTGaussianTrainer`: its `calc_importance` and its `merge_two_3DGS`, each behind its own switch."""
    _patch_importance_module(mod)
    _patch_merge_module(mod)


def _patch_importance_module(mod):
    # (on since the kernel route was measured faster than a render and a full backward per view at both sizes:
    #  profiles/importance_probe.txt)
    if os.environ.get("GSR_AUTOPATCH_IMPORTANCE", "1") == "0":
        return
    cls = getattr(mod, "HTGaussianTrainer", None)
    if cls is None or "calc_importance" not in vars(cls) or any(c is cls for c, _, _ in _patched_trainer_classes):
        return
    _patched_trainer_classes.append((cls, "calc_importance", vars(cls)["calc_importance"]))
    cls.calc_importance = staticmethod(calc_importance_fused)


def add_densification_stats_fused(self, viewspace_point_tensor, update_filter):
    """Drop-in body of `HTGaussianModel.add_densification_stats` (/root/reference/scene/gaussian_model_ht.py:718-721): the same
    sums as masked adds over N instead of three boolean-mask gathers / scatters (each a `nonzero` and a host synchronisation)."""
    if isinstance(update_filter, LazyMask):
        update_filter = update_filter.as_subclass(torch.Tensor)
    g = viewspace_point_tensor.grad
    if g is None or update_filter.dtype != torch.bool or update_filter.dim() != 1 or update_filter.shape[0] != self.denom.shape[0]:
        orig = next((f for c, a, f in _patched_render_classes if a == "add_densification_stats" and isinstance(self, c)), None)
        if orig is None:
            raise RuntimeError("gsr_autopatch.add_densification_stats_fused: needs a [N] boolean filter and a populated .grad")
        return orig(self, viewspace_point_tensor, update_filter)
    acc, den = self.xyz_gradient_accum, self.denom
    if g.is_cuda and all(t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad for t in (acc, den, g)) and \
            update_filter.is_contiguous() and acc.numel() == den.numel() == update_filter.shape[0] and tuple(g.shape) == (den.shape[0], 3):
        _ops().densify_stats_add_(acc, den, g, update_filter)       # one launch (gsr_densify_stats_add)
        return
    f = update_filter.unsqueeze(1)
    self.xyz_gradient_accum += torch.where(f, torch.norm(g[:, :2], dim=-1, keepdim=True), torch.zeros((), device=g.device, dtype=g.dtype))
    self.denom += f.to(self.denom.dtype)


def _patch_render_module(mod):
    if os.environ.get("GSR_AUTOPATCH_RENDER", "1") == "0":
        return
    for cname, attr, fn in (("CF3DGS_Render", "render", render_fused),
                            ("HTGaussianModel", "add_densification_stats", add_densification_stats_fused)):
        cls = getattr(mod, cname, None)
        if cls is None or not hasattr(cls, attr) or any(c is cls and a == attr for c, a, _ in _patched_render_classes):
            continue
        _patched_render_classes.append((cls, attr, getattr(cls, attr)))
        setattr(cls, attr, fn)


# ---- GaussianTrainer.load_viewpoint_cam: the frame cache; HTGaussianModel.get_RT: poses that stay on the device ---------------------------
class DevicePose(torch.Tensor):
    """What the patched `HTGaussianModel.get_RT` returns: the pose tensor itself (same storage, same autograd history) under a type whose
    `.cpu()` returns the object unchanged -- the trainer's `get_RT(fidx).detach().cpu()` (ht3dgs_trainer.py:539, :559, :615, :897 ...) then
    waits for nothing, and the patched `load_viewpoint_cam` takes the pose where it is.  `.detach()` and indexing keep the type; `.numpy()` /
    `np.asarray` deliver the host values (one copy, the wait the reference had); any torch function that also takes a genuine CPU tensor
    (`pose_dict[...].cpu() @ pose` with a `pose_dict` loaded from a file, ht3dgs_trainer.py:561) sees the pose as the CPU tensor the
    reference would have had; a function of DevicePoses alone (the same statement with the `pose_dict` stage A filled from `get_RT()`)
    returns a DevicePose; everything else -- a pose combined with a plain device tensor -- sees the plain tensor."""

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        me = args[0] if args else None
        if isinstance(me, DevicePose):
            if func is torch.Tensor.cpu:
                return me
            if func in (torch.Tensor.detach, torch.Tensor.__getitem__):
                with torch._C.DisableTorchFunctionSubclass():
                    out = func(*args, **kwargs)
                    return out.as_subclass(DevicePose) if isinstance(out, torch.Tensor) else out
            if func in (torch.Tensor.numpy, torch.Tensor.__array__):
                with torch._C.DisableTorchFunctionSubclass():
                    return func(me.as_subclass(torch.Tensor).detach().cpu(), *args[1:], **kwargs)
        from torch.utils._pytree import tree_map
        with torch._C.DisableTorchFunctionSubclass():
            flat = []
            tree_map(lambda a: flat.append(a) if isinstance(a, torch.Tensor) else None, (args, kwargs))
            to_host = any(not isinstance(a, DevicePose) and a.device.type == "cpu" for a in flat)

            def plain(a):
                if isinstance(a, DevicePose):
                    a = a.as_subclass(torch.Tensor)
                    return a.cpu() if to_host else a
                return a
            only_poses = bool(flat) and all(isinstance(a, DevicePose) for a in flat)
            args, kwargs = tree_map(plain, (args, kwargs))
            out = func(*args, **kwargs)
            # poses combined with poses alone stay poses: `pose_dict[...]` holds `get_RT().detach()` results (ht3dgs_trainer.py:379-380,
            # :424-428), so `pose_dict[...].detach().cpu() @ pose_train` (:561) is such a product -- a CPU tensor in the reference; here a
            # DevicePose, which `.numpy()`, the patched loader and the original loader's hand-over all take
            return out.as_subclass(DevicePose) if only_poses and type(out) is torch.Tensor else out


def get_RT_device(self, idx=None):
    """Drop-in body of `HTGaussianModel.get_RT` (/root/reference/scene/gaussian_model_ht.py:150-166): the original's tensor as a
    `DevicePose`."""
    orig = next((f for c, a, f in _patched_frame_classes if a == "get_RT" and isinstance(self, c)), None)
    if orig is None:
        raise RuntimeError("gsr_autopatch.get_RT_device: needs the original HTGaussianModel.get_RT")
    out = orig(self, idx)
    return out.as_subclass(DevicePose) if type(out) is torch.Tensor else out


def _plain_pose(pose):
    with torch._C.DisableTorchFunctionSubclass():
        return pose.as_subclass(torch.Tensor) if isinstance(pose, DevicePose) else pose


def _frame_budget_bytes() -> int:
    return int(float(os.environ.get("GSR_AUTOPATCH_FRAMES_MB", "16384")) * (1 << 20))


_FRAME_FIELDS = ("uid", "colmap_id", "FoVx", "FoVy", "image_name", "intrinsics", "depth", "optical_flow", "mask_for_relative_pose", "mask",
                 "data_device", "image_width", "image_height", "gt_alpha_mask", "zfar", "znear", "trans", "scale", "projection_matrix", "focal_x",
                 "focal_y")


def _frame_entry(cam):
    """What is kept of a camera the original loader built, or None when it is not the camera the cache can hand out again (no device
    image, fields missing, a projection the kernel does not restate)."""
    image = getattr(cam, "original_image", None)
    if not isinstance(cam, torch.nn.Module) or type(image) is not torch.Tensor or image.dim() != 3 or (_REQUIRE_CUDA and not image.is_cuda):
        return None
    if any(not hasattr(cam, k) for k in _FRAME_FIELDS) or getattr(cam, "gt_alpha_mask", None) is not None:
        return None
    K = cam.intrinsics
    try:
        fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    except Exception:
        return None
    if not (fx > 0 and fy > 0) or tuple(cam.projection_matrix.shape) != (4, 4) or cam.projection_matrix.device != image.device:
        return None
    return {"cls": type(cam), "image": image, "version": image._version, "bytes": image.numel() * image.element_size(),
            "fields": {k: getattr(cam, k) for k in _FRAME_FIELDS}, "K": (fx, fy, cx, cy), "identity": None}


def _camera_from_entry(e, R, T, view, full, center, vfi):
    """A `Camera` with the attributes `Camera.__init__` sets (cameras.py:35-103), without running it."""
    cam = object.__new__(e["cls"])
    torch.nn.Module.__init__(cam)
    for k, v in e["fields"].items():
        setattr(cam, k, v)
    cam.R, cam.T, cam.vfi = R, T, vfi
    cam.original_image = e["image"]
    cam.world_view_transform, cam.full_proj_transform, cam.camera_center = view, full, center
    return cam


def load_viewpoint_cam_cached(self, idx, pose=None, load_depth=False, pose_to_train=False, load_vfi=False):
    """Drop-in body of `GaussianTrainer.load_viewpoint_cam` (/root/reference/trainer/trainer.py:989-1142): same arguments, a camera with the
    same attributes.  See the module docstring for what is cached and what runs the original."""
    orig = next((f for c, a, f in _patched_frame_classes if a == "load_viewpoint_cam" and isinstance(self, c)), None)
    if orig is None:
        raise RuntimeError("gsr_autopatch.load_viewpoint_cam_cached: needs the original GaussianTrainer.load_viewpoint_cam")

    def original():
        # the reference's own statements, on the host pose they were written for (a DevicePose is copied down here: the old cost)
        # and so is any other device tensor, unless the call asks for a camera that stays differentiable in the pose it was given
        host = pose
        if isinstance(pose, DevicePose):
            host = _plain_pose(pose).cpu()
        elif isinstance(pose, torch.Tensor) and pose.device.type != "cpu" and not pose_to_train:
            host = pose.detach().cpu()
        return orig(self, idx, pose=host, load_depth=load_depth, pose_to_train=pose_to_train, load_vfi=load_vfi)

    # the trainable-pose camera, a pose or an index this loader does not recognise: the original, nothing kept
    if pose_to_train or not isinstance(idx, numbers.Integral) or \
            (pose is not None and not (isinstance(pose, torch.Tensor) and tuple(pose.shape) == (4, 4))):
        return original()
    # work the cache cannot know -- the original's side effects, `mono_depth[idx]` and `vfi[...]` not there yet: the original runs (and its
    # frame is kept like any first call's)
    side_effects = bool(load_depth) and idx not in getattr(self, "mono_depth", {})
    vfi_key = f"{idx}_to_{idx + 1}"
    if load_vfi and not (idx + 1 < len(self.data) and vfi_key in getattr(self, "vfi", {})):
        side_effects = True
    frames = self.__dict__.setdefault("_gsr_frames", {"entries": {}, "bytes": 0})
    e = frames["entries"].get(idx)
    if e is not None and e["image"]._version != e["version"]:        # somebody wrote into the cached plane: rebuild it from the original
        frames["bytes"] -= e["bytes"]
        del frames["entries"][idx]
        e = None
    if e is None or side_effects or (pose is None and e["identity"] is None):
        cam = original()
        if e is None:
            e = _frame_entry(cam)
            if e is None or frames["bytes"] + e["bytes"] > _frame_budget_bytes():
                return cam                                           # not a frame the cache holds (or no room): the original path, every time
            frames["entries"][idx] = e
            frames["bytes"] += e["bytes"]
        if pose is None:                                             # (the identity camera's tensors do not depend on the frame's image)
            e["identity"] = (cam.R, cam.T, cam.world_view_transform, cam.full_proj_transform, cam.camera_center)
        if cam.original_image is not e["image"]:                     # (a second original call made a second plane: hand out the kept one)
            cam.original_image = e["image"]
        return cam
    vfi = self.vfi[vfi_key] if load_vfi else None                    # a vfi image that is there is attached as the original does
    if pose is None:
        R, T, view, full, center = e["identity"]
        return _camera_from_entry(e, R, T, view, full, center, vfi)
    p = _plain_pose(pose).detach()
    dev = e["image"].device
    if p.device != dev or p.dtype != torch.float32:                  # a host pose: one small upload, then the kernel as for a device pose
        p = p.to(device=dev, dtype=torch.float32)
    fx, fy, cx, cy = e["K"]
    f = e["fields"]
    view, full, center = _ops().camera_from_pose(p, fx, fy, cx, cy, int(f["image_width"]), int(f["image_height"]), float(f["znear"]), float(f["zfar"]))
    # R, T: numpy blocks of a host pose, as the original keeps them; views of a device pose (a DevicePose's deliver numpy on `.numpy()`)
    keep = pose.detach()
    R, T = (keep[:3, :3].numpy(), keep[:3, 3].numpy()) if type(pose) is torch.Tensor and pose.device.type == "cpu" else (keep[:3, :3], keep[:3, 3])
    return _camera_from_entry(e, R, T, view, full, center, vfi)


def _patch_frames_module(mod):
    if os.environ.get("GSR_AUTOPATCH_FRAMES", "1") == "0":
        return
    for cname, attr, fn in (("GaussianTrainer", "load_viewpoint_cam", load_viewpoint_cam_cached), ("HTGaussianModel", "get_RT", get_RT_device)):
        cls = getattr(mod, cname, None)
        if cls is None or not hasattr(cls, attr) or any(c is cls and a == attr for c, a, _ in _patched_frame_classes):
            continue
        _patched_frame_classes.append((cls, attr, getattr(cls, attr)))
        setattr(cls, attr, fn)


# ---- HTGaussianModel.densify_and_prune / prune_points: the model resized by the resize kernels ------------------------------------------
# The reference's surgery (/root/reference/scene/gaussian_model_ht.py:548-695) is boolean indexing and `torch.cat` tensor by tensor -- an
# append for the clones, an append for the split children, a prune of the split parents, a final prune -- every boolean index a `nonzero`
# with a host wait.  The two methods below make the SAME selections with the model's own torch statements, turn them into one flag byte
# per row and hand the rows to gsr_resize_plan / gsr_resize_apply (resize.py): one host wait, one launch per call that moves every
# parameter and moment.  The kernels order rows and copy bytes; every float is computed by torch, from the model's own activations.
_patched_resize_classes = []        # [(class, attribute, original function)]
_GROUP_ATTR = dict(zip(FUSED_NAMES, RAW_NAMES))
_STAT_NAMES = ("xyz_gradient_accum", "denom", "max_radii2D")
_RESIZE_DEFAULT = "1"


def _resize():
    return importlib.import_module("3dgs_hierarchical_training_amd.resize")


def _resize_original(self, attr):
    orig = next((f for c, a, f in _patched_resize_classes if a == attr and isinstance(self, c)), None)
    if orig is None:
        raise RuntimeError(f"gsr_autopatch: this call needs the original HTGaussianModel.{attr}")
    return orig


def _resize_entries(self):
    """`_resize_layout` behind the switch of the resize patch."""
    if os.environ.get("GSR_AUTOPATCH_RESIZE", _RESIZE_DEFAULT) == "0":
        return None
    return _resize_layout(self)


def _resize_layout(self):
    """[(group, attribute, parameter, state or None)] in the optimizer's group order when the model has the layout the resize kernels take,
    else None: exactly the six named groups of one parameter each, which are the model's six raw tensors; those, the moments that exist and
    the three statistics tensors float32, contiguous, N rows, on one device (the GPU); 0 < N < 2^31."""
    opt = getattr(self, "optimizer", None)
    groups = getattr(opt, "param_groups", None)
    if groups is None or not hasattr(opt, "state") or len(groups) != 6 or sorted(g.get("name", "") for g in groups) != sorted(FUSED_NAMES):
        return None
    x = getattr(self, "_xyz", None)
    if not torch.is_tensor(x) or x.dim() != 2 or (_REQUIRE_CUDA and not x.is_cuda):
        return None
    n = x.shape[0]
    if not 0 < n < 2 ** 31:
        return None
    ok = lambda t, shape=None: torch.is_tensor(t) and t.dtype == torch.float32 and t.device == x.device and t.is_contiguous() and \
        t.dim() >= 1 and t.shape[0] == n and (shape is None or t.shape == shape)
    entries = []
    for g in groups:
        ps = g["params"]
        if torch.is_tensor(ps) or len(ps) != 1 or ps[0] is not getattr(self, _GROUP_ATTR[g["name"]], None) or not ok(ps[0]):
            return None
        st = opt.state.get(ps[0], None)
        if st is not None and not (ok(st.get("exp_avg"), ps[0].shape) and ok(st.get("exp_avg_sq"), ps[0].shape)):
            return None
        entries.append((g, _GROUP_ATTR[g["name"]], ps[0], st))
    if not all(ok(getattr(self, k, None)) for k in _STAT_NAMES):
        return None
    return entries


def _install_resized(self, entries, out):
    """What the reference's `_prune_optimizer` / `cat_tensors_to_optimizer` leave behind, from the tensors of one gsr_resize_apply: every
    parameter a fresh `nn.Parameter` leaf (`.grad` None), the group's state dict re-keyed to it with `step` kept and the moments replaced."""
    opt, out = self.optimizer, iter(out)
    for g, attr, old, st in entries:
        new = torch.nn.Parameter(next(out).requires_grad_(True))
        if st is not None:
            st["exp_avg"], st["exp_avg_sq"] = next(out), next(out)
            del opt.state[old]
            opt.state[new] = st
        g["params"][0] = new
        setattr(self, attr, new)


def _resize_sources(entries, children=None):
    """The table of one gsr_resize_apply over the parameters and the moments that exist: (src, kinds, child); `children` maps a group's name
    to the [2 nSplit, ...] rows its surviving split children take."""
    R = _resize()
    src, kinds, child = [], [], []
    for g, attr, p, st in entries:
        rows = (children or {}).get(g["name"])
        src.append(p.detach()); kinds.append(R.PARAM if rows is None else R.CHILD_SOURCED); child.append(rows)
        if st is not None:
            src += [st["exp_avg"], st["exp_avg_sq"]]; kinds += [R.MOMENT, R.MOMENT]; child += [None, None]
    return src, kinds, child


def _normal_draw(mean, std):
    """The reference's draw `torch.normal(mean=mean, std=std)` on the default generator, taken apart: torch evaluates that call as a standard
    normal fill of the output, times `std`, plus `mean` -- after a validity check of `std` (all >= 0) that reads the device back, twice in
    this build, which would make three host waits of the call's one.  `std` here is the model's own scaling activation.  The same samples
    and the same generator state to the bit: the tests hold this against the arm that calls `torch.normal` itself."""
    return torch.empty_like(std).normal_(0.0, 1.0).mul_(std).add_(mean)


def prune_points_fused(self, mask):
    """Drop-in body of `HTGaussianModel.prune_points` (/root/reference/scene/gaussian_model_ht.py:548-582): the rows where `mask` is True
    leave the six parameters, the moments that exist and the three statistics tensors.  One host wait (the row count) and two launches of
    gsr_resize_apply -- the parameters with their moments, then the statistics -- instead of 21 boolean-index gathers."""
    entries = _resize_entries(self)
    if entries is None or not (isinstance(mask, torch.Tensor) and mask.dtype == torch.bool and mask.dim() == 1 and
                               mask.shape[0] == self._xyz.shape[0] and mask.device == self._xyz.device):
        return _resize_original(self, "prune_points")(self, mask)
    R = _resize()
    with torch.no_grad():
        n = self._xyz.shape[0]
        flags = ((~mask.as_subclass(torch.Tensor)).to(torch.uint8) * R.KEEP).contiguous()
        plan, meta = R.resize_plan(flags)
        counts = R.read_counts(meta)                                   # the call's one host wait
        src, kinds, child = _resize_sources(entries)
        _install_resized(self, entries, R.resize_apply(plan, meta, n, counts, src, kinds, child))
        stats = R.resize_apply(plan, meta, n, counts, [getattr(self, k) for k in _STAT_NAMES], [R.PARAM] * 3)      # (21 tensors exceed one table)
        for k, t in zip(_STAT_NAMES, stats):
            setattr(self, k, t)


def densify_and_prune_fused(self, max_grad, min_opacity, extent, max_screen_size):
    """Drop-in body of `HTGaussianModel.densify_and_prune` (/root/reference/scene/gaussian_model_ht.py:631-695).  Every selection is the
    reference's own statement evaluated on the N rows the call starts with; what the reference decides about a row it appended follows from
    the row it was copied from:
      * a clone carries its parent's parameters, so the final prune removes it iff it removes the parent;
      * a cloned row is never split: its padded gradient is 0 and max_grad > 0 (anything else runs the original);
      * a split parent is removed right after its children were appended, whatever the final prune thinks of it;
      * a child has its parent's opacity and the scale get_scaling / (0.8 * 2) taken through the model's inverse activation and its
        activation, and `max_radii2D` is all zeros at the final prune.
    The rows come out as the reference's append / append / prune / prune leaves them: kept rows, clones, children copy 0, children copy 1.
    The children's positions and scales are the reference's statements on index_select(split rows) -- the same shapes, also when nothing is
    split, and the same draw on the default generator as the reference's `torch.normal(mean=zeros, std=stds)` (`_normal_draw`)."""
    entries = _resize_entries(self)
    helpers = sys.modules.get(type(self).__module__)
    build_rotation = getattr(helpers, "build_rotation", None)
    if entries is None or not max_grad > 0 or build_rotation is None or \
            not all(hasattr(self, k) for k in ("get_scaling", "get_opacity", "scaling_activation", "scaling_inverse_activation", "percent_dense")):
        return _resize_original(self, "densify_and_prune")(self, max_grad, min_opacity, extent, max_screen_size)
    R = _resize()
    with torch.no_grad():
        n, dev = self._xyz.shape[0], self._xyz.device
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        scaling = self.get_scaling
        smax = torch.max(scaling, dim=1).values
        clone = torch.logical_and(torch.norm(grads, dim=-1) >= max_grad, smax <= self.percent_dense * extent)
        split = torch.logical_and(grads.squeeze(-1) >= max_grad, smax > self.percent_dense * extent)
        gone = (self.get_opacity < min_opacity).squeeze(-1)              # the final prune's predicate on a row as it stands
        child_gone = gone
        if max_screen_size:
            on_screen = bool(0.0 > max_screen_size)                      # (max_radii2D is all zeros at the final prune)
            gone = gone | on_screen | (smax > 0.1 * extent)
            child_scaling = self.scaling_activation(self.scaling_inverse_activation(scaling / (0.8 * 2)))
            child_gone = child_gone | on_screen | (child_scaling.max(dim=1).values > 0.1 * extent)
        flags = ((~split & ~gone).to(torch.uint8) * R.KEEP + (clone & ~gone).to(torch.uint8) * R.CLONE
                 + split.to(torch.uint8) * R.SPLIT + (split & ~child_gone).to(torch.uint8) * R.CHILD)
        plan, meta = R.resize_plan(flags)
        counts = R.read_counts(meta)                                     # the call's one host wait
        nA, nB, nC, nS = counts[:4]
        rows = R.plan_segment(plan, n, R.L.GSR_RESIZE_PLAN_SPLIT_ROWS, nS)
        parent_scaling = scaling.index_select(0, rows)
        stds = parent_scaling.repeat(2, 1)
        means = torch.zeros((stds.size(0), 3), device=dev)
        samples = _normal_draw(means, stds)
        rots = build_rotation(self._rotation.index_select(0, rows)).repeat(2, 1, 1)
        positions = getattr(self, "get_xyz", self._xyz)                  # (the posed means where the model poses them, as the reference reads them)
        children = {"xyz": torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + positions.index_select(0, rows).repeat(2, 1),
                    "scaling": self.scaling_inverse_activation(parent_scaling.repeat(2, 1) / (0.8 * 2))}
        src, kinds, child = _resize_sources(entries, children if nS else None)
        _install_resized(self, entries, R.resize_apply(plan, meta, n, counts, src, kinds, child))
        nout = nA + nB + 2 * nC
        self.xyz_gradient_accum = torch.zeros((nout, 1), device=dev)
        self.denom = torch.zeros((nout, 1), device=dev)
        self.max_radii2D = torch.zeros((nout,), device=dev)
        if dev.type == "cuda" and os.environ.get("GSR_AUTOPATCH_EMPTY_CACHE", "1") != "0":
            torch.cuda.empty_cache()


def _patch_resize_module(mod):
    if os.environ.get("GSR_AUTOPATCH_RESIZE", _RESIZE_DEFAULT) == "0":
        return
    cls = getattr(mod, "HTGaussianModel", None)
    for attr, fn in (("densify_and_prune", densify_and_prune_fused), ("prune_points", prune_points_fused)):
        if cls is None or not hasattr(cls, attr) or any(c is cls and a == attr for c, a, _ in _patched_resize_classes):
            continue
        _patched_resize_classes.append((cls, attr, getattr(cls, attr)))
        setattr(cls, attr, fn)


# ---- HTGaussianTrainer.merge_two_3DGS: the selection and the row move of a merge on the merge kernels ----------------------------------------
# The reference's merge (trainer/ht3dgs_trainer.py:214-272) scores both models, drops the `prune_ratio` lowest-scoring rows of
# each (`amax`, `topk`, a zero fill and an indexed store per mask), prunes the destination tensor by tensor, gathers the kept source rows
# tensor by tensor and appends them with six `torch.cat` and twelve moment `cat`s.  The body below keeps the reference's order of calls and
# its torch statements wherever a float is computed (the importance through the class's own `calc_importance`, the moved points), and hands
# the decisions and the bytes to the kernels: gsr_select_smallest per model, gsr_resize_plan per model, ONE gsr_merge_apply over the
# destination's six parameters and the moments that exist.
#
# THE TIE RULE is this patch's own: among rows whose score equals the k-th smallest, the rows with the LOWEST ROW NUMBERS go
# (gsr_select_smallest, `np.argsort(key, kind="stable")[:k]`); `torch.topk` promises nothing there.  Where the scores at the threshold are
# distinct the result is the unpatched trainer's to the bit.  Where they tie -- typically unseen Gaussians with a score of exactly 0 -- the
# number of rows dropped is the same, every row strictly below the threshold is dropped, and the tied rows that go are the lowest-numbered.
_patched_merge_classes = []         # [(class, attribute, original function)]
_MERGE_DEFAULT = "1"


def _merge():
    return importlib.import_module("3dgs_hierarchical_training_amd.merge")


def _merge_original(self):
    orig = next((f for c, a, f in _patched_merge_classes if a == "merge_two_3DGS" and isinstance(self, c)), None)
    if orig is None:
        raise RuntimeError("gsr_autopatch: this call needs the original HTGaussianTrainer.merge_two_3DGS")
    return orig


def _merge_source_tensors(g):
    """The six raw tensors of a merge's source model under the tensor checks of `_resize_layout` (its optimizer is not needed), else None."""
    ts = [getattr(g, k, None) for k in RAW_NAMES]
    x = ts[0]
    if not torch.is_tensor(x) or x.dim() != 2 or (_REQUIRE_CUDA and not x.is_cuda) or not 0 < x.shape[0] < 2 ** 31:
        return None
    if not all(torch.is_tensor(t) and t.dtype == torch.float32 and t.device == x.device and t.is_contiguous() and t.dim() >= 1 and
               t.shape[0] == x.shape[0] for t in ts):
        return None
    return ts


def _merge_setup(self, gs_render_dst, gs_render_src, transform_matrix):
    """(destination entries, source tensors, prune_ratio) when the patched merge serves this call, else None.  Reads attributes only: no
    camera is loaded, nothing is rendered or written."""
    if os.environ.get("GSR_AUTOPATCH_MERGE", _MERGE_DEFAULT) == "0":
        return None
    g_dst, g_src = getattr(gs_render_dst, "gaussians", None), getattr(gs_render_src, "gaussians", None)
    if g_dst is None or g_src is None or g_dst is g_src:
        return None
    entries, src = _resize_layout(g_dst), _merge_source_tensors(g_src)
    if entries is None or src is None:
        return None
    dst = [getattr(g_dst, k) for k in RAW_NAMES]
    if any(a.shape[1:] != b.shape[1:] or a.dtype != b.dtype or a.device != b.device for a, b in zip(dst, src)):
        return None
    if tuple(dst[0].shape[1:]) != (3,) or dst[0].shape[0] < 2 or src[0].shape[0] < 2:      # (`amax(-1).squeeze()` loses its dimension at N = 1)
        return None
    T = transform_matrix
    if not (type(T) is torch.Tensor and tuple(T.shape) == (4, 4) and T.dtype == torch.float32 and T.device == dst[0].device):
        return None
    ratio = getattr(getattr(self, "pipe_cfg", None), "prune_ratio", None)
    if not isinstance(ratio, numbers.Real) or not 0 <= ratio <= 1:
        return None
    return entries, src, ratio


def _merge_importance_ok(imp, like) -> bool:
    return type(imp) is torch.Tensor and imp.dtype == torch.float32 and imp.device == like.device and imp.dim() == 2 and \
        imp.shape[0] == like.shape[0] and 1 <= imp.shape[1] <= _merge().L.GSR_SELECT_MAX_COLUMNS


def _merge_reference_tail(g_dst, g_src, importance_dst, importance_src, transform_matrix, ratio):
    """The reference's own statements from the importance on (ht3dgs_trainer.py:234-271), through the model's methods."""
    dev = g_dst._xyz.device
    masks = []
    for g, importance in ((g_dst, importance_dst), (g_src, importance_src)):
        score = importance.amax(-1).squeeze()
        _, lowest = torch.topk(score, int(score.shape[0] * ratio), largest=False)
        mask = torch.zeros((g._xyz.shape[0], 1), device=dev)
        mask[lowest, :] = 1
        masks.append(mask.bool())
    g_dst.prune_points(masks[0].squeeze())
    n = len(g_src._xyz)
    points_homogeneous = torch.cat([g_src._xyz, torch.ones((n, 1), device=dev)], dim=1)
    aligned_xyz_homogeneous = points_homogeneous @ transform_matrix.T
    aligned_xyz = aligned_xyz_homogeneous[:, :3] / aligned_xyz_homogeneous[:, 3].unsqueeze(1)
    valid = ~(masks[1].squeeze())
    g_dst.densification_postfix(aligned_xyz[valid], g_src._features_dc[valid], g_src._features_rest[valid], g_src._opacity[valid],
                                g_src._scaling[valid], g_src._rotation[valid])


def merge_two_3DGS_fused(self, gs_render_dst, gs_render_src, transform_matrix, to_visit_frames_dst=None, to_visit_frames_src=None):
    """Drop-in body of `HTGaussianTrainer.merge_two_3DGS` (trainer/ht3dgs_trainer.py:214-272): same arguments, the same log
    lines, the same `load_viewpoint_cam` calls in the same order, both scores through `HTGaussianTrainer.calc_importance` as the class holds
    it at the call.  Then gsr_select_smallest per model on the [N, C] importance as it stands (no `amax`, `topk` or indexed store), the
    reference's three statements for the moved points on all source rows, two gsr_resize_plan and one gsr_merge_apply over the destination's
    six parameters and the moments that exist (kept rows copied, appended rows zero: what `_prune_optimizer` and `cat_tensors_to_optimizer`
    leave), installed as the resize patch installs (fresh `nn.Parameter` leaves, `.grad` None, state re-keyed with `step` kept; a deferred
    Adam update that was planned on the replaced tensors is dropped by `step()`, as after `prune_points`), statistics zeroed.  The kept
    counts are N - int(N * prune_ratio) by construction, so the call does not wait for the device at all.  Nothing of the source model is
    written.  Ties at the threshold: see THE TIE RULE above.  The switch off, a model outside the resize patch's layout, two models of unlike
    trailing shapes / dtype / device, a `transform_matrix` that is not a float32 [4,4] tensor on that device, a `prune_ratio` outside [0, 1]
    or a model of fewer than 2 rows run the ORIGINAL method, decided before anything is loaded or rendered; an importance of another shape,
    dtype or device (or wider than GSR_SELECT_MAX_COLUMNS) finishes the call with the reference's own statements on that importance."""
    setup = _merge_setup(self, gs_render_dst, gs_render_src, transform_matrix)
    if setup is None:
        return _merge_original(self)(self, gs_render_dst, gs_render_src, transform_matrix, to_visit_frames_dst, to_visit_frames_src)
    entries, src, ratio = setup
    trainer_cls = next((c for c, a, _ in _patched_merge_classes if a == "merge_two_3DGS" and isinstance(self, c)), type(self))
    g_dst, g_src = gs_render_dst.gaussians, gs_render_src.gaussians
    n_dst, n_src, dev = g_dst._xyz.shape[0], g_src._xyz.shape[0], g_dst._xyz.device
    self.logger.info(f"The number of 3D Gaussians in the first 3DGS before merging: {n_dst}")
    self.logger.info(f"The number of 3D Gaussians in the second 3DGS before merging: {n_src}")
    importance = []
    for g, render, frames in ((g_dst, gs_render_dst, to_visit_frames_dst), (g_src, gs_render_src, to_visit_frames_src)):
        cameras = []
        for fidx in frames:
            pose = g.get_RT(fidx).detach().cpu() if not g.rotate_seq else None
            cameras.append(self.load_viewpoint_cam(fidx, pose=pose, load_depth=True))
        importance.append(trainer_cls.calc_importance(render, cameras, self.pipe_cfg))
    with torch.no_grad():
        if not (_merge_importance_ok(importance[0], g_dst._xyz) and _merge_importance_ok(importance[1], g_src._xyz)):
            _merge_reference_tail(g_dst, g_src, importance[0], importance[1], transform_matrix, ratio)
        else:
            M, R = _merge(), _resize()
            k_dst, k_src = int(n_dst * ratio), int(n_src * ratio)
            keep_dst = M.select_smallest(importance[0].contiguous(), k_dst)[1]
            keep_src = M.select_smallest(importance[1].contiguous(), k_src)[1]
            points_homogeneous = torch.cat([src[0], torch.ones((n_src, 1), device=dev)], dim=1)
            aligned_xyz_homogeneous = points_homogeneous @ transform_matrix.T
            aligned_xyz = aligned_xyz_homogeneous[:, :3] / aligned_xyz_homogeneous[:, 3].unsqueeze(1)
            plan_dst, meta = R.resize_plan(keep_dst)
            plan_src, _ = R.resize_plan(keep_src)
            kept_dst, kept_src = n_dst - k_dst, n_src - k_src          # (what the two metas hold; reading them would be the call's one wait)
            by_attr = dict(zip(RAW_NAMES, [aligned_xyz] + [t.detach() for t in src[1:]]))
            src_a, src_b, kinds = [], [], []
            for _, attr, p, st in entries:
                src_a.append(p.detach()); src_b.append(by_attr[attr]); kinds.append(M.PARAM)
                if st is not None:
                    src_a += [st["exp_avg"], st["exp_avg_sq"]]; src_b += [None, None]; kinds += [M.MOMENT, M.MOMENT]
            _install_resized(g_dst, entries, M.merge_apply(plan_dst, meta, n_dst, kept_dst, plan_src, n_src, kept_src, src_a, src_b, kinds))
            n = kept_dst + kept_src
            g_dst.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
            g_dst.denom = torch.zeros((n, 1), device=dev)
            g_dst.max_radii2D = torch.zeros((n,), device=dev)
    self.logger.info(f"The number of 3D Gaussians in the merged 3DGS: {g_dst._xyz.shape[0]}")


def _patch_merge_module(mod):
    if os.environ.get("GSR_AUTOPATCH_MERGE", _MERGE_DEFAULT) == "0":
        return
    cls = getattr(mod, "HTGaussianTrainer", None)
    if cls is None or not hasattr(cls, "merge_two_3DGS") or any(c is cls for c, _, _ in _patched_merge_classes):
        return
    _patched_merge_classes.append((cls, "merge_two_3DGS", cls.merge_two_3DGS))
    cls.merge_two_3DGS = merge_two_3DGS_fused


# ---- utils.image_utils.psnr: the training PSNR the trainer evaluates on every iteration (ht3dgs_trainer.py:138) ---------------------
IMAGE_UTILS_MODULES = ("utils.image_utils",)
_patched_psnr = []                  # [(module, attribute, original function)]


def psnr_fused(img1, img2):
    """Drop-in body of `psnr` (/root/reference/utils/image_utils.py:16-18): per-channel 20 log10(1 / sqrt(mse)), [C, 1], in two
    launches (gsr_psnr) instead of the statement's nine.  Anything but two same-shaped float32 GPU images runs the original."""
    if torch.is_tensor(img1) and torch.is_tensor(img2) and img1.is_cuda and img2.is_cuda and img1.dtype == torch.float32 and \
            img2.dtype == torch.float32 and img1.dim() >= 2 and img1.shape == img2.shape and img1.numel() > 0 and \
            not (torch.is_grad_enabled() and (img1.requires_grad or img2.requires_grad)):
        return _ops().psnr(img1, img2)
    orig = next((f for m, a, f in _patched_psnr if a == "psnr"), None)
    if orig is None:
        mse = (((img1 - img2)) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
        return 20 * torch.log10(1.0 / torch.sqrt(mse))
    return orig(img1, img2)


def _patch_image_utils_module(mod):
    if os.environ.get("GSR_AUTOPATCH_PSNR", "1") == "0":
        return
    orig = getattr(mod, "psnr", None)
    if orig is None or orig is psnr_fused or any(m is mod for m, _, _ in _patched_psnr):
        return
    _patched_psnr.append((mod, "psnr", orig))
    mod.psnr = psnr_fused
    # modules that did `from utils.image_utils import psnr` before this patch hold the original under their own name
    for other in list(sys.modules.values()):
        if other is not None and other is not mod and getattr(other, "__dict__", {}).get("psnr") is orig:
            _patched_psnr.append((other, "psnr", orig))
            other.psnr = psnr_fused


def _patch_loss_module(mod):
    cls = getattr(mod, "Loss", None)
    if cls is None or any(c is cls for c, _ in _patched_loss_classes):
        return
    _patched_loss_classes.append((cls, cls.forward))
    cls.forward = loss_forward


def _patch_render_and_pose_module(mod):
    """`scene.gaussian_model_ht` holds the render wrapper, `HTGaussianModel.get_RT` and the model's surgery."""
    _patch_render_module(mod)
    _patch_frames_module(mod)
    _patch_resize_module(mod)


class _PostImportFinder(importlib.abc.MetaPathFinder):
    """Patches `trainer.losses` / `scene.gaussian_model_ht` / `utils.image_utils` / `trainer.ht3dgs_trainer` / `trainer.trainer` right after they have
    been executed, whenever that import happens."""

    def find_spec(self, fullname, path, target=None):
        if (fullname not in LOSS_MODULES and fullname not in RENDER_MODULES and fullname not in IMAGE_UTILS_MODULES
                and fullname not in TRAINER_MODULES and fullname not in FRAME_MODULES) or not _applied:
            return None
        patch = _patch_loss_module if fullname in LOSS_MODULES else _patch_render_and_pose_module if fullname in RENDER_MODULES \
            else _patch_trainer_module if fullname in TRAINER_MODULES else _patch_frames_module if fullname in FRAME_MODULES \
            else _patch_image_utils_module
        for finder in sys.meta_path:
            if finder is self or not hasattr(finder, "find_spec"):
                continue
            spec = finder.find_spec(fullname, path, target)
            if spec is not None and spec.loader is not None and hasattr(spec.loader, "exec_module"):
                loader = spec.loader
                orig_exec = loader.exec_module

                def exec_module(module, _orig=orig_exec, _patch=patch):
                    _orig(module)
                    if _applied:
                        _patch(module)
                try:
                    loader.exec_module = exec_module
                except Exception:
                    return None
                return spec
        return None


_FINDER = _PostImportFinder()


def apply():
    """Switch the patches on (idempotent)."""
    global _applied
    if _applied:
        return
    _applied = True
    torch.optim.Adam = _AdamDispatch       # (the reference looks the class up as `torch.optim.Adam` at call time, gaussian_model_ht.py:289)
    if _FINDER not in sys.meta_path:
        sys.meta_path.insert(0, _FINDER)
    for name in LOSS_MODULES:
        if name in sys.modules:
            _patch_loss_module(sys.modules[name])
    for name in RENDER_MODULES:
        if name in sys.modules:
            _patch_render_and_pose_module(sys.modules[name])
    for name in FRAME_MODULES:
        if name in sys.modules:
            _patch_frames_module(sys.modules[name])
    for name in IMAGE_UTILS_MODULES:
        if name in sys.modules:
            _patch_image_utils_module(sys.modules[name])
    for name in TRAINER_MODULES:
        if name in sys.modules:
            _patch_trainer_module(sys.modules[name])


def remove():
    """Switch the patches off again (tests, A/B runs)."""
    global _applied
    if not _applied:
        return
    _applied = False
    torch.optim.Adam = _ORIG_ADAM
    if _FINDER in sys.meta_path:
        sys.meta_path.remove(_FINDER)
    while _patched_loss_classes:
        cls, fwd = _patched_loss_classes.pop()
        cls.forward = fwd
    while _patched_render_classes:
        cls, attr, fn = _patched_render_classes.pop()
        setattr(cls, attr, fn)
    while _patched_psnr:
        mod, attr, fn = _patched_psnr.pop()
        setattr(mod, attr, fn)
    while _patched_trainer_classes:
        cls, attr, fn = _patched_trainer_classes.pop()
        setattr(cls, attr, fn)
    while _patched_frame_classes:
        cls, attr, fn = _patched_frame_classes.pop()
        setattr(cls, attr, fn)
    while _patched_merge_classes:
        cls, attr, fn = _patched_merge_classes.pop()
        setattr(cls, attr, fn)
    while _patched_resize_classes:
        cls, attr, fn = _patched_resize_classes.pop()
        setattr(cls, attr, fn)


if os.environ.get("GSR_AUTOPATCH", "1") != "0":
    apply()


if __name__ == "__main__":      # python -m gsr_autopatch script.py [args...]: run a script (e.g. the reference's run.py) under the patches
    import runpy
    if len(sys.argv) < 2:
        raise SystemExit("usage: python -m gsr_autopatch <script.py> [args...]")
    sys.argv = sys.argv[1:]
    sys.path.insert(0, os.path.dirname(os.path.abspath(sys.argv[0])))
    runpy.run_path(sys.argv[0], run_name="__main__")
