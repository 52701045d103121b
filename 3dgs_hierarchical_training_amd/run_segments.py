#!/usr/bin/env python3
"""BASELINE config 4: hierarchical training with one leaf segment per GPU and a point-to-point exchange at each merge.

  python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port P \
         3dgs_hierarchical_training_amd/run_segments.py --frames 40 --leaf-gaussians 200000
  python 3dgs_hierarchical_training_amd/run_segments.py --local --segments 8      # whole tree on one GPU, in order

Stage B of `HTGaussianTrainer.hierarchical_training` (/root/reference/trainer/ht3dgs_trainer.py:710-813) re-cut for
eight GPUs:

  reference (one GPU, sequential)                       here (rank r = leaf r)
  ------------------------------------------------      ---------------------------------------------------------------
  for each leaf: init_leaf_3DGS + train_leaf_3DGS       every rank trains its own leaf at the same time, no communication
    :729-753
  after every second segment: merge_two_3DGS            level k: ranks (2^(k+1) j, 2^(k+1) j + 2^k) pair up; both compute
    (importance of both, prune both, move the             their own child's importance at the same time, the source ships
    source by inverse(get_RT(src.start_fidx)),            the UN-PRUNED child + drop mask + frames + poses over its own
    append) :767-780, :214-272                            xGMI link, the destination applies the masks, moves, appends
  poses of the source's frames chained on :783-790      same, from the (replicated) relative-pose table of stage A
  train_nonleaf_3DGS_phase1 with the two frozen         same, on the destination rank; the teachers are the two un-pruned
    children as teachers for virtual views :757,          children it now holds (its own snapshot + the received one)
    :815-900
  train_nonleaf_3DGS_phase2 on the real frames :762     same

Source ranks are idle after their send (tree reduction: 8 -> 4 -> 2 -> 1 busy GPUs).  Frames, targets and relative
poses are synthetic (sequence.py); the relative-pose table stands for stage A's result (stage_a.py shards that stage).

`RankRunner` holds one rank's state; `run_local` plays all ranks in turn on one device through `LocalTransport`
(senders of a level before its receivers) -- the same code path, and the reference's own execution order.
Every rank prints one JSON line per phase: leaf, and per level {importance_ms, send_ms | recv_ms, bytes, ...}.
"""
import argparse
import functools
import importlib
import json
import os
import random
import sys
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import torch

if __package__ in (None, ""):      # executed as a script: make the oddly named package importable
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if _root not in sys.path:
        sys.path.insert(0, _root)
    _pkg = importlib.import_module("3dgs_hierarchical_training_amd")
    hierarchy = importlib.import_module("3dgs_hierarchical_training_amd.hierarchy")
    segments = importlib.import_module("3dgs_hierarchical_training_amd.segments")
    sequence = importlib.import_module("3dgs_hierarchical_training_amd.sequence")
    ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
    densify = importlib.import_module("3dgs_hierarchical_training_amd.densify")
    pose_mod = importlib.import_module("3dgs_hierarchical_training_amd.pose")
    host_mod = importlib.import_module("3dgs_hierarchical_training_amd.host")
    stage_a = importlib.import_module("3dgs_hierarchical_training_amd.stage_a")
    cameras = importlib.import_module("3dgs_hierarchical_training_amd.cameras")
    pose_fit = importlib.import_module("3dgs_hierarchical_training_amd.pose_fit")
else:
    from . import cameras, densify, hierarchy, segments, sequence
    from . import host as host_mod
    from . import stage_a
    from . import pose as pose_mod
    from . import pose_fit
    from . import train_step as ts


def emit_line(rec):
    """One report record = one line = ONE write (several ranks share the launcher's stdout: print() issues the text and the
    newline separately and the lines of two ranks can interleave)."""
    sys.stdout.write(json.dumps(rec) + "\n")
    sys.stdout.flush()


@dataclass
class HTConfig:
    """Iteration counts follow /root/reference/arguments/full/Tanks/Ballroom.yml:5-16 in meaning; the defaults are
    shortened so the harness finishes in minutes."""
    frames: int = 40
    width: int = 980
    height: int = 545
    sh_degree: int = 3                          # max_sh_degree: 16 stored coefficients
    start_sh_degree: int = 0                    # active degree of a new leaf (gaussian_model_ht.py:68) ...
    sh_up_every: int = 1000                     # ... raised after every this many global iterations (ht3dgs_trainer.py:580-581)
    gt_gaussians: int = 400_000
    leaf_gaussians: int = 200_000
    leaf_iters_per_frame: int = 30              # single_step
    phase1_iters_per_frame: int = 5             # mss_phase1_iteration_per_frame (50 in Ballroom.yml)
    phase1_ratio: float = 0.5                   # mss_phase1_ratio
    phase2_iters_per_frame: List[int] = field(default_factory=lambda: [10, 10, 10])   # num_iterations_per_frame_each_level
    prune_ratio: float = 0.5                    # Ballroom.yml:44
    importance_views: int = 0                   # 0 = all of the child's frames (the reference), k = every (len/k)-th
    eval_pose_iters: int = 0                    # evaluate(): Adam iterations of a test-time pose fit of every frame before it is rendered (pose_fit.fit_poses;
                                                # the start is the pose the run ended with); 0 = render at the run's poses, as ever
    eval_views_per_call: int = 1                # frames of that fit that share a launch chain (1 = frame by frame)
    importance_views_per_call: int = 1          # views of a model one launch chain of the merge's importance takes (hierarchy.group_views):
                                                # 1 = a forward and a pass per view (default), 2..16 = gsr_importance_accumulate_views
    densify: bool = False
    seed: int = 0
    optimizer: str = "hip"
    fused: bool = True
    stage_a_concurrency: int = 2                # frame pairs fitted at the same time per GPU (streams + host threads), stage_a.run_stage_a
    stage_a_batch: int = 0                      # frame pairs fitted in ONE launch chain per GPU (stage_a.fit_pairs_batched, GsrBatch); 1 = off;
                                                # 0 = automatic: 4 per chain with two chains at a time when the host has the CPUs for two launching
                                                # threads (39 pairs: 6.3 s), 8 per chain otherwise (6.9 s); round 2's one pair per chain on two streams: 8.1 s
    stage_a_lambda_depth: float = 0.0           # weight of the depth term in both phases of a stage-A fit (the reference's lambda_depth with
                                                # depth_loss_type 'invariant', ht3dgs_trainer.py:354, :392); 0 = photometric only
    stage_a_early_exit: str = "host"            # how a stage-A image phase ends (stage_a.fit_pair): 'host' = the host looks every 50 iterations (a
                                                # batch waits for all its models); 'device' = each model retires at its own iteration, on the device
    stage_a_init: str = "pixels"                # a stage-A model's initialisation: 'pixels' = sequence.pixel_scene (a strided pixel grid, built on the
                                                # host); 'voxels' = sequence.depth_scene (every pixel, voxel grid 0.01, create_from_pcd: the reference's, on the device)
    densify_route: str = "torch"                # how a densification resizes the model: 'torch' = boolean indexing and torch.cat per tensor; 'kernel' =
                                                # gsr_resize_plan / gsr_resize_apply (resize.py): the same result to the bit, one host wait, one row-moving launch
    merge_route: str = "torch"                  # how a merge picks and moves its rows: 'torch' = amax, topk, boolean gathers and torch.cat; 'kernel' =
                                                # gsr_select_smallest and gsr_merge_apply (merge.py): one host wait; ties at the threshold go by row number
    device_cameras: bool = False                # phase 1's virtual views from poses kept on the device: cameras.virtual_view + settings_from_pose, two
                                                # launches per view instead of host matrix work and eight uploads; a camera may differ from the host
                                                # route's in the last float32 bit, so the default stays the host route
    leaf_batch: int = 0                         # --local: leaves with the same number of frames trained up to this many at a time in ONE launch chain
                                                # (batched.BatchedGaussianParams; with densify: densify.BatchedDensifier on the batched resize kernels);
                                                # 0 and 1 = one leaf after the other
    fit_pose: bool = False                      # refine each frame's pose while training on it (training_setup(fit_pose=True), :733)
    pose_lr: float = 1e-5                       # Adam with eps 1e-15 moves a pose by ~lr per step whatever the gradient: on these
                                                # frames (1-2 px of motion per frame) 5e-6..2e-5 gains 0.4-0.6 dB over fixed stage-A
                                                # poses, 1e-4 loses 0.5 dB (tools/pose_lr_sweep.sh); the reference's rotation_lr is 1e-3


class Segment:
    """One 3DGS model and what the trainer keeps next to it (`gs_render.start_fidx / to_visit_frames /
    global_iteration`, :733-735, :766; `get_RT`, gaussian_model_ht.py:150-160)."""

    def __init__(self, params, frames: List[int], start_fidx: int, poses: Dict[int, torch.Tensor], global_iteration: int = 0):
        self.params, self.frames, self.start_fidx, self.poses, self.global_iteration = params, list(frames), start_fidx, dict(poses), global_iteration
        self.densifier = None
        self.pose_states = {}        # frame -> train_step.PoseState, while its pose is being refined (cfg.fit_pose)

    def pose_state(self, f: int, template, device, lr: float):
        ps = self.pose_states.get(f)
        if ps is None:
            ps = self.pose_states[f] = ts.CameraPoseState(template, self.poses[f], device, lr=lr)
            if f == self.start_fidx:
                ps.freeze()          # the segment's start frame fixes the gauge
        return ps

    def sync_poses(self):
        """Refined transforms back into the pose table (what merges, importance views and evaluation read).  The pose states --
        tangent numbers, Adam moments, step counts -- live as long as the segment does, as the reference's per-frame
        `camera_optimizer[fidx]` lives from one `training_setup` to the next (gaussian_model_ht.py:296-311); a merge builds a new
        Segment and with it fresh states."""
        for f, ps in self.pose_states.items():
            if ps.steps or f not in self.poses:
                self.poses[f] = ps.matrix()

    def pose_tensor(self) -> torch.Tensor:
        return torch.stack([self.poses[f] for f in self.frames])


class RankRunner:
    def __init__(self, rank: int, world: int, transport, seq, cfg: HTConfig, device, log=None, importance_fn=None,
                 step_fn=None, teacher_render_fn=None):
        """importance_fn / step_fn / teacher_render_fn replace the three places that reach the HIP rasterizer; the
        GPU-less gloo tests pass stand-ins so that the tree walk, the messages and the bookkeeping run on CPU."""
        self.rank, self.world, self.tr, self.seq, self.cfg, self.dev = rank, world, transport, seq, cfg, device
        check_importance_views_per_call(cfg)
        self.importance_fn = importance_fn or hierarchy.calc_importance
        if importance_fn is None and cfg.importance_views_per_call > 1:
            self.importance_fn = functools.partial(hierarchy.calc_importance, views_per_call=int(cfg.importance_views_per_call))
        self.step_fn = step_fn
        self.teacher_render_fn = teacher_render_fn or hierarchy.render_raw
        self.level = world.bit_length() - 1
        self.parts = sequence.partition(cfg.frames, self.level)
        self.schedule = segments.merge_schedule(world)
        self.rng = random.Random(cfg.seed * 1000 + rank)
        self.seg: Optional[Segment] = None
        self.teachers = None
        self.log = log if log is not None else emit_line
        self.report = []

    def _emit(self, rec):
        rec = {"rank": self.rank, **rec}
        self.report.append(rec)
        self.log(rec)

    # ---- helpers ---------------------------------------------------------------------------------------------------
    def _settings(self, seg: Segment, f: int):
        """Raster settings of frame f under the segment's current pose of it -- built once per (frame, pose): a draw of a frame
        that was drawn before reuses the device tensors (building them is CPU matrix work + four host-to-device copies, a
        quarter of a leaf's wall time when done per draw)."""
        cache = seg.__dict__.setdefault("_settings_cache", {})
        pose = seg.poses[f]
        hit = cache.get(f)
        if hit is not None and hit[0] is pose:
            return hit[1]
        st = self.seq.settings_for_pose(pose)
        cache[f] = (pose, st)
        return st

    def _device_pose(self, seg: Segment, f: int) -> torch.Tensor:
        """Frame f's pose on the device, uploaded once per pose object (cfg.device_cameras)."""
        cache = seg.__dict__.setdefault("_device_poses", {})
        pose = seg.poses[f]
        hit = cache.get(f)
        if hit is None or hit[0] is not pose:
            hit = cache[f] = (pose, pose.detach().float().contiguous().to(self.dev))
        return hit[1]

    def _importance_views(self, seg: Segment):
        fr = seg.frames
        k = self.cfg.importance_views
        if k and len(fr) > k:
            fr = fr[::max(1, len(fr) // k)][:k]
        return [ts.with_sh_degree(self._settings(seg, f), seg.params.active_sh_degree) if self.step_fn is None else self._settings(seg, f)
                for f in fr]

    def _step(self, seg: Segment, settings, target, next_settings=None):
        """next_settings: the camera of the NEXT step when it is already drawn -- its preprocess then rides in this step's
        backward (train_step / "prepare in backward")."""
        seg.global_iteration += 1
        if self.step_fn is not None:
            return self.step_fn(seg, settings, target)
        up = self._sh_up(seg)
        ts.train_step(seg.params, settings, target, fused_optimizer=self.cfg.fused, densifier=seg.densifier,
                      iteration=seg.global_iteration, next_settings=next_settings,
                      next_sh_degree=min(seg.params.active_sh_degree + 1, seg.params.max_sh_degree) if up else None)
        if up:
            seg.params.oneup_sh_degree()

    def _sh_up(self, seg: Segment) -> bool:
        """`if self.global_iteration % 1000 == 0: oneupSHdegree()` after the step (ht3dgs_trainer.py:580-581, :636-637, :909-910)."""
        return self.cfg.sh_up_every > 0 and seg.global_iteration % self.cfg.sh_up_every == 0

    def _steps_over(self, seg: Segment, frames_drawn):
        """Train on a pre-drawn list of frames (the frame of step k + 1 is known at step k)."""
        if self.cfg.fit_pose and self.step_fn is None:
            # pose refinement: frame f's camera tensors are functions of Exp(delta_f) * pose_f; after each render of frame f its six
            # tangent numbers take one Adam step and the camera is rewritten in place (one kernel, train_step.CameraPoseState).
            # The segment's start frame fixes the gauge and is not refined.
            states = [seg.pose_state(v, self._settings(seg, v), self.dev, self.cfg.pose_lr) for v in frames_drawn]
            for k, v in enumerate(frames_drawn):
                seg.global_iteration += 1
                up = self._sh_up(seg)
                ts.train_step(seg.params, states[k].settings, self.seq.target(v), fused_optimizer=self.cfg.fused, densifier=seg.densifier,
                              iteration=seg.global_iteration, pose=states[k], next_pose=states[k + 1] if k + 1 < len(states) else None,
                              next_sh_degree=min(seg.params.active_sh_degree + 1, seg.params.max_sh_degree) if up else None)
                if up:
                    seg.params.oneup_sh_degree()
            seg.sync_poses()
            return
        st = [self._settings(seg, v) for v in frames_drawn]
        for k, v in enumerate(frames_drawn):
            self._step(seg, st[k], self.seq.target(v), st[k + 1] if k + 1 < len(st) else None)

    def _new_densifier(self, seg: Segment):
        if self.cfg.densify:
            seg.densifier = densify.Densifier(seg.params, scene_extent=5.0, cfg=densify.DensifyConfig(
                densify_from_iter=50, densification_interval=100, opacity_reset_interval=3000,
                max_points=4 * seg.params.num_points), seed=self.rank, route=self.cfg.densify_route)

    # ---- leaf (:729-753) ---------------------------------------------------------------------------------------------
    def train_leaf(self):
        cfg = self.cfg
        frames = self.parts[self.level][self.rank]
        start = frames[0]
        scene = self.seq.leaf_scene(start, cfg.leaf_gaussians, seed=cfg.seed + 17 * self.rank)
        params = ts.GaussianParams(scene, self.dev, optimizer=cfg.optimizer)
        params.active_sh_degree = min(cfg.start_sh_degree, params.max_sh_degree)      # a new model starts at degree 0 (gaussian_model_ht.py:68)
        seg = Segment(params, frames, start, {start: torch.eye(4)})
        self._new_densifier(seg)
        t0 = time.perf_counter()
        visited, steps = [start], 0
        for f in frames[1:]:
            seg.poses[f] = self.seq.rel_pose(f - 1, f) @ seg.poses[f - 1]          # :739-741
            visited.append(f)
            drawn = [self.rng.choice(visited) for _ in range(cfg.leaf_iters_per_frame)]   # sample_a_training_frame, :482-505
            self._steps_over(seg, drawn)
            steps += len(drawn)
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)
        self.seg = seg
        self._emit({"phase": "leaf", "frames": [frames[0], frames[-1]], "steps": steps, "gaussians": params.num_points,
                    "ms": 1e3 * (time.perf_counter() - t0)})

    # ---- merge (:767-793, :214-272) ----------------------------------------------------------------------------------
    def role(self, k: int):
        return segments.partner(self.rank, self.schedule[k])

    def merge_send(self, k: int):
        seg, self.tr.rank = self.seg, self.rank
        st = hierarchy.merge_send(self.tr, self.role(k)[1], seg.params.raw(), self._importance_views(seg), self.cfg.prune_ratio,
                                  frames=seg.frames, poses=seg.pose_tensor(), start_fidx=seg.start_fidx,
                                  global_iteration=seg.global_iteration, importance_fn=self.importance_fn,
                                  sh_degree=seg.params.active_sh_degree, route=self.cfg.merge_route)
        self.seg = None          # this GPU is free from here on
        self._emit({"phase": "merge", "level": k, **st})

    def merge_recv(self, k: int):
        seg, self.tr.rank = self.seg, self.rank
        # child coordinates -> this model's coordinates: inverse of get_RT(child.start_fidx), :778-780.  The child's
        # start frame is one of this model's own frames (the partitions overlap by two frames).
        src_to_dst = lambda msg: torch.linalg.inv(seg.poses[msg["start_fidx"]])
        out = hierarchy.merge_recv(self.tr, self.role(k)[1], seg.params.raw(), self._importance_views(seg),
                                   self.cfg.prune_ratio, src_to_dst, importance_fn=self.importance_fn, route=self.cfg.merge_route)
        child = out["child"]
        # teachers render at the active degree their model was trained at: the destination's own, and the child's as its message
        # states it (uneven frame splits or iteration counts can leave the two on different sides of an oneupSHdegree boundary)
        tdeg = seg.params.active_sh_degree
        cdeg = child.get("sh_degree", -1)
        cdeg = tdeg if cdeg is None or cdeg < 0 else min(int(cdeg), seg.params.max_sh_degree)
        own_teacher = {"seg": {kk: v.clone() for kk, v in out["teachers"][0].items()}, "start_fidx": seg.start_fidx,
                       "frames": list(seg.frames), "sh_degree": tdeg}
        child_teacher = {"seg": out["teachers"][1], "start_fidx": child["start_fidx"], "frames": list(child["frames"]), "sh_degree": cdeg}
        self.teachers = [own_teacher, child_teacher]
        for f in child["frames"]:                                                    # :783-790
            if f not in seg.poses:
                seg.poses[f] = self.seq.rel_pose(f - 1, f) @ seg.poses[f - 1]
        frames = sorted(set(seg.frames + child["frames"]))                           # :796
        # (the merged model keeps the destination's active degree: `restore` carries it, gaussian_model_ht.py:107-124)
        params = ts.GaussianParams.from_raw(out["merged"], self.dev, sh_degree=seg.params.active_sh_degree, optimizer=self.cfg.optimizer)
        self.seg = Segment(params, frames, seg.start_fidx, seg.poses, global_iteration=0)   # :792-793
        self._new_densifier(self.seg)
        self._emit({"phase": "merge", "level": k, "sh_degree_dst": tdeg, "sh_degree_child": cdeg, "sh_degree_merged": tdeg,
                    **{kk: v for kk, v in out.items() if kk not in ("merged", "teachers", "child")}})

    # ---- non-leaf training (:757-764, :815-900) ------------------------------------------------------------------------
    def train_nonleaf(self, k: int):
        cfg, seg = self.cfg, self.seg
        frames = seg.frames
        t0 = time.perf_counter()
        n1 = cfg.phase1_iters_per_frame * len(frames)
        virtual = 0
        for _ in range(n1):
            f = self.rng.choice(frames)
            if self.rng.random() < cfg.phase1_ratio:
                alpha = self.rng.random()
                if f == frames[-1]:
                    f -= 1
                if f + 1 not in seg.poses:
                    continue
                teacher = next((t for t in self.teachers[::-1] if f >= t["start_fidx"] and f in t["frames"]), None)
                if teacher is None:
                    raise ValueError(f"frame {f} belongs to no child")
                if cfg.device_cameras:       # the view and its teacher-relative twin in one launch, a camera each in one more; nothing on the host
                    p, p_wrt_teacher = cameras.virtual_view(self._device_pose(seg, f), self._device_pose(seg, f + 1), alpha,
                                                            base=self._device_pose(seg, teacher["start_fidx"]))
                    st_teacher = self.seq.settings_for_pose(p_wrt_teacher)
                    pseudo = self.teacher_render_fn(teacher["seg"], ts.with_sh_degree(st_teacher, teacher["sh_degree"]) if self.step_fn is None else st_teacher)
                    self._step(seg, self.seq.settings_for_pose(p), pseudo)
                    virtual += 1
                    continue
                p = pose_mod.interpolate_pose(seg.poses[f], seg.poses[f + 1], alpha)     # get_virtual_view, :462-479
                p_wrt_teacher = p @ torch.linalg.inv(seg.poses[teacher["start_fidx"]])    # :874
                pseudo = self.teacher_render_fn(teacher["seg"], ts.with_sh_degree(self.seq.settings_for_pose(p_wrt_teacher), teacher["sh_degree"])
                                                if self.step_fn is None else self.seq.settings_for_pose(p_wrt_teacher))
                self._step(seg, self.seq.settings_for_pose(p), pseudo)
                virtual += 1
            else:
                self._step(seg, self._settings(seg, f), self.seq.target(f))
        self.teachers = None                                                               # :758-760
        lvl = self.level - 1 - k
        per = cfg.phase2_iters_per_frame[min(lvl, len(cfg.phase2_iters_per_frame) - 1)]
        n2 = per * len(frames)
        self._steps_over(seg, [self.rng.choice(frames) for _ in range(n2)])
        if self.dev.type == "cuda":
            torch.cuda.synchronize(self.dev)
        self._emit({"phase": "nonleaf", "level": k, "phase1_steps": n1, "virtual_views": virtual, "phase2_steps": n2,
                    "gaussians": seg.params.num_points, "ms": 1e3 * (time.perf_counter() - t0)})

    def evaluate(self) -> float:
        """Mean PSNR of the final model over its frames.  cfg.eval_pose_iters > 0: every frame's pose is first fitted against the frozen
        model (pose_fit.fit_poses from the pose the run ended with, cfg.eval_views_per_call frames per launch chain -- the reference's
        test-time fit of eval_nvs); an 'eval' record carries the PSNR before and after, the PSNR after is returned.  The segment keeps
        the poses it had."""
        seg, tot = self.seg, 0.0
        with torch.no_grad():
            for f in seg.frames:
                img = ts.render_image(seg.params, self._settings(seg, f))[0]     # (the render-only forward: nothing kept behind the image)
                mse = ((img - self.seq.target(f)) ** 2).mean().clamp_min(1e-12)
                tot += float(-10.0 * torch.log10(mse))
        before = tot / len(seg.frames)
        n = int(self.cfg.eval_pose_iters)
        if n <= 0:
            return before
        t0 = time.perf_counter()
        start = torch.stack([seg.poses[f].detach().float().cpu() for f in seg.frames])      # [F,4,4] world-to-camera
        origin = -(start[:, :3, :3].transpose(1, 2) @ start[:, :3, 3:]).squeeze(-1)         # the cameras' centres: the SH view origin
        ident = ts.with_sh_degree(self.seq.settings_for_pose(torch.eye(4)), seg.params.active_sh_degree)
        M, info = pose_fit.fit_poses(seg.params.raw(), ident, torch.stack([self.seq.target(f) for f in seg.frames]), init=start.to(self.dev),
                                     iters=n, lr=float(self.cfg.pose_lr), views_per_call=int(self.cfg.eval_views_per_call),
                                     sh_origin=origin.to(self.dev) if seg.params.active_sh_degree > 0 else None)
        fitted, tot = M.detach().cpu(), 0.0
        with torch.no_grad():
            for k, f in enumerate(seg.frames):
                pose = torch.eye(4)
                pose[:3] = fitted[k]
                img = ts.render_image(seg.params, self.seq.settings_for_pose(pose))[0]
                mse = ((img - self.seq.target(f)) ** 2).mean().clamp_min(1e-12)
                tot += float(-10.0 * torch.log10(mse))
        after = tot / len(seg.frames)
        self._emit({"phase": "eval", "pose_iters": n, "views_per_call": info["views_per_call"], "launch_chains": info["launch_chains"],
                    "psnr_before": before, "psnr_after": after, "ms": 1e3 * (time.perf_counter() - t0)})
        return after

    # ---- one rank's whole run (distributed) ----------------------------------------------------------------------------
    def link_selftest(self, all_ok=None) -> bool:
        """1 MB along every edge of the merge tree this rank takes part in, before any training (segments.link_selftest).
        all_ok: callable(bool) -> bool that combines the ranks' verdicts (an all-reduce); every rank then leaves together."""
        self.tr.rank = self.rank
        st = segments.link_selftest(self.tr, self.schedule, self.dev)
        good = st["ok"] if all_ok is None else all_ok(st["ok"])
        self._emit({"phase": "link_selftest", **st, "all_ranks_ok": good})
        if not good:
            self._emit({"phase": "error", "error": "merge-tree link self-test failed", "pairs": [p for p in st["pairs"] if not p["ok"]]})
        return good

    def run(self, barrier=None, all_ok=None):
        # a rank whose link self-test failed must not leave alone while its peers walk on to a merge that then never completes: with
        # more than one rank the verdicts have to be combined
        if all_ok is None and self.world > 1 and not isinstance(self.tr, segments.LocalTransport):
            raise RuntimeError("RankRunner.run: with world > 1 pass all_ok (a MIN all-reduce of the ranks' link self-test verdicts)")
        if not self.link_selftest(all_ok):
            raise SystemExit(3)
        self.train_leaf()
        for k in range(len(self.schedule)):
            if barrier is not None:
                barrier()
            if self.seg is None:
                continue
            r = self.role(k)
            if r is None:
                continue
            if r[0] == "send":
                self.merge_send(k)
            else:
                self.merge_recv(k)
                self.train_nonleaf(k)
        return self.seg


LEAF_BATCH_MAX = 16      # models of one batched store (include/gsr.h GSR_RESIZE_MAX_MODELS)


def check_importance_views_per_call(cfg: HTConfig):
    """`importance_views_per_call` is 1 .. hierarchy.MAX_VIEWS_PER_CALL, refused before a device is touched."""
    n = int(cfg.importance_views_per_call)
    if not 1 <= n <= hierarchy.MAX_VIEWS_PER_CALL:
        raise ValueError(f"importance_views_per_call: 1..{hierarchy.MAX_VIEWS_PER_CALL} views share a launch chain, got {n}")


def check_eval_pose(cfg: HTConfig):
    """`eval_pose_iters` >= 0 and `eval_views_per_call` in 1 .. 16, refused before a device is touched."""
    if int(cfg.eval_pose_iters) < 0:
        raise ValueError(f"eval_pose_iters must not be negative, got {cfg.eval_pose_iters}")
    pose_fit.check_views_per_call(int(cfg.eval_views_per_call))


def check_leaf_batch(cfg: HTConfig, local: bool):
    """The combinations `leaf_batch` >= 2 serves, refused before a device is touched: the local walk, without pose refinement."""
    n = int(cfg.leaf_batch)
    if n < 0:
        raise ValueError("leaf_batch must not be negative")
    if n < 2:
        return
    if n > LEAF_BATCH_MAX:
        raise ValueError(f"leaf_batch: at most {LEAF_BATCH_MAX} leaves share a batch")
    if not local:
        raise ValueError("leaf_batch >= 2 needs --local: with one leaf per rank there is nothing to batch")
    if cfg.fit_pose:
        raise ValueError("leaf_batch >= 2 does not refine poses (--fit-pose trains one camera per step)")


def leaf_groups(leaf_parts: List[List[int]], leaf_batch: int) -> List[List[int]]:
    """The leaves (their ranks) that train together: leaves with the same number of frames advance in lockstep, so they are grouped by it,
    in rank order, and cut into batches of `leaf_batch` at most.  partition(40, 3) gives leaves of 6, 7, 7, 7, 6, 7, 7, 7 frames: ranks
    [0, 4] and [1, 2, 3, 5, 6, 7]."""
    by_len: Dict[int, List[int]] = {}
    for r, frames in enumerate(leaf_parts):
        by_len.setdefault(len(frames), []).append(r)
    n = max(1, int(leaf_batch))
    return [ranks[i: i + n] for ranks in by_len.values() for i in range(0, len(ranks), n)]


def train_leaves_batched(group: List["RankRunner"]):
    """`RankRunner.train_leaf` for several leaves with the same number of frames, as one batch: one parameter store, one launch chain per
    step.  Every runner's own `rng` draws its frames in the order the leaf alone would draw them; the cameras of a step go through
    `batch_settings`; with cfg.densify one `BatchedDensifier` resizes all models at once (seeds[b] = the rank, the cap of model b four
    times its first size, as `_new_densifier` gives a leaf alone).  At the end every runner receives its model as a `GaussianParams` of
    its own (fresh optimizer: `merge_recv` builds a new one anyway), its Segment and its "leaf" report line."""
    batched = importlib.import_module("3dgs_hierarchical_training_amd.batched")
    r0 = group[0]
    cfg, seq, dev = r0.cfg, r0.seq, r0.dev
    frames = [rr.parts[rr.level][rr.rank] for rr in group]
    assert len({len(f) for f in frames}) == 1, "the leaves of a batch have the same number of frames"
    scenes = [seq.leaf_scene(f[0], cfg.leaf_gaussians, seed=cfg.seed + 17 * rr.rank) for rr, f in zip(group, frames)]
    batch = batched.BatchedGaussianParams(scenes, dev, optimizer=cfg.optimizer)
    batch.active_sh_degree = min(cfg.start_sh_degree, batch.max_sh_degree)
    segs = [Segment(None, f, f[0], {f[0]: torch.eye(4)}) for f in frames]
    densifier = None
    if cfg.densify:
        densifier = densify.BatchedDensifier(batch, scene_extent=5.0, cfg=densify.DensifyConfig(
            densify_from_iter=50, densification_interval=100, opacity_reset_interval=3000), seeds=[rr.rank for rr in group],
            max_points=[4 * n for n in batch.counts])
    t0 = time.perf_counter()
    visited, steps, iteration = [[f[0]] for f in frames], 0, 0
    for j in range(1, len(frames[0])):
        drawn = []
        for rr, seg, fr, vis in zip(group, segs, frames, visited):
            f = fr[j]
            seg.poses[f] = seq.rel_pose(f - 1, f) @ seg.poses[f - 1]
            vis.append(f)
            drawn.append([rr.rng.choice(vis) for _ in range(cfg.leaf_iters_per_frame)])
        views = [batched.batch_settings([rr._settings(seg, d[k]) for rr, seg, d in zip(group, segs, drawn)], dev)
                 for k in range(cfg.leaf_iters_per_frame)]
        for k, view in enumerate(views):
            iteration += 1
            up = cfg.sh_up_every > 0 and iteration % cfg.sh_up_every == 0
            ts.train_step(batch, view, torch.stack([seq.target(d[k]) for d in drawn]), fused_optimizer=cfg.fused, densifier=densifier,
                          iteration=iteration, next_settings=views[k + 1] if k + 1 < len(views) else None,
                          next_sh_degree=min(batch.active_sh_degree + 1, batch.max_sh_degree) if up else None)
            if up:
                batch.oneup_sh_degree()
        steps += len(views)
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    ms = 1e3 * (time.perf_counter() - t0)
    for b, (rr, seg, fr) in enumerate(zip(group, segs, frames)):
        seg.params = ts.GaussianParams.from_raw({k: v.clone() for k, v in batch.model_raw(b).items()}, dev, sh_degree=batch.active_sh_degree,
                                                optimizer=cfg.optimizer)
        seg.global_iteration = iteration
        rr.seg = seg
        rr._emit({"phase": "leaf", "frames": [fr[0], fr[-1]], "steps": steps, "gaussians": seg.params.num_points, "ms": ms / len(group),
                  "leaf_batch": len(group), "batch_ms": ms})


def train_leaves_local(runners: List["RankRunner"], cfg: HTConfig):
    """The leaf phase of the local walk: one leaf after the other, or with cfg.leaf_batch >= 2 the groups of `leaf_groups` as batches."""
    if cfg.leaf_batch >= 2:
        for ranks in leaf_groups(runners[0].parts[runners[0].level], cfg.leaf_batch):
            if len(ranks) == 1:
                runners[ranks[0]].train_leaf()
            else:
                train_leaves_batched([runners[r] for r in ranks])
    else:
        for rr in runners:
            rr.train_leaf()


def run_local(world: int, seq, cfg: HTConfig, device, log=None):
    """All ranks in turn on one device (the reference's execution order).  Returns (root RankRunner, report)."""
    check_leaf_batch(cfg, local=True)
    tr = segments.LocalTransport(world)
    runners = [RankRunner(r, world, tr, seq, cfg, device, log=log) for r in range(world)]
    train_leaves_local(runners, cfg)
    for k in range(len(runners[0].schedule)):
        pairs = runners[0].schedule[k]
        for dst, src in pairs:
            runners[src].merge_send(k)
        for dst, src in pairs:
            runners[dst].merge_recv(k)
            runners[dst].train_nonleaf(k)
    return runners[0], [rec for rr in runners for rec in rr.report]


def run_stage_a_on(seq, cfg, dev, spec, rank: int, world: int, group=None, log=None, gather_device=None):
    """Stage A of hierarchical_training (ht3dgs_trainer.py:697-698) on this rank's share of the frame pairs; every rank ends
    with the full pose table and adopts it.  Returns the report record."""
    n_points, image_iters, pose_iters = spec
    t0 = time.perf_counter()
    mine = stage_a.pairs_of_rank(cfg.frames, rank, world)
    for f in sorted({q for p in mine for q in (p, p + 1)}):      # targets / depths rendered once, on the main stream, before the workers start
        seq.target(f)
    for p in mine:
        seq.depth(p)
    # concurrent fits per GPU, as far as the host allows: every fitting thread keeps about one CPU busy (launching, polling for the
    # instance count), and the ranks of a node share the container's CPU quota
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", "1" if world == 1 else str(world)))
    conc = max(1, min(cfg.stage_a_concurrency, host_mod.usable_cpus()[0] // (2 * max(1, local_world))))
    batch = cfg.stage_a_batch if cfg.stage_a_batch > 0 else (4 if conc > 1 else 8)
    # the kernels' limits on a batch (include/gsr.h GsrBatch): 16 models per launch chain, B * tile rows <= 4095
    tiles_y = (cfg.height + 15) // 16
    batch = max(1, min(batch, 16, 4095 // max(1, tiles_y)))
    table = stage_a.run_stage_a(cfg.frames, lambda p: stage_a.fit_pair(seq, p, dev, n_points=n_points, single_image_iters=image_iters,
                                                                        pose_iters=pose_iters, seed=cfg.seed,
                                                                        lambda_depth=cfg.stage_a_lambda_depth, early_exit=cfg.stage_a_early_exit,
                                                                        init=cfg.stage_a_init),
                                gather_device or dev, rank=rank, world=world, group=group, concurrency=conc, fit_device=dev,
                                batch=batch,
                                batch_fn=lambda ps: stage_a.fit_pairs_batched(seq, ps, dev, n_points=n_points, single_image_iters=image_iters,
                                                                              pose_iters=pose_iters, seed=cfg.seed,
                                                                              lambda_depth=cfg.stage_a_lambda_depth, early_exit=cfg.stage_a_early_exit,
                                                                              init=cfg.stage_a_init))
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    err = max(float((table[f"rel_pose_{p}_to_{p + 1}"].cpu() - seq.true_rel_pose(p, p + 1)).abs().max()) for p in range(cfg.frames - 1))
    ident = max(float((torch.eye(4) - seq.true_rel_pose(p, p + 1)).abs().max()) for p in range(cfg.frames - 1))
    seq.use_pose_table(table)
    rec = {"rank": rank, "phase": "stage_a", "pairs_total": cfg.frames - 1, "pairs_here": len(stage_a.pairs_of_rank(cfg.frames, rank, world)),
           "gaussians": n_points, "image_iters": image_iters, "pose_iters": pose_iters,
           "pairs_at_a_time": batch * conc if batch > 1 else conc,
           "mode": f"batched: {batch} pairs per launch chain, {conc} chain(s) at a time" if batch > 1 else f"{conc} stream(s), one pair each",
           "ms": 1e3 * (time.perf_counter() - t0),
           "max_abs_pose_error": err, "identity_guess_error": ident}
    (log or emit_line)(rec)
    return rec


def self_launch(a):
    """`python run_segments.py --ranks N` with no launcher around it: become the launcher (VERDICT r4 item 1 -- a bare command must
    never turn into a one-rank walk of an N-segment job)."""
    import socket
    import subprocess
    if not a.launch_check and not a.one_device:
        ndev = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if ndev < a.ranks:
            emit_line({"phase": "error", "error": f"--ranks {a.ranks} but {ndev} GPU(s) visible to this process: refusing to start"})
            raise SystemExit(3)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    raise SystemExit(subprocess.call(cmd, env=env))


def launch_check(a):
    """The process group and the merge tree's edges, nothing else: rank ids all_gathered, `segments.link_selftest` along every
    (dst, src) pair of every level, verdicts combined by the MIN all-reduce the real run uses.  Host tensors under gloo."""
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if a.ranks and a.ranks != world:
        if rank == 0:
            emit_line({"phase": "error", "error": f"--ranks {a.ranks} but WORLD_SIZE={world}"})
        raise SystemExit(2)
    on_dev = a.backend == "nccl"
    dev = torch.device("cuda", 0 if a.one_device else int(os.environ.get("LOCAL_RANK", "0"))) if on_dev else torch.device("cpu")
    if on_dev:
        torch.cuda.set_device(dev)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group(a.backend, device_id=dev if on_dev else None)
    ids = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
    dist.all_gather(ids, torch.tensor([rank], dtype=torch.int64, device=dev))
    tr = segments.DistTransport()
    st = segments.link_selftest(tr, segments.merge_schedule(world), dev)
    flag = torch.tensor([1.0 if st["ok"] else 0.0], device=dev)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    dist.barrier()
    if rank == 0:
        emit_line({"phase": "launch_check", "world": world, "backend": a.backend, "ranks_seen": sorted(int(t.item()) for t in ids),
                   "selftest_ok": bool(flag.item() >= 1.0), "edges_of_rank0": st["pairs"]})
    dist.destroy_process_group()


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--local", action="store_true", help="walk the whole tree on one GPU (no process group)")
    ap.add_argument("--segments", type=int, default=8, help="leaf segments for --local (otherwise WORLD_SIZE)")
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--width", type=int, default=980)
    ap.add_argument("--height", type=int, default=545)
    ap.add_argument("--gt-gaussians", type=int, default=400_000)
    ap.add_argument("--leaf-gaussians", type=int, default=200_000)
    ap.add_argument("--leaf-iters", type=int, default=30)
    ap.add_argument("--phase1-iters", type=int, default=5)
    ap.add_argument("--phase2-iters", type=int, default=10)
    ap.add_argument("--importance-views", type=int, default=0)
    ap.add_argument("--importance-views-per-call", type=int, default=1,
                    help="views of a model that one launch chain of the merge's importance takes: 1 = a forward and a pass per view "
                         "(default); 2..16 = runs of views go through the views entry, one host wait per run")
    ap.add_argument("--eval-pose-iters", type=int, default=0,
                    help="fit every frame's pose against the final model for this many Adam iterations before the evaluation renders it "
                         "(from the pose the run ended with); the PSNR before and after goes into an 'eval' record.  0 = off (default)")
    ap.add_argument("--eval-views-per-call", type=int, default=1,
                    help="frames of that fit that share one launch chain: 1 = frame by frame (default); 2..16 = chunks of frames through the "
                         "views entries (one render, one loss, one backward and one pose step per chunk and iteration)")
    ap.add_argument("--densify", action="store_true")
    ap.add_argument("--pose-lr", type=float, default=None)
    ap.add_argument("--fit-pose", action="store_true", help="refine every frame's pose while training on it (the reference's "
                                                            "camera_optimizer): one pose-step kernel per train step")
    ap.add_argument("--backend", default="nccl")
    ap.add_argument("--stage-a", type=int, nargs=3, metavar=("GAUSSIANS", "IMAGE_ITERS", "POSE_ITERS"), default=None,
                    help="run stage A first (relative pose of every consecutive frame pair: single-image 3DGS of frame p, then the "
                         "SE(3) fit on frame p+1; pairs round-robin over the ranks, one all_gather) and chain ITS poses in stage B "
                         "instead of the synthetic ground truth.  The reference's counts are 1000 and 300 iterations")
    ap.add_argument("--sh-up-every", type=int, default=1000, help="raise the active SH degree after every this many global iterations of a "
                                                                  "model (the reference: 1000; a new leaf starts at degree 0)")
    ap.add_argument("--stage-a-batch", type=int, default=0, help="frame pairs of stage A fitted in one launch chain (GsrBatch); 0 = automatic "
                                                                "(4 per chain, two chains at a time; 8 when the host has CPUs for one launching "
                                                                "thread only), 1 = one pair per chain, two chains at a time (round 2)")
    ap.add_argument("--stage-a-lambda-depth", type=float, default=0.0, help="weight of the scale-and-shift-invariant depth term in stage A's "
                                                                            "image and pose fits (against the frame's depth map); 0 = off")
    ap.add_argument("--stage-a-early-exit", choices=("host", "device"), default="host",
                    help="end of a stage-A image phase: host = PSNR looked at by the host every 50 iterations, a batch runs until all its models "
                         "have passed (default); device = every model retires at its own first iteration past 500 with PSNR > 35 dB, decided "
                         "and applied on the device -- the pose table then does not depend on which pairs share a batch")
    ap.add_argument("--stage-a-init", choices=("pixels", "voxels"), default="pixels",
                    help="a stage-A model's initialisation: pixels = one Gaussian per strided pixel, built on the host (default); voxels = every "
                         "pixel un-projected, voxel grid of 0.01, create_from_pcd -- the reference's initialisation, built on the device")
    ap.add_argument("--densify-route", choices=("torch", "kernel"), default="torch",
                    help="how a densification resizes the model: torch = boolean indexing and torch.cat per tensor (default); kernel = the "
                         "resize kernels, the same result to the bit with one host wait and one launch that moves every row")
    ap.add_argument("--leaf-batch", type=int, default=0,
                    help="--local: train up to this many leaves with the same number of frames in one launch chain (one batched store; with "
                         "--densify the batched resize kernels resize all its models at once); 0 or 1 = one leaf after the other (default)")
    ap.add_argument("--merge-route", choices=("torch", "kernel"), default="torch",
                    help="how a merge picks the Gaussians it drops and appends the rest: torch = amax, topk, boolean gathers and torch.cat "
                         "(default); kernel = the selection and row-move kernels, one host wait; rows tied at the threshold are dropped by row number")
    ap.add_argument("--device-cameras", action="store_true",
                    help="phase 1's virtual views from poses kept on the device (cameras.virtual_view + settings_from_pose: two launches per view, no "
                         "host matrix work or uploads); a camera may differ from the host route's in the last float32 bit.  Default: the host route")
    ap.add_argument("--one-device", action="store_true", help="every rank on cuda:0 (with --backend gloo: the multi-process walk on a "
                                                              "one-GPU box; messages are staged through host memory)")
    ap.add_argument("--ranks", type=int, default=0, help="as a BARE command (WORLD_SIZE unset): start this many ranks of this very script "
                                                         "under torch.distributed.run (one per GPU, rendezvous on 127.0.0.1) and exit with their code; "
                                                         "fewer visible devices than ranks: a JSON error line and exit code 3")
    ap.add_argument("--launch-check", action="store_true", help="launcher plumbing only (needs no GPU with --backend gloo): form the process "
                                                                "group, run the link self-test along every edge of the merge tree, report, leave")
    return ap


def parse_args(argv=None):
    """The command line, with what can be refused without a device refused here."""
    ap = build_parser()
    a = ap.parse_args(argv)
    if not 1 <= a.importance_views_per_call <= hierarchy.MAX_VIEWS_PER_CALL:
        ap.error(f"--importance-views-per-call: 1..{hierarchy.MAX_VIEWS_PER_CALL} expected, got {a.importance_views_per_call}")
    if a.eval_pose_iters < 0:
        ap.error(f"--eval-pose-iters: a non-negative count expected, got {a.eval_pose_iters}")
    if not 1 <= a.eval_views_per_call <= 16:
        ap.error(f"--eval-views-per-call: 1..16 expected, got {a.eval_views_per_call}")
    return a


def main():
    a = parse_args()
    if a.ranks > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(a)
    if a.launch_check:
        return launch_check(a)
    cfg = HTConfig(frames=a.frames, width=a.width, height=a.height, gt_gaussians=a.gt_gaussians, leaf_gaussians=a.leaf_gaussians,
                   leaf_iters_per_frame=a.leaf_iters, phase1_iters_per_frame=a.phase1_iters, phase2_iters_per_frame=[a.phase2_iters] * 3,
                   importance_views=a.importance_views, importance_views_per_call=a.importance_views_per_call, densify=a.densify, fit_pose=a.fit_pose, stage_a_batch=a.stage_a_batch, stage_a_lambda_depth=a.stage_a_lambda_depth, stage_a_early_exit=a.stage_a_early_exit, stage_a_init=a.stage_a_init, densify_route=a.densify_route, merge_route=a.merge_route, sh_up_every=a.sh_up_every,
                   device_cameras=a.device_cameras, leaf_batch=a.leaf_batch, eval_pose_iters=a.eval_pose_iters,
                   eval_views_per_call=a.eval_views_per_call)
    check_leaf_batch(cfg, local=a.local)
    check_eval_pose(cfg)
    if a.pose_lr is not None:
        cfg.pose_lr = a.pose_lr
    if not torch.cuda.is_available():
        raise SystemExit("run_segments.py needs a ROCm GPU (no CPU fallback in the product path)")
    host_mod.cap_host_threads()   # the container's CPU quota, not the visible core count (host.py)
    if a.local:
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        seq = sequence.FrameSequence(cfg.frames, cfg.gt_gaussians, cfg.width, cfg.height, dev, seed=cfg.seed)
        t0 = time.perf_counter()
        if a.stage_a:
            run_stage_a_on(seq, cfg, dev, a.stage_a, 0, 1)
        root, _ = run_local(a.segments, seq, cfg, dev)
        emit_line({"phase": "done", "world": a.segments, "mode": "local", "gaussians": root.seg.params.num_points,
                   "psnr": root.evaluate(), "total_s": time.perf_counter() - t0})
        return
    import torch.distributed as dist
    rank, world, local_rank = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("LOCAL_RANK", "0"))
    if a.ranks and a.ranks != world:
        if rank == 0:
            emit_line({"phase": "error", "error": f"--ranks {a.ranks} but WORLD_SIZE={world}"})
        raise SystemExit(2)
    if not a.one_device and torch.cuda.device_count() <= local_rank:
        emit_line({"phase": "error", "rank": rank, "error": f"LOCAL_RANK={local_rank} has no device: {torch.cuda.device_count()} GPU(s) visible"})
        raise SystemExit(3)
    if a.one_device and a.backend == "nccl":
        raise SystemExit("--one-device needs --backend gloo (RCCL refuses two ranks on one device)")
    dev = torch.device("cuda", 0 if a.one_device else local_rank)
    torch.cuda.set_device(dev)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group(a.backend, device_id=dev if a.backend == "nccl" else None)
    seq = sequence.FrameSequence(cfg.frames, cfg.gt_gaussians, cfg.width, cfg.height, dev, seed=cfg.seed)
    rr = RankRunner(rank, world, segments.DistTransport(host_staging=(a.backend != "nccl")), seq, cfg, dev)
    t0 = time.perf_counter()
    if a.stage_a:   # (gloo gathers host tensors; the table is tiny -- 192 bytes per pair)
        run_stage_a_on(seq, cfg, dev, a.stage_a, rank, world, gather_device=dev if a.backend == "nccl" else torch.device("cpu"))
    def all_ok(mine: bool) -> bool:
        flag = torch.tensor([1.0 if mine else 0.0], device=dev if a.backend == "nccl" else "cpu")
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        return bool(flag.item() >= 1.0)
    rr.run(barrier=dist.barrier, all_ok=all_ok)
    dist.barrier()
    if rank == 0:
        emit_line({"phase": "done", "world": world, "mode": a.backend, "gaussians": rr.seg.params.num_points,
                   "psnr": rr.evaluate(), "total_s": time.perf_counter() - t0})
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
