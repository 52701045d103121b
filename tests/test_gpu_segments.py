"""BASELINE config 4 on one GPU: the 8-leaf hierarchical run walked sequentially on cuda:0 through the SAME code the
one-process-per-GPU launcher runs (run_segments.RankRunner), with the in-process LocalTransport standing for the RCCL
point-to-point exchange.  The merge is checked against merge_two_3DGS semantics
(/root/reference/trainer/ht3dgs_trainer.py:233-271) with the float64 oracle's importance."""
import importlib

import numpy as np
import pytest
import torch

import parity
from oracle import binding

pytestmark = pytest.mark.gpu

rs = importlib.import_module("3dgs_hierarchical_training_amd.run_segments")
hier = importlib.import_module("3dgs_hierarchical_training_amd.hierarchy")
seg_mod = importlib.import_module("3dgs_hierarchical_training_amd.segments")
sequence = importlib.import_module("3dgs_hierarchical_training_amd.sequence")
ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")


def _oracle_importance(raw, views):
    """calc_importance (:1427-1462) from the float64 oracle: sum over views of |dL/dSH| with dL/dimage = 1 inside the
    clamp's pass-through range, / pixels."""
    cpu = {k: v.detach().cpu() for k, v in raw.items()}
    N = cpu["_xyz"].shape[0]
    acc, npix = np.zeros((N, 16, 3)), 0
    for rs_ in views:
        kw = dict(means3D=cpu["_xyz"], opacities=torch.sigmoid(cpu["_opacity"]), viewmatrix=rs_.viewmatrix.cpu(),
                  projmatrix=rs_.projmatrix.cpu(), campos=rs_.campos.cpu(), bg=rs_.bg.cpu(), image_height=rs_.image_height,
                  image_width=rs_.image_width, tanfovx=rs_.tanfovx, tanfovy=rs_.tanfovy, sh_degree=rs_.sh_degree, scale_modifier=1.0,
                  shs=torch.cat((cpu["_features_dc"], cpu["_features_rest"]), 1).contiguous(), scales=torch.exp(cpu["_scaling"]),
                  rotations=torch.nn.functional.normalize(cpu["_rotation"]))
        o = binding.OracleRender(**kw)
        color = o.forward()[0]
        g = ((color >= 0) & (color <= 1)).astype(np.float32)
        acc += np.abs(o.backward(g, None, None)["shs"])
        npix += rs_.image_height * rs_.image_width
        o.close()
    return acc.reshape(N, 48) / npix


def test_eight_leaf_tree_on_one_gpu():
    dev = torch.device("cuda:0")
    cfg = rs.HTConfig(frames=40, width=192, height=144, gt_gaussians=6000, leaf_gaussians=2500, leaf_iters_per_frame=12,
                      phase1_iters_per_frame=3, phase2_iters_per_frame=[6, 6, 6], prune_ratio=0.5)
    seq = sequence.FrameSequence(cfg.frames, cfg.gt_gaussians, cfg.width, cfg.height, dev, seed=4)
    tr = seg_mod.LocalTransport(8)
    captured = {}

    def importance(seg, views):                       # the product's, recorded for the first pair
        imp = hier.calc_importance(seg, views)
        captured.setdefault(len(captured), ({k: v.detach().clone() for k, v in seg.items()}, list(views), imp.clone()))
        return imp

    log = []
    runners = [rs.RankRunner(r, 8, tr, seq, cfg, dev, log=log.append, importance_fn=importance) for r in range(8)]
    for rr in runners:
        rr.train_leaf()
    psnr_leaf0 = runners[0].evaluate()
    pre = {r: {k: v.clone() for k, v in runners[r].seg.params.raw().items()} for r in (0, 1)}
    pose01 = runners[0].seg.poses[runners[1].seg.start_fidx].clone()
    for k, pairs in enumerate(runners[0].schedule):
        for dst, src in pairs:
            runners[src].merge_send(k)
        for dst, src in pairs:
            runners[dst].merge_recv(k)
            if k == 0 and dst == 0:
                merged01 = {kk: v.clone() for kk, v in runners[0].seg.params.raw().items()}
                t_own, t_child = runners[0].teachers       # both UN-pruned children are held as the frozen teachers
                assert torch.equal(t_own["seg"]["_xyz"], pre[0]["_xyz"]) and torch.equal(t_child["seg"]["_xyz"], pre[1]["_xyz"])
                assert t_child["start_fidx"] == runners[0].parts[3][1][0]
            runners[dst].train_nonleaf(k)

    # ---- structure of the walk -----------------------------------------------------------------------------------------
    root = runners[0]
    assert all(r.seg is None for r in runners[1:])
    assert root.seg.frames == list(range(cfg.frames)) and sorted(root.seg.poses) == list(range(cfg.frames))
    n = cfg.leaf_gaussians
    for _ in range(3):
        n = 2 * (n - n // 2)
    assert root.seg.params.num_points == n
    merges = [r for r in log if r["phase"] == "merge"]
    assert len(merges) == 14 and sum(1 for m in merges if m["role"] == "src") == 7
    for m in merges:
        assert m["importance_ms"] > 0 and m["bytes"] >= (m["n"] if m["role"] == "src" else m["n_child"]) * 237
    for f in (0, 17, 39):                                # chained poses equal the ground-truth camera track
        assert torch.allclose(root.seg.poses[f], seq.w2c[f] @ torch.linalg.inv(seq.w2c[0]), atol=1e-5)

    # ---- merge (0 <- 1) against merge_two_3DGS semantics with the ORACLE's importance ---------------------------------------
    # level 0 runs the four senders (ranks 1, 3, 5, 7) first, then the four receivers (0, 2, 4, 6)
    (raw1, views1, imp1), (raw0, views0, imp0) = captured[0], captured[4]
    assert torch.equal(raw0["_xyz"], pre[0]["_xyz"]) and torch.equal(raw1["_xyz"], pre[1]["_xyz"])
    keep_rows = []
    for raw, views, imp in ((raw0, views0, imp0), (raw1, views1, imp1)):
        ref = _oracle_importance(raw, views)
        assert np.abs(imp.cpu().numpy() - ref).max() <= 2e-3 * ref.max()
        score = ref.max(1)
        N = score.shape[0]
        kdrop = int(N * cfg.prune_ratio)
        order = np.argsort(score, kind="stable")
        thr = score[order[kdrop - 1]]
        drop_ref = np.zeros(N, bool); drop_ref[order[:kdrop]] = True
        drop_hip = hier.prune_mask(imp, cfg.prune_ratio).cpu().numpy()
        assert drop_hip.sum() == kdrop
        diff = drop_ref != drop_hip                        # only Gaussians whose score sits at the threshold may swap sides
        assert diff.mean() < 0.01
        assert np.all(np.abs(score[diff] - thr) <= 5e-3 * max(thr, 1e-12))
        keep_rows.append(~drop_hip)
    T = torch.linalg.inv(pose01).to(dev)
    xyz1 = pre[1]["_xyz"] @ T[:3, :3].t() + T[:3, 3]
    k0, k1 = torch.from_numpy(keep_rows[0]).to(dev), torch.from_numpy(keep_rows[1]).to(dev)
    assert torch.allclose(merged01["_xyz"], torch.cat((pre[0]["_xyz"][k0], xyz1[k1])), atol=1e-6)
    for key in ("_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        assert torch.equal(merged01[key], torch.cat((pre[0][key][k0], pre[1][key][k1])))

    # ---- the merged, fine-tuned root explains ALL frames (a leaf only saw an eighth of the track) -------------------------
    psnr_root = root.evaluate()
    print(f"PSNR leaf 0 over its {len(runners[0].parts[3][0])} frames {psnr_leaf0:.2f} dB; root over all {cfg.frames} frames {psnr_root:.2f} dB")
    assert psnr_root > 17.0


def test_stage_a_pair_fit_recovers_the_relative_pose():
    """compute_relative_pose (:336-380) on the HIP rasterizer for one frame pair: single-image 3DGS, then the SE(3) fit."""
    sa = importlib.import_module("3dgs_hierarchical_training_amd.stage_a")
    dev = torch.device("cuda:0")
    seq = sequence.FrameSequence(6, 40000, 480, 360, dev, seed=2, step_angle=0.015, step_shift=0.02)
    rel = sa.fit_pair(seq, 2, dev, n_points=40000, single_image_iters=200, pose_iters=250, pose_lr=1e-3)
    gt = seq.rel_pose(2, 3)
    err0 = (torch.eye(4) - gt)[:3].abs().max().item()
    err = (rel - gt)[:3].abs().max().item()
    print(f"relative pose error {err:.4f} (identity start {err0:.4f})")
    assert err < 0.35 * err0
    d = sa.run_stage_a(3, lambda p: gt if p == 0 else torch.eye(4), dev, rank=0, world=1)
    assert sorted(d) == ["rel_pose_0_to_1", "rel_pose_1_to_2"] and torch.allclose(d["rel_pose_0_to_1"].cpu(), gt)


def test_tree_walked_by_four_processes_sharing_the_gpu():
    """The one-process-per-rank launcher itself (run_segments.py under torch.distributed.run: stage A sharded over the ranks with its
    all_gather, then RankRunner.run with barriers and the point-to-point exchange at every merge): four processes, all on cuda:0,
    gloo with the messages staged through host memory --
    everything but the RCCL transport is what the 8-GPU run executes.  Every level must report its exchange (bytes of the
    un-pruned child + mask) and the root must end with a model that explains all frames."""
    import json
    import os
    import socket
    import subprocess
    import sys
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # round 5: the BARE command -- `run_segments.py --ranks 4` starts torch.distributed.run on itself (no launcher around it)
    cmd = [sys.executable, os.path.join(root, "3dgs_hierarchical_training_amd", "run_segments.py"), "--ranks", "4", "--backend", "gloo",
           "--one-device", "--frames", "20", "--width", "320", "--height", "240", "--gt-gaussians", "60000", "--leaf-gaussians", "30000",
           "--leaf-iters", "20", "--phase1-iters", "3", "--phase2-iters", "6", "--stage-a", "20000", "150", "100"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    # PYTORCH_NVML_BASED_CUDA_CHECK: torch.distributed.run's agent asks torch.cuda.is_available(), which would otherwise open the GPU
    # in the agent too -- with it the device is counted through amd-smi, and only this process and the four ranks hold the GPU
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", PYTORCH_NVML_BASED_CUDA_CHECK="1")
    out = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    recs = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    # stage A first: 19 frame pairs round-robin over the four ranks (5 + 5 + 5 + 4), one all_gather, every rank holds the table;
    # stage B then chains the ESTIMATED poses
    sa = sorted((r["rank"], r["pairs_here"]) for r in recs if r.get("phase") == "stage_a")
    assert sa == [(0, 5), (1, 5), (2, 5), (3, 4)]
    for r in recs:
        if r.get("phase") == "stage_a":
            assert r["max_abs_pose_error"] < 0.5 * r["identity_guess_error"], r     # (the frames move by ~1 pixel at this size)
    leaves = [r for r in recs if r.get("phase") == "leaf"]
    merges = [r for r in recs if r.get("phase") == "merge"]
    done = [r for r in recs if r.get("phase") == "done"]
    assert sorted(r["rank"] for r in leaves) == [0, 1, 2, 3]
    # level 0: (0 <- 1), (2 <- 3); level 1: (0 <- 2): three senders, three receivers, matching byte counts
    src = sorted((r["level"], r["rank"], r["peer"], r["bytes"]) for r in merges if r["role"] == "src")
    dst = sorted((r["level"], r["peer"], r["rank"], r["bytes"]) for r in merges if r["role"] == "dst")
    assert [x[:3] for x in src] == [(0, 1, 0), (0, 3, 2), (1, 2, 0)] and src == dst
    assert all(b > 30000 * 236 for *_, b in src)               # the UN-pruned child travels (236 B per Gaussian) + mask + poses
    assert len(done) == 1 and done[0]["world"] == 4 and done[0]["mode"] == "gloo"
    assert done[0]["psnr"] > 20.0, done[0]      # stage B chains stage A's ESTIMATED poses here (46.9 dB with the true ones)
    print(f"4 processes on one GPU: root PSNR {done[0]['psnr']:.2f} dB, {done[0]['gaussians']} Gaussians, {done[0]['total_s']:.1f} s")


def test_bench_line_at_two_ranks_on_one_gpu():
    """bench.py's N > 1 path (one process per rank under torch.distributed.run, barrier + max-over-ranks timing, one merge level with
    the point-to-point exchange, rank 0 prints ONE line) run with two processes that share cuda:0 over gloo.  Only the shape of the
    result is checked -- two processes on one GPU measure nothing."""
    import json
    import os
    import socket
    import subprocess
    import sys
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # round 5: the BARE command -- bench.py starts torch.distributed.run itself when --gpus > 1 and no launcher is around it
    # (tests/test_launch_cpu.py covers the launcher's refusals; the explicit torch.distributed.run form is what the 4-process walk uses)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2", "--gaussians", "200000", "--full"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", GSR_BENCH_BACKEND="gloo", GSR_BENCH_ONE_DEVICE="1", PYTORCH_NVML_BASED_CUDA_CHECK="1")  # (see above)
    out = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines                       # rank 0 alone prints
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["warmup"] == 2 and d["scaling"] == "weak" and d["higher_is_better"] is True
    assert abs(d["value"] - 2 * 1000.0 / d["ms_per_step"]) < 1e-6 * d["value"]          # whole-job aggregate over both ranks
    assert "roofline" in d and d["roofline"]["frac"] > 0 and "cpu_baseline" not in d      # cpu_baseline: rank 0 at N = 1 only
    m = d["merge"]
    assert m["pairs"] == 1 and m["merge_bytes"] > 200000 * 236 and m["merge_ms"] > 0 and m["gaussians_merged_max"] == 200000
    # the process group's self-diagnosis: both ranks answered, the 64 MiB exchange of the one level-0 pair came back intact
    r = d["rccl"]
    assert r["world"] == 2 and r["ranks_seen"] == [0, 1] and r["all_ranks_present"] and r["backend"] == "gloo" and r["payload_ok"]
    assert list(r["link_GBps"]) == ["0<->1"] and r["link_GBps"]["0<->1"] > 0
    assert d["spec_overflows"] >= 0 and d["config"]["views"] == 8


def test_pose_refinement_in_stage_b_improves_on_noisy_relative_poses():
    """--fit-pose: every frame's pose is refined while its segment trains on it (the reference's camera_optimizer, one
    gsr_pose_step_camera kernel per train step).  With a relative-pose table that is off (what an imperfect stage A leaves), the
    refined run explains the frames better than the run that keeps the table fixed, and its poses end closer to the truth."""
    dev = torch.device("cuda:0")
    pose_mod = importlib.import_module("3dgs_hierarchical_training_amd.pose")
    res = {}
    for fit in (False, True):
        cfg = rs.HTConfig(frames=12, width=480, height=360, gt_gaussians=60000, leaf_gaussians=60000, leaf_iters_per_frame=60,
                          phase1_iters_per_frame=2, phase2_iters_per_frame=[20, 20, 20], fit_pose=fit, pose_lr=2e-5)
        seq = sequence.FrameSequence(cfg.frames, cfg.gt_gaussians, cfg.width, cfg.height, dev, seed=cfg.seed)
        g = torch.Generator().manual_seed(11)
        table = {}
        for p in range(cfg.frames - 1):
            noise = pose_mod.se3_exp(torch.cat((0.003 * torch.randn(3, generator=g), 0.0008 * torch.randn(3, generator=g))))
            table[f"rel_pose_{p}_to_{p + 1}"] = noise @ seq.true_rel_pose(p, p + 1)
        seq.use_pose_table(table)
        root, _ = rs.run_local(2, seq, cfg, dev, log=lambda r: None)
        err = max(float((root.seg.poses[f] - seq.w2c[f] @ torch.linalg.inv(seq.w2c[0]))[:3].abs().max()) for f in root.seg.frames)
        res[fit] = (root.evaluate(), err)
    print(f"fixed noisy poses: PSNR {res[False][0]:.2f} dB, worst pose entry off by {res[False][1]:.4f}; refined: {res[True][0]:.2f} dB, {res[True][1]:.4f}")
    assert res[True][0] > res[False][0] + 0.3 and res[True][1] < res[False][1]


def _free_port():
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    return port


def test_rccl_process_group_at_world_one_through_bench():
    """the RCCL backend initialised for real (backend "nccl" IS RCCL on ROCm) on the one GPU a box has --
    `GSR_BENCH_FORCE_DIST=1 python bench.py`: the process group comes up on the device, the collectives this code uses anywhere
    (all_gather, all_reduce SUM / MIN, broadcast, barrier) run on device tensors and return the right values, the timed region's
    barriers are RCCL barriers, and the line says so.  Point-to-point needs a second rank: unmeasured."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0", GSR_BENCH_FORCE_DIST="1")
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1", "--gaussians", "100000",
                          "--full", "--no-extras"], cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    r = d["rccl"]
    assert r["backend"] == "nccl" and r["world"] == 1 and r["ranks_seen"] == [0] and r["all_ranks_present"], r
    assert r["collectives_ok"] is True and "all_gather" in r["collectives"] and "barrier" in r["collectives"], r
    assert r["p2p_self_pair"]["ok"] is True and r["p2p_self_pair"]["bytes"] == 64 << 20, r          # RCCL's send / recv kernels on device tensors
    assert d["n_gpus"] == 1 and d["value"] > 0


def test_merge_level_travels_through_rccl_point_to_point_on_one_gpu():
    """The one merge level of bench.py at world 1 with the process group up: the un-pruned child + mask go through
    segments.DistTransport as a self pair -- RCCL's point-to-point kernels on device tensors, the path `dist.send / recv` take on a
    real node, executed for the first time in round 5."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0", GSR_BENCH_FORCE_DIST="1", GSR_BENCH_MERGE="1")
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1", "--gaussians", "100000",
                          "--full", "--no-extras", "--no-cpu-baseline"], cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    m = d["merge"]
    assert "RCCL" in m["transport"] and m["merge_bytes"] > 100000 * 236 and m["gaussians_merged"] == 100000 and m["merge_ms"] > 0, m


def test_plain_bench_run_is_the_headline_of_a_full_run(tmp_path):
    """A plain `bench.py` run stops at the headline: the line has the contract's keys and none of what `--full` measures after the
    timed steps.  Both runs train the same model over the same steps, so --dump-outputs writes the same arrays bit for bit."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    lines = {}
    for mode in ("plain", "full"):
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "2", "--gaussians", "100000",
               "--dump-outputs", str(tmp_path / mode)] + (["--full", "--no-extras", "--no-cpu-baseline"] if mode == "full" else [])
        out = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        js = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(js) == 1, js
        lines[mode] = json.loads(js[0])
    p, f = lines["plain"], lines["full"]
    for k in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup"):
        assert p[k] == f[k], k
    assert p["value"] > 0 and abs(p["value"] - 1000.0 / p["ms_per_step"]) < 1e-6 * p["value"]
    for k in ("stage_ms", "fwd_bwd_ms", "roofline", "rccl", "merge", "cpu_baseline", "dropin", "other_workloads", "host_us"):
        assert k not in p, k
    assert "stage_ms" in f and "roofline" in f and "rccl" in f
    assert p["dump_outputs"]["arrays"] == f["dump_outputs"]["arrays"]
    for name in p["dump_outputs"]["arrays"]:
        a, b = np.load(tmp_path / "plain" / (name + ".npy")), np.load(tmp_path / "full" / (name + ".npy"))
        assert a.dtype == b.dtype and np.array_equal(a, b), name


def test_child_message_over_rccl_as_a_self_pair():
    """segments.send_child / recv_child on DEVICE tensors over backend nccl, one rank addressing itself (tests/helpers/
    rccl_selfpair_child.py): header, 200 k un-pruned rows (47 MB), mask, frames, poses arrive intact."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "helpers", "rccl_selfpair_child.py")], cwd=root, env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert d["ok"] is True and d["backend"] == "nccl" and d["over_wire"] is True and d["bytes"] == d["recv_bytes"] > 200000 * 237, d


def test_bare_bench_command_refuses_more_gpus_than_the_box_has():
    import json
    import os
    import subprocess
    import sys
    if torch.cuda.device_count() >= 2:
        pytest.skip("two devices present")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "GSR_BENCH_ONE_DEVICE")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 3 and len(lines) == 1 and lines[0]["value"] is None and lines[0]["n_gpus"] == 2 and "1 GPU(s) visible" in lines[0]["error"]


def test_run_segments_at_world_one_over_rccl():
    """`run_segments.py --backend nccl` as ONE rank: init_process_group("nccl", device_id=...), stage A's all_gather of the pose
    rows on DEVICE tensors, the link self-test's MIN all-reduce, RankRunner.run's barriers -- every RCCL call of the launcher
    except the point-to-point exchange (which needs a peer) executes."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(root, "3dgs_hierarchical_training_amd", "run_segments.py"), "--backend", "nccl",
           "--frames", "6", "--width", "320", "--height", "240", "--gt-gaussians", "40000", "--leaf-gaussians", "20000",
           "--leaf-iters", "10", "--phase1-iters", "2", "--phase2-iters", "4", "--stage-a", "10000", "60", "40"]
    out = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    recs = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    sa = [r for r in recs if r.get("phase") == "stage_a"]
    assert len(sa) == 1 and sa[0]["pairs_here"] == 5 and sa[0]["max_abs_pose_error"] < sa[0]["identity_guess_error"]
    done = [r for r in recs if r.get("phase") == "done"]
    assert len(done) == 1 and done[0]["world"] == 1 and done[0]["mode"] == "nccl" and done[0]["psnr"] > 15.0, done
    assert not [r for r in recs if r.get("phase") == "error"]
