"""GPU: the device-side single-image initialisation (include/gsr.h version 118; csrc/voxel_kernels.hip, pointcloud.py) -- the voxel grid
against the numpy float64 oracle of tests/voxel_common.py from identical float32 inputs, the un-projection against the float32 formula
evaluated with torch on the CPU, the ctypes route against the op, scene_from_depth against its three steps, and stage A's init="voxels".

Tolerances.  Voxel assignment is float64 IEEE arithmetic on both sides: M, the counts and the order agree exactly.  The means are float64
sums rounded once to float32; the oracle adds sequentially, the kernels add long segments as a tree, so the float64 sums can differ in
their last bits, which moves the single float32 rounding by at most one ulp (np.spacing of the oracle's value).  Un-projection: z is a
copy; x and y are a float32 subtraction, division and product, each correctly rounded on both sides -- one ulp is allowed, bit-identical
is expected and was observed on an MI355X for all three sizes."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import voxel_common as VC

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _pc():
    return importlib.import_module("3dgs_hierarchical_training_amd.pointcloud")


def _run(points, colors, voxel_size):
    dev = _dev()
    p = torch.from_numpy(np.ascontiguousarray(points)).to(dev)
    c = None if colors is None else torch.from_numpy(np.ascontiguousarray(colors)).to(dev)
    op, oc, counts, dropped = _pc().voxel_down_sample(p, c, voxel_size, return_counts=True)
    return op, oc, counts, dropped


@pytest.mark.parametrize("name", list(VC.CASES))
def test_voxel_grid_matches_the_oracle(name):
    points, colors, voxel_size = VC.CASES[name]
    ref = VC.oracle_of(name)
    assert ref["status"] == 0
    op, oc, counts, dropped = _run(points, colors, voxel_size)
    M = ref["points"].shape[0]
    print(f"[voxel {name}] N={points.shape[0]} M={M} longest segment={int(ref['counts'].max()) if M else 0} dropped={ref['dropped']}")
    assert tuple(op.shape) == (M, 3) and tuple(counts.shape) == (M,) and counts.dtype == torch.int32 and op.dtype == torch.float32
    assert dropped == ref["dropped"]
    got_counts = counts.cpu().numpy().astype(np.int64)
    assert np.array_equal(got_counts, ref["counts"]), "the same counts row for row (and so the same order)"
    assert int(got_counts.sum()) + dropped == points.shape[0]
    off = VC.assert_within_one_ulp(op.cpu().numpy(), ref["points"], f"{name}: points")
    if colors is None:
        assert oc is None
    else:
        assert tuple(oc.shape) == (M, 3)
        off += VC.assert_within_one_ulp(oc.cpu().numpy(), ref["colors"], f"{name}: colours")
    print(f"[voxel {name}] elements that differ from the oracle by their last bit: {off}")
    # a repeat of the call is bit-identical
    op2, oc2, counts2, dropped2 = _run(points, colors, voxel_size)
    assert torch.equal(op, op2) and torch.equal(counts, counts2) and dropped2 == dropped
    assert colors is None or torch.equal(oc, oc2)


def test_an_index_past_2_21_raises():
    points, colors, voxel_size = VC.OVERFLOW_CASE
    assert VC.voxel_oracle(points, colors, voxel_size)["status"] == 1
    with pytest.raises(RuntimeError, match="2\\^21"):
        _run(points, colors, voxel_size)
    # the library is in order afterwards
    op, _, counts, _ = _run(*VC.CASES["n65"])
    assert np.array_equal(counts.cpu().numpy(), VC.oracle_of("n65")["counts"])


def test_empty_cloud_and_an_input_that_requires_grad():
    dev = _dev()
    op, oc, counts, dropped = _pc().voxel_down_sample(torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev), 0.01, return_counts=True)
    assert tuple(op.shape) == (0, 3) and tuple(oc.shape) == (0, 3) and tuple(counts.shape) == (0,) and dropped == 0
    points, colors, voxel_size = VC.CASES["n4097"]
    p = torch.from_numpy(points).to(dev).requires_grad_(True)
    c = torch.from_numpy(colors).to(dev).requires_grad_(True)
    op, oc = _pc().voxel_down_sample(p, c, voxel_size)
    assert not op.requires_grad and not oc.requires_grad and p.grad is None
    ref, _, _, _ = _run(points, colors, voxel_size)
    assert torch.equal(op, ref)
    # the op itself takes such inputs too (it has no backward: nothing flows to them)
    E = importlib.import_module("3dgs_hierarchical_training_amd._ext")
    raw = E.load().voxel_down_sample(p, c, voxel_size)
    assert torch.equal(raw[0].detach(), ref) and raw[3] == 0 and p.grad is None


def _depth_case(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    depth = 0.3 + 9.0 * torch.rand(H, W, generator=g)
    image = torch.rand(3, H, W, generator=g)
    K = (0.61 * W + 0.37, 0.83 * H + 0.11, 0.5 * W + 1.7, 0.5 * H - 2.3)      # fx != fy, principal point off the centre
    return depth, image, K


@pytest.mark.parametrize("H,W", [(17, 23), (48, 64), (96, 128)])
def test_unprojection_matches_the_float32_formula(H, W):
    depth, image, K = _depth_case(H, W, H * W)
    ref_p, ref_c = VC.depth_to_points_oracle(depth, image, *K)
    dev = _dev()
    pts, cols = _pc().depth_to_points(depth.to(dev), image.to(dev), K)
    pts, cols = pts.cpu(), cols.cpu()
    assert tuple(pts.shape) == (H * W, 3) and tuple(cols.shape) == (H * W, 3)
    assert torch.equal(pts[:, 2], ref_p[:, 2]), "z is the depth, bit for bit"
    off = VC.assert_within_one_ulp(pts[:, :2].numpy(), ref_p[:, :2].numpy(), "x, y")
    print(f"[unprojection {H}x{W}] x / y elements that are not bit-identical with the float32 formula: {off}")
    assert torch.equal(cols, ref_c), "colours are gathers"
    # a 3x3 matrix gives the same call; without an image there are no colours
    Km = torch.tensor([[K[0], 0.0, K[2]], [0.0, K[1], K[3]], [0.0, 0.0, 1.0]], dtype=torch.float64)
    p2, c2 = _pc().depth_to_points(depth.to(dev), None, Km)
    assert c2 is None and torch.equal(p2.cpu(), pts)


def test_ctypes_route_equals_the_op():
    L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
    lib, dev = L.load(), _dev()
    H, W = 48, 64
    depth, image, K = _depth_case(H, W, 7)
    depth[5, 6] = float("nan")
    d, im = depth.to(dev), image.to(dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    n = H * W
    pts, cols = torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev)
    L.check(lib.gsr_depth_to_points(d.data_ptr(), im.data_ptr(), H, W, K[0], K[1], K[2], K[3], pts.data_ptr(), cols.data_ptr(), stream),
            "gsr_depth_to_points")
    op_pts, op_cols = _pc().depth_to_points(d, im, K)
    assert torch.equal(pts[torch.isfinite(pts).all(1)], op_pts[torch.isfinite(op_pts).all(1)]) and torch.equal(cols, op_cols)
    out_p, out_c = torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev)
    out_n, meta = torch.empty(n, dtype=torch.int32, device=dev), torch.full((4,), -7, dtype=torch.int64, device=dev)
    sb = lib.gsr_voxel_scratch_bytes(n)
    scratch = torch.empty(sb, dtype=torch.uint8, device=dev)
    L.check(lib.gsr_voxel_down_sample(pts.data_ptr(), cols.data_ptr(), n, 0.05, out_p.data_ptr(), out_c.data_ptr(), out_n.data_ptr(),
                                      meta.data_ptr(), scratch.data_ptr(), sb, stream), "gsr_voxel_down_sample")
    M, dropped, status, zero = meta.cpu().tolist()
    op_p, op_c, op_n, op_dropped = _pc().voxel_down_sample(op_pts, op_cols, 0.05, return_counts=True)
    assert (M, dropped, status, zero) == (op_p.shape[0], op_dropped, 0, 0) and dropped == 1
    assert torch.equal(out_p[:M], op_p) and torch.equal(out_c[:M], op_c) and torch.equal(out_n[:M], op_n)
    # N == 0: meta is written, nothing else is needed
    meta.fill_(-7)
    L.check(lib.gsr_voxel_down_sample(None, None, 0, 0.05, None, None, None, meta.data_ptr(), None, 0, stream), "gsr_voxel_down_sample")
    assert meta.cpu().tolist() == [0, 0, 0, 0]


@pytest.fixture(scope="module")
def seq():
    sequence = importlib.import_module("3dgs_hierarchical_training_amd.sequence")
    return sequence.FrameSequence(2, 20_000, 128, 96, _dev(), seed=2)


def test_scene_from_depth_is_its_three_steps(seq):
    pc = _pc()
    ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
    from simple_knn._C import distCUDA2
    dev = _dev()
    depth, image, K = seq.depth(0).clamp_min(0.21), seq.target(0), seq.intrinsics()
    assert depth.is_cuda and image.is_cuda and tuple(depth.shape) == (96, 128)
    scene = pc.scene_from_depth(depth, image, K, voxel_size=0.01)
    pts, cols = pc.voxel_down_sample(*pc.depth_to_points(depth, image, K), 0.01)
    steps = pc.scene_from_points(pts, cols)
    for k in ("means3D", "shs", "scales", "rotations", "opacities"):
        assert torch.equal(scene[k], steps[k]), k
    n = pts.shape[0]
    assert 0 < n <= 96 * 128 and torch.equal(scene["means3D"], pts)
    assert torch.equal(scene["scales"], torch.sqrt(distCUDA2(pts).clamp_min(1e-7))[:, None].repeat(1, 3))
    assert tuple(scene["shs"].shape) == (n, 16, 3) and torch.equal(scene["shs"][:, 0], (cols - 0.5) / 0.28209479177387814)
    assert not scene["shs"][:, 1:].any()
    assert torch.equal(scene["rotations"], torch.tensor([1.0, 0, 0, 0], device=dev).expand(n, 4))
    assert torch.equal(scene["opacities"], torch.full((n, 1), 0.1, device=dev))
    params = ts.GaussianParams(scene, dev)
    params.active_sh_degree = 0
    ident = ts.with_sh_degree(seq.settings_for_pose(torch.eye(4)), 0)
    pkg = ts.train_step(params, ident, image)
    assert torch.isfinite(pkg["loss"]).all()
    assert all(bool(torch.isfinite(v).all()) for v in params.raw().values())
    # FrameSequence.depth_scene: the same chain, uncovered pixels dropped as NaN
    ds = seq.depth_scene(0)
    assert ds["means3D"].is_cuda and ds["means3D"].shape[0] <= n and bool((ds["means3D"][:, 2] > 0.21).all())


def test_stage_a_from_voxels(seq):
    stage_a = importlib.import_module("3dgs_hierarchical_training_amd.stage_a")
    dev = _dev()
    fit = dict(single_image_iters=200, pose_iters=100)
    info = {}
    pose = stage_a.fit_pair(seq, 0, dev, init="voxels", info=info, **fit)
    assert tuple(pose.shape) == (4, 4) and bool(torch.isfinite(pose).all())
    R = pose[:3, :3].double()
    assert float((R @ R.t() - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-4
    assert info["loss_last"] < info["loss_first"], info
    # the batched entry with one pair, under early_exit='device': the single fit's pose bit for bit
    single = stage_a.fit_pair(seq, 0, dev, init="voxels", early_exit="device", **fit)
    batched = stage_a.fit_pairs_batched(seq, [0], dev, init="voxels", early_exit="device", **fit)
    assert torch.equal(batched[0], single)
    # reported, not asserted: how well either initialisation recovers the true relative pose at these counts
    gt = seq.true_rel_pose(0, 1)
    pix = stage_a.fit_pair(seq, 0, dev, init="pixels", **fit)
    err = lambda m: float((m - gt)[:3].abs().max())
    print(f"[stage A 128x96, 200 + 100 iterations] max |pose - truth|: voxels {err(pose):.3e}, pixels {err(pix):.3e}, identity {err(torch.eye(4)):.3e}; "
          f"image-phase loss {info['loss_first']:.4f} -> {info['loss_last']:.4f}")
