"""CPU: the depth term on stacks of planes -- the torch restatement (train_step.depth_loss: the sum of the per-image losses, every image
with its own fit), the library's new exports (gsr_depth_loss_*_batched, version 114) and the shape / device errors of the fused entry."""
import importlib

import numpy as np
import pytest
import torch

import depth_loss_common as D

ts = importlib.import_module("3dgs_hierarchical_training_amd.train_step")
loss_mod = importlib.import_module("3dgs_hierarchical_training_amd.loss")
L = importlib.import_module("3dgs_hierarchical_training_amd._lib")
NEW = ["gsr_depth_loss_workspace_bytes_batched", "gsr_depth_loss_forward_batched", "gsr_depth_loss_backward_batched",
       "gsr_depth_loss_forward_terms_batched"]


def _stack(H=23, W=31, B=3):
    ps, gs = zip(*(D.scene(H, W, seed=21 + b) for b in range(B)))
    p, g = np.stack(ps), np.stack(gs)
    g[1] = 0.0           # an image without a valid pixel
    return torch.from_numpy(p).double(), torch.from_numpy(g).double()


@pytest.mark.parametrize("kind", ["l1", "invariant"])
@pytest.mark.parametrize("four_d", [False, True])
def test_restatement_on_a_stack_is_the_sum_of_the_per_plane_calls(kind, four_d):
    p, g = _stack()
    ps = (p[:, None] if four_d else p).clone().requires_grad_(True)
    v = ts.depth_loss(ps, g if four_d else g[:, None], kind)
    v.backward()
    total, grads = 0.0, []
    for b in range(p.shape[0]):
        pb = p[b].clone().requires_grad_(True)
        vb = ts.depth_loss(pb, g[b], kind)
        vb.backward()
        total = total + vb.detach()
        grads.append(pb.grad)
    assert v.dim() == 0 and ps.grad.shape == ps.shape
    assert abs(float(v.detach()) - float(total)) <= 1e-14 * max(1.0, abs(float(total)))
    assert torch.equal(ps.grad.reshape(p.shape), torch.stack(grads))
    if kind == "invariant":
        assert not ps.grad.reshape(p.shape)[1].any() and float(ts.depth_loss(p[1], g[1], kind)) == 0.0
    _, s, t, M = ts.depth_loss(p, g, kind, return_fit=True)
    assert len(s) == len(t) == len(M) == 3
    with pytest.raises(RuntimeError):
        ts.depth_loss(p, g[:2], kind)


def test_library_exports_the_batched_depth_entries():
    lib = L.load()
    assert lib.gsr_version() >= 114
    for name in NEW:
        assert name in L.EXPORTS and hasattr(lib, name), name
    one = lib.gsr_depth_loss_workspace_bytes(97, 131)
    assert lib.gsr_depth_loss_workspace_bytes_batched(1, 97, 131) == one
    five = lib.gsr_depth_loss_workspace_bytes_batched(5, 97, 131)
    assert five % 8 == 0 and 4 * one < five <= 5 * one
    # argument checks come before any launch: no device is needed to see them
    ws = (np.zeros(16, dtype=np.float64)).ctypes.data
    for images, kind, wsp in ((0, 1, ws), (-1, 1, ws), (2, 7, ws), (2, 1, ws + 4), (2, 1, None)):
        assert lib.gsr_depth_loss_forward_batched(ws, ws, images, 4, 4, kind, 0.02, 20.0, 1.0, wsp, ws, ws, None) != 0
        assert lib.gsr_depth_loss_forward_terms_batched(ws, ws, images, 4, 4, kind, 0.02, 20.0, 1.0, wsp, ws, ws, None, None) != 0
        assert lib.gsr_depth_loss_backward_batched(ws, ws, images, 4, 4, kind, 0.02, 20.0, 1.0, wsp, None, ws, None) != 0
    assert lib.gsr_depth_loss_forward_batched(None, ws, 2, 4, 4, 1, 0.02, 20.0, 1.0, ws, ws, ws, None) != 0
    assert lib.gsr_depth_loss_forward_batched(ws, ws, 2, 4, 4, 1, 0.02, 20.0, 1.0, ws, ws, None, None) != 0
    assert lib.gsr_depth_loss_forward_terms_batched(ws, ws, 2, 4, 4, 1, 0.02, 20.0, 1.0, ws, ws, None, None, None) != 0


def test_fused_depth_loss_on_stacks_has_no_cpu_path_and_checks_shapes():
    p, g = _stack()
    p, g = p.float(), g.float()
    for dp, dg in ((p, g), (p[:, None], g), (p, g[:, None])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            loss_mod.fused_depth_loss(dp, dg, "invariant")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss_mod.fused_training_loss_report(torch.zeros(3, 3, 23, 31), torch.zeros(3, 3, 23, 31), p[:, None], g, lambda_depth=0.1)
    for dp, dg in ((p, g[:2]), (p[:, None], g[:2]), (p, g[:, :, :30]), (p[:, None].expand(3, 2, 23, 31), g)):
        with pytest.raises(RuntimeError, match="of one B and one plane size"):
            loss_mod.fused_depth_loss(dp, dg, "invariant")
