"""The retire rule of a launch chain (include/gsr.h gsr_batch_retire, gsr_forward_retire) restated in float64 numpy: what the device
kernels are held against.  Shared by tests/test_batch_retire_cpu.py and tests/test_gpu_batch_retire.py."""
import numpy as np


def image_mse(render: np.ndarray, target: np.ndarray) -> np.ndarray:
    """Per-image MSE of clamp(render, 0, 1) against target: render / target are float32 [B, C, H, W]; the clamp is taken in float32 (it
    selects one of three float32 values), every difference and square in float64, the mean over the image in float64.  Returns B doubles."""
    assert render.dtype == np.float32 and target.dtype == np.float32 and render.shape == target.shape and render.ndim == 4
    d = np.clip(render, np.float32(0), np.float32(1)).astype(np.float64) - target.astype(np.float64)
    return (d * d).reshape(render.shape[0], -1).sum(axis=1) / float(render[0].size)


def retire_rule(retired_at, mse, step: int, mse_bar: float, exit_after: int) -> np.ndarray:
    """The table after the decision of step `step`: entry b becomes `step` when it is 0, step > exit_after and mse[b] < mse_bar (strict);
    a set entry is never changed."""
    out = np.array(retired_at, dtype=np.int32).copy()
    for b in range(out.shape[0]):
        if out[b] == 0 and step > exit_after and float(mse[b]) < float(mse_bar):
            out[b] = step
    return out


def render_is_culled(entry: int, step: int) -> bool:
    """The render of step `step` culls a model exactly when it was retired BEFORE that step."""
    return entry != 0 and entry < step


def adam_runs(entry: int, step: int) -> bool:
    """The Adam update of step `step` runs for a model that is active or was retired AT that step (the reference steps its optimizer
    before it breaks)."""
    return entry == 0 or entry >= step


def mse_bar(psnr_exit: float) -> float:
    return 10.0 ** (-float(psnr_exit) / 10.0)
