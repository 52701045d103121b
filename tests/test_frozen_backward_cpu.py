"""CPU: the host side of the frozen backward (include/gsr.h, GsrBackwardArgs "frozen call") -- the library version, the route
inference of rasterizer.frozen_backward_route over its truth table, the refusals of frozen=True that must come before anything
touches a device, and the schema of torch.ops.gsr.rasterize_backward_frozen."""
import importlib
import itertools

import pytest
import torch

R = importlib.import_module("3dgs_hierarchical_training_amd.rasterizer")
E = importlib.import_module("3dgs_hierarchical_training_amd._ext")
L = importlib.import_module("3dgs_hierarchical_training_amd._lib")


def test_library_version_and_counter():
    lib = L.load()
    assert lib.gsr_version() >= 115
    assert lib.gsr_get_counter(b"frozen_backward_calls") >= 0          # (an unknown name gives -1)


def test_route_inference_truth_table(monkeypatch):
    """None: frozen exactly when no parameter wants a gradient, there is no fused Adam (nor densify_stats) and the camera or the
    transform wants one; means2D never changes the route.  False: never.  True: always, or a RuntimeError where it cannot be served."""
    assert R.FROZEN_BY_INFERENCE in (True, False)
    for by_inference in (True, False):
        monkeypatch.setattr(R, "FROZEN_BY_INFERENCE", by_inference)
        for param, m2d, cam, xf, adam, dens in itertools.product((False, True), repeat=6):
            want = by_inference and (cam or xf) and not (param or adam or dens)
            assert R.frozen_backward_route(param, m2d, cam, xf, adam, dens) is want, (param, m2d, cam, xf, adam, dens)
            assert R.frozen_backward_route(param, m2d, cam, xf, adam, dens, frozen=None) is want
            assert R.frozen_backward_route(param, m2d, cam, xf, adam, dens, frozen=False) is False
            if adam or dens or not (cam or xf):
                with pytest.raises(RuntimeError, match="frozen=True"):
                    R.frozen_backward_route(param, m2d, cam, xf, adam, dens, frozen=True)
            else:
                assert R.frozen_backward_route(param, m2d, cam, xf, adam, dens, frozen=True) is True
        assert R._frozen_code(None) == (-1 if by_inference else 0) and R._frozen_code(True) == 1 and R._frozen_code(False) == 0


@pytest.mark.parametrize("binding_route", ["extension", "ctypes"])
@pytest.mark.parametrize("extra", ["fused_adam", "prepare_next", "densify_stats"])
def test_frozen_true_is_refused_before_anything_touches_a_device(extra, binding_route, monkeypatch):
    """CPU tensors: the "no CPU fallback" error of the device check would come next -- the frozen refusal comes first."""
    if binding_route == "ctypes":
        monkeypatch.setenv("GSR_BINDING", "ctypes")
    n = 4
    z = lambda *s: torch.zeros(*s)
    rs = R.GaussianRasterizationSettings(image_height=16, image_width=16, tanfovx=0.5, tanfovy=0.5, bg=z(3), scale_modifier=1.0,
                                         viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0, campos=z(3), prefiltered=False,
                                         debug=False)
    kw = {extra: object() if extra != "densify_stats" else (z(n), z(n), z(n))}
    with pytest.raises(RuntimeError, match="frozen=True is not served together with fused_adam, prepare_next or densify_stats"):
        R.rasterize_gaussians_raw(z(n, 3), z(n, 3), z(n, 1, 3), z(n, 15, 3), z(n, 1), z(n, 3), z(n, 4), rs, frozen=True, **kw)
    # without frozen=True the same call reaches the device check
    with pytest.raises(RuntimeError, match="ROCm/HIP device"):
        R.rasterize_gaussians_raw(z(n, 3), z(n, 3), z(n, 1, 3), z(n, 15, 3), z(n, 1), z(n, 3), z(n, 4), rs, frozen=True)


def test_the_frozen_op_and_its_schema():
    ops = E.load()
    s = str(ops.rasterize_backward_frozen.default._schema)
    tensors = ("means3D", "sh", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp", "sh_rest", "viewmatrix", "projmatrix",
               "campos", "bg", "points_transform", "geom", "image", "binning", "meta", "grad_color", "grad_depth", "grad_alpha")
    want = ("gsr::rasterize_backward_frozen(" + ", ".join("Tensor " + t for t in tensors) +
            ", int image_height, int image_width, float tanfovx, float tanfovy, float scale_modifier, int sh_degree, bool raw_params, "
            "bool need_means2D, bool need_viewmatrix, bool need_projmatrix, bool need_campos, bool need_points_transform, "
            "int[] batch_first_block, Tensor? sh_origin=None) -> Tensor[]")
    assert s == want, s
    # the full backward's schema is as it was (densify_stats, radii and no need_means2D), and rasterize gained a trailing default
    full = str(ops.rasterize_backward.default._schema)
    assert "need_means2D" not in full and "Tensor(a!)[] densify_stats, Tensor radii, int[] batch_first_block, Tensor? sh_origin=None) -> Tensor[]" in full
    assert str(ops.rasterize.default._schema).count("Tensor? sh_origin=None, int frozen=-1) -> ") == 1


def test_the_public_functions_take_the_keyword():
    import inspect
    # (the module takes it in its constructor: forward() keeps exactly the reference's keyword set, tests/test_oracle_golden.py)
    for fn in (R.rasterize_gaussians_raw, R.rasterize_gaussians, R.GaussianRasterizer.__init__):
        p = inspect.signature(fn).parameters["frozen"]
        assert p.default is None
    assert "frozen" not in inspect.signature(R.GaussianRasterizer.forward).parameters
    assert R.GaussianRasterizer(None).frozen is None and R.GaussianRasterizer(None, frozen=False).frozen is False
