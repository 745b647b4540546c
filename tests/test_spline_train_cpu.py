"""The yardstick of the spline training tests (tests/spline_chain.py) checked without a GPU: its forward against the
per-edge numpy oracle, its gradients against finite differences, and the library's new backward entry points."""
import numpy as np
import pytest
import torch

import spline_chain as sc
from oracle import spatial_oracle


@pytest.mark.parametrize("cfg", sc.CONFIGS, ids=lambda c: f"deg{c[0]}_D{c[1]}")
@pytest.mark.parametrize("norm", [True, False])
def test_restatement_forward_matches_the_oracle(cfg, norm):
    degree, D, ks, op = cfg
    inputs, _, ei = sc.make_inputs(3, 40, 300, cfg, 5, 7, root=True, dtype=torch.float64)
    basis, wi = sc.spline_basis(inputs["pseudo"], ks, op, degree)
    ob, owi = spatial_oracle.spline_basis(inputs["pseudo"].numpy(), ks, op, degree)
    assert np.array_equal(wi.numpy(), owi)
    assert np.abs(basis.numpy() - ob).max() <= 1e-12
    xe = inputs["x"][ei[1]]
    ow = spatial_oracle.spline_weighting(xe.numpy(), inputs["weight"].numpy(), ob, owi)
    assert np.abs(sc.spline_weighting(xe, inputs["weight"], basis, wi).numpy() - ow).max() <= 1e-12
    out = sc.spline_conv(inputs["x"], ei, inputs["pseudo"], inputs["weight"], ks, op, degree, norm, inputs["root_weight"], inputs["bias"])
    want = spatial_oracle.spline_conv(inputs["x"].numpy(), ei.numpy(), inputs["pseudo"].numpy(), inputs["weight"].numpy(), ks, op,
                                      degree, norm, inputs["root_weight"].numpy(), inputs["bias"].numpy())
    assert np.abs(out.numpy() - want).max() <= 1e-12


@pytest.mark.parametrize("cfg", sc.CONFIGS, ids=lambda c: f"deg{c[0]}_D{c[1]}")
def test_restatement_gradcheck(cfg):
    degree, D, ks, op = cfg
    inputs, _, ei = sc.make_inputs(4, 6, 14, cfg, 2, 3, root=True, dtype=torch.float64)   # pseudo keeps 1e-2 from every knot
    leaves = [inputs[k].clone().requires_grad_(True) for k in ("x", "pseudo", "weight", "root_weight", "bias")]

    def fn(x, pseudo, weight, root, bias):
        return sc.spline_conv(x, ei, pseudo, weight, ks, op, degree, True, root, bias)

    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-7, rtol=1e-5)


def test_library_exports_the_backward_entry_points():
    import gnnops
    from gnnops import _lib

    lib = gnnops.load_library()
    for name in ("gnnops_spline_basis_bw", "gnnops_spline_weighting_bw_basis", "gnnops_spline_weighting_bw_weight",
                 "gnnops_spline_weighting_bw_weight_workspace_bytes"):
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    # host-only query: two fp32 partial tables per chunk of at most 8192 (edge, combination) pairs, nothing for an empty call
    assert lib.gnnops_spline_weighting_bw_weight_workspace_bytes(0, 8, 64, 64) == 0
    ws = lib.gnnops_spline_weighting_bw_weight_workspace_bytes(5_000_000, 8, 64, 64)
    chunks = -(-5_000_000 * 8 // 8192)
    assert ws == chunks * 2 * 64 * 64 * 4


def test_spline_layer_and_shim_surface():
    import inspect

    import torch_spline_conv
    from gnnops import autograd, conv

    assert {"spline_basis", "spline_weighting", "spline_conv"} <= set(torch_spline_conv.__all__)
    for name in ("_SplineBasis", "_SplineWeighting", "_SplineConv"):
        assert issubclass(getattr(autograd, name), torch.autograd.Function)
    layer = conv.SplineConv(3, 4, dim=2, kernel_size=5, degree=1, aggr="mean")
    assert tuple(layer.weight.shape) == (25, 3, 4) and tuple(layer.root.shape) == (3, 4) and tuple(layer.bias.shape) == (4,)
    assert list(inspect.signature(layer.forward).parameters) == ["x", "edge_index", "edge_attr"]
    with pytest.raises(ValueError):
        conv.SplineConv(3, 4, dim=2, kernel_size=5, aggr="max")
