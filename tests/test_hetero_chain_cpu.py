"""tests/hetero_chain.py against a second formulation that shares none of its code (a per-row loop and per-relation dense
adjacency products, ~20 nodes), and its gradients against torch.autograd.gradcheck (~6 nodes). Float64 on the CPU throughout."""
import pytest
import torch

import hetero_chain as hc

F64 = torch.float64


def _close(a, b):
    assert a.shape == b.shape
    if a.numel() == 0:
        return
    assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1.0)


@pytest.mark.parametrize("lengths", [[5, 0, 7, 1], [0, 0, 4], [9], [3, 2, 0], [0], []], ids=str)
@pytest.mark.parametrize("with_bias", [False, True], ids=["plain", "bias"])
def test_segment_matmul_against_the_row_loop(lengths, with_bias):
    g = torch.Generator().manual_seed(len(lengths) + 10 * with_bias)
    T, M = len(lengths), sum(lengths)
    x, w = torch.randn(M, 5, generator=g, dtype=F64), torch.randn(T, 5, 3, generator=g, dtype=F64)
    b = torch.randn(T, 3, generator=g, dtype=F64) if with_bias else None
    types = torch.repeat_interleave(torch.arange(T), torch.tensor(lengths, dtype=torch.int64)) if T else torch.zeros(0, dtype=torch.int64)
    got = hc.segment_matmul_ref(x, hc.ptr_of(lengths), w, b)
    _close(got, hc.rowwise_matmul(x, types, w, b))


@pytest.mark.parametrize("with_bias", [False, True], ids=["plain", "bias"])
def test_hetero_linear_against_the_row_loop(with_bias):
    g = torch.Generator().manual_seed(3)
    types = torch.randint(0, 4, (21,), generator=g)
    types[types == 2] = 0                      # a type without a row
    P = {"weight": torch.randn(4, 6, 5, generator=g, dtype=F64)}
    if with_bias:
        P["bias"] = torch.randn(4, 5, generator=g, dtype=F64)
    x = torch.randn(21, 6, generator=g, dtype=F64)
    _close(hc.hetero_linear_ref(P, x, types, 4), hc.rowwise_matmul(x, types, P["weight"], P.get("bias")))


@pytest.mark.parametrize("aggr", ["mean", "sum"])
@pytest.mark.parametrize("num_bases", [None, 2], ids=["full", "bases"])
@pytest.mark.parametrize("root_weight", [True, False], ids=["root", "no_root"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
def test_rgcn_against_dense_adjacency(aggr, num_bases, root_weight, bias):
    n, e, R = 20, 90, 5
    ei, et = hc.graph(7, n, e, R)
    assert not bool((ei[1] == 3).any()) and not bool((et == 1).any())
    P = hc.rgcn_params(11, 6, 4, R, num_bases, root_weight, bias)
    x = torch.randn(n, 6, generator=torch.Generator().manual_seed(5), dtype=F64)
    _close(hc.rgcn_ref(P, x, ei, et, R, aggr), hc.rgcn_dense(P, x, ei, et, R, aggr))


def test_gradients_of_the_chain():
    g = torch.Generator().manual_seed(9)
    lengths = [2, 0, 3, 1]
    x = torch.randn(6, 3, generator=g, dtype=F64, requires_grad=True)
    w = torch.randn(4, 3, 2, generator=g, dtype=F64, requires_grad=True)
    b = torch.randn(4, 2, generator=g, dtype=F64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x, w, b: hc.segment_matmul_ref(x, hc.ptr_of(lengths), w, b), (x, w, b))
    types = torch.tensor([2, 0, 3, 0, 2, 2])
    assert torch.autograd.gradcheck(lambda x, w, b: hc.hetero_linear_ref({"weight": w, "bias": b}, x, types, 4), (x, w, b))
    ei, et = hc.graph(13, 6, 14, 3)
    for aggr in ("mean", "sum"):
        for num_bases in (None, 2):
            P = hc.rgcn_params(17, 3, 2, 3, num_bases, True, True)
            names = sorted(P)
            leaves = [P[k].clone().requires_grad_(True) for k in names]
            assert torch.autograd.gradcheck(lambda x, *ps: hc.rgcn_ref(dict(zip(names, ps)), x, ei, et, 3, aggr), (x, *leaves))
