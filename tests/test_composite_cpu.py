"""The yardstick of the composite and scatter-backward tests (tests/composite_chain.py) checked without a GPU: its forward
against oracle.composite and torch's own per-group functions, its gradients against finite differences, hand-worked answers
for every special-value rule of csrc/composite.hip, the properties each input table of test_composite_gpu.py is named for,
and the self-error table its bars are taken from (printed; recorded in tests/golden/composite_self_error.json)."""
import json
import math
import os
import warnings

import numpy as np
import pytest
import torch

import composite_chain as cc
from helpers import GOLDEN
from oracle import oracle

warnings.filterwarnings("ignore", message="index_reduce")
INF = float("inf")


def _problem(seed, shape, dim, N):
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(shape, generator=g, dtype=torch.float64) * 3
    row = cc.row_index(g, shape[dim], N)
    return src, row


# ---- the float64 chain against the project's oracle, torch and finite differences -----------------------------------------
@pytest.mark.parametrize("mode", cc.MODES)
def test_chain_matches_the_numpy_oracle(mode):
    src, row = _problem(1, (300, 6), 0, 40)
    src = src.float().double()
    m, unbiased = cc.split_mode(mode)
    got = cc.composite(src, row, 0, 40, m, unbiased=unbiased).numpy()
    want = oracle.composite(src.float().numpy(), row.numpy(), 40, m, unbiased=unbiased)
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6)     # the oracle is sequential fp32


@pytest.mark.parametrize("shape,dim", [((300, 5), 0), ((2, 300, 3), 1), ((3, 300), -1)], ids=["dim0", "dim1_of_3d", "last_dim"])
def test_chain_matches_torch_per_group(shape, dim):
    N = 40
    src, row = _problem(2, shape, dim, N)
    x = src.movedim(dim, 0)
    outs = {m: cc.composite(src, row, dim, N, *cc.split_mode(m)[:1], unbiased=cc.split_mode(m)[1]).movedim(dim, 0) for m in cc.MODES}
    for n in range(N):
        rows = torch.nonzero(row == n).flatten()
        v = x[rows]
        if rows.numel() == 0:
            assert (outs["logsumexp"][n] == math.log(1e-12)).all() and (outs["std"][n] == 0).all()
            continue
        assert (outs["softmax"][rows] - torch.softmax(v, 0)).abs().max() <= 1e-14
        assert (outs["log_softmax"][rows] - torch.log_softmax(v, 0)).abs().max() <= 1e-11      # eps = 1e-12 inside the log
        assert (outs["logsumexp"][n] - torch.logsumexp(v, 0)).abs().max() <= 1e-11
        c = rows.numel()
        if c > 1:
            assert (outs["std"][n] * math.sqrt((c - 1 + 1e-6) / (c - 1)) - v.std(0)).abs().max() <= 1e-12
            assert (outs["std_biased"][n] * math.sqrt((c + 1e-6) / c) - v.std(0, unbiased=False)).abs().max() <= 1e-12
        else:
            assert (outs["std"][n] == 0).all() and (outs["std_biased"][n] == 0).all()


@pytest.mark.parametrize("mode", cc.MODES)
def test_chain_gradcheck(mode):
    g = torch.Generator().manual_seed(3)
    row = torch.tensor([4, 2, 2, 4, 1, 4, 2, 4, 4])            # groups 0 and 3 empty, group 1 has one member
    src = torch.randn(2, 9, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    m, unbiased = cc.split_mode(mode)
    assert torch.autograd.gradcheck(lambda x: cc.composite(x, row, 1, 5, m, unbiased=unbiased), [src], eps=1e-6, atol=1e-7, rtol=1e-5)


def test_reductions_and_selections_match_the_oracle_and_gradcheck():
    g = torch.Generator().manual_seed(4)
    row = torch.tensor([4, 2, 2, 4, 1, 4, 2, 4, 4])
    src = torch.randn(2, 9, 3, generator=g, dtype=torch.float64)
    for reduce in ("sum", "mean", "min", "max"):
        arg = cc.oracle_arg(src, row, 1, 6, reduce, torch.float32) if reduce in ("min", "max") else None
        want = oracle.scatter(src.float().numpy(), row.numpy(), dim=1, dim_size=6, reduce=reduce)
        want = want[0] if isinstance(want, tuple) else want
        got = cc.reduce_rows(src.float().double(), row, 1, 6, reduce, arg)
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-6, atol=1e-6)
        leaf = src.clone().requires_grad_(True)
        assert torch.autograd.gradcheck(lambda x: cc.reduce_rows(x, row, 1, 6, reduce, arg), [leaf], eps=1e-6, atol=1e-7)
    table = torch.randn(2, 6, 3, generator=g, dtype=torch.float64)
    assert np.array_equal(cc.select(table, 1, row).numpy(), oracle.index_select(table.numpy(), 1, row.numpy()))
    full = torch.randint(0, 6, (2, 9, 3), generator=g)
    assert np.array_equal(cc.select(table, 1, full).numpy(), oracle.gather(table.numpy(), 1, full.numpy()))


def test_min_max_gradient_goes_to_one_position_among_ties():
    src = torch.tensor([[1.0], [3.0], [3.0], [0.0], [-0.0]], dtype=torch.float64)
    row = torch.tensor([0, 0, 0, 1, 1])
    R = torch.tensor([[5.0], [7.0]], dtype=torch.float64)
    for reduce in ("max", "min"):
        arg = cc.oracle_arg(src, row, 0, 2, reduce, torch.float32)
        out, dx = cc.reduce_grads(src, row, 0, 2, reduce, R, arg)
        assert int((dx != 0).sum()) == 2 and float(dx.sum()) == 12.0          # torch's amax would split 5 into 2.5 + 2.5
        assert torch.equal(dx.flatten().nonzero().flatten(), arg.flatten().sort().values)
        _, dx32 = cc.reduce_grads(src, row, 0, 2, reduce, R, arg, rnd=torch.float32)
        assert torch.equal(dx32, dx)


# ---- hand-worked special values -----------------------------------------------------------------------------------------
def _all_modes(src, row, N):
    return {m: cc.composite(torch.tensor(src, dtype=torch.float64).view(-1, 1), torch.tensor(row), 0, N, *cc.split_mode(m)[:1],
                            unbiased=cc.split_mode(m)[1]).flatten().tolist() for m in cc.MODES}


def test_a_masked_member_of_a_finite_group():
    o = _all_modes([0.0, -INF, 0.0], [0, 0, 0], 1)
    assert o["softmax"] == [0.5, 0.0, 0.5]
    assert o["log_softmax"][1] == -INF and abs(o["log_softmax"][0] - math.log(0.5)) < 1e-12
    assert abs(o["logsumexp"][0] - math.log(2.0)) < 1e-12


def test_a_wholly_masked_group():
    o = _all_modes([-INF, -INF, 1.0], [0, 0, 1], 2)
    assert math.isnan(o["softmax"][0]) and math.isnan(o["softmax"][1]) and o["softmax"][2] == 1.0     # exp(-inf) / 0
    assert o["log_softmax"][:2] == [-INF, -INF] and abs(o["log_softmax"][2]) < 1e-11                 # -inf - log(0 + eps)
    assert o["logsumexp"][0] == -INF and abs(o["logsumexp"][1] - 1.0) < 1e-11                         # -inf + log(0 + eps)
    x = np.array([[-np.inf], [-np.inf], [1.0]], dtype=np.float32)
    ix = np.array([0, 0, 1])
    assert np.isnan(oracle.composite(x, ix, 2, "softmax")[:2]).all() and oracle.composite(x, ix, 2, "softmax")[2, 0] == 1.0
    assert (oracle.composite(x, ix, 2, "log_softmax")[:2] == -np.inf).all()
    assert oracle.composite(x, ix, 2, "logsumexp")[0, 0] == -np.inf


def test_an_empty_group():
    o = _all_modes([2.0], [1], 3)
    for n in (0, 2):                                         # max := 0, sum = 0: 0 + log(eps); std 0
        assert o["logsumexp"][n] == math.log(1e-12) and o["std"][n] == 0.0 and o["std_biased"][n] == 0.0
    assert o["softmax"] == [1.0]


def test_a_one_member_group_under_std():
    o = _all_modes([3.0, 1.0, 5.0], [0, 1, 1], 2)
    assert o["std"][0] == 0.0 and o["std_biased"][0] == 0.0
    assert o["std"][1] == math.sqrt(8.0 / (1 + 1e-6)) and o["std_biased"][1] == math.sqrt(8.0 / (2 + 1e-6))
    src = torch.tensor([[3.0], [1.0], [5.0]], dtype=torch.float64)
    for mode in ("std", "std_biased"):                       # the lone member's gradient is 0, not 0 * inf
        _, dx = cc.composite_grads(src, torch.tensor([0, 1, 1]), 0, 2, mode, torch.ones(2, 1, dtype=torch.float64))
        assert dx[0, 0] == 0.0 and torch.isfinite(dx).all() and dx[1, 0] < 0 < dx[2, 0]
        _, dx16 = cc.composite_grads(src, torch.tensor([0, 1, 1]), 0, 2, mode, torch.ones(2, 1, dtype=torch.float64), rnd=torch.float16)
        assert dx16[0, 0] == 0.0 and (dx16 - dx).abs().max() <= 2e-3


# ---- the tables of test_composite_gpu.py have the properties their cases are named for ---------------------------------
def _sizes(row, N):
    return torch.bincount(row, minlength=N)


@pytest.mark.parametrize("case", cc.FORWARD, ids=lambda c: c.name)
def test_forward_tables(case):
    for dtype in case.dtypes:
        src, row, N = cc.fwd_inputs(case, dtype)
        sizes = _sizes(row, N)
        assert row.numel() == src.size(case.dim()) and int(row.max()) == N - 1           # an implicit dim_size finds N
        assert {0, 1, 8, 9} <= set(sizes.tolist()), "groups of exactly 0, 1, 8 and 9 members"
        K = case.k(dtype)
        B = int(np.prod(case.lead)) if case.lead else 1
        branch = cc.dispatch_branch(B, row.numel(), 1 if K is None else K, int(sizes.max()), dtype, aligned=not case.offset1)
        assert branch == case.branch_of(dtype), (case.name, dtype, branch)
        if "hub" in case.name:
            assert int(sizes.max()) > cc.T_HUB and B == 1 and row.numel() > cc.T_HUB
        elif "stream" in case.name:
            assert int(sizes.max()) == 20000 and B == 2 and branch.endswith("_stream")
        else:
            assert int(sizes.max()) <= cc.T_HUB
        if case.name.startswith("elem") and not case.offset1:
            assert (1 if K is None else K) % cc.VEC[dtype] != 0
        if case.offset1:
            assert K % cc.VEC[dtype] == 0
            t = cc.place(src.to(dtype), True, "cpu")
            assert t.is_contiguous() and t.data_ptr() % 16 == t.element_size() and torch.equal(t, src.to(dtype))
        if case.default_dim:
            assert K is None and B == 4 and case.dim() == src.dim() - 1
        if case.lead:
            assert B > 1 and src.dim() == len(case.lead) + (1 if K is None else 2)
        x = src.movedim(case.dim(), 0)
        if case.values == "offsets":
            assert float(src.abs().max()) <= (3.0e4 if dtype == torch.float16 else 1.1e4)
            assert float(src.abs().min()) >= cc.OFFSET[dtype] - 16 and float(src.min()) < 0 < float(src.max())
            big = torch.nonzero(sizes >= 8).flatten()[0]
            assert float(x[row == big].max() - x[row == big].min()) >= 16                 # a spread of about 30 inside a group
        elif case.values == "masked":
            assert bool(torch.isinf(src).any())
            m = torch.full((N,) + tuple(x.shape[1:]), -INF, dtype=x.dtype).index_reduce(0, row, x, "amax")
            assert bool(torch.isfinite(m[sizes > 0]).all()), "every group keeps a finite max"
        elif case.values == "all_neg_inf":
            assert bool((x[row == 3] == -INF).all()) and int(sizes[3]) == 9 and bool(torch.isfinite(x[(row != 3) & (row != 6)]).all())
        else:
            assert bool(torch.isfinite(src).all())
        if case.values == "mean1e4":
            assert abs(float(src.mean()) - 1e4) < 1 and 0.8 < float(src.std()) < 1.2
        for mode in case.modes:                               # every reference output is representable in the storage type
            want, _ = cc.composite_grads(src, row, case.dim(), N, mode)
            fin = torch.isfinite(want)
            assert bool(torch.isfinite(want[fin].to(dtype)).all())
            if case.values not in ("masked", "all_neg_inf"):
                assert bool(fin.all()), (case.name, mode, dtype)
            elif case.values == "masked":
                assert not bool(torch.isnan(want).any())


@pytest.mark.parametrize("case", cc.BACKWARD, ids=lambda c: c.name)
def test_backward_tables(case):
    for dtype in cc.DTYPES:
        for mode in case.modes:
            src, row, N, dim, R = cc.bwd_inputs(case, dtype, mode)
            sizes = _sizes(row, N)
            assert {0, 1, 8, 9} <= set(sizes.tolist())
            assert (int(sizes.max()) > cc.T_HUB) == case.hub
            if case.masked:
                x = src.movedim(dim, 0)
                m = torch.full((N,) + tuple(x.shape[1:]), -INF, dtype=x.dtype).index_reduce(0, row, x, "amax")
                assert bool(torch.isinf(src).any()) and bool(torch.isfinite(m[sizes > 0]).all())
            out, dx = cc.composite_grads(src, row, dim, N, mode, R)
            assert out.shape == R.shape and dx.shape == src.shape
            assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dx.to(dtype)).all())
            assert not bool(torch.isnan(out).any())


@pytest.mark.parametrize("case", cc.ROUTES, ids=lambda c: c.name)
def test_route_tables(case):
    for dtype in cc.DTYPES:
        src, row, Nout, dim, R = cc.route_inputs(case, dtype)
        sizes = _sizes(row, Nout)
        assert int(row.max()) == case.N - 1 and Nout == case.N + case.extra
        assert {0, 1} <= set(sizes.tolist())
        if case.big:
            assert int(sizes[5]) == 70000 > 65504 > cc.T_HUB and int(sizes[4]) > 256        # a bf16 count above 256 is rounded
            assert float(torch.tensor(float(sizes[4])).to(torch.bfloat16)) != float(sizes[4]) or int(sizes[4]) % 2 == 0
        if case.ties:
            x = src.movedim(dim, 0)
            assert float((x[0::2][: x[1::2].size(0)] == x[1::2]).double().mean()) > 0.5 and bool((x == 0).any())   # duplicated rows
            assert bool(torch.signbit(x[x == 0]).any()) and not bool(torch.signbit(x[x == 0]).all())     # both zeros
            for reduce in ("min", "max"):                     # some output is reached by its extreme value more than once
                arg = cc.oracle_arg(src, row, dim, Nout, reduce, dtype)
                out = cc.reduce_rows(src, row, dim, Nout, reduce, arg).movedim(dim, 0)
                hits = torch.zeros_like(out).index_add(0, row, (x == out[row]).double())
                assert int((hits > 1).sum()) > 10
        assert cc.route_inputs(case, dtype, sorted_index=True)[1].diff().min() >= 0


def test_print_self_error_table(capsys):
    """The numbers the bars of test_composite_gpu.py are 4 x of. The recording the GPU test reads has an entry for every case,
    and where the storage type's rounding decides the figure (>= 1e-4) the recording agrees with this run."""
    table = cc.self_error_table()
    with open(os.path.join(GOLDEN, "composite_self_error.json")) as f:
        recorded = json.load(f)
    with capsys.disabled():
        print("\nself error of tests/composite_chain.py (rounded fp32 chain against the float64 chain, relative to max |reference|)")
        for k, v in table.items():
            print(f"  {k:72s} {v:.3e}")
    assert set(recorded) == set(table)
    for k, v in table.items():
        assert v == v and v >= 0
        if v >= 1e-4:
            assert recorded[k] / 1.5 <= v <= recorded[k] * 1.5, (k, v, recorded[k])
