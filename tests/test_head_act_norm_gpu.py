"""gnnops.conv.head_act_norm (csrc/norm.hip) against the float64 chain of tests/norm_chain.py: ``out`` and the gradients of
sum(out * R) with respect to a, bias, gamma and beta, as max |got - want| / max |want| per tensor.
    shape    H in {1, 3, 4} x C in {1, 5, 8, 64, 136, 1024} x three types, N = 257, ``a`` a column block of a wider matrix (one case
             dense); each of bias / relu / scale / norm absent; H * C = 8192 as 1 x 8192 and 8 x 1024; 8200 raises
    rows     N in {0, 1, 63, 64, 65} at 64 rows per wave; N = 70 000 with C = 8: many partial rows, the backward's grid wraps
    values   constant rows (var = 0), fully dropped rows, a zero in gamma, rows of mean 1e4 and spread 1, rows the ReLU kills
    grads    g from out.sum() (expanded) and from a transposed consumer; two runs bit-identical; the raw call refuses requires_grad
Bars: fp32 3e-5 and fp16 1e-2 are the project's (conv_chain.PROJECT_BAR) for the shape and rows tables; bf16 and the values table:
4 x the chain's distance from itself in float32 with the library's roundings, per case and tensor
(tests/golden/head_act_norm_self_error.json, measured on the CPU from the chain alone)."""
import pytest
import torch

import chain_harness as ch
import norm_chain as nc

pytestmark = pytest.mark.gpu

SELF_ERROR = nc.load_self_error()
_reference = ch.Reference(lambda case, dtype, ones=False: nc.case_grads(case, dtype, ones=ones))


@pytest.fixture(scope="module")
def conv():
    return ch.load_conv()


def _leaves(case, dtype):
    ops, R = nc.inputs(case, dtype)
    leaf = {n: (v.to(dtype).cuda().requires_grad_(n != "k") if v is not None else None) for n, v in ops.items()}
    return leaf, R.to(dtype).cuda()


def _call(conv, case, leaf):
    a = nc.place(leaf["a"], case.layout)
    if case.layout == "block":
        assert a.stride(0) != case.H * case.C
    out = conv.head_act_norm(a, case.H, leaf["bias"], case.relu, leaf["k"], leaf["gamma"], leaf["beta"])
    assert out.dtype == a.dtype and out.requires_grad and out.shape == (case.N, case.C)
    return out


def _device_run(conv, case, dtype):
    leaf, R = _leaves(case, dtype)
    out = _call(conv, case, leaf)
    (out.float() * R.float()).sum().backward()
    return out, leaf


def _run_case(conv, case, dtype):
    want_out, want = _reference(case, dtype)
    out, leaf = _device_run(conv, case, dtype)
    ch.judge_case(case, dtype, "out", out, want_out, SELF_ERROR)
    for n, w in want.items():
        ch.judge_case(case, dtype, n, leaf[n].grad, w, SELF_ERROR)
    assert leaf["k"] is None or leaf["k"].grad is None
    return out, leaf


@pytest.mark.parametrize("case,dtype", **ch.params(nc.SHAPES))
def test_shapes(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(nc.ROWS))
def test_rows(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(nc.VALUES))
def test_values(conv, case, dtype):
    out, leaf = _run_case(conv, case, dtype)
    rows = list(nc.SPECIAL_ROWS)
    if case.values in ("dropped", "negative"):       # d = 0 along the row: out is beta, and nothing flows back into the row
        assert torch.equal(out[rows].detach(), leaf["beta"].detach().expand(len(rows), -1))
        assert float(leaf["a"].grad[rows].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", nc.DTYPES, ids=[nc.DNAME[d] for d in nc.DTYPES])
def test_no_rows(conv, dtype):
    a = torch.zeros((0, 24), dtype=dtype, device="cuda", requires_grad=True)
    vec = [torch.ones(8, dtype=dtype, device="cuda", requires_grad=True) for _ in range(3)]
    out = conv.head_act_norm(a, 3, vec[0], True, None, vec[1], vec[2])
    assert out.shape == (0, 8) and out.dtype == dtype
    out.sum().backward()
    assert a.grad.shape == (0, 24)
    for v in vec:
        assert v.grad is not None and float(v.grad.abs().max()) == 0.0


def test_row_width_limit(conv):
    a = torch.zeros((3, 8200), device="cuda")
    with pytest.raises(RuntimeError, match="8192"):
        conv.head_act_norm(a, 1)
    with pytest.raises(RuntimeError, match="8192"):
        conv.head_act_norm(a, 8, norm_weight=torch.ones(1025, device="cuda"))
    import ctypes

    import gnnops
    from gnnops import _lib

    out = torch.zeros((3, 8200), device="cuda")
    rc = gnnops.load_library().gnnops_head_act_norm(a.data_ptr(), 8200, None, None, None, None, out.data_ptr(), None, 3, 1, 8200, 1,
                                                    ctypes.c_float(1e-5), 0, None)
    assert rc != 0 and "8192" in _lib.load().gnnops_last_error().decode()


GRAD_CASE = nc.SHAPES[[c.name for c in nc.SHAPES].index("H3-C136")]


def test_expanded_gradient(conv):
    """out.sum(): autograd hands the backward one expanded scalar (strides 0, 0)."""
    want_out, want = _reference(GRAD_CASE, torch.float32, True)
    leaf, _ = _leaves(GRAD_CASE, torch.float32)
    out = _call(conv, GRAD_CASE, leaf)
    out.sum().backward()
    for n, w in want.items():
        ch.judge_case(GRAD_CASE, torch.float32, n, leaf[n].grad, w, SELF_ERROR)


def test_transposed_gradient(conv):
    """A consumer W @ out.t() hands the backward a transposed gradient: copied, the same numbers."""
    want_out, want = _reference(GRAD_CASE, torch.float32)
    leaf, R = _leaves(GRAD_CASE, torch.float32)
    out = _call(conv, GRAD_CASE, leaf)
    out.t().backward(R.t().contiguous())
    for n, w in want.items():
        ch.judge_case(GRAD_CASE, torch.float32, n, leaf[n].grad, w, SELF_ERROR)


@pytest.mark.parametrize("case", [GRAD_CASE, nc.ROWS[-1], nc.SHAPES[-2]], ids=lambda c: c.name)
def test_same_bits_on_two_runs(conv, case):
    runs = []
    for _ in range(2):
        out, leaf = _device_run(conv, case, torch.float32)
        runs.append([out.detach().clone()] + [leaf[n].grad.clone() for n in nc.GRAD_NAMES if leaf[n] is not None])
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_forward_without_grad_is_the_same_launch(conv):
    leaf, _ = _leaves(GRAD_CASE, torch.float16)
    out = _call(conv, GRAD_CASE, leaf)
    with torch.no_grad():
        plain = conv.head_act_norm(nc.place(leaf["a"], GRAD_CASE.layout), GRAD_CASE.H, leaf["bias"], True, leaf["k"], leaf["gamma"], leaf["beta"])
    assert not plain.requires_grad and torch.equal(plain, out.detach())


def test_refusals(conv):
    a, bias = torch.rand(10, 8), torch.rand(4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        conv.head_act_norm(a, 2, bias)
    a, bias = a.cuda(), bias.cuda()
    with pytest.raises(NotImplementedError, match="requires grad"):
        conv._norm_forward(a.clone().requires_grad_(True), 2, bias, True, None, None, None, 1e-5, False)
    with pytest.raises(NotImplementedError, match="requires grad"):
        conv._norm_forward(a, 2, bias.clone().requires_grad_(True), True, None, None, None, 1e-5, False)
    with pytest.raises(RuntimeError, match="not differentiated"):
        conv.head_act_norm(a, 2, bias, scale=torch.ones(10, 4, device="cuda", requires_grad=True))
    with pytest.raises(RuntimeError, match="heads"):
        conv.head_act_norm(a, 3)
    with pytest.raises(RuntimeError, match="norm_bias without norm_weight"):
        conv.head_act_norm(a, 2, norm_bias=bias)
