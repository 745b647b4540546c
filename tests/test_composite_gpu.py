"""scatter_softmax / scatter_log_softmax / scatter_logsumexp / scatter_std (csrc/composite.hip) in every kernel form, and the
backward of the composite and scatter / segment / gather ops (gnnops/autograd.py), through the torch_scatter shim on the GPU,
against the float64 CPU restatement tests/composite_chain.py on the same storage-rounded inputs. Every case is built from the
conditions of dispatch<T>() and carries the branch it takes in its id (test_composite_cpu.py asserts that the tables have
those properties); gradients are those of sum(out * R) for a random R, the reference is torch autograd of the float64 chain.

Non-finite reference values (a masked member's log_softmax, a wholly masked group) must be met exactly. Everywhere else the
distance is max |got - want| / max |want| or, under the project's own fp32 bars, elementwise:
    fp32, groups below the hub threshold      rtol 2e-6, atol 2e-6   (tests/test_segment_autograd_gpu.py::test_composite_ops)
    fp32 hubs against float64                 rtol 2e-5, atol 2e-6   (::test_composite_hub_groups)
    fp32 gradients of the composite ops       rtol 2e-5, atol 2e-6; std rtol 5e-5, atol 5e-6   (::test_composite_backward, _std_)
    fp32 mean backward                        rtol 1e-6, atol 1e-7   (::test_scatter_backward)
    fp32 backward of the selections           rtol 1e-6, atol 1e-6   (::test_index_select_and_gather_backward)
    routings (sum / min / max backward, min / max and selection forward, arg)   exactly equal
Every other bar is 4 x the self error of that very case: composite_chain run in fp32 with its intermediates rounded to the
storage type against itself in float64, measured on the CPU from the chain alone (test_composite_cpu.py prints the table;
tests/golden/composite_self_error.json is its recording, one entry per case, mode and type). Worst self errors per family:
    forward            fp16 4.2e-4 (bar 1.7e-3)   bf16 3.8e-3 (bar 1.5e-2)   fp32: large offsets 2.4e-7 (softmax; logsumexp 4.9e-8),
                       std on 1e4 + randn 1.8e-6, the 20 000-member streaming group 3.6e-6 (softmax)
    composite backward fp16 out 4.6e-4, grad 4.0e-3 (logsumexp)    bf16 out 3.7e-3, grad 3.0e-2 (logsumexp, masked members)
    mean backward      d src * count: fp16 2.0e-3 (the 70 000-member group: g / 70 000 is subnormal in fp16), bf16 3.4e-3;
                       out fp16 3.9e-4, bf16 2.1e-3
    selection backward fp16 3.6e-4    bf16 3.4e-3     fp32 with 70 000 contributions to one row 7.2e-6
A mean's gradient is compared after multiplying by the size of its group (composite_chain.times_count): against the largest
gradient of the tensor a 70 000-member group could lose its gradient altogether unnoticed. That is how these tests found that
the mean backward of scatter / segment_csr / segment_coo counted in the storage type: an fp16 count of 70 000 is inf and the
group's gradient 0 (error 0.75 of max against a bar of 8.0e-3). The counts are float32 now, whatever the storage type."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import composite_chain as cc
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "composite_self_error.json")) as _f:
    SELF_ERROR = json.load(_f)
F32 = torch.float32
SMALL, HUB, GRAD, GRAD_STD, MEAN, SELECT = (2e-6, 2e-6), (2e-5, 2e-6), (2e-5, 2e-6), (5e-5, 5e-6), (1e-6, 1e-7), (1e-6, 1e-6)
REDUCES = ("sum", "mean", "min", "max")


@pytest.fixture(scope="module")
def ts():
    import gnnops
    import torch_scatter

    gnnops.load_library()
    gnnops.set_plan_cache(False)
    yield torch_scatter
    gnnops.set_plan_cache(True)


def _judge(got, want, what, fp32_bar=None, key=None):
    """fp32_bar (rtol, atol): one of the project's own bars; key: 4 x the recorded self error of that case."""
    assert got is not None, f"{what}: nothing returned"
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert cc.same_specials(got, want), f"{what}: NaN / infinities are not where the reference has them"
    fin = torch.isfinite(want)
    err = cc.rel_err(got, want)
    if fp32_bar is not None:
        print(f"{what}: {err:.3e} of max (bar rtol {fp32_bar[0]:.0e} atol {fp32_bar[1]:.0e})")
        np.testing.assert_allclose(got[fin].numpy(), want[fin].numpy(), rtol=fp32_bar[0], atol=fp32_bar[1], err_msg=what)
    else:
        bar = 4 * SELF_ERROR[key]
        print(f"{what}: {err:.3e} of max (bar {bar:.3e} = 4 x self error, {key})")
        assert err <= bar, f"{what}: error {err:.3e} of max exceeds {bar:.3e} (4 x self error of {key})"


def _exact(got, want, what):
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(got, want), f"{what}: {int((got != want).sum())} of {got.numel()} elements differ"


def _call(ts, mode, src, index, dim, dim_size):
    m, unbiased = cc.split_mode(mode)
    kw = {} if dim is None else {"dim": dim}
    if m == "std":
        return ts.scatter_std(src, index, dim_size=dim_size, unbiased=unbiased, **kw)
    return {"softmax": ts.scatter_softmax, "log_softmax": ts.scatter_log_softmax, "logsumexp": ts.scatter_logsumexp}[m](
        src, index, dim_size=dim_size, **kw)


# ---- forward --------------------------------------------------------------------------------------------------------------
_FWD = [(c, m, d) for c in cc.FORWARD for d in c.dtypes for m in c.modes]


@pytest.mark.parametrize("case,mode,dtype", _FWD, ids=[f"{c.name}[{c.branch_of(d)}]-{m}-{cc.DNAME[d]}" for c, m, d in _FWD])
def test_composite_forward(ts, case, mode, dtype):
    import gnnops

    src, row, N = cc.fwd_inputs(case, dtype)
    want, _ = cc.composite_grads(src, row, case.dim(), N, mode)
    dev = cc.place(src.to(dtype), case.offset1, "cuda")
    assert dev.is_contiguous() and (dev.data_ptr() % 16 != 0) == case.offset1
    index = gnnops.Plan(row.cuda(), N) if case.plan else row.cuda()
    got = _call(ts, mode, dev, index, None if case.default_dim else case.dim(), None if case.implicit else N)
    assert got.dtype == dtype
    what = f"{case.name} {mode} {cc.DNAME[dtype]}"
    if dtype == F32 and case.bar != "self":
        _judge(got, want, what, fp32_bar=HUB if case.bar == "hub" else SMALL)
    else:
        _judge(got, want, what, key=f"fwd/{case.name}/{mode}/{cc.DNAME[dtype]}")


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=lambda d: cc.DNAME[d])
@pytest.mark.parametrize("mode", cc.MODES)
@pytest.mark.parametrize("form", ["rows_g2_kc1", "elem_K7"])
def test_csr_form_through_the_c_abi_equals_the_plan_path(ts, form, mode, dtype):
    """perm == NULL (contiguous segments of a sorted index) straight through gnnops_segment_composite: bit-equal to the plan
    path on the same sorted index, because the order inside each group is the same."""
    from gnnops import _lib, ops, segment

    case = cc.FORWARD_BY_NAME["rows_2lanes_implicit_dim_size" if form == "rows_g2_kc1" else "elem_K7"]
    src, row, N = cc.fwd_inputs(case, dtype)
    row = row.sort().values.cuda()
    dev = src.to(dtype).cuda()
    via_plan = _call(ts, mode, dev, row, 0, N)
    m, unbiased = cc.split_mode(mode)
    rowptr = segment.rowptr_from_sorted(row, N)
    out = torch.empty_like(via_plan)
    param = (1.0 if unbiased else 0.0) if m == "std" else (0.0 if m == "softmax" else 1e-12)
    rc = _lib.load().gnnops_segment_composite(dev.data_ptr(), rowptr.data_ptr(), None, out.data_ptr(), 1, dev.size(0), dev.size(1), N,
                                              {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}[dtype],
                                              segment._MODES[m], ctypes.c_double(param), ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    a, b = out.cpu().view(torch.int16 if dtype != F32 else torch.int32), via_plan.cpu().view(torch.int16 if dtype != F32 else torch.int32)
    assert torch.equal(a, b), f"{int((a != b).sum())} elements differ in bits"
    want, _ = cc.composite_grads(src, row.cpu(), 0, N, mode)
    if dtype == F32:
        _judge(out, want, f"csr {form} {mode}", fp32_bar=SMALL)


# ---- backward of the composite ops ---------------------------------------------------------------------------------------
_BWD = [(c, m, d) for c in cc.BACKWARD for d in cc.DTYPES for m in c.modes]


@pytest.mark.parametrize("case,mode,dtype", _BWD, ids=[f"{c.name}-{m}-{cc.DNAME[d]}" for c, m, d in _BWD])
def test_composite_backward(ts, case, mode, dtype):
    src, row, N, dim, R = cc.bwd_inputs(case, dtype, mode)
    want_out, want_dx = cc.composite_grads(src, row, dim, N, mode, R)
    leaf = src.to(dtype).cuda().requires_grad_(True)
    out = _call(ts, mode, leaf, row.cuda(), dim, N)
    assert out.grad_fn is not None
    out.backward(R.to(dtype).cuda())
    what = f"{case.name} {mode} {cc.DNAME[dtype]}"
    key = f"bwd/{case.name}/{mode}/{cc.DNAME[dtype]}"
    if dtype == F32:
        _judge(out, want_out, what + " out", fp32_bar=HUB if case.hub else SMALL)
        _judge(leaf.grad, want_dx, what + " d src", fp32_bar=GRAD_STD if mode.startswith("std") else GRAD)
    else:
        _judge(out, want_out, what + " out", key=key + "/out")
        _judge(leaf.grad, want_dx, what + " d src", key=key + "/grad")


# ---- backward of scatter / segment / gather ----------------------------------------------------------------------------
def _dtype_id(d):
    return cc.DNAME[d]


def _check_reduce(out, leaf, case, reduce, dtype, src, row, Nout, dim, R, tag, what):
    arg = None
    if reduce in ("min", "max"):
        out, got_arg = out
        arg = cc.oracle_arg(src, row, dim, Nout, reduce, dtype)
        assert torch.equal(got_arg.cpu(), arg), f"{what}: arg differs from the oracle's at {int((got_arg.cpu() != arg).sum())} places"
    assert out.grad_fn is not None
    want_out, want_dx = cc.reduce_grads(src, row, dim, Nout, reduce, R, arg)
    out.backward(R.to(dtype).cuda())
    if reduce == "mean":                                     # gradients times the group's size: every group on the scale of R
        key = f"mean/{case.name}/{tag}/{cc.DNAME[dtype]}"
        got_dx = cc.times_count(leaf.grad.detach().double().cpu(), row, dim, Nout)
        want_dx = cc.times_count(want_dx, row, dim, Nout)
        if dtype == F32:
            _judge(got_dx, want_dx, what + " d src * count", fp32_bar=MEAN)
        else:
            _judge(out, want_out, what + " out", key=key + "/out")
            _judge(got_dx, want_dx, what + " d src * count", key=key + "/grad")
    else:
        if reduce != "sum":
            _exact(out, want_out, what + " out")
        _exact(leaf.grad, want_dx, what + " d src")          # pure routing of R


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=_dtype_id)
@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("case", cc.ROUTES, ids=lambda c: c.name)
def test_scatter_backward(ts, case, reduce, dtype):
    src, row, Nout, dim, R = cc.route_inputs(case, dtype)
    leaf = src.to(dtype).cuda().requires_grad_(True)
    out = ts.scatter(leaf, row.cuda(), dim, dim_size=None if case.implicit else Nout, reduce=reduce)
    _check_reduce(out, leaf, case, reduce, dtype, src, row, Nout, dim, R, "unsorted", f"scatter {reduce} {case.name} {cc.DNAME[dtype]}")


_DIM0 = [c for c in cc.ROUTES if not c.lead]


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=_dtype_id)
@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("form", ["csr", "coo"])
@pytest.mark.parametrize("case", _DIM0, ids=lambda c: c.name)
def test_segment_backward(ts, case, form, reduce, dtype):
    src, row, Nout, dim, R = cc.route_inputs(case, dtype, sorted_index=True)
    leaf = src.to(dtype).cuda().requires_grad_(True)
    if form == "csr":
        indptr = torch.zeros(Nout + 1, dtype=torch.int64)
        indptr[1:] = torch.bincount(row, minlength=Nout).cumsum(0)
        out = ts.segment_csr(leaf, indptr.cuda(), reduce=reduce)
    else:
        out = ts.segment_coo(leaf, row.cuda(), dim_size=None if case.implicit else Nout, reduce=reduce)
    _check_reduce(out, leaf, case, reduce, dtype, src, row, Nout, dim, R, "sorted", f"segment_{form} {reduce} {case.name} {cc.DNAME[dtype]}")


def _check_select(out, leaf, case, kind, dtype, table, index, dim, R, what):
    assert out.grad_fn is not None
    want_out, want_dx = cc.select_grads(table, dim, index, R)
    _exact(out, want_out, what + " out")
    out.backward(R.to(dtype).cuda())
    if dtype == F32 and not case.big:
        _judge(leaf.grad, want_dx, what + " d input", fp32_bar=SELECT)
    else:
        _judge(leaf.grad, want_dx, what + " d input", key=f"select/{case.name}/{kind}/{cc.DNAME[dtype]}")


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=_dtype_id)
@pytest.mark.parametrize("form", ["csr", "coo"])
@pytest.mark.parametrize("case", _DIM0, ids=lambda c: c.name)
def test_gather_csr_coo_backward(ts, case, form, dtype):
    table, index, dim, R = cc.select_inputs(case, dtype, "sorted")
    leaf = table.to(dtype).cuda().requires_grad_(True)
    if form == "csr":
        indptr = torch.zeros(table.size(0) + 1, dtype=torch.int64)
        indptr[1:] = torch.bincount(index, minlength=table.size(0)).cumsum(0)
        out = ts.gather_csr(leaf, indptr.cuda())
    else:
        out = ts.gather_coo(leaf, index.cuda())
    _check_select(out, leaf, case, "sorted", dtype, table, index, dim, R, f"gather_{form} {case.name} {cc.DNAME[dtype]}")


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=_dtype_id)
@pytest.mark.parametrize("kind", ["index_select", "gather"])
@pytest.mark.parametrize("case", cc.ROUTES, ids=lambda c: c.name)
def test_index_select_and_gather_backward(ts, case, kind, dtype):
    from gnnops import autograd as ga

    table, index, dim, R = cc.select_inputs(case, dtype, kind)
    leaf = table.to(dtype).cuda().requires_grad_(True)
    out = ga.index_select(leaf, dim, index.cuda()) if kind == "index_select" else ga.gather(leaf, dim, index.cuda())
    _check_select(out, leaf, case, kind, dtype, table, index, dim, R, f"{kind} {case.name} {cc.DNAME[dtype]}")
