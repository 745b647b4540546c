"""gnnops.conv.edge_reduce with operands that require grad (`_EdgeReduce`, gnnops_edge_grad in csrc/conv.hip) on the GPU against
the float64 propagate-order chain of tests/conv_chain.py (tied to oracle/conv_oracle.py, gradcheck and hand-worked values by
test_conv_chain_cpu.py): the forward, and the gradients of a random linear functional sum(out * R) with respect to q, p, w and
add, per tensor as max |got - want| / max |want|; a mean's gradients after scaling by the degree (conv_chain.mean_scales).
One test per table of conv_chain.py, whose cases are built from the conditions of the dispatch:
    dispatch    copy / cgconv / cgconv with w / film x sum / mean x K in {1, 4, 8, 13, 64, 200} x three types; operands plain or as
                16-byte-aligned column blocks of a wider matrix, and at K = 64 off 16 bytes by whole elements (the element form)
    shape       E = 0; one destination (K = 1 with out.sum(): a gradient of stride 0); more sources than destinations and the
                reverse; rows without an edge; duplicate edges; E on both sides of the one-launch plan and of 1024
    gridwrap    more than 8192 x 256 pieces: the grid-stride loop of edge_grad_kernel iterates
    hub         a destination with 9000 and with 70 000 incoming edges, a source with 9000 outgoing ones (csrc/hub.h: 8192)
    saturation  cgconv pre-activations over [-30, 30], around the softplus series / log seam, and a block of rows at +-100
Bars: fp32 3e-5 and fp16 1e-2 (film 3e-2) are those of test_conv_train_gpu.py. bf16, the hub table and the saturation table
have no precedent: 4 x the chain's distance from itself when run in float32 with the library's roundings, per case and tensor
(tests/golden/conv_self_error.json, measured on the CPU from the chain alone). The +-100 block is held to the same per-tensor
measure as everything else — its underflowing elements are compared too, nothing is left out — and must be finite.
The plan-cache test runs a copy and a cgconv backward over one edge_index object in both orders: bit-equal to each run alone."""
import pytest
import torch

import chain_harness as ch
import conv_chain as cc

pytestmark = pytest.mark.gpu

SELF_ERROR = cc.load_self_error()


@pytest.fixture(scope="module")
def conv():
    return ch.load_conv()


def _device_run(conv, case, dtype, ops, ei, R, edge_index=None):
    """(out, {name: leaf}) after backward of sum(out * R) (out.sum() for the ``ones`` cases)."""
    leaf = {k: (v.to(dtype).cuda().requires_grad_(True) if v is not None else None) for k, v in ops.items()}
    view = {k: cc.place(v, case.layout) for k, v in leaf.items()}
    if case.layout != "plain":
        es = torch.empty((), dtype=dtype).element_size()
        for k, v in view.items():
            if v is not None and v.size(0) > 1:
                aligned = v.data_ptr() % 16 == 0 and (v.stride(0) * es) % 16 == 0
                assert aligned == (case.layout == "block"), (k, v.data_ptr() % 16, v.stride(0))
    functor = "cgconv" if case.functor == "cgconv_w" else case.functor
    out = conv.edge_reduce(functor, view["q"], ei.cuda() if edge_index is None else edge_index, case.n_dst, p=view["p"], w=view["w"],
                           add=view["add"], aggr=(case.aggr,))
    assert out.dtype == dtype and out.requires_grad
    if case.ones:
        out.sum().backward()
    else:
        (out.float() * R.to(dtype).cuda().float()).sum().backward()
    return out, leaf


def _run_case(conv, case, dtype):
    ops, ei, R = cc.inputs(case, dtype)
    want_out, want, scales = cc.case_grads(case, dtype)
    out, leaf = _device_run(conv, case, dtype, ops, ei, R)
    ch.judge_case(case, dtype, "out", out, want_out, SELF_ERROR)
    for k, w in want.items():       # a mean's gradients are compared degree-scaled
        ch.judge_case(case, dtype, k, leaf[k].grad, w, SELF_ERROR, transform=lambda t, k=k: cc.scaled(k, t, scales))


@pytest.mark.parametrize("case,dtype", **ch.params(cc.DISPATCH))
def test_dispatch(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(cc.SHAPES))
def test_shape_edges(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(cc.GRIDWRAP))
def test_grid_wrap(conv, case, dtype):
    assert case.pieces(dtype) > cc.GRID_PIECES
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(cc.HUBS))
def test_hubs(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(cc.SATURATION))
def test_saturation(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("cache", [True, False], ids=["cache_on", "cache_off"])
@pytest.mark.parametrize("E", [500, 30000], ids=["one_launch_plan", "radix_plan"])
@pytest.mark.parametrize("order", ["copy_then_cgconv", "cgconv_then_copy"])
def test_plan_cache_orders(conv, order, E, cache):
    """The source-side plan is cached under (edge_index, tag 0) with a companion by the copy backward and without one by the
    cgconv backward; the destination plan comes with or without its column. Whichever runs first over one edge_index object,
    every gradient is bit-equal to that of the run alone on a fresh edge_index."""
    import gnnops

    assert cc.small_plan_fits(500, 300) and not cc.small_plan_fits(30000, 300)
    cases = {"copy": cc.Case("cache", "copy", "copy", "mean", 8, E, 300, 300, add=True),
             "cgconv": cc.Case("cache", "cgconv", "cgconv_w", "mean", 8, E, 300, 300)}
    ops, ei, R = {}, None, {}
    for k, c in cases.items():
        ops[k], e, R[k] = cc.inputs(c, torch.float32, seed=7)
        ei = e if ei is None else ei            # one graph for both passes
    assert ei.size(1) == E

    def run(name, edge_index):
        out, leaf = _device_run(conv, cases[name], torch.float32, ops[name], ei, R[name], edge_index=edge_index)
        return [out.detach().clone()] + [v.grad.clone() for v in leaf.values() if v is not None]

    gnnops.set_plan_cache(cache)
    try:
        alone = {k: run(k, ei.cuda()) for k in cases}
        shared = ei.cuda()
        for name in (("copy", "cgconv") if order == "copy_then_cgconv" else ("cgconv", "copy")) * 2:   # cold, then from the cache
            for a, b in zip(run(name, shared), alone[name]):
                assert torch.equal(a, b), (name, order)
    finally:
        gnnops.set_plan_cache(True)
