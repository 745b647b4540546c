"""gnnops.conv.edge_attention and gnnops.conv.GATv2Conv (csrc/attention.hip: one forward pass with an online softmax, one
destination-ordered backward pass) on the GPU against the float64 propagate-order chain of tests/attention_chain.py (tied to a
dense masked softmax, gradcheck and a hand-worked example by test_attention_chain_cpu.py): out, and the gradients of a random
linear functional sum(out * R) with respect to q, p and att, per tensor as max |got - want| / max |want|.
    shape    H in {1, 3, 4} x C in {1, 5, 8, 64, 136} x three types, 257 sources -> 300 destinations, q and p as column blocks of
             a wider matrix (one case dense)
    seams    destinations with 0, 1, 7, 8, 9, 63, 64, 65 and 129 edges in one graph: the unroll steps and the run of 64 edge ids
    range    scores of a destination hundreds apart (a softmax without a running maximum overflows), rows whose scores strictly
             ascend (the maximum changes at every edge), strictly descend, and are all equal
    heavy    destinations with 8193 and 20 000 edges among ordinary rows: one lane group walks each
    plan     E = 24576 / 24577, the two sides of the one-launch plan; cache on and off; a backward whose source plan is built cold
    edges    repeated edges and self loops in the raw op; E = 0
Bars: fp32 3e-5 and fp16 1e-2 are the project's (conv_chain.PROJECT_BAR) for the shape / seams / plan / edges tables; bf16 and the
range and heavy tables have no precedent: 4 x the chain's distance from itself in float32 with the library's roundings, per case
and tensor (tests/golden/attention_self_error.json, measured on the CPU from the chain alone)."""
import pytest
import torch

import attention_chain as ac
import chain_harness as ch

pytestmark = pytest.mark.gpu

SELF_ERROR = ac.load_self_error()
_reference = ch.Reference(ac.case_grads)


@pytest.fixture(scope="module")
def conv():
    return ch.load_conv()


def _device_run(conv, case, dtype, edge_index=None):
    ops, ei, R = ac.inputs(case, dtype)
    leaf = {k: v.to(dtype).cuda().requires_grad_(True) for k, v in ops.items()}
    q, p = ac.place(leaf["q"], case.layout), ac.place(leaf["p"], case.layout)
    if case.layout == "block":
        assert q.stride(0) != case.H * case.C and p.stride(0) != case.H * case.C
    out = conv.edge_attention(q, p, leaf["att"], ei.cuda() if edge_index is None else edge_index, case.n_dst, case.H, case.slope)
    assert out.dtype == dtype and out.requires_grad and out.shape == (case.n_dst, case.H * case.C)
    (out.float() * R.to(dtype).cuda().float()).sum().backward()
    return out, leaf


def _run_case(conv, case, dtype):
    want_out, want = _reference(case, dtype)
    out, leaf = _device_run(conv, case, dtype)
    ch.judge_case(case, dtype, "out", out, want_out, SELF_ERROR)
    for k, w in want.items():
        ch.judge_case(case, dtype, k, leaf[k].grad, w, SELF_ERROR)
    return out


@pytest.mark.parametrize("case,dtype", **ch.params(ac.SHAPES))
def test_shapes(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(ac.SEAMS))
def test_degree_seams(conv, case, dtype):
    out = _run_case(conv, case, dtype)
    assert float(out[0].detach().abs().max()) == 0.0   # the destination without an edge


@pytest.mark.parametrize("case,dtype", **ch.params(ac.RANGE))
def test_online_rescale(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(ac.HEAVY))
def test_heavy_destinations(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(ac.PLAN))
def test_both_sides_of_the_one_launch_plan(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(ac.EDGES[:1]))
def test_repeated_edges_and_self_loops(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("dtype", ac.DTYPES, ids=[ac.DNAME[d] for d in ac.DTYPES])
def test_no_edges(conv, dtype):
    case = ac.EDGES[1]
    assert case.E == 0
    out, leaf = _device_run(conv, case, dtype)
    assert float(out.abs().max()) == 0.0
    for k, v in leaf.items():
        assert v.grad is not None and v.grad.shape == v.shape and float(v.grad.abs().max()) == 0.0, k
    ops, ei, _ = ac.inputs(case, dtype)
    dev = {k: v.to(dtype).cuda() for k, v in ops.items()}
    _, lse = conv._attention_forward(dev["q"], dev["p"], dev["att"], ei.cuda(), case.n_dst, case.H, case.slope)
    assert lse.shape == (case.n_dst, case.H) and lse.dtype == torch.float32 and bool(torch.isneginf(lse).all())


def test_lse_is_written(conv):
    case = ac.SEAMS[0]
    ops, ei, _ = ac.inputs(case, torch.float32)
    dev = {k: v.float().cuda() for k, v in ops.items()}
    _, lse = conv._attention_forward(dev["q"], dev["p"], dev["att"], ei.cuda(), case.n_dst, case.H, case.slope)
    _, want = ac.attention(ops["q"], ops["p"], ops["att"], ei, case.n_dst, case.H, case.slope)
    assert bool(torch.isneginf(lse[0]).all())
    assert ac.rel_err(lse[1:].double().cpu(), want[1:]) <= ac.PROJECT_BAR[torch.float32]


@pytest.mark.parametrize("cache", [True, False], ids=["cache_on", "cache_off"])
@pytest.mark.parametrize("case", ac.PLAN, ids=[c.name for c in ac.PLAN])
def test_plan_routes(conv, case, cache):
    """Forward then backward over one edge_index object, twice (cold, then from the cache); and a backward whose source plan is
    built cold (the caches cleared between forward and backward): every tensor bit-equal to the run on a fresh edge_index."""
    import gnnops

    _, ei, _ = ac.inputs(case, torch.float32)
    snap = lambda out, leaf: [out.detach().clone()] + [v.grad.clone() for v in leaf.values()]   # noqa: E731
    gnnops.set_plan_cache(cache)
    try:
        alone = snap(*_device_run(conv, case, torch.float32))
        shared = ei.cuda()
        for _ in range(2):
            for a, b in zip(snap(*_device_run(conv, case, torch.float32, edge_index=shared)), alone):
                assert torch.equal(a, b)
        # cold source plan: forward, drop every cached plan, backward
        ops, _, R = ac.inputs(case, torch.float32)
        leaf = {k: v.float().cuda().requires_grad_(True) for k, v in ops.items()}
        out = conv.edge_attention(leaf["q"], leaf["p"], leaf["att"], shared, case.n_dst, case.H, case.slope)
        gnnops.clear_plan_cache()
        (out * R.float().cuda()).sum().backward()
        for a, b in zip(snap(out, leaf), alone):
            assert torch.equal(a, b)
    finally:
        gnnops.set_plan_cache(True)


# ---- the layer ----------------------------------------------------------------------------------------------------------------
def test_state_dict_follows_pyg(conv):
    layer = conv.GATv2Conv(16, 32, heads=4, concat=False)
    state = layer.state_dict()
    assert {k: tuple(v.shape) for k, v in state.items()} == ac.PYG_STATE
    other = conv.GATv2Conv(16, 32, heads=4, concat=False)
    other.load_state_dict({k: torch.full_like(v, 0.5) for k, v in state.items()})       # a state_dict with PyG's key names loads
    assert float(other.att.min()) == 0.5
    assert tuple(conv.GATv2Conv(16, 32, heads=4).bias.shape) == (128,)
    shared = conv.GATv2Conv(16, 32, heads=4, share_weights=True)
    assert shared.lin_r is shared.lin_l and set(shared.state_dict()) == set(ac.PYG_STATE)
    assert "bias" not in conv.GATv2Conv(16, 32, bias=False).state_dict() and conv.GATv2Conv(16, 32, bias=False).lin_l.bias is None


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("lc", ac.LAYER_CASES, ids=[c.name for c in ac.LAYER_CASES])
def test_layer_forward_and_gradients(conv, lc, dtype):
    from conv_chain import _compare

    layer, inputs, _, run_dev, run_ref, _ = lc.setup(dtype)
    _compare(layer.cuda(), run_dev, lambda P, **kw: run_ref(P, **kw), inputs, ac.PROJECT_BAR[dtype])


def test_one_optimiser_step(conv):
    """GATv2Conv(16, 32, heads=4, concat=False): one SGD step on the device against the same step on the float64 restatement,
    compared on the updated parameters."""
    lc = ac.LAYER_CASES[1]
    assert (lc.cin, lc.cout, lc.heads, lc.concat) == (16, 32, 4, False)
    layer, inputs, _, run_dev, run_ref, shape = lc.setup(torch.float32)
    layer = layer.cuda()
    P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in layer.named_parameters()}
    coef = ac._rand(torch.Generator().manual_seed(99), *shape)
    opt = torch.optim.SGD(layer.parameters(), lr=0.5)
    ref_opt = torch.optim.SGD(list(P.values()), lr=0.5)
    (run_dev(layer, inputs["x"].cuda()) * coef.cuda()).sum().backward()
    (run_ref(P, inputs["x"].double()) * coef.double()).sum().backward()
    opt.step()
    ref_opt.step()
    for k, v in layer.named_parameters():
        err = ac.rel_err(v.detach().double().cpu(), P[k].detach())
        moved = float((P[k].grad * 0.5).abs().max())
        print(f"{k}: {err:.3e} after a step of at most {moved:.3e}")
        assert moved > 1e-3, k                                   # the step is no rounding error
        assert err <= ac.PROJECT_BAR[torch.float32], (k, err)


def test_same_bits_on_two_runs(conv):
    lc = ac.LAYER_CASES[0]
    layer, inputs, _, run_dev, _, shape = lc.setup(torch.float32)
    layer = layer.cuda()
    coef = ac._rand(torch.Generator().manual_seed(99), *shape).cuda()
    runs = []
    for _ in range(2):
        layer.zero_grad(set_to_none=True)
        x = inputs["x"].cuda().requires_grad_(True)
        out = run_dev(layer, x)
        (out * coef).sum().backward()
        runs.append([out.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in layer.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_self_loop_cache_keeps_the_plans_warm(conv):
    """The augmented edge_index is kept per edge_index object and version: the second call hands the op the SAME tensor (so its
    plans hit); an in-place write to the caller's tensor, or set_plan_cache(False), rebuilds it."""
    import gnnops

    layer = conv.GATv2Conv(8, 4, heads=2).cuda()
    ei = torch.randint(0, 50, (2, 300), device="cuda")
    x = torch.rand(50, 8, device="cuda")
    with torch.no_grad():
        first = layer(x, ei)
        kept = layer._looped[3]
        assert torch.equal(kept.cpu(), ac.with_self_loops(ei.cpu(), 50))
        assert torch.equal(layer(x, ei), first) and layer._looped[3] is kept
        ei[0, 0] = (ei[0, 0] + 1) % 50
        layer(x, ei)
        assert layer._looped[3] is not kept
        gnnops.set_plan_cache(False)
        try:
            layer(x, ei)
            assert layer._looped is None
        finally:
            gnnops.set_plan_cache(True)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(conv):
    q, p, att = torch.rand(10, 8), torch.rand(10, 8), torch.rand(8)
    ei = torch.randint(0, 10, (2, 30))
    with pytest.raises(RuntimeError, match="no CPU path"):
        conv.edge_attention(q, p, att, ei, 10, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        conv.GATv2Conv(8, 4, heads=2)(torch.rand(10, 8), ei)
    q, p, att, ei = q.cuda(), p.cuda(), att.cuda(), ei.cuda()
    with pytest.raises(RuntimeError, match="does not divide"):
        conv.edge_attention(q, p, att, ei, 10, 3)
    with pytest.raises(RuntimeError, match="edge_attention: q must be 2-D"):
        conv.edge_attention(q[:, :6], p, att, ei, 10, 2)                      # rows narrower than H * C
    wide = torch.rand(10, 8200, device="cuda")
    with pytest.raises(RuntimeError, match="8192"):
        conv.edge_attention(wide, wide, torch.rand(8200, device="cuda"), ei, 10, 2)
    layer = conv.GATv2Conv(8, 4, heads=2, dropout=0.1).cuda()
    with pytest.raises(NotImplementedError, match="dropout"):
        layer(torch.rand(10, 8, device="cuda"), ei)
    layer.eval()
    assert layer(torch.rand(10, 8, device="cuda"), ei).shape == (10, 8)
    with pytest.raises(RuntimeError, match="add_self_loops=False"):
        conv.GATv2Conv(8, 4, heads=2).cuda()((torch.rand(10, 8, device="cuda"), torch.rand(10, 8, device="cuda")), ei)


def test_widest_row(conv):
    """H * C = 8192 in one head: the 128-pieces-per-lane instance, against the chain."""
    g = torch.Generator().manual_seed(5)
    n, C = 6, 8192
    ei = torch.stack([torch.randint(0, n, (20,), generator=g), torch.randint(0, n - 1, (20,), generator=g)])
    ops = {"q": ac._rand(g, n, C).double(), "p": ac._rand(g, n, C).double(), "att": (ac._rand(g, C) / 64).double()}
    R = ac._rand(g, n, C).double()
    ops = {k: v.float().double() for k, v in ops.items()}
    want_out, want = ac.attention_grads(ops, ei, n, 1, 0.2, R.float().double())
    leaf = {k: v.float().cuda().requires_grad_(True) for k, v in ops.items()}
    out = conv.edge_attention(leaf["q"], leaf["p"], leaf["att"], ei.cuda(), n, 1)
    (out * R.float().cuda()).sum().backward()
    assert ac.rel_err(out.detach().double().cpu(), want_out) <= ac.PROJECT_BAR[torch.float32]
    for k, w in want.items():
        assert ac.rel_err(leaf[k].grad.double().cpu(), w) <= ac.PROJECT_BAR[torch.float32], k


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_gradient_layouts_autograd_hands_over(conv, dtype):
    """out.sum().backward() arrives as an expanded scalar (strides 0, 0), a consumer working on out.t() as a transposed gradient:
    the op and the concat=True layer take both, and give what a dense gradient of the same values gives, bit for bit."""
    case = ac.SHAPES[7]
    ops, ei, _ = ac.inputs(case, dtype)
    ei = ei.cuda()
    # eighths: the four-term sums of W's columns are exact in every type, whichever way a product orders them
    W = (torch.randint(-4, 5, (4, case.n_dst), generator=torch.Generator().manual_seed(3)).float() / 8).to(dtype).cuda()

    def grads(functional):
        leaf = {k: v.to(dtype).cuda().requires_grad_(True) for k, v in ops.items()}
        functional(conv.edge_attention(leaf["q"], leaf["p"], leaf["att"], ei, case.n_dst, case.H, case.slope)).backward()
        return [leaf[k].grad for k in ("q", "p", "att")]

    ones = torch.ones(case.n_dst, case.H * case.C, dtype=dtype, device="cuda")
    for a, b in zip(grads(lambda out: out.sum()), grads(lambda out: (out * ones).sum())):
        assert a is not None and torch.equal(a, b)
    dense_t = (W.t() @ torch.ones(4, case.H * case.C, dtype=dtype, device="cuda")).contiguous()
    for a, b in zip(grads(lambda out: (W @ out).sum()), grads(lambda out: (out * dense_t).sum())):
        assert torch.equal(a, b)
    for a, b in zip(grads(lambda out: (out.t() @ W.t()).sum()), grads(lambda out: (out * dense_t).sum())):
        assert torch.equal(a, b)
    want_out, want = ac.attention_grads(ops, ei.cpu(), case.n_dst, case.H, case.slope, torch.ones(case.n_dst, case.H * case.C, dtype=torch.float64))
    for k, got in zip(("q", "p", "att"), grads(lambda out: out.sum())):
        assert ac.rel_err(got.double().cpu(), want[k]) <= ac.PROJECT_BAR[dtype], k
    lc = ac.LAYER_CASES[0]
    assert lc.concat
    layer, inputs, _, run_dev, _, _ = lc.setup(dtype)
    layer = layer.cuda()
    x = inputs["x"].to(dtype).cuda().requires_grad_(True)
    run_dev(layer, x).sum().backward()
    first = [x.grad.clone()] + [p.grad.clone() for p in layer.parameters()]
    layer.zero_grad(set_to_none=True)
    x.grad = None
    out = run_dev(layer, x)
    (out * torch.ones_like(out)).sum().backward()
    for a, b in zip(first, [x.grad] + [p.grad for p in layer.parameters()]):
        assert torch.equal(a, b)
