"""gnnops.conv.edge_attention(..., u=) and gnnops.conv.GATv2Conv(edge_dim=) (csrc/attention.hip: the "has u" instances of
attention_fwd_kernel / attention_bwd_kernel) on the GPU against the float64 propagate-order chain of tests/attention_edge_chain.py
(tied to the older chain, a dense masked softmax, gradcheck and a hand-worked self-loop fill by test_attention_edge_chain_cpu.py): out,
and the gradients of a random linear functional sum(out * R) with respect to q, p, att and u, per tensor as max |got - want| / max |want|.
    shape    the SHAPES table of attention_chain.py: H in {1, 3, 4} x C in {1, 5, 8, 64, 136} x three types, dense and misaligned layouts
             (every pieces-per-lane instance and the single-element access path)
    seams    destinations with 0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65 and 129 edges: the steps of the halved unrolls, forward and backward,
             and the run of 64 edge ids; the edge list shuffled (perm no identity), and sorted by destination with perm = NULL
    range    scores of a destination hundreds apart          heavy    destinations with 8193 and 20 000 edges among ordinary rows
    edges    repeated edges and self loops; E = 0; a destination without edges
    widest   H * C = 8192 in one head; zero: u = 0 bit-identical to the call without u; two runs: the same bits
Bars: conv_chain.PROJECT_BAR (fp32 3e-5, fp16 1e-2) for the shape / seams / edges tables and the layers; 4 x the chain's distance from
itself (tests/golden/attention_edge_self_error.json) for bf16 and the range and heavy tables — the rule of test_attention_gpu.py."""
import pytest
import torch

import attention_chain as ac
import attention_edge_chain as ec
import chain_harness as ch

pytestmark = pytest.mark.gpu

SELF_ERROR = ec.load_self_error()
FAMILY = "v2"
_reference = ch.Reference(lambda case, dtype, sorted_edges: ec.case_grads(FAMILY, case, dtype, sorted_edges=sorted_edges))


@pytest.fixture(scope="module")
def conv():
    return ch.load_conv()


def _device_run(conv, case, dtype, sorted_edges=False, u="case"):
    ops, ei, R = ec.inputs_u(case, dtype, sorted_edges)
    leaf = {k: v.to(dtype).cuda().requires_grad_(True) for k, v in ops.items()}
    if u is None:
        del leaf["u"]
    elif u == "zero":
        leaf["u"] = torch.zeros_like(leaf["u"]).requires_grad_(True)
    q, p = ac.place(leaf["q"], case.layout), ac.place(leaf["p"], case.layout)
    out = conv.edge_attention(q, p, leaf["att"], ei.cuda(), case.n_dst, case.H, case.slope, u=leaf.get("u"))
    assert out.dtype == dtype and out.requires_grad and out.shape == (case.n_dst, case.H * case.C)
    (out.float() * R.to(dtype).cuda().float()).sum().backward()
    return out, leaf


def _run_case(conv, case, dtype, sorted_edges=False):
    want_out, want = _reference(case, dtype, sorted_edges)
    out, leaf = _device_run(conv, case, dtype, sorted_edges)
    assert set(leaf) == set(want) == {"q", "p", "att", "u"}
    ch.judge_case(case, dtype, "out", out, want_out, SELF_ERROR, key=ec.key(FAMILY, case, dtype, "out"))
    for k, w in want.items():
        ch.judge_case(case, dtype, k, leaf[k].grad, w, SELF_ERROR, key=ec.key(FAMILY, case, dtype, k))
    return out, leaf


@pytest.mark.parametrize("case,dtype", **ch.params(ec.V2["shape"]))
def test_shapes(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(ec.V2["seams"]))
def test_degree_seams(conv, case, dtype):
    out, _ = _run_case(conv, case, dtype)
    assert float(out[0].detach().abs().max()) == 0.0   # the destination without an edge


@pytest.mark.parametrize("case,dtype", **ch.params(ec.V2["seams"]))
def test_degree_seams_sorted_by_destination(conv, case, dtype):
    """The same edges sorted by destination. Through the plan (whose perm is then the identity in value), and through the raw
    launches with perm = NULL: the same bits."""
    out, leaf = _run_case(conv, case, dtype, sorted_edges=True)
    ops, ei, R = ec.inputs_u(case, dtype, sorted_edges=True)
    dev = {k: v.to(dtype).cuda() for k, v in ops.items()}
    ei = ei.cuda()
    with torch.no_grad():
        raw, lse = conv._attention_forward(dev["q"], dev["p"], dev["att"], ei, case.n_dst, case.H, case.slope, dev["u"], identity_perm=True)
        assert torch.equal(raw, out.detach())
        g = R.to(dtype).cuda()
        gq, d_p, d_att, d_u, _, _ = conv._attention_backward(dev["q"], dev["p"], dev["att"], dev["u"], ei, raw, lse, g, case.n_dst, case.H,
                                                             case.slope, identity_perm=True)
    assert torch.equal(d_p, leaf["p"].grad) and torch.equal(d_att, leaf["att"].grad) and torch.equal(d_u, leaf["u"].grad)


@pytest.mark.parametrize("case,dtype", **ch.params(ec.V2["range"]))
def test_online_rescale(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(ec.V2["heavy"]))
def test_heavy_destinations(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(ec.V2["edges"][:1]))
def test_repeated_edges_and_self_loops(conv, case, dtype):
    out, _ = _run_case(conv, case, dtype)
    assert float(out[3].detach().abs().max()) == 0.0   # destination 3 has no edge: a zero row
    ops, ei, _ = ec.inputs_u(case, dtype)
    dev = {k: v.to(dtype).cuda() for k, v in ops.items()}
    _, lse = conv._attention_forward(dev["q"], dev["p"], dev["att"], ei.cuda(), case.n_dst, case.H, case.slope, dev["u"])
    assert bool(torch.isneginf(lse[3]).all()) and bool(torch.isfinite(lse[4]).all())


@pytest.mark.parametrize("dtype", ec.DTYPES, ids=[ec.DNAME[d] for d in ec.DTYPES])
def test_no_edges(conv, dtype):
    case = ec.V2["edges"][1]
    assert case.E == 0
    out, leaf = _device_run(conv, case, dtype)
    assert float(out.abs().max()) == 0.0
    for k, v in leaf.items():
        assert v.grad is not None and v.grad.shape == v.shape and float(v.grad.abs().sum()) == 0.0, k
    assert leaf["u"].grad.shape == (0, case.H * case.C)
    ops, ei, _ = ec.inputs_u(case, dtype)
    dev = {k: v.to(dtype).cuda() for k, v in ops.items()}
    _, lse = conv._attention_forward(dev["q"], dev["p"], dev["att"], ei.cuda(), case.n_dst, case.H, case.slope, dev["u"])
    assert lse.shape == (case.n_dst, case.H) and bool(torch.isneginf(lse).all())


def test_widest_row(conv):
    """H * C = 8192 in one head with u: the 128-pieces-per-lane instance, against the chain."""
    g = torch.Generator().manual_seed(5)
    n, C, e = 6, 8192, 20
    ei = torch.stack([torch.randint(0, n, (e,), generator=g), torch.randint(0, n - 1, (e,), generator=g)])
    ops = {"q": ec._rand(g, n, C), "p": ec._rand(g, n, C), "att": ec._rand(g, C) / 64, "u": ec._rand(g, e, C)}
    R = ec._rand(g, n, C).double()
    ops = {k: v.float().double() for k, v in ops.items()}
    want_out, want = ec.attention_u_grads(ops, ei, n, 1, 0.2, R)
    leaf = {k: v.float().cuda().requires_grad_(True) for k, v in ops.items()}
    out = conv.edge_attention(leaf["q"], leaf["p"], leaf["att"], ei.cuda(), n, 1, u=leaf["u"])
    (out * R.float().cuda()).sum().backward()
    assert ec.rel_err(out.detach().double().cpu(), want_out) <= ec.PROJECT_BAR[torch.float32]
    for k, w in want.items():
        assert ec.rel_err(leaf[k].grad.double().cpu(), w) <= ec.PROJECT_BAR[torch.float32], k


ZERO_CASES = [ec.V2["shape"][7], ec.V2["shape"][4], ec.V2["seams"][2], ec.V2["shape"][-1], ec.V2["heavy"][0]]


@pytest.mark.parametrize("case,dtype", **ch.params(ZERO_CASES))
def test_zero_u_is_the_call_without_u(conv, case, dtype):
    a_out, a = _device_run(conv, case, dtype, u=None)
    b_out, b = _device_run(conv, case, dtype, u="zero")
    assert torch.equal(a_out, b_out)
    for k in ("q", "p", "att"):
        assert torch.equal(a[k].grad, b[k].grad), k
    assert b["u"].grad is not None and b["u"].grad.shape == b["u"].shape


def test_same_bits_on_two_runs(conv):
    for case in (ec.V2["heavy"][1], ec.V2["shape"][7], ec.V2["seams"][2]):
        a_out, a = _device_run(conv, case, torch.float32)
        b_out, b = _device_run(conv, case, torch.float32)
        assert torch.equal(a_out, b_out)
        for k in a:
            assert torch.equal(a[k].grad, b[k].grad), k


def test_u_alone_requiring_grad_goes_through_autograd(conv):
    case = ec.V2["shape"][7]
    ops, ei, R = ec.inputs_u(case, torch.float32)
    dev = {k: v.float().cuda() for k, v in ops.items()}
    u = dev["u"].clone().requires_grad_(True)
    out = conv.edge_attention(dev["q"], dev["p"], dev["att"], ei.cuda(), case.n_dst, case.H, case.slope, u=u)
    assert out.requires_grad
    (out * R.float().cuda()).sum().backward()
    _, want = _reference(case, torch.float32, False)
    assert ec.rel_err(u.grad.double().cpu(), want["u"]) <= ec.PROJECT_BAR[torch.float32]
    with torch.no_grad():
        assert not conv.edge_attention(dev["q"], dev["p"], dev["att"], ei.cuda(), case.n_dst, case.H, case.slope, u=dev["u"]).requires_grad


# ---- the layer ----------------------------------------------------------------------------------------------------------------
V2_LAYERS = [c for c in ec.LAYER_CASES if c.kind == "gatv2"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("lc", V2_LAYERS, ids=[c.name for c in V2_LAYERS])
def test_layer_forward_and_gradients(conv, lc, dtype):
    from conv_chain import _compare

    layer, inputs, _, run_dev, run_ref, _ = lc.setup(dtype)
    _compare(layer.cuda(), run_dev, lambda P, **kw: run_ref(P, **kw), inputs, ec.PROJECT_BAR[dtype])


def test_one_optimiser_step(conv):
    """GATv2Conv(16, 32, heads=4, concat=False, edge_dim=3): one SGD step on the device against the same step on the float64
    restatement, compared on the updated parameters."""
    lc = V2_LAYERS[1]
    layer, inputs, _, run_dev, run_ref, shape = lc.setup(torch.float32)
    layer = layer.cuda()
    P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in layer.named_parameters()}
    assert "lin_edge.weight" in P
    coef = ec._rand(torch.Generator().manual_seed(99), *shape)
    opt = torch.optim.SGD(layer.parameters(), lr=0.5)
    ref_opt = torch.optim.SGD(list(P.values()), lr=0.5)
    (run_dev(layer, inputs["x"].cuda(), inputs["ea"].cuda()) * coef.cuda()).sum().backward()
    (run_ref(P, inputs["x"].double(), inputs["ea"].double()) * coef.double()).sum().backward()
    opt.step()
    ref_opt.step()
    for k, v in layer.named_parameters():
        err = ec.rel_err(v.detach().double().cpu(), P[k].detach())
        moved = float((P[k].grad * 0.5).abs().max())
        print(f"{k}: {err:.3e} after a step of at most {moved:.3e}")
        assert moved > 1e-3, k                                   # the step is no rounding error
        assert err <= ec.PROJECT_BAR[torch.float32], (k, err)


def test_state_dict_follows_pyg(conv):
    layer = conv.GATv2Conv(16, 32, heads=4, concat=False, edge_dim=3)
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == ec.GATV2_EDGE_STATE
    assert layer.lin_edge.bias is None
    bound = (6.0 / (3 + 128)) ** 0.5                             # glorot
    assert float(layer.lin_edge.weight.abs().max()) <= bound and float(layer.lin_edge.weight.abs().max()) > 0.5 * bound
    plain = conv.GATv2Conv(16, 32, heads=4, concat=False)
    assert {k: tuple(v.shape) for k, v in plain.state_dict().items()} == ac.PYG_STATE and not hasattr(plain, "lin_edge")


def test_self_loop_attributes_and_cache(conv):
    """The augmented index stays cached across calls with edge features; the attributes are rebuilt per call from edge_attr."""
    layer = conv.GATv2Conv(8, 4, heads=2, edge_dim=2).cuda()
    ei = torch.randint(0, 50, (2, 300), device="cuda")
    x, ea = torch.rand(50, 8, device="cuda"), torch.rand(300, 2, device="cuda")
    with torch.no_grad():
        first = layer(x, ei, ea)
        kept = layer._looped[3]
        assert torch.equal(kept.cpu(), ac.with_self_loops(ei.cpu(), 50))
        assert torch.equal(layer(x, ei, ea), first) and layer._looped[3] is kept
        assert not torch.equal(layer(x, ei, ea * 2), first)
    rows = layer._edge_rows(ea, ei, 50, True)
    assert ec.rel_err(rows.double().cpu(), ec.looped_attr(ei.cpu(), ea.double().cpu(), 50, "mean")) <= 1e-6


def test_refusals(conv):
    ei = torch.randint(0, 10, (2, 30), device="cuda")
    x, ea = torch.rand(10, 8, device="cuda"), torch.rand(30, 3, device="cuda")
    with pytest.raises(ValueError, match="fill_value"):
        conv.GATv2Conv(8, 4, heads=2, edge_dim=3, fill_value="max")
    layer = conv.GATv2Conv(8, 4, heads=2, edge_dim=3).cuda()
    with pytest.raises(RuntimeError, match="needs edge_attr"):
        layer(x, ei)
    with pytest.raises(RuntimeError, match="without edge_dim"):
        conv.GATv2Conv(8, 4, heads=2).cuda()(x, ei, ea)
    with pytest.raises(RuntimeError, match="edge_attr must be"):
        layer(x, ei, ea[:29])
    with pytest.raises(RuntimeError, match="edge_attr must be"):
        layer(x, ei, ea[:, :2])
    with pytest.raises(RuntimeError, match="no CPU path"):
        layer(x, ei, ea.cpu())
    assert layer(x, ei, ea).shape == (10, 8)
    q, p, att = torch.rand(10, 8, device="cuda"), torch.rand(10, 8, device="cuda"), torch.rand(8, device="cuda")
    with pytest.raises(RuntimeError, match="edge_attention: u must be"):
        conv.edge_attention(q, p, att, ei, 10, 2, u=torch.rand(29, 8, device="cuda"))
    with pytest.raises(RuntimeError, match="edge_attention: u must be"):
        conv.edge_attention(q, p, att, ei, 10, 2, u=torch.rand(30, 4, device="cuda"))
    with pytest.raises(RuntimeError, match="same dtype"):
        conv.edge_attention(q, p, att, ei, 10, 2, u=torch.rand(30, 8, device="cuda").half())
    with pytest.raises(RuntimeError, match="no CPU path"):
        conv.edge_attention(q, p, att, ei, 10, 2, u=torch.rand(30, 8))


def test_gateconv_still_runs(conv):
    import gate_chain as gc
    from conv_chain import _compare

    lc = next(c for c in gc.LAYER_CASES if c.name == "gate-edge_dim3")
    layer, inputs, _, run_dev, run_ref = lc.setup(torch.float32)
    _compare(layer.cuda(), run_dev, lambda P, **kw: run_ref(P, **kw), inputs, gc.PROJECT_BAR[torch.float32])
