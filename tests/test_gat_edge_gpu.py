"""gnnops.conv.edge_attention_v1(..., edge_score=) and gnnops.conv.GATConv(edge_dim=) (csrc/attention.hip: the "has c" instances of
gate_fwd_kernel / gate_bwd_kernel) on the GPU against the float64 propagate-order chain of tests/attention_edge_chain.py: out, and the
gradients of a random linear functional sum(out * R) with respect to q, d, att and edge_score, per tensor as max |got - want| / max |want|.
The tables, the degree seams (shuffled, and sorted by destination with perm = NULL), the zero-term and two-run checks and the bars are those
of test_attention_edge_gpu.py, on the second family of the attention pass."""
import pytest
import torch

import attention_edge_chain as ec
import chain_harness as ch
import gate_chain as gc

pytestmark = pytest.mark.gpu

SELF_ERROR = ec.load_self_error()
FAMILY = "v1"
_reference = ch.Reference(lambda case, dtype, sorted_edges: ec.case_grads(FAMILY, case, dtype, sorted_edges=sorted_edges))


@pytest.fixture(scope="module")
def conv():
    return ch.load_conv()


def _device_run(conv, case, dtype, sorted_edges=False, c="case"):
    ops, ei, R = ec.inputs_c(case, dtype, sorted_edges)
    leaf = {k: v.to(dtype).cuda().requires_grad_(True) for k, v in ops.items()}
    if c is None:
        del leaf["c"]
    elif c == "zero":
        leaf["c"] = torch.zeros_like(leaf["c"]).requires_grad_(True)
    q, d = gc.place(leaf["q"], case.layout), gc.place(leaf["d"], case.layout)
    out = conv.edge_attention_v1(q, d, leaf["att"], ei.cuda(), case.n_dst, case.H, negative_slope=case.slope, edge_score=leaf.get("c"))
    assert out.dtype == dtype and out.requires_grad and out.shape == (case.n_dst, case.H * case.C)
    (out.float() * R.to(dtype).cuda().float()).sum().backward()
    return out, leaf


def _run_case(conv, case, dtype, sorted_edges=False):
    want_out, want = _reference(case, dtype, sorted_edges)
    out, leaf = _device_run(conv, case, dtype, sorted_edges)
    assert set(leaf) == set(want) == {"q", "d", "att", "c"}
    ch.judge_case(case, dtype, "out", out, want_out, SELF_ERROR, key=ec.key(FAMILY, case, dtype, "out"))
    for k, w in want.items():
        ch.judge_case(case, dtype, k, leaf[k].grad, w, SELF_ERROR, key=ec.key(FAMILY, case, dtype, k))
    return out, leaf


@pytest.mark.parametrize("case,dtype", **ch.params(ec.V1["shape"]))
def test_shapes(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(ec.V1["seams"]))
def test_degree_seams(conv, case, dtype):
    out, _ = _run_case(conv, case, dtype)
    assert float(out[0].detach().abs().max()) == 0.0   # the destination without an edge


@pytest.mark.parametrize("case,dtype", **ch.params(ec.V1["seams"]))
def test_degree_seams_sorted_by_destination(conv, case, dtype):
    """The same edges sorted by destination, through the plan and through the raw launches with perm = NULL: the same bits."""
    out, leaf = _run_case(conv, case, dtype, sorted_edges=True)
    ops, ei, R = ec.inputs_c(case, dtype, sorted_edges=True)
    dev = {k: v.to(dtype).cuda() for k, v in ops.items()}
    ei = ei.cuda()
    with torch.no_grad():
        raw, lse = conv._v1_forward(dev["q"], dev["d"], dev["att"], ei, case.n_dst, case.H, None, None, case.slope, None, dev["c"], identity_perm=True)
        assert torch.equal(raw, out.detach())
        g = R.to(dtype).cuda()
        _, d_d, d_att, d_c, _, _ = conv._v1_backward(dev["q"], dev["d"], dev["att"], None, dev["c"], None, ei, raw, lse, g, case.n_dst, case.H,
                                                     None, case.slope, identity_perm=True)
    assert torch.equal(d_d, leaf["d"].grad) and torch.equal(d_att, leaf["att"].grad) and torch.equal(d_c, leaf["c"].grad)


@pytest.mark.parametrize("case,dtype", **ch.params(ec.V1["range"]))
def test_online_rescale(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(ec.V1["heavy"]))
def test_heavy_destinations(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(ec.V1["edges"][:1]))
def test_repeated_edges_and_self_loops(conv, case, dtype):
    out, _ = _run_case(conv, case, dtype)
    assert float(out[3].detach().abs().max()) == 0.0   # destination 3 has no edge: a zero row


@pytest.mark.parametrize("dtype", ec.DTYPES, ids=[ec.DNAME[d] for d in ec.DTYPES])
def test_no_edges(conv, dtype):
    case = ec.V1["edges"][1]
    assert case.E == 0
    out, leaf = _device_run(conv, case, dtype)
    assert float(out.detach().abs().max()) == 0.0
    for k, v in leaf.items():
        assert v.grad is not None and v.grad.shape == v.shape and float(v.grad.abs().sum()) == 0.0, k
    assert leaf["c"].grad.shape == (0, case.H)
    ops, ei, _ = ec.inputs_c(case, dtype)
    dev = {k: v.to(dtype).cuda() for k, v in ops.items()}
    _, lse = conv._v1_forward(dev["q"], dev["d"], dev["att"], ei.cuda(), case.n_dst, case.H, None, None, case.slope, None, dev["c"])
    assert lse.shape == (case.n_dst, case.H) and bool(torch.isneginf(lse).all())


def test_widest_row(conv):
    """H * C = 8192 in one head with the edge term: the 128-pieces-per-lane instance, against the chain."""
    g = torch.Generator().manual_seed(5)
    n, C, e = 6, 8192, 20
    ei = torch.stack([torch.randint(0, n, (e,), generator=g), torch.randint(0, n - 1, (e,), generator=g)])
    ops = {"q": ec._rand(g, n, C), "d": ec._rand(g, n, 1), "att": ec._rand(g, C) / 64, "c": ec._rand(g, e, 1)}
    R = ec._rand(g, n, C).double()
    ops = {k: v.float().double() for k, v in ops.items()}
    want_out, want = ec.attention_c_grads(ops, ei, n, 1, 0.2, R)
    leaf = {k: v.float().cuda().requires_grad_(True) for k, v in ops.items()}
    out = conv.edge_attention_v1(leaf["q"], leaf["d"], leaf["att"], ei.cuda(), n, 1, edge_score=leaf["c"])
    (out * R.float().cuda()).sum().backward()
    assert ec.rel_err(out.detach().double().cpu(), want_out) <= ec.PROJECT_BAR[torch.float32]
    for k, w in want.items():
        assert ec.rel_err(leaf[k].grad.double().cpu(), w) <= ec.PROJECT_BAR[torch.float32], k


ZERO_CASES = [ec.V1["shape"][7], ec.V1["shape"][4], ec.V1["seams"][2], ec.V1["shape"][-1], ec.V1["heavy"][0]]


@pytest.mark.parametrize("case,dtype", **ch.params(ZERO_CASES))
def test_zero_edge_score_is_the_call_without_it(conv, case, dtype):
    a_out, a = _device_run(conv, case, dtype, c=None)
    b_out, b = _device_run(conv, case, dtype, c="zero")
    assert torch.equal(a_out, b_out)
    for k in ("q", "d", "att"):
        assert torch.equal(a[k].grad, b[k].grad), k
    assert b["c"].grad is not None and b["c"].grad.shape == b["c"].shape


def test_same_bits_on_two_runs(conv):
    for case in (ec.V1["heavy"][1], ec.V1["shape"][7], ec.V1["seams"][2]):
        a_out, a = _device_run(conv, case, torch.float32)
        b_out, b = _device_run(conv, case, torch.float32)
        assert torch.equal(a_out, b_out)
        for k in a:
            assert torch.equal(a[k].grad, b[k].grad), k


def test_edge_score_alone_requiring_grad_goes_through_autograd(conv):
    case = ec.V1["shape"][7]
    ops, ei, R = ec.inputs_c(case, torch.float32)
    dev = {k: v.float().cuda() for k, v in ops.items()}
    c = dev["c"].clone().requires_grad_(True)
    out = conv.edge_attention_v1(dev["q"], dev["d"], dev["att"], ei.cuda(), case.n_dst, case.H, negative_slope=case.slope, edge_score=c)
    assert out.requires_grad
    (out * R.float().cuda()).sum().backward()
    _, want = _reference(case, torch.float32, False)
    assert ec.rel_err(c.grad.double().cpu(), want["c"]) <= ec.PROJECT_BAR[torch.float32]


# ---- the layer ----------------------------------------------------------------------------------------------------------------
V1_LAYERS = [c for c in ec.LAYER_CASES if c.kind == "gat"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("lc", V1_LAYERS, ids=[c.name for c in V1_LAYERS])
def test_layer_forward_and_gradients(conv, lc, dtype):
    from conv_chain import _compare

    layer, inputs, _, run_dev, run_ref, _ = lc.setup(dtype)
    _compare(layer.cuda(), run_dev, lambda P, **kw: run_ref(P, **kw), inputs, ec.PROJECT_BAR[dtype])


def test_one_optimiser_step(conv):
    """GATConv(16, 32, heads=4, concat=False, edge_dim=3): one SGD step on the device against the same step on the float64
    restatement, compared on the updated parameters."""
    lc = V1_LAYERS[1]
    layer, inputs, _, run_dev, run_ref, shape = lc.setup(torch.float32)
    layer = layer.cuda()
    P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in layer.named_parameters()}
    assert "lin_edge.weight" in P and "att_edge" in P
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
    layer = conv.GATConv(16, 32, heads=4, concat=False, edge_dim=3)
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == ec.GAT_EDGE_STATE
    assert layer.lin_edge.bias is None
    plain = conv.GATConv(16, 32, heads=4, concat=False)
    assert {k: tuple(v.shape) for k, v in plain.state_dict().items()} == gc.GAT_STATE
    assert not hasattr(plain, "lin_edge") and not hasattr(plain, "att_edge")


def test_refusals(conv):
    ei = torch.randint(0, 10, (2, 30), device="cuda")
    x, ea = torch.rand(10, 8, device="cuda"), torch.rand(30, 3, device="cuda")
    with pytest.raises(ValueError, match="fill_value"):
        conv.GATConv(8, 4, heads=2, edge_dim=3, fill_value="add")
    layer = conv.GATConv(8, 4, heads=2, edge_dim=3).cuda()
    with pytest.raises(RuntimeError, match="needs edge_attr"):
        layer(x, ei)
    with pytest.raises(RuntimeError, match="without edge_dim"):
        conv.GATConv(8, 4, heads=2).cuda()(x, ei, ea)
    with pytest.raises(RuntimeError, match="edge_attr must be"):
        layer(x, ei, ea[:29])
    with pytest.raises(RuntimeError, match="edge_attr must be"):
        layer(x, ei, ea[:, :2])
    assert layer(x, ei, ea).shape == (10, 8)
    q, d, att = torch.rand(10, 8, device="cuda"), torch.rand(10, 2, device="cuda"), torch.rand(8, device="cuda")
    with pytest.raises(RuntimeError, match="edge_attention_v1: edge_score must be"):
        conv.edge_attention_v1(q, d, att, ei, 10, 2, edge_score=torch.rand(30, 1, device="cuda"))
    with pytest.raises(RuntimeError, match="same dtype"):
        conv.edge_attention_v1(q, d, att, ei, 10, 2, edge_score=torch.rand(30, 2, device="cuda").half())
    with pytest.raises(NotImplementedError, match="together"):
        conv.edge_attention_v1(q, d, att, ei, 10, 2, u=torch.rand(30, 8, device="cuda"), edge_score=torch.rand(30, 2, device="cuda"))


def test_gateconv_still_runs(conv):
    from conv_chain import _compare

    lc = next(c for c in gc.LAYER_CASES if c.name == "gate-edge_dim1")
    layer, inputs, _, run_dev, run_ref = lc.setup(torch.float32)
    _compare(layer.cuda(), run_dev, lambda P, **kw: run_ref(P, **kw), inputs, gc.PROJECT_BAR[torch.float32])
