"""gnnops.conv.edge_attention_v1 and the layers on it — GATConv, GATEConv, AttentiveFP (csrc/attention.hip: gate_fwd_kernel /
gate_bwd_kernel) — on the GPU against the float64 propagate-order chain of tests/gate_chain.py (tied to a dense masked softmax,
gradcheck and a hand-worked example by test_gate_chain_cpu.py): out, and the gradients of a random linear functional sum(out * R) with
respect to q, d, att and u, per tensor as max |got - want| / max |want|.
    shape    H in {1, 3, 4} x C in {1, 5, 8, 64, 136} x three types x {u absent / present} x {row_slope None / 0.01}; 257 sources ->
             300 destinations, q and d as column blocks of a wider matrix (one case dense, four off 16 bytes: 2 and 4 pieces per lane)
    seams    destinations with 0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65 and 129 edges in one graph: U - 1, U, U + 1 of every unroll of the
             new kernels (8, 4, 2, 1) and the run of 64 edge ids
    range    scores of a destination hundreds apart, rows whose scores strictly ascend, strictly descend, and are all equal
    heavy    destinations with 8193 and 20 000 edges among ordinary rows
    mask     edge_scale with one destination's edges ALL dropped; a mask of ones bit-equal to no mask
    plan     E = 24576 / 24577; cache on and off; a backward whose source plan is built cold
    edges    repeated edges and self loops; E = 0
Bars: conv_chain.PROJECT_BAR (fp32 3e-5, fp16 1e-2) for the shape / seams / plan / edges tables and the layers; 4 x the chain's
distance from itself (tests/golden/gate_attention_self_error.json) for bf16 and the range, heavy and mask tables."""
import pytest
import torch

import chain_harness as ch
import gate_chain as gc

pytestmark = pytest.mark.gpu

SELF_ERROR = gc.load_self_error()
_reference = ch.Reference(gc.case_grads)


@pytest.fixture(scope="module")
def conv():
    return ch.load_conv()


def _call(conv, case, leaf, ei, ks, layout=None):
    layout = case.layout if layout is None else layout
    q, d = gc.place(leaf["q"], layout), gc.place(leaf["d"], layout)
    return conv.edge_attention_v1(q, d, leaf["att"], ei, case.n_dst, case.H, u=leaf.get("u"), row_slope=case.row_slope,
                                  negative_slope=case.slope, edge_scale=ks)


def _device_run(conv, case, dtype, edge_index=None, edge_scale="case"):
    ops, ei, R, ks = gc.inputs(case, dtype)
    leaf = {k: v.to(dtype).cuda().requires_grad_(True) for k, v in ops.items()}
    if edge_scale == "case":
        edge_scale = None if ks is None else ks.to(dtype).cuda()
    out = _call(conv, case, leaf, ei.cuda() if edge_index is None else edge_index, edge_scale)
    assert out.dtype == dtype and out.requires_grad and out.shape == (case.n_dst, case.H * case.C)
    (out.float() * R.to(dtype).cuda().float()).sum().backward()
    return out, leaf


def _run_case(conv, case, dtype):
    want_out, want = _reference(case, dtype)
    out, leaf = _device_run(conv, case, dtype)
    assert set(leaf) == set(want)
    ch.judge_case(case, dtype, "out", out, want_out, SELF_ERROR)
    for k, w in want.items():
        ch.judge_case(case, dtype, k, leaf[k].grad, w, SELF_ERROR)
    return out, leaf


@pytest.mark.parametrize("case,dtype", **ch.params(gc.SHAPES))
def test_shapes(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(gc.SEAMS))
def test_degree_seams(conv, case, dtype):
    out, _ = _run_case(conv, case, dtype)
    assert float(out[0].detach().abs().max()) == 0.0   # the destination without an edge


@pytest.mark.parametrize("case,dtype", **ch.params(gc.RANGE))
def test_online_rescale(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(gc.HEAVY))
def test_heavy_destinations(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(gc.MASK))
def test_edge_scale_with_a_dead_destination(conv, case, dtype):
    out, leaf = _run_case(conv, case, dtype)
    assert float(out[gc.MASK_DEAD_DST].detach().abs().max()) == 0.0       # every edge dropped: exactly zero
    assert all(bool(torch.isfinite(v.grad).all()) for v in leaf.values())


@pytest.mark.parametrize("case,dtype", **ch.params(gc.MASK))
def test_mask_of_ones_is_no_mask(conv, case, dtype):
    _, ei, _, _ = gc.inputs(case, dtype)
    ones = torch.ones(ei.size(1), case.H, dtype=dtype, device="cuda")
    a_out, a = _device_run(conv, case, dtype, edge_scale=None)
    b_out, b = _device_run(conv, case, dtype, edge_scale=ones)
    assert torch.equal(a_out, b_out)
    for k in a:
        assert torch.equal(a[k].grad, b[k].grad), k


@pytest.mark.parametrize("case,dtype", **ch.params(gc.PLAN))
def test_both_sides_of_the_one_launch_plan(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(gc.EDGES[:1]))
def test_repeated_edges_and_self_loops(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("dtype", gc.DTYPES, ids=[gc.DNAME[d] for d in gc.DTYPES])
def test_no_edges(conv, dtype):
    case = gc.EDGES[1]
    assert case.E == 0 and case.has_u
    out, leaf = _device_run(conv, case, dtype)
    assert float(out.detach().abs().max()) == 0.0
    for k, v in leaf.items():
        assert v.grad is not None and v.grad.shape == v.shape and float(v.grad.abs().sum()) == 0.0, k
    assert leaf["u"].grad.shape == (0, case.H * case.C)
    ops, ei, _, _ = gc.inputs(case, dtype)
    dev = {k: v.to(dtype).cuda() for k, v in ops.items()}
    _, lse = conv._v1_forward(dev["q"], dev["d"], dev["att"], ei.cuda(), case.n_dst, case.H, dev["u"], case.row_slope, case.slope, None)
    assert lse.shape == (case.n_dst, case.H) and lse.dtype == torch.float32 and bool(torch.isneginf(lse).all())


def test_lse_is_written(conv):
    case = gc.SEAMS[1]
    ops, ei, _, _ = gc.inputs(case, torch.float32)
    dev = {k: v.float().cuda() for k, v in ops.items()}
    _, lse = conv._v1_forward(dev["q"], dev["d"], dev["att"], ei.cuda(), case.n_dst, case.H, dev.get("u"), case.row_slope, case.slope, None)
    _, want = gc.attention_v1(ops["q"], ops["d"], ops["att"], ei, case.n_dst, case.H, ops.get("u"), case.row_slope, case.slope)
    assert bool(torch.isneginf(lse[0]).all())
    assert gc.rel_err(lse[1:].double().cpu(), want[1:]) <= gc.PROJECT_BAR[torch.float32]


def test_raw_call_when_nothing_requires_grad(conv):
    case = gc.SHAPES[0]
    ops, ei, _, _ = gc.inputs(case, torch.float32)
    dev = {k: v.float().cuda() for k, v in ops.items()}
    out = _call(conv, case, dev, ei.cuda(), None)
    assert not out.requires_grad and out.grad_fn is None


@pytest.mark.parametrize("cache", [True, False], ids=["cache_on", "cache_off"])
@pytest.mark.parametrize("case", gc.PLAN, ids=[c.name for c in gc.PLAN])
def test_plan_routes(conv, case, cache):
    """Forward then backward over one edge_index object, twice (cold, then from the cache); and a backward whose source plan is
    built cold (the caches cleared between forward and backward): every tensor bit-equal to the run on a fresh edge_index."""
    import gnnops

    ops, ei, R, _ = gc.inputs(case, torch.float32)
    snap = lambda out, leaf: [out.detach().clone()] + [v.grad.clone() for v in leaf.values()]   # noqa: E731
    gnnops.set_plan_cache(cache)
    try:
        alone = snap(*_device_run(conv, case, torch.float32))
        shared = ei.cuda()
        for _ in range(2):
            for a, b in zip(snap(*_device_run(conv, case, torch.float32, edge_index=shared)), alone):
                assert torch.equal(a, b)
        leaf = {k: v.float().cuda().requires_grad_(True) for k, v in ops.items()}
        out = _call(conv, case, leaf, shared, None)
        gnnops.clear_plan_cache()
        (out * R.float().cuda()).sum().backward()
        for a, b in zip(snap(out, leaf), alone):
            assert torch.equal(a, b)
    finally:
        gnnops.set_plan_cache(True)


def test_same_bits_on_two_runs(conv):
    for case in (gc.HEAVY[1], gc.SHAPES[7]):
        a_out, a = _device_run(conv, case, torch.float32)
        b_out, b = _device_run(conv, case, torch.float32)
        assert torch.equal(a_out, b_out)
        for k in a:
            assert torch.equal(a[k].grad, b[k].grad), k


def test_widest_row(conv):
    """H * C = 8192 in one head: the 128-pieces-per-lane instance with u, against the chain."""
    g = torch.Generator().manual_seed(5)
    n, C, e = 6, 8192, 20
    ei = torch.stack([torch.randint(0, n, (e,), generator=g), torch.randint(0, n - 1, (e,), generator=g)])
    ops = {"q": gc._rand(g, n, C), "d": gc._rand(g, n, 1), "att": gc._rand(g, C) / 64, "u": gc._rand(g, e, C)}
    R = gc._rand(g, n, C).double()
    ops = {k: v.float().double() for k, v in ops.items()}
    want_out, want = gc.attention_grads(ops, ei, n, 1, 0.01, 0.2, None, R)
    leaf = {k: v.float().cuda().requires_grad_(True) for k, v in ops.items()}
    out = conv.edge_attention_v1(leaf["q"], leaf["d"], leaf["att"], ei.cuda(), n, 1, u=leaf["u"], row_slope=0.01)
    (out * R.float().cuda()).sum().backward()
    assert gc.rel_err(out.detach().double().cpu(), want_out) <= gc.PROJECT_BAR[torch.float32]
    for k, w in want.items():
        assert gc.rel_err(leaf[k].grad.double().cpu(), w) <= gc.PROJECT_BAR[torch.float32], k


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_gradient_layouts_autograd_hands_over(conv, dtype):
    """out.sum().backward() arrives as an expanded scalar (strides 0, 0), a consumer working on out.t() as a transposed gradient:
    the op takes both, and gives what a dense gradient of the same values gives, bit for bit."""
    case = next(c for c in gc.SHAPES if (c.H, c.C, c.variant) == (3, 8, "gate"))
    ops, ei, _, _ = gc.inputs(case, dtype)
    ei = ei.cuda()
    W = (torch.randint(-4, 5, (4, case.n_dst), generator=torch.Generator().manual_seed(3)).float() / 8).to(dtype).cuda()

    def grads(functional):
        leaf = {k: v.to(dtype).cuda().requires_grad_(True) for k, v in ops.items()}
        functional(_call(conv, case, leaf, ei, None, layout="plain")).backward()
        return [leaf[k].grad for k in ("q", "d", "att", "u")]

    ones = torch.ones(case.n_dst, case.H * case.C, dtype=dtype, device="cuda")
    for a, b in zip(grads(lambda out: out.sum()), grads(lambda out: (out * ones).sum())):
        assert a is not None and torch.equal(a, b)
    dense_t = (W.t() @ torch.ones(4, case.H * case.C, dtype=dtype, device="cuda")).contiguous()
    for a, b in zip(grads(lambda out: (W @ out).sum()), grads(lambda out: (out * dense_t).sum())):
        assert torch.equal(a, b)
    for a, b in zip(grads(lambda out: (out.t() @ W.t()).sum()), grads(lambda out: (out * dense_t).sum())):
        assert torch.equal(a, b)
    _, want = gc.attention_grads(ops, ei.cpu(), case.n_dst, case.H, case.row_slope, case.slope, None,
                                 torch.ones(case.n_dst, case.H * case.C, dtype=torch.float64))
    for k, got in zip(("q", "d", "att", "u"), grads(lambda out: out.sum())):
        assert gc.rel_err(got.double().cpu(), want[k]) <= gc.PROJECT_BAR[dtype], k


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(conv):
    q, d, att = torch.rand(10, 8), torch.rand(10, 2), torch.rand(8)
    ei = torch.randint(0, 10, (2, 30))
    with pytest.raises(RuntimeError, match="no CPU path"):
        conv.edge_attention_v1(q, d, att, ei, 10, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        conv.GATConv(8, 4, heads=2)(torch.rand(10, 8), ei)
    with pytest.raises(RuntimeError, match="no CPU path"):
        conv.GATEConv(8, 4, 1)(torch.rand(10, 8), ei, torch.rand(30, 1))
    q, d, att, ei = q.cuda(), d.cuda(), att.cuda(), ei.cuda()
    with pytest.raises(RuntimeError, match="edge_attention_v1: heads = 3 does not divide"):
        conv.edge_attention_v1(q, d, att, ei, 10, 3)
    with pytest.raises(RuntimeError, match="edge_attention_v1: q must be 2-D"):
        conv.edge_attention_v1(q[:, :6], d, att, ei, 10, 2)                      # rows narrower than H * C
    with pytest.raises(RuntimeError, match="edge_attention_v1: operands must have the same dtype"):
        conv.edge_attention_v1(q, d.half(), att, ei, 10, 2)
    with pytest.raises(RuntimeError, match="edge_attention_v1: d "):
        conv.edge_attention_v1(q, d[:, :1], att, ei, 10, 2)                      # fewer columns than heads
    with pytest.raises(RuntimeError, match="edge_attention_v1: d has one row per destination"):
        conv.edge_attention_v1(q, d[:9], att, ei, 10, 2)
    with pytest.raises(RuntimeError, match="edge_attention_v1: u must be"):
        conv.edge_attention_v1(q, d, att, ei, 10, 2, u=torch.rand(29, 8, device="cuda"))
    with pytest.raises(RuntimeError, match="edge_attention_v1: edge_scale must be"):
        conv.edge_attention_v1(q, d, att, ei, 10, 2, edge_scale=torch.rand(30, 1, device="cuda"))
    wide = torch.rand(10, 8200, device="cuda")
    with pytest.raises(RuntimeError, match="edge_attention_v1.*8192"):
        conv.edge_attention_v1(wide, d, torch.rand(8200, device="cuda"), ei, 10, 2)
    with pytest.raises(RuntimeError, match="add_self_loops=False"):
        conv.GATConv(8, 4, heads=2).cuda()((torch.rand(10, 8, device="cuda"), torch.rand(10, 8, device="cuda")), ei)


# ---- the layers ---------------------------------------------------------------------------------------------------------------
def test_state_dicts_follow_pyg(conv):
    layer = conv.GATConv(16, 32, heads=4, concat=False)
    state = layer.state_dict()
    assert {k: tuple(v.shape) for k, v in state.items()} == gc.GAT_STATE
    assert layer.lin_dst is layer.lin_src and float(layer.bias.abs().max()) == 0.0
    other = conv.GATConv(16, 32, heads=4, concat=False)
    other.load_state_dict({k: torch.full_like(v, 0.5) for k, v in state.items()})
    assert float(other.att_dst.min()) == 0.5 and float(other.lin_src.weight.min()) == 0.5
    pair = conv.GATConv((16, 9), 32, heads=4)
    assert pair.lin_dst is not pair.lin_src and tuple(pair.lin_dst.weight.shape) == (128, 9) and tuple(pair.bias.shape) == (128,)
    assert "bias" not in conv.GATConv(16, 32, bias=False).state_dict()
    gate = conv.GATEConv(12, 16, 3)
    assert {k: tuple(v.shape) for k, v in gate.state_dict().items()} == gc.GATE_STATE
    conv.GATEConv(12, 16, 3).load_state_dict({k: torch.full_like(v, 0.25) for k, v in gate.state_dict().items()})
    model = conv.AttentiveFP(8, 16, 3, edge_dim=1, num_layers=3, num_timesteps=2)
    keys = set(model.state_dict())
    want = {"lin1.weight", "lin1.bias", "lin2.weight", "lin2.bias"}
    want |= {f"atom_convs.0.{k}" for k in gc.GATE_STATE} | {f"atom_convs.{i}.{k}" for i in (1, 2) for k in gc.GAT_STATE}
    want |= {f"mol_conv.{k}" for k in gc.GAT_STATE}
    want |= {f"{g}.{k}" for g in ("atom_grus.0", "atom_grus.1", "atom_grus.2", "mol_gru") for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
    assert keys == want
    assert tuple(model.state_dict()["atom_convs.0.lin1.weight"].shape) == (16, 17) and tuple(model.state_dict()["lin2.weight"].shape) == (3, 16)
    conv.AttentiveFP(8, 16, 3, edge_dim=1, num_layers=3, num_timesteps=2).load_state_dict(model.state_dict())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("lc", gc.LAYER_CASES, ids=[c.name for c in gc.LAYER_CASES])
def test_layer_forward_and_gradients(conv, lc, dtype):
    from conv_chain import _compare

    layer, inputs, _, run_dev, run_ref = lc.setup(dtype)
    _compare(layer.cuda(), run_dev, lambda P, **kw: run_ref(P, **kw), inputs, gc.PROJECT_BAR[dtype])


def test_attention_dropout_in_training(conv):
    """GATConv(dropout=0.5) in training: the mask the layer draws under a fixed seed, drawn again the same way and fed to the
    restatement as edge_scale."""
    from conv_chain import _compare

    lc = gc.LAYER_CASES[0]
    layer, inputs, ei, run_dev, run_ref = lc.setup(torch.float32)
    layer.dropout = 0.5
    layer = layer.cuda().train()
    e = gc.with_self_loops(ei, 200).size(1)
    torch.manual_seed(77)
    mask = conv._dropout_scale(e, lc.heads, 0.5, torch.float32, torch.device("cuda")).double().cpu()
    assert set(mask.unique().tolist()) == {0.0, 2.0}

    def seeded(layer, x):
        torch.manual_seed(77)
        return run_dev(layer, x)

    _compare(layer, seeded, lambda P, x: run_ref(P, x, edge_scale=mask), inputs, gc.PROJECT_BAR[torch.float32])
    layer.eval()
    with torch.no_grad():
        x = inputs["x"].cuda()
        assert torch.equal(run_dev(layer, x), run_dev(layer, x))       # no mask in eval


def _model_and_batch(conv, dropout=0.0):
    torch.manual_seed(3)
    model = conv.AttentiveFP(8, 16, 3, edge_dim=1, num_layers=3, num_timesteps=2, dropout=dropout).cuda()
    x, ei, ea, batch = gc.molecules()
    return model, x, ei, ea, batch


def test_attentive_fp_one_optimiser_step(conv):
    """One SGD step of AttentiveFP(8, 16, 3, edge_dim=1, num_layers=3, num_timesteps=2) on 5 molecules of 4 to 9 atoms against the
    same step on the float64 restatement, compared on the updated parameters."""
    model, x, ei, ea, batch = _model_and_batch(conv)
    P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in model.named_parameters()}
    coef = gc._rand(torch.Generator().manual_seed(99), 5, 3)
    opt = torch.optim.SGD(model.parameters(), lr=0.5)
    ref_opt = torch.optim.SGD(list(P.values()), lr=0.5)
    out = model(x.cuda(), ei.cuda(), ea.cuda(), batch.cuda())
    ref = gc.attentive_fp_ref(P, 3, 2, x.double(), ei, ea.double(), batch, 5)
    assert out.shape == (5, 3)
    err = gc.rel_err(out.detach().double().cpu(), ref.detach())
    print(f"forward: {err:.3e}")
    assert err <= gc.PROJECT_BAR[torch.float32]
    (out * coef.cuda()).sum().backward()
    (ref * coef.double()).sum().backward()
    opt.step()
    ref_opt.step()
    for k, v in model.named_parameters():
        err = gc.rel_err(v.detach().double().cpu(), P[k].detach())
        moved = float((P[k].grad * 0.5).abs().max())
        print(f"{k}: {err:.3e} after a step of at most {moved:.3e}")
        # the read-out adds d[i] to every edge of molecule i and all its scores lie on one side of the kink or the other only by
        # chance: where they do the softmax does not move with d, and d att_dst is zero but for rounding
        assert moved > 1e-5 or k == "mol_conv.att_dst", k
        assert err <= gc.PROJECT_BAR[torch.float32], (k, err)


def test_attentive_fp_eval_with_dropout_runs(conv):
    model, x, ei, ea, batch = _model_and_batch(conv, dropout=0.3)
    model.eval()
    with torch.no_grad():
        a = model(x.cuda(), ei.cuda(), ea.cuda(), batch.cuda())
        b = model(x.cuda(), ei.cuda(), ea.cuda(), batch.cuda(), num_graphs=5)
    assert a.shape == (5, 3) and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    model.train()
    out = model(x.cuda(), ei.cuda(), ea.cuda(), batch.cuda())       # training with the reference's dropout: masks drawn, gradients flow
    out.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
