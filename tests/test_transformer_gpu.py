"""gnnops.conv.edge_attention_dot and gnnops.conv.TransformerConv (csrc/attention.hip, dot_fwd_kernel / dot_bwd_kernel: one forward
pass with an online softmax, one destination-ordered backward pass) on the GPU against the float64 propagate-order chain of
tests/transformer_chain.py (tied to a dense masked softmax, gradcheck and a hand-worked example by test_transformer_chain_cpu.py):
out, and the gradients of a random linear functional sum(out * R) with respect to qry, k, v (and u), per tensor as
max |got - want| / max |want|.
    shape    H in {1, 3, 4} x C in {1, 5, 8, 64, 136} x three types, 257 sources -> 300 destinations; qry a column block of a wider
             matrix, k and v two blocks of one matrix (one case dense); with u for (3, 8), (1, 136), (4, 64)
    seams    destinations with 0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65 and 129 edges in one graph: every unroll step (4 forward; 2 and 1
             backward) with its neighbours, and the run of 64 edge ids; without and with u
    range    scores of a destination hundreds apart, rows whose scores strictly ascend, strictly descend, and are all equal
    heavy    destinations with 8193 and 20 000 edges among ordinary rows: one wave walks each
    plan     E = 24576 / 24577, the two sides of the one-launch plan; cache on and off; a backward whose source plan is built cold
    edges    repeated edges and self loops; E = 0
    scale    an explicit edge_scale of zeros and 1 / (1 - p) against the chain with that mask; all ones = the bits of the call without
    layer    TransformerConv against transformer_ref: concat, mean of heads, beta, edge_dim, no root weight, bipartite; dropout
Bars: fp32 3e-5 and fp16 1e-2 are the project's (conv_chain.PROJECT_BAR) for the shape / seams / plan / edges tables and the layers;
bf16 and the range and heavy tables: 4 x the chain's distance from itself in float32 with the library's roundings, per case and
tensor (tests/golden/transformer_self_error.json, measured on the CPU from the chain alone)."""
import pytest
import torch

import chain_harness as ch
import transformer_chain as tc

pytestmark = pytest.mark.gpu

SELF_ERROR = tc.load_self_error()
_reference = ch.Reference(tc.case_grads)


@pytest.fixture(scope="module")
def conv():
    return ch.load_conv()


def _placed(leaf, case):
    """qry as a column block of a wider matrix; k and v as two column blocks of ONE matrix (dense copies for layout plain)."""
    if case.layout == "plain":
        return leaf["qry"], leaf["k"], leaf["v"]
    HC = case.H * case.C
    w = (HC + 7) // 8 * 8
    kv = torch.cat([torch.nn.functional.pad(leaf["k"], (8, w - HC)), torch.nn.functional.pad(leaf["v"], (0, w - HC + 8))], dim=1)
    k, v = kv[:, 8:8 + HC], kv[:, 8 + w:8 + w + HC]
    assert k.stride(0) == v.stride(0) == 2 * w + 16 and k.data_ptr() != v.data_ptr()
    qry = tc.place(leaf["qry"], "block")
    assert qry.stride(0) != HC
    return qry, k, v


def _device_run(conv, case, dtype, edge_index=None, edge_scale=None):
    ops, ei, R = tc.inputs(case, dtype)
    leaf = {name: t.to(dtype).cuda().requires_grad_(True) for name, t in ops.items()}
    qry, k, v = _placed(leaf, case)
    ks = None if edge_scale is None else edge_scale.to(dtype).cuda()
    out = conv.edge_attention_dot(qry, k, v, ei.cuda() if edge_index is None else edge_index, case.n_dst, case.H, scale=tc.scale_of(case),
                                  u=leaf.get("u"), edge_scale=ks)
    assert out.dtype == dtype and out.requires_grad and out.shape == (case.n_dst, case.H * case.C)
    (out.float() * R.to(dtype).cuda().float()).sum().backward()
    return out, leaf


def _run_case(conv, case, dtype):
    want_out, want = _reference(case, dtype)
    out, leaf = _device_run(conv, case, dtype)
    ch.judge_case(case, dtype, "out", out, want_out, SELF_ERROR)
    assert set(want) == set(leaf)
    for name, w in want.items():
        ch.judge_case(case, dtype, name, leaf[name].grad, w, SELF_ERROR)
    return out


@pytest.mark.parametrize("case,dtype", **ch.params(tc.SHAPES))
def test_shapes(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(tc.SEAMS))
def test_degree_seams(conv, case, dtype):
    out = _run_case(conv, case, dtype)
    assert tc.SEAM_DEGREES[0] == 0 and float(out[0].detach().abs().max()) == 0.0   # the destination without an edge: exactly zero


@pytest.mark.parametrize("case,dtype", **ch.params(tc.RANGE))
def test_online_rescale(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(tc.HEAVY))
def test_heavy_destinations(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(tc.PLAN))
def test_both_sides_of_the_one_launch_plan(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case,dtype", **ch.params(tc.EDGES[:2]))
def test_repeated_edges_and_self_loops(conv, case, dtype):
    _run_case(conv, case, dtype)


@pytest.mark.parametrize("case", tc.EDGES[2:], ids=[c.name for c in tc.EDGES[2:]])
@pytest.mark.parametrize("dtype", tc.DTYPES, ids=[tc.DNAME[d] for d in tc.DTYPES])
def test_no_edges(conv, case, dtype):
    assert case.E == 0
    out, leaf = _device_run(conv, case, dtype)
    assert float(out.abs().max()) == 0.0
    for name, t in leaf.items():         # zero, as edge_attention gives
        assert t.grad is not None and t.grad.shape == t.shape and float(t.grad.abs().max() if t.numel() else 0.0) == 0.0, name
    ops, ei, _ = tc.inputs(case, dtype)
    dev = {name: t.to(dtype).cuda() for name, t in ops.items()}
    _, lse = conv._dot_forward(dev["qry"], dev["k"], dev["v"], ei.cuda(), case.n_dst, case.H, tc.scale_of(case), dev.get("u"))
    assert lse.shape == (case.n_dst, case.H) and lse.dtype == torch.float32 and bool(torch.isneginf(lse).all())


def test_lse_is_written_and_the_empty_row_matches_edge_attention(conv):
    case = tc.SEAMS[0]
    ops, ei, _ = tc.inputs(case, torch.float32)
    dev = {name: t.float().cuda() for name, t in ops.items()}
    _, lse = conv._dot_forward(dev["qry"], dev["k"], dev["v"], ei.cuda(), case.n_dst, case.H, tc.scale_of(case))
    _, want = tc.attention(ops["qry"], ops["k"], ops["v"], ei, case.n_dst, case.H, tc.scale_of(case))
    assert bool(torch.isneginf(lse[0]).all())
    assert tc.rel_err(lse[1:].double().cpu(), want[1:]) <= tc.PROJECT_BAR[torch.float32]
    out_v2, lse_v2 = conv._attention_forward(dev["k"], dev["qry"], dev["k"][0].contiguous(), ei.cuda(), case.n_dst, case.H, 0.2)
    assert torch.equal(lse_v2[0], lse[0]) and float(out_v2[0].abs().max()) == 0.0


@pytest.mark.parametrize("cache", [True, False], ids=["cache_on", "cache_off"])
@pytest.mark.parametrize("case", tc.PLAN, ids=[c.name for c in tc.PLAN])
def test_plan_routes(conv, case, cache):
    """Forward then backward over one edge_index object, twice (cold, then from the cache); and a backward whose source plan is
    built cold (the caches cleared between forward and backward): every tensor bit-equal to the run on a fresh edge_index."""
    import gnnops

    _, ei, _ = tc.inputs(case, torch.float32)
    snap = lambda out, leaf: [out.detach().clone()] + [t.grad.clone() for t in leaf.values()]   # noqa: E731
    gnnops.set_plan_cache(cache)
    try:
        alone = snap(*_device_run(conv, case, torch.float32))
        shared = ei.cuda()
        for _ in range(2):
            for a, b in zip(snap(*_device_run(conv, case, torch.float32, edge_index=shared)), alone):
                assert torch.equal(a, b)
        ops, _, R = tc.inputs(case, torch.float32)
        leaf = {name: t.float().cuda().requires_grad_(True) for name, t in ops.items()}
        qry, k, v = _placed(leaf, case)
        out = conv.edge_attention_dot(qry, k, v, shared, case.n_dst, case.H, scale=tc.scale_of(case))
        gnnops.clear_plan_cache()
        (out * R.float().cuda()).sum().backward()
        for a, b in zip(snap(out, leaf), alone):
            assert torch.equal(a, b)
    finally:
        gnnops.set_plan_cache(True)


# ---- the dropout scale ----------------------------------------------------------------------------------------------------------
SCALE_CASES = [tc.SHAPES[7], tc.SHAPES[-3]]        # H3-C8 without u, H3-C8 with u


@pytest.mark.parametrize("case,dtype", **ch.params(SCALE_CASES))
def test_explicit_edge_scale(conv, case, dtype):
    """edge_scale of zeros and 1 / (1 - p) entries: the chain with that mask. The bar of bf16 is 4 x the self error of the chain
    WITH the mask, computed here on the CPU from the chain alone."""
    assert (case.H, case.C) == (3, 8)
    mask = tc.dropout_mask(case)
    assert set(mask.unique().tolist()) == {0.0, 2.0}
    ops, ei, R = tc.inputs(case, dtype)
    want_out, want = tc.dot_grads(ops, ei, case.n_dst, case.H, tc.scale_of(case), R, ks=mask)
    self_error = {}           # the table in place of the recorded one, under the same keys
    if case.self_bar(dtype):
        out_r, gr_r = tc.dot_grads(ops, ei, case.n_dst, case.H, tc.scale_of(case), R, rnd=dtype, ks=mask)
        self_error = {case.key(dtype, "out"): tc.rel_err(out_r, want_out),
                      **{case.key(dtype, name): tc.rel_err(gr_r[name], want[name]) for name in want}}
    out, leaf = _device_run(conv, case, dtype, edge_scale=mask)
    ch.judge_case(case, dtype, "out", out, want_out, self_error)
    for name, w in want.items():
        ch.judge_case(case, dtype, name, leaf[name].grad, w, self_error)


@pytest.mark.parametrize("case,dtype", **ch.params(SCALE_CASES))
def test_edge_scale_of_ones_gives_the_same_bits(conv, case, dtype):
    _, ei, _ = tc.inputs(case, dtype)
    plain_out, plain = _device_run(conv, case, dtype)
    ones_out, ones = _device_run(conv, case, dtype, edge_scale=torch.ones(ei.size(1), case.H, dtype=torch.float64))
    assert torch.equal(plain_out, ones_out)
    for name in plain:
        assert torch.equal(plain[name].grad, ones[name].grad), name


@pytest.mark.parametrize("case", [tc.SEAMS[0], tc.SEAMS[2], tc.HEAVY[0]], ids=lambda c: f"{c.table}-{c.name}")
def test_same_bits_on_two_runs(conv, case):
    runs = []
    for _ in range(2):
        out, leaf = _device_run(conv, case, torch.float32)
        runs.append([out.detach().clone()] + [t.grad.clone() for t in leaf.values()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_k_and_v_of_different_pitch_are_copied(conv):
    """Two separate matrices of different widths: the bits of two dense matrices (what the copies are)."""
    import dataclasses

    case = dataclasses.replace(tc.SHAPES[7], layout="plain")       # the same values: the draws depend on table and name alone
    ops, ei, R = tc.inputs(case, torch.float32)
    ref_out, ref = _device_run(conv, case, torch.float32)
    leaf = {name: t.float().cuda().requires_grad_(True) for name, t in ops.items()}
    k = torch.nn.functional.pad(leaf["k"], (0, 8))[:, :case.H * case.C]
    v = torch.nn.functional.pad(leaf["v"], (0, 24))[:, :case.H * case.C]
    assert k.stride(0) != v.stride(0)
    out = conv.edge_attention_dot(leaf["qry"], k, v, ei.cuda(), case.n_dst, case.H)     # scale = None: 1 / sqrt(C)
    (out * R.float().cuda()).sum().backward()
    assert torch.equal(out, ref_out)
    for name in leaf:
        assert torch.equal(leaf[name].grad, ref[name].grad), name


# ---- the layer ----------------------------------------------------------------------------------------------------------------
def test_state_dict_follows_pyg(conv):
    layer = conv.TransformerConv(16, 32, heads=4, concat=False, beta=True, edge_dim=8)
    state = layer.state_dict()
    assert {name: tuple(t.shape) for name, t in state.items()} == tc.PYG_STATE
    other = conv.TransformerConv(16, 32, heads=4, concat=False, beta=True, edge_dim=8)
    other.load_state_dict({name: torch.full_like(t, 0.5) for name, t in state.items()})       # a state_dict with PyG's key names loads
    assert float(other.lin_beta.weight.min()) == 0.5
    plain = conv.TransformerConv(16, 32, heads=4).state_dict()
    assert set(plain) == {f"lin_{n}.{p}" for n in ("key", "query", "value", "skip") for p in ("weight", "bias")}
    assert tuple(plain["lin_skip.weight"].shape) == (128, 16)
    assert tuple(conv.TransformerConv(16, 32, heads=4, beta=True).lin_beta.weight.shape) == (1, 384)
    assert not any(name.startswith("lin_skip") or name.startswith("lin_beta")
                   for name in conv.TransformerConv(16, 32, heads=4, beta=True, root_weight=False).state_dict())
    pair = conv.TransformerConv((10, 13), 8, heads=3).state_dict()
    assert tuple(pair["lin_key.weight"].shape) == (24, 10) and tuple(pair["lin_query.weight"].shape) == (24, 13)
    assert tuple(pair["lin_skip.weight"].shape) == (24, 13)
    assert "lin_key.bias" not in conv.TransformerConv(16, 32, bias=False).state_dict()


def _compare(layer, run_dev, run_ref, inputs, tol):
    """conv_chain._compare (the same draws, the same functional, the same per-tensor measure) for every tensor but one:
    d lin_key.bias is ZERO in exact arithmetic. The key bias adds qry[i] . b to every score of destination i, a softmax does not move
    when all its scores shift together, so sum_e ds[e] = 0 per destination and d b = sum_e ds[e] * scale * qry[i] = 0: the reference's
    own value is its rounding noise and cannot be the scale of the comparison. The device sums the same rows d k[n, :] for d b (weights
    1) and for d lin_key.weight (weights x[n, c], |x| <= 1), so the rounding error of d b lives on the scale of d lin_key.weight: that
    tensor's max |want| is the denominator, and the bar stays ``tol``."""
    from conv_chain import _check, _rand

    dev = {name: t.clone().to(next(layer.parameters()).dtype).cuda().requires_grad_(True) for name, t in inputs.items()}
    out = run_dev(layer, **dev)
    coef = _rand(torch.Generator().manual_seed(99), *out.shape)
    (out.float() * coef.cuda()).sum().backward()
    P = {name: t.detach().double().cpu().requires_grad_(True) for name, t in layer.named_parameters()}
    ref_in = {name: dev[name].detach().double().cpu().requires_grad_(True) for name in inputs}
    ref = run_ref(P, **ref_in)
    _check(out, ref.detach(), tol, "forward")
    (ref * coef.double()).sum().backward()
    for name in inputs:
        _check(dev[name].grad, ref_in[name].grad, tol, f"d {name}")
    for name, p in layer.named_parameters():
        want = P[name].grad if P[name].grad is not None else torch.zeros_like(P[name])
        if name == "lin_key.bias":
            scale = float(P["lin_key.weight"].grad.abs().max())
            assert scale > 1e-3 and float(want.abs().max()) <= 1e-12 * scale            # zero but for float64 rounding
            err = float((p.grad.double().cpu() - want).abs().max()) / scale
            print(f"d {name}: {err:.3e} of the scale of d lin_key.weight (bar {tol:.3e})")
            assert err <= tol, f"d {name}: {err:.3e} of the scale of d lin_key.weight exceeds {tol:.1e}"
        else:
            _check(p.grad, want, tol, f"d {name}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("lc", tc.LAYER_CASES, ids=[c.name for c in tc.LAYER_CASES])
def test_layer_forward_and_gradients(conv, lc, dtype):
    layer, inputs, _, run_dev, run_ref, _ = lc.setup(dtype)
    _compare(layer.cuda(), run_dev, lambda P, **kw: run_ref(P, **kw), inputs, tc.PROJECT_BAR[dtype])


def test_attention_dropout_in_training(conv):
    """TransformerConv(dropout=0.5) in training: the mask the layer draws under a fixed seed, drawn again the same way and fed to the
    restatement as edge_scale; eval ignores dropout."""
    lc = tc.LAYER_CASES[3]
    assert lc.edge_dim == 8
    layer, inputs, ei, run_dev, run_ref, _ = lc.setup(torch.float32, dropout=0.5)
    layer = layer.cuda().train()
    torch.manual_seed(77)
    mask = conv._dropout_scale(ei.size(1), lc.heads, 0.5, torch.float32, torch.device("cuda")).double().cpu()
    assert set(mask.unique().tolist()) == {0.0, 2.0}

    def seeded(layer, **kw):
        torch.manual_seed(77)
        return run_dev(layer, **kw)

    _compare(layer, seeded, lambda P, **kw: run_ref(P, edge_scale=mask, **kw), inputs, tc.PROJECT_BAR[torch.float32])
    layer.eval()
    with torch.no_grad():
        dev = {name: t.cuda() for name, t in inputs.items()}
        a = run_dev(layer, **dev)
        assert torch.equal(a, run_dev(layer, **dev))                 # no mask in eval
        layer.dropout = 0.0
        assert torch.equal(a, run_dev(layer, **dev))                 # and the output of the layer without dropout


def test_layer_same_bits_on_two_runs(conv):
    lc = tc.LAYER_CASES[3]
    layer, inputs, _, run_dev, _, shape = lc.setup(torch.float32)
    layer = layer.cuda()
    coef = tc._rand(torch.Generator().manual_seed(99), *shape).cuda()
    runs = []
    for _ in range(2):
        layer.zero_grad(set_to_none=True)
        dev = {name: t.cuda().requires_grad_(True) for name, t in inputs.items()}
        out = run_dev(layer, **dev)
        (out * coef).sum().backward()
        runs.append([out.detach().clone()] + [t.grad.clone() for t in dev.values()] + [p.grad.clone() for p in layer.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(conv):
    qry, k, v = torch.rand(10, 8), torch.rand(10, 8), torch.rand(10, 8)
    ei = torch.randint(0, 10, (2, 30))
    with pytest.raises(RuntimeError, match="no CPU path"):
        conv.edge_attention_dot(qry, k, v, ei, 10, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        conv.TransformerConv(8, 4, heads=2)(torch.rand(10, 8), ei)
    qry, k, v, ei = qry.cuda(), k.cuda(), v.cuda(), ei.cuda()
    with pytest.raises(RuntimeError, match="does not divide"):
        conv.edge_attention_dot(qry, k, v, ei, 10, 3)
    with pytest.raises(RuntimeError, match="same dtype"):
        conv.edge_attention_dot(qry, k.half(), v.half(), ei, 10, 2)
    with pytest.raises(RuntimeError, match="same dtype"):
        conv.edge_attention_dot(qry, k, v.half(), ei, 10, 2)
    with pytest.raises(RuntimeError, match="edge_attention_dot: v must be 2-D"):
        conv.edge_attention_dot(qry, k, v[:, :6], ei, 10, 2)                   # rows narrower than H * C
    wide = torch.rand(10, 8200, device="cuda")
    with pytest.raises(RuntimeError, match="8192"):
        conv.edge_attention_dot(wide, wide, wide, ei, 10, 2)
    with pytest.raises(RuntimeError, match="edge_scale must be"):
        conv.edge_attention_dot(qry, k, v, ei, 10, 2, edge_scale=torch.ones(30, 3, device="cuda"))
    with pytest.raises(RuntimeError, match="without edge_dim"):
        conv.TransformerConv(8, 4, heads=2).cuda()(torch.rand(10, 8, device="cuda"), ei, torch.rand(30, 2, device="cuda"))
    with pytest.raises(TypeError):
        conv.TransformerConv(8, 4, heads=2).cuda()(torch.rand(10, 8, device="cuda"), ei, return_attention_weights=True)
