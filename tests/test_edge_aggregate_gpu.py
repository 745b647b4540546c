"""GPU suite: gnnops.conv.edge_aggregate (the multi-aggregator edge pass with a backward, gnnops_edge_multi_grad in csrc/conv.hip)
and PNAConv training on it, against the float64 chain of tests/pna_chain.py.

Gradients of a random linear functional of the output, for q, p and w, measured with conv_chain._check (max |got - want| over the
gradient's scale). Bars, the project's: fp32 3e-5, fp16 1e-2 (conv_chain.PROJECT_BAR); bf16 8 x the fp16 bar (three fewer
mantissa bits). Operands lie on a grid of 1 / 1024 (pna_chain.grid): every message is exact in float32 and in float64, so the kernel
and the chain pick the same arg and meet the same ties. Graphs are N = 300, E = 2400 unless a test says otherwise."""
import pytest
import torch

import conv_chain as cc
import pna_chain as pc
from conv_chain import _check

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
BAR = {F32: cc.PROJECT_BAR[F32], F16: cc.PROJECT_BAR[F16], BF16: 8 * cc.PROJECT_BAR[F16]}
AVG = {"log": 2.1, "lin": 8.0}
N, E = 300, 2400
PNA_AGGR, PNA_SCAL = ("mean", "min", "max", "std"), ("identity", "amplification", "attenuation")


@pytest.fixture(scope="module")
def conv():
    import gnnops
    from gnnops import conv as c

    gnnops.load_library()
    return c


@pytest.fixture(scope="module")
def graph():
    ei = cc._graph(21, N, E)          # destination 3 has no edge, destination 5 at least 40
    return ei, ei.cuda()


def operands(functor, has_w, n_src, n_dst, n_edges, K, dtype, seed=0):
    """{"q", "p", "w"}: CPU tensors of the storage type on the grid (bf16 rounds the grid to 8 bits: still exact sums), or None."""
    g = torch.Generator().manual_seed(1000 + seed)
    q = pc.grid(g, n_src, K).to(dtype)
    p = pc.grid(g, n_dst, K).to(dtype) if functor == "add" else None
    w = pc.grid(g, n_edges, K).to(dtype) if (functor == "add" and has_w) else None
    return {"q": q, "p": p, "w": w}


def run(conv, functor, ops, ei, ei_dev, n_dst, aggr, scalers, dtype, layout="plain", functional="random"):
    """-> (out, {name: grad}) on the device and the same from the float64 chain, for d sum(out * R)."""
    leaves = {k: (v.cuda().requires_grad_(True) if v is not None else None) for k, v in ops.items()}
    placed = {k: cc.place(v, layout) for k, v in leaves.items()}
    out = conv.edge_aggregate(functor, placed["q"], ei_dev, n_dst, p=placed["p"], w=placed["w"], aggr=aggr, scalers=scalers,
                              avg_deg=AVG if scalers else None)
    g = torch.Generator().manual_seed(77)
    if functional == "ones":          # out.sum(): autograd hands the backward one expanded scalar (strides 0, 0)
        R = torch.ones(out.shape)
        out.sum().backward()
    elif functional == "transposed":  # the gradient arrives as the transpose of a [width, n_dst] matrix
        Rt = pc.grid(g, out.size(1), out.size(0)).to(dtype)
        R = Rt.t().float()
        (out.t() * Rt.cuda()).sum().backward()
    elif functional == "one_row":     # one row for every destination: an expanded row, row pitch 0, read in place
        r = pc.grid(g, out.size(1)).to(dtype)
        R = r.float().expand(out.shape)
        (out.sum(0) * r.cuda()).sum().backward()
    else:
        R = pc.grid(g, *out.shape).to(dtype).float()
        (out.float() * R.cuda()).sum().backward()
    want_out, want = pc.aggregate_grads(functor, ops, ei, n_dst, aggr, scalers, AVG if scalers else None, R)
    return out.detach(), {k: v.grad for k, v in leaves.items() if v is not None}, want_out, want


def compare(got_out, got, want_out, want, dtype, what=""):
    _check(got_out, want_out, BAR[dtype], f"{what} forward")
    for k in want:
        _check(got[k], want[k], BAR[dtype], f"{what} d {k}")


# ---- dispatch ---------------------------------------------------------------------------------------------------------------
# K = 200 spans two column chunks of the forward's lane layout in every storage type (more than 64 lanes of 4 bytes)
@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("K", [1, 8, 11, 128, 200])
@pytest.mark.parametrize("scalers", [(), pc.SCALERS], ids=["noscal", "scal5"])
@pytest.mark.parametrize("aggr", [pc.AGGREGATORS, ("min",), ("std", "max")], ids=["all5", "min", "std_max"])
@pytest.mark.parametrize("functor,has_w", [("add", False), ("add", True), ("copy", False)], ids=["add", "add_w", "copy"])
def test_dispatch(conv, graph, functor, has_w, aggr, scalers, K, dtype):
    ei, ei_dev = graph
    ops = operands(functor, has_w, N, N, E, K, dtype, seed=K)
    compare(*run(conv, functor, ops, ei, ei_dev, N, aggr, scalers, dtype), dtype)


# ---- rows -------------------------------------------------------------------------------------------------------------------
ROW_EMPTY, ROW_ONE, ROW_65, ROW_EQUAL = 3, 7, 9, 11


def rows_graph():
    """The module's graph with destination 7 left one edge, destination 9 given 65 (one more than the 64-id run of the
    wave-per-row form) and destination 11 four edges from sources 20 .. 23, whose rows the tests make equal."""
    ei = cc._graph(22, N, E).clone()
    src, dst = ei[0], ei[1]
    dst[(dst == ROW_ONE) | (dst == ROW_65) | (dst == ROW_EQUAL)] = 12
    dst[100] = ROW_ONE
    dst[200:265] = ROW_65
    dst[300:304] = ROW_EQUAL
    src[300:304] = torch.arange(20, 24)
    return ei


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("K", [8, 128], ids=["K8-lane_groups", "K128-wave_per_row"])
def test_rows_of_0_1_65_and_equal_messages(conv, K, dtype):
    ei = rows_graph()
    deg = torch.bincount(ei[1], minlength=N)
    assert [int(deg[r]) for r in (ROW_EMPTY, ROW_ONE, ROW_65, ROW_EQUAL)] == [0, 1, 65, 4]
    ops = operands("add", True, N, N, E, K, dtype, seed=5)
    ops["q"][20:24] = ops["q"][20]          # destination 11: four equal messages (dyadic values, degree 4: var is exactly 0)
    ops["w"][300:304] = ops["w"][300]
    got_out, got, want_out, want = run(conv, "add", ops, ei, ei.cuda(), N, pc.AGGREGATORS, PNA_SCAL, dtype)
    compare(got_out, got, want_out, want, dtype)
    assert not bool(got["p"][ROW_EMPTY].any()), "d p of a destination without edges"
    # one edge / equal messages: var = 0, so std passes nothing and d w of those edges is what sum, mean, min and max send
    fac = torch.stack(pc.scaler_factors(ei[1], N, PNA_SCAL, AVG)).squeeze(-1)       # [S, N]
    R = pc.grid(torch.Generator().manual_seed(77), *got_out.shape).to(dtype).double().view(N, len(PNA_SCAL), 5, K)
    ga = (R * fac.t().reshape(N, -1, 1, 1)).sum(1)                                   # [N, 5, K]: sum, mean, min, max, std
    one = ga[ROW_ONE]
    _check(got["w"][100], one[0] + one[1] + one[2] + one[3], BAR[dtype], "d w of the single edge")
    eq = ga[ROW_EQUAL]
    _check(got["w"][300], eq[0] + eq[1] / 4 + eq[2] + eq[3], BAR[dtype], "d w of the first of four equal messages")
    _check(got["w"][301:304], (eq[0] + eq[1] / 4).expand(3, K), BAR[dtype], "d w of the other three")


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_a_destination_of_9000_edges(conv, dtype):
    """More than the 8192 edges at which the forward may reduce a destination piecewise; the backward walks it with one lane group."""
    n_src, n_dst, K = 400, 40, 8
    ei = cc.hub_graph(23, n_src, n_dst, 3000, 9000)
    assert int(torch.bincount(ei[1], minlength=n_dst)[cc.HUB_DST]) == 9000
    ops = operands("add", True, n_src, n_dst, ei.size(1), K, dtype, seed=6)
    got_out, got, want_out, want = run(conv, "add", ops, ei, ei.cuda(), n_dst, PNA_AGGR, PNA_SCAL, dtype)
    # the hub's members hold 1 / 9000 of the mean's and std's gradient: compared on the scale of the rest, as the bars are defined
    compare(got_out, got, want_out, want, dtype)


# ---- ties -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
def test_ties_send_min_and_max_to_the_smaller_edge_id(conv, dtype):
    """Destination 0 has exactly two edges, 50 (from source 30) and 17 (from source 31), with identical q and w rows: both attain
    the min and the max in every column. aggr = (min, max): edge 17 gets the whole gradient, edge 50 and source 30 nothing."""
    K = 8
    ei = cc._graph(24, N, E).clone()
    ei[1][ei[1] == 0] = 1
    ei[0][(ei[0] == 30) | (ei[0] == 31)] = 32
    ei[:, 50] = torch.tensor([30, 0])
    ei[:, 17] = torch.tensor([31, 0])
    ops = operands("add", True, N, N, E, K, dtype, seed=7)
    ops["q"][31] = ops["q"][30]
    ops["w"][17] = ops["w"][50]
    got_out, got, want_out, want = run(conv, "add", ops, ei, ei.cuda(), N, ("min", "max"), (), dtype)
    compare(got_out, got, want_out, want, dtype)
    R = pc.grid(torch.Generator().manual_seed(77), *got_out.shape).to(dtype)
    both = (R[0, :K].float() + R[0, K:].float()).to(dtype)       # d m of edge 17: the min's and the max's gradient, rounded once
    assert torch.equal(got["w"][17].cpu(), both) and bool((both != 0).any())
    assert not bool(got["w"][50].any()) and not bool(got["q"][30].any())
    assert torch.equal(got["q"][31].cpu(), both)
    if dtype == F32:      # the zero / nonzero pattern of the whole per-edge gradient, exactly
        assert torch.equal(got["w"].cpu() != 0, want["w"] != 0)


# ---- layouts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("layout", ["block", "misaligned"])
def test_operands_as_column_blocks(conv, graph, layout, dtype):
    ei, ei_dev = graph
    ops = operands("add", True, N, N, E, 24, dtype, seed=8)
    compare(*run(conv, "add", ops, ei, ei_dev, N, PNA_AGGR, PNA_SCAL, dtype, layout=layout), dtype)


def test_q_and_p_as_blocks_of_one_product(conv, graph):
    """PNAConv's own layout: [p | q] = one [N, 2K] product, w narrower than its buffer; the gradients come back zero-padded."""
    ei, ei_dev = graph
    K = 16
    ops = operands("add", True, N, N, E, K, F32, seed=9)
    pq = torch.cat([ops["p"], ops["q"]], 1).cuda().requires_grad_(True)
    wide = torch.nn.functional.pad(ops["w"], (0, 4)).cuda().requires_grad_(True)
    out = conv.edge_aggregate("add", pq[:, K:], ei_dev, N, p=pq, w=wide, aggr=PNA_AGGR, scalers=PNA_SCAL, avg_deg=AVG)
    R = pc.grid(torch.Generator().manual_seed(77), *out.shape)
    (out * R.cuda()).sum().backward()
    _, want = pc.aggregate_grads("add", ops, ei, N, PNA_AGGR, PNA_SCAL, AVG, R)
    _check(pq.grad, torch.cat([want["p"], want["q"]], 1), BAR[F32], "d [p | q]")
    _check(wide.grad, torch.nn.functional.pad(want["w"], (0, 4)), BAR[F32], "d w, padded")


@pytest.mark.parametrize("functional", ["ones", "one_row", "transposed"])
def test_gradient_layouts_autograd_hands_over(conv, graph, functional):
    ei, ei_dev = graph
    ops = operands("add", True, N, N, E, 8, F32, seed=10)
    compare(*run(conv, "add", ops, ei, ei_dev, N, PNA_AGGR, PNA_SCAL, F32, functional=functional), F32, functional)


# ---- determinism, forward, degenerate sizes ---------------------------------------------------------------------------------
def test_two_backward_runs_give_the_same_bits(conv, graph):
    ei, ei_dev = graph
    ops = operands("add", True, N, N, E, 128, F16, seed=11)
    a = run(conv, "add", ops, ei, ei_dev, N, pc.AGGREGATORS, pc.SCALERS, F16)[1]
    b = run(conv, "add", ops, ei, ei_dev, N, pc.AGGREGATORS, pc.SCALERS, F16)[1]
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["f32", "f16", "bf16"])
def test_forward_is_edge_reduce_bit_for_bit(conv, graph, dtype):
    _, ei_dev = graph
    for functor, has_w in (("add", True), ("copy", False)):
        ops = {k: (v.cuda() if v is not None else None) for k, v in operands(functor, has_w, N, N, E, 24, dtype, seed=12).items()}
        kw = dict(p=ops["p"], w=ops["w"], aggr=PNA_AGGR, scalers=PNA_SCAL, avg_deg=AVG)
        with torch.no_grad():
            want = conv.edge_reduce(functor, ops["q"], ei_dev, N, **kw)
            assert torch.equal(conv.edge_aggregate(functor, ops["q"], ei_dev, N, **kw), want)
        tracked = conv.edge_aggregate(functor, ops["q"].clone().requires_grad_(True), ei_dev, N, **kw)
        assert tracked.requires_grad and torch.equal(tracked.detach(), want)


def test_no_edges_and_no_destinations(conv):
    q = torch.rand(5, 8, device="cuda", requires_grad=True)
    p = torch.rand(4, 8, device="cuda", requires_grad=True)
    w = torch.rand(0, 8, device="cuda", requires_grad=True)
    out = conv.edge_aggregate("add", q, torch.zeros((2, 0), dtype=torch.int64, device="cuda"), 4, p=p, w=w, aggr=("sum", "max"))
    assert out.shape == (4, 16) and not bool(out.any())
    out.sum().backward()
    assert not bool(q.grad.any()) and not bool(p.grad.any()) and w.grad.shape == (0, 8)
    q.grad = None
    out = conv.edge_aggregate("copy", q, torch.zeros((2, 0), dtype=torch.int64, device="cuda"), 0, aggr=("sum", "max"))
    assert out.shape == (0, 16)
    out.sum().backward()
    assert q.grad.shape == q.shape and not bool(q.grad.any())
    with pytest.raises(NotImplementedError, match="affine"):
        conv.edge_aggregate("cgconv", q, torch.zeros((2, 0), dtype=torch.int64, device="cuda"), 4, p=p)


# ---- the layer --------------------------------------------------------------------------------------------------------------
PNA_CFGS = [dict(i=8, o=24, towers=2, edge=None, divide=False, pre=1, post=1),       # the two of test_conv_train_gpu.test_pna_gradients
            dict(i=16, o=32, towers=4, edge=3, divide=True, pre=2, post=2),
            dict(i=1, o=32, towers=1, edge=None, divide=False, pre=1, post=1)]        # the app benchmark's in 1: the edge pass at K = 1


@pytest.mark.parametrize("cfg", PNA_CFGS, ids=["towers2", "towers4-edge-divide-pre2-post2", "in1-K1"])
def test_pna_gradients_on_the_fused_route(conv, cfg):
    """PNAConv with gradients takes the split product and ONE differentiable edge pass; against torch-CPU float64 autograd of the
    propagate-order chain (pna_chain.pna_ref), inputs, edge features and every parameter at test_pna_gradients' 1e-4."""
    torch.manual_seed(6)
    n, e = N, E
    ei = cc._graph(8, n, e)
    deg_hist = torch.bincount(torch.bincount(ei[1], minlength=n))
    layer = conv.PNAConv(cfg["i"], cfg["o"], list(PNA_AGGR), list(PNA_SCAL), deg_hist, edge_dim=cfg["edge"], towers=cfg["towers"],
                         divide_input=cfg["divide"], pre_layers=cfg["pre"], post_layers=cfg["post"]).cuda()
    g = torch.Generator().manual_seed(10)
    inputs = {"x": cc._rand(g, n, cfg["i"])}
    if cfg["edge"]:
        inputs["ea"] = cc._rand(g, e, cfg["edge"])
    ei_dev = ei.cuda()
    cc._compare(layer, lambda layer, x, ea=None: layer(x, ei_dev, ea),
                lambda P, x, ea=None: pc.pna_ref(P, ei, n, cfg, PNA_AGGR, PNA_SCAL, layer.avg_deg, x, ea), inputs, 1e-4)


def test_a_pna_layer_trains(conv):
    torch.manual_seed(7)
    ei = cc._graph(9, N, E)
    deg_hist = torch.bincount(torch.bincount(ei[1], minlength=N))
    layer = conv.PNAConv(16, 8, list(PNA_AGGR), list(PNA_SCAL), deg_hist, towers=2).cuda()
    g = torch.Generator().manual_seed(11)
    x, y, ei = cc._rand(g, N, 16).cuda(), cc._rand(g, N, 8).cuda(), ei.cuda()
    opt = torch.optim.Adam(layer.parameters(), lr=1e-2)
    losses = []
    for _ in range(15):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(layer(x, ei), y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses
