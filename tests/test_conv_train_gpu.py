"""GPU suite: TRAINING through gnnops.conv (VERDICT r2 missing #2; the reference's OpProfiler.py:259-292 profiles a train loop,
app_bm/groq_script.py:135-137 calls its layer with grad enabled).

Each test builds a layer on the device, copies its parameters into a float64 CPU restatement of the SAME layer written the
way MessagePassing.propagate runs it (per-edge gather, concat, Linear per edge, message, index_add_ by destination) and lets
torch's CPU autograd differentiate that chain. The product differentiates its split-product form with its own kernels
(gnnops.autograd.addmm, `_EdgeReduce`: transposed-plan gather for copy messages, gnnops_edge_grad + two segment sums for
cgconv / film). Gradients of a random linear functional of the output must agree: inputs, edge features and every parameter.
Bar: fp32 — 3e-5 of the gradient's scale; fp16 — 1e-2 (storage rounding of the per-edge gradient rows).
CGConv's chain is the reference's own layer text (groq_script.py:91-109); GIN / SAGE / FiLM restate PyG 2.0.2: parity unpinned.
The restatements and the comparison helpers live in tests/conv_chain.py, shared with test_conv_edge_train_gpu.py (the edge pass
alone at every branch of its dispatch).
"""
import pytest
import torch

import conv_chain as cc
from conv_chain import _check, _compare, _graph, _rand, _scatter64  # noqa: F401  (the restatements and helpers both conv files share)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def conv():
    import gnnops
    from gnnops import conv as c

    gnnops.load_library()
    return c


TOLS = {torch.float32: 3e-5, torch.float16: 1e-2}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("channels,dim,aggr", [(16, 0, "add"), (32, 5, "add"), ((24, 16), 3, "mean"), (11, 0, "add")])
def test_cgconv_gradients(conv, dtype, channels, dim, aggr):
    torch.manual_seed(1)
    c_src, c_dst = (channels, channels) if isinstance(channels, int) else channels
    bip = not isinstance(channels, int)
    n_src, n_dst, e = (29, 29, 56) if channels == 11 else (300, 300 if not bip else 210, 2500)
    layer = conv.CGConv(channels, dim, aggr=aggr).to(dtype).cuda()
    ei = _graph(2, n_dst, e, n_src=n_src)
    g = torch.Generator().manual_seed(5)
    inputs = {"x": _rand(g, n_src, c_src)}
    if bip:
        inputs["xd"] = _rand(g, n_dst, c_dst)
    if dim:
        inputs["ea"] = _rand(g, e, dim)

    def run_dev(layer, x, xd=None, ea=None):
        return layer((x, xd) if bip else x, ei.cuda(), ea)

    def run_ref(P, x, xd=None, ea=None):           # groq_script.py:91-109
        return cc.cgconv_ref(P, ei, n_dst, aggr, bip, x, xd, ea)

    _compare(layer, run_dev, run_ref, inputs, TOLS[dtype])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("train_eps", [False, True])
def test_gin_gradients(conv, dtype, train_eps):
    torch.manual_seed(2)
    layer = conv.GINConv(torch.nn.Linear(24, 40), eps=0.3, train_eps=train_eps).to(dtype).cuda()
    ei = _graph(3, 250, 2000)
    g = torch.Generator().manual_seed(6)

    def run_ref(P, x):
        return cc.gin_ref(P, ei, 250, P["eps"] if train_eps else 0.3, x)

    _compare(layer, lambda layer, x: layer(x, ei.cuda()), run_ref, {"x": _rand(g, 250, 24)}, TOLS[dtype])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("root_weight", [True, False])
def test_sage_gradients(conv, dtype, root_weight):
    torch.manual_seed(3)
    layer = conv.SAGEConv(20, 36, root_weight=root_weight).to(dtype).cuda()
    ei = _graph(4, 250, 2000)
    g = torch.Generator().manual_seed(7)

    def run_ref(P, x):
        return cc.sage_ref(P, ei, 250, root_weight, x)

    _compare(layer, lambda layer, x: layer(x, ei.cuda()), run_ref, {"x": _rand(g, 250, 20)}, TOLS[dtype])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("relations,aggr", [(1, "mean"), (3, "mean"), (1, "add")])
def test_film_gradients(conv, dtype, relations, aggr):
    torch.manual_seed(4)
    o = 24
    layer = conv.FiLMConv(12, o, num_relations=relations, aggr=aggr).to(dtype).cuda()
    n, e = 220, 1800
    ei = _graph(5, n, e)
    et = torch.randint(0, relations, (e,), generator=torch.Generator().manual_seed(8))
    g = torch.Generator().manual_seed(9)

    def run_dev(layer, x):
        return layer(x, ei.cuda(), et.cuda() if relations > 1 else None)

    def rd(t):              # conv_chain.film_ref: the per-node projections rounded as the device keeps them (straight-through)
        return t if dtype == torch.float32 else t + (t.to(dtype).double() - t).detach()

    def run_ref(P, x):
        return cc.film_ref(P, ei, et, n, o, relations, aggr, x, rd)

    _compare(layer, run_dev, run_ref, {"x": _rand(g, n, 12)}, TOLS[dtype] * (3 if dtype == torch.float16 else 1))


@pytest.mark.parametrize("cfg", [dict(i=8, o=24, towers=2, edge=None, divide=False, pre=1, post=1),
                                 dict(i=16, o=32, towers=4, edge=3, divide=True, pre=2, post=2)])
def test_pna_gradients(conv, cfg):
    """PNAConv (mean / min / max / std x identity / amplification / attenuation): in a graph that needs gradients the layer
    runs the propagate-order chain on this package's differentiable ops; against torch-CPU float64 autograd of the same
    chain (PyG 2.0.2 definitions: parity unpinned). Random float messages: min / max have unique arguments."""
    torch.manual_seed(6)
    n, e, T = 300, 2400, cfg["towers"]
    ei = _graph(8, n, e)
    deg_hist = torch.bincount(torch.bincount(ei[1], minlength=n))
    aggr, scal = ["mean", "min", "max", "std"], ["identity", "amplification", "attenuation"]
    layer = conv.PNAConv(cfg["i"], cfg["o"], aggr, scal, deg_hist, edge_dim=cfg["edge"], towers=T, divide_input=cfg["divide"],
                         pre_layers=cfg["pre"], post_layers=cfg["post"]).cuda()
    g = torch.Generator().manual_seed(10)
    inputs = {"x": _rand(g, n, cfg["i"])}
    if cfg["edge"]:
        inputs["ea"] = _rand(g, e, cfg["edge"])
    F = cfg["i"] // T if cfg["divide"] else cfg["i"]
    avg = layer.avg_deg

    def run_dev(layer, x, ea=None):
        return layer(x, ei.cuda(), ea)

    def mlp(P, name, z, layers):
        z = z @ P[f"{name}.0.weight"].t() + P[f"{name}.0.bias"]
        for li in range(1, layers):
            z = torch.relu(z) @ P[f"{name}.{2 * li}.weight"].t() + P[f"{name}.{2 * li}.bias"]
        return z

    def run_ref(P, x, ea=None):
        src, dst = ei
        xt = x.view(n, T, F) if cfg["divide"] else x.view(n, 1, F).expand(n, T, F)
        en = ea @ P["edge_encoder.weight"].t() + P["edge_encoder.bias"] if ea is not None else None
        deg = torch.bincount(dst, minlength=n).clamp(min=1).double().unsqueeze(1)
        outs = []
        for t in range(T):
            xin = xt[:, t]
            m = mlp(P, f"pre_nns.{t}", torch.cat([xin[dst], xin[src]] + ([en] if en is not None else []), -1), cfg["pre"])
            mean = _scatter64(m, dst, n, "mean")
            mn = torch.full((n, F), float("inf"), dtype=torch.float64).scatter_reduce(0, dst.view(-1, 1).expand(-1, F), m, "amin", include_self=True)
            mx = torch.full((n, F), float("-inf"), dtype=torch.float64).scatter_reduce(0, dst.view(-1, 1).expand(-1, F), m, "amax", include_self=True)
            has = (torch.bincount(dst, minlength=n) > 0).unsqueeze(1)
            mn, mx = torch.where(has, mn, torch.zeros_like(mn)), torch.where(has, mx, torch.zeros_like(mx))
            std = torch.sqrt(torch.relu(_scatter64(m * m, dst, n, "mean") - mean * mean) + 1e-5)
            out = torch.cat([mean, mn, mx, std], -1)
            out = torch.cat([out, out * (torch.log(deg + 1) / avg["log"]), out * (avg["log"] / torch.log(deg + 1))], -1)
            outs.append(mlp(P, f"post_nns.{t}", torch.cat([xin, out], -1), cfg["post"]))
        return torch.cat(outs, -1) @ P["lin.weight"].t() + P["lin.bias"]

    _compare(layer, run_dev, run_ref, inputs, 1e-4)


def test_a_two_layer_gnn_trains(conv):
    """OpProfiler.py:259-292 in miniature: CGConv -> relu -> SAGEConv -> mean readout, Adam, twenty steps on a fixed random
    graph: the loss falls, every parameter moves, nothing is NaN — and the weights the packed-operand cache hands out after
    training (under no_grad) are the TRAINED ones."""
    torch.manual_seed(5)
    n, e, d = 400, 3000, 32
    ei = _graph(6, n, e).cuda()
    g = torch.Generator().manual_seed(10)
    x = _rand(g, n, d).cuda()
    y = _rand(g, n, 8).cuda()
    l1, l2 = conv.CGConv(d, 0).cuda(), conv.SAGEConv(d, 8).cuda()
    with torch.no_grad():
        before_eval = l2(torch.relu(l1(x, ei)), ei).clone()       # fills the packed-weight caches with the initial weights
    params = list(l1.parameters()) + list(l2.parameters())
    start = [p.detach().clone() for p in params]
    opt = torch.optim.Adam(params, lr=1e-2)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(l2(torch.relu(l1(x, ei)), ei), y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(l == l for l in losses) and losses[-1] < 0.7 * losses[0], losses
    assert all(not torch.equal(a, b.detach()) for a, b in zip(start, params))
    with torch.no_grad():
        after_eval = l2(torch.relu(l1(x, ei)), ei)
        ref = torch.nn.functional.mse_loss(after_eval, y)
    assert not torch.equal(before_eval, after_eval) and float(ref) < losses[0]


def test_edge_reduce_forms_without_a_backward_refuse(conv):
    q = torch.rand(50, 8, device="cuda", requires_grad=True)
    ei = torch.randint(0, 50, (2, 300), device="cuda")
    with pytest.raises(NotImplementedError, match="backward"):
        conv.edge_reduce("copy", q, ei, 50, aggr=("max",))
    with pytest.raises(NotImplementedError, match="backward"):
        conv.edge_reduce("copy", q, ei, 50, aggr=("sum", "mean"))
    with pytest.raises(NotImplementedError, match="backward"):
        conv.edge_reduce("add", q, ei, 50, p=torch.rand(50, 8, device="cuda"))
    out = conv.edge_reduce("copy", q, ei, 50, aggr=("mean",))
    out.sum().backward()
    deg = torch.bincount(ei[1], minlength=50).clamp(min=1).float()
    want = torch.zeros(50, device="cuda").index_add_(0, ei[0], 1.0 / deg[ei[1]])
    torch.testing.assert_close(q.grad, want.unsqueeze(1).expand(50, 8), rtol=1e-5, atol=1e-6)


# ---- bipartite GIN / SAGE, and a mean over a destination whose degree fp16 cannot hold -------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("kind", ["gin", "sage"])
def test_bipartite_gin_and_sage_gradients(conv, dtype, kind):
    """x = (x_src [300, 20], x_dst [210, 28]): the sources and the destinations are different node sets of different widths
    (GIN adds the root to the aggregate, so its two widths are equal)."""
    torch.manual_seed(7)
    n_src, n_dst, e, c_src = 300, 210, 2500, 20
    c_dst = c_src if kind == "gin" else 28
    ei = _graph(11, n_dst, e, n_src=n_src)
    g = torch.Generator().manual_seed(12)
    inputs = {"x": _rand(g, n_src, c_src), "xd": _rand(g, n_dst, c_dst)}
    if kind == "gin":
        layer = conv.GINConv(torch.nn.Linear(c_src, 40), eps=0.3).to(dtype).cuda()

        def run_ref(P, x, xd):
            src, dst = ei
            h = _scatter64(x[src], dst, n_dst, "sum") + 1.3 * xd
            return h @ P["nn.weight"].t() + P["nn.bias"]
    else:
        layer = conv.SAGEConv((c_src, c_dst), 36, root_weight=True).to(dtype).cuda()

        def run_ref(P, x, xd):
            return cc.sage_ref(P, ei, n_dst, True, x, xd)

    _compare(layer, lambda layer, x, xd: layer((x, xd), ei.cuda()), run_ref, inputs, TOLS[dtype])


@pytest.mark.parametrize("case", cc.LAYER_CASES, ids=[f"{c.name}-{cc.DNAME[c.dtype]}" for c in cc.LAYER_CASES])
def test_layers_in_bf16_and_over_a_70000_edge_destination(conv, case):
    """bf16 for CGConv / GIN / SAGE / FiLM at the cases of the tests above (same seeds, shapes and graphs), and SAGE and
    CGConv(aggr="mean") in fp16 and bf16 on a bipartite graph whose destination 5 has 70 000 incoming edges from sources 0 .. 49,
    which feed nothing else: 70 000 is inf in fp16, so a degree counted in the storage type zeroes the hub's gradient and that of
    the fifty sources; d x is compared after scaling by the degree (conv_chain.mean_scales).
    Bars: 4 x the distance of the layer's library-order chain (float32; the per-node products, the edge pass output, g / deg, the
    per-edge gradient rows and the segment sums rounded to the storage type) from the float64 chain, per tensor, recorded in
    tests/golden/conv_self_error.json and re-derived by test_conv_chain_cpu.py. 1 / 70 000 of a gradient is subnormal in fp16,
    which costs the hub's per-edge rows most of their bits: that chain alone is 1.5e-2 from float64 on the degree-scaled d x of
    CGConv, so this file's fp16 bar of 1e-2 is not attainable by any fp16 storage of those rows."""
    recorded = cc.load_self_error()
    layer, inputs, run_dev, run_ref, shape, scale, ei = case.setup()
    if case.kind.startswith("hub"):
        deg = torch.bincount(ei[1], minlength=shape[0])
        assert int(deg[cc.HUB_DST]) == 70000 and (case.dtype != torch.float16 or bool(torch.isinf(deg.to(case.dtype)[cc.HUB_DST])))
    names = ["forward"] + [f"d {k}" for k in list(inputs) + [k for k, _ in layer.named_parameters()]]
    bars = {k: 4 * recorded[case.key(k)] for k in names}
    assert all(0 < b < 0.1 for b in bars.values()), bars
    _compare(layer.cuda(), run_dev, run_ref, inputs, bars, scale_rows=scale)
