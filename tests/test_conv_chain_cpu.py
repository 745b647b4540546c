"""The yardstick of the conv training tests (tests/conv_chain.py) checked without a GPU: its forward against
oracle/conv_oracle.py, its gradients against finite differences and hand-worked values, the library-order chain (``rnd``)
against the recorded self-error table and against the bug class it is there to catch, and the property every input table of
test_conv_edge_train_gpu.py is named for."""
import math

import numpy as np
import pytest
import torch

import chain_harness as ch
import conv_chain as cc
from oracle import conv_oracle

F64 = torch.float64


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=F64) * 2 - 1


def _small(functor, seed=3, n_src=7, n_dst=5, E=30, K=3, grid=False):
    g = torch.Generator().manual_seed(seed)
    ei = torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.randint(0, n_dst, (E,), generator=g)])
    ei[1][ei[1] == 2] = 1                                    # destination 2 is isolated
    nq, np_, nw = cc.PARTS[functor]
    draw = (lambda *s: torch.randint(-16, 17, s, generator=g).double() / 16) if grid else (lambda *s: _rand(g, *s))
    ops = {"q": draw(n_src, nq * K), "p": draw(n_dst, np_ * K) if np_ else None, "w": draw(E, nw * K) if nw else None,
           "add": _rand(g, n_dst, K)}
    return ops, ei, _rand(g, n_dst, K)


# ---- forward: the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aggr", ["sum", "mean"])
@pytest.mark.parametrize("dim", [0, 3])
def test_cgconv_pass_equals_the_oracle_layer(aggr, dim):
    """The per-node split z W = x_i W_i + x_j W_j + e W_e fed to edge_pass gives the oracle's CGConv (float64, to rounding)."""
    g = torch.Generator().manual_seed(1)
    n, E, c = 12, 60, 5
    x, ea = _rand(g, n, c), (_rand(g, E, dim) if dim else None)
    Wf, Ws, bf, bs = _rand(g, c, 2 * c + dim), _rand(g, c, 2 * c + dim), _rand(g, c), _rand(g, c)
    ei = torch.randint(0, n, (2, E), generator=g)
    W = torch.cat([Wf, Ws], 0)
    p = x @ W[:, :c].t() + torch.cat([bf, bs])
    q = x @ W[:, c:2 * c].t()
    w = ea @ W[:, 2 * c:].t() if dim else None
    got = cc.edge_pass("cgconv", q, p, w, x, ei, n, aggr)
    want = conv_oracle.cg_conv(x.numpy(), ei.numpy(), Wf.numpy(), bf.numpy(), Ws.numpy(), bs.numpy(), None if ea is None else ea.numpy(),
                               aggr="add" if aggr == "sum" else aggr)
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=1e-13)
    P = {"lin_f.weight": Wf, "lin_f.bias": bf, "lin_s.weight": Ws, "lin_s.bias": bs}
    layer = cc.cgconv_ref(P, ei, n, "add" if aggr == "sum" else aggr, False, x, ea=ea)
    np.testing.assert_allclose(layer.numpy(), want, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("aggr", ["sum", "mean"])
def test_copy_and_film_passes_equal_the_oracle(aggr):
    g = torch.Generator().manual_seed(2)
    n, E, c, o = 11, 50, 4, 3
    x = _rand(g, n, c)
    ei = torch.randint(0, n, (2, E), generator=g)
    got = cc.edge_pass("copy", x, None, None, None, ei, n, aggr)
    np.testing.assert_allclose(got.numpy(), conv_oracle.scatter(x.numpy()[ei[0].numpy()], ei[1].numpy(), n, aggr), rtol=1e-12, atol=1e-13)
    Wl, bl, Wr = _rand(g, o, c), _rand(g, o), _rand(g, o, c)
    P = {"lin_l.weight": Wl, "lin_l.bias": bl, "lin_r.weight": Wr}
    np.testing.assert_allclose(cc.sage_ref(P, ei, n, True, x).numpy(), conv_oracle.sage_conv(x.numpy(), ei.numpy(), Wl.numpy(), bl.numpy(), Wr.numpy()),
                               rtol=1e-12, atol=1e-13)
    Pg = {"nn.weight": Wl, "nn.bias": bl}
    np.testing.assert_allclose(cc.gin_ref(Pg, ei, n, 0.3, x).numpy(), conv_oracle.gin_conv(x.numpy(), ei.numpy(), Wl.numpy(), bl.numpy(), 0.3),
                               rtol=1e-12, atol=1e-13)
    # film: p = [beta | gamma] of the destination, q = W x of the source; the oracle's layer minus its skip term
    Wr_, Wfilm, bfilm, Wskip, Wfs = _rand(g, o, c), _rand(g, 2 * o, c), _rand(g, 2 * o), _rand(g, o, c), _rand(g, 2 * o, c)
    f = x @ Wfilm.t() + bfilm
    fs = x @ Wfs.t()
    skip = torch.relu(fs[:, o:] * (x @ Wskip.t()) + fs[:, :o])
    got = cc.edge_pass("film", x @ Wr_.t(), f, None, skip, ei, n, aggr)
    want = conv_oracle.film_conv(x.numpy(), ei.numpy(), [Wr_.numpy()], [(Wfilm.numpy(), bfilm.numpy())], Wskip.numpy(), Wfs.numpy(),
                                 aggr="add" if aggr == "sum" else aggr)
    np.testing.assert_allclose(got.numpy(), want, rtol=1e-12, atol=1e-13)
    Pf = {"film_skip.weight": Wfs, "lin_skip.weight": Wskip, "films.0.weight": Wfilm, "films.0.bias": bfilm, "lins.0.weight": Wr_}
    ref = cc.film_ref(Pf, ei, None, n, o, 1, "add" if aggr == "sum" else aggr, x, lambda t: t)
    np.testing.assert_allclose(ref.numpy(), want, rtol=1e-12, atol=1e-13)


# ---- gradients ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aggr", ["sum", "mean"])
@pytest.mark.parametrize("functor", cc.FUNCTORS)
def test_gradcheck(functor, aggr):
    ops, ei, _ = _small(functor)
    if functor == "film":              # keep every pre-activation 0.05 away from the kink of relu
        a = ops["p"][ei[1]][:, 3:] * ops["q"][ei[0]] + ops["p"][ei[1]][:, :3]
        assert float(a.abs().min()) > 1e-3
    names = [k for k, v in ops.items() if v is not None]
    leaves = [ops[k].clone().requires_grad_(True) for k in names]

    def fn(*ts):
        d = dict(zip(names, ts))
        return cc.edge_pass(functor, d["q"], d.get("p"), d.get("w"), d.get("add"), ei, 5, aggr)

    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("aggr", ["sum", "mean"])
@pytest.mark.parametrize("functor", cc.FUNCTORS)
def test_library_order_chain_is_the_same_mathematics(functor, aggr):
    """``rnd=float32`` rounds nothing that float32 arithmetic does not: the hand-written backward steps equal autograd to 1e-5."""
    ops, ei, R = _small(functor, grid=functor == "film", E=60, K=5)
    ops = {k: (v.float().double() if v is not None else None) for k, v in ops.items()}
    out, grads = cc.edge_grads(functor, ops, ei, 5, aggr, R.float().double())
    out_r, grads_r = cc.edge_grads(functor, ops, ei, 5, aggr, R.float().double(), rnd=torch.float32)
    assert set(grads) == set(grads_r) == {k for k, v in ops.items() if v is not None}
    assert cc.rel_err(out_r, out) < 1e-6
    for k in grads:
        assert cc.rel_err(grads_r[k], grads[k]) < 1e-5, k


def test_hand_worked_single_edge():
    """One edge 1 -> 0, K = 1, z_f = 0.5, z_s = -0.25, add = 2, R = 3."""
    ei = torch.tensor([[1], [0]])
    ops = {"q": torch.tensor([[9.0, 9.0], [0.2, 0.25]], dtype=F64), "p": torch.tensor([[0.3, -0.5]], dtype=F64), "w": None,
           "add": torch.tensor([[2.0]], dtype=F64)}
    out, gr = cc.edge_grads("cgconv", ops, ei, 1, "mean", torch.tensor([[3.0]], dtype=F64))
    sg, sp = 1 / (1 + math.exp(-0.5)), math.log1p(math.exp(-0.25))
    assert abs(float(out) - (sg * sp + 2.0)) < 1e-15
    want = [3 * sp * sg * (1 - sg), 3 * sg / (1 + math.exp(0.25))]
    assert torch.allclose(gr["p"], torch.tensor([want], dtype=F64), atol=1e-15)
    assert torch.allclose(gr["q"], torch.tensor([[0.0, 0.0], want], dtype=F64), atol=1e-15)
    assert float(gr["add"]) == 3.0
    out, gr = cc.edge_grads("copy", {"q": ops["q"], "p": None, "w": None, "add": None}, ei, 1, "sum", torch.tensor([[3.0, -1.0]], dtype=F64))
    assert out.tolist() == [[0.2, 0.25]] and gr["q"].tolist() == [[0.0, 0.0], [3.0, -1.0]]


def test_hand_worked_mean_and_isolated_destination():
    """Destination 0 has edges from sources 0, 0 (a duplicate) and 1; destination 1 none: out = add there, d q = R / 3 per edge."""
    ei = torch.tensor([[0, 0, 1], [0, 0, 0]])
    q = torch.tensor([[3.0], [6.0]], dtype=F64)
    add = torch.tensor([[1.0], [5.0]], dtype=F64)
    R = torch.tensor([[9.0], [7.0]], dtype=F64)
    for rnd in (None, torch.float16):
        out, gr = cc.edge_grads("copy", {"q": q, "p": None, "w": None, "add": add}, ei, 2, "mean", R, rnd=rnd)
        assert out.tolist() == [[5.0], [5.0]] and gr["q"].tolist() == [[6.0], [3.0]] and gr["add"].tolist() == R.tolist()
    s = cc.mean_scales(ei, 3, 2)
    assert s["p"].flatten().tolist() == [3.0, 1.0] and s["w"].flatten().tolist() == [3.0] * 3 and s["q"].flatten().tolist() == [3.0, 3.0, 1.0]


def test_film_at_a_pre_activation_of_zero_has_gradient_zero():
    """gamma * q + beta = 0.5 * 0.5 - 0.25 = 0 exactly: message 0, and gradient 0 to all three like torch.relu — in both chains."""
    ei = torch.tensor([[0, 0], [0, 1]])
    ops = {"q": torch.tensor([[0.5]], dtype=F64), "p": torch.tensor([[-0.25, 0.5], [0.25, 0.5]], dtype=F64), "w": None, "add": None}
    R = torch.tensor([[2.0], [4.0]], dtype=F64)
    for rnd in (None, torch.float32, torch.bfloat16):
        out, gr = cc.edge_grads("film", ops, ei, 2, "sum", R, rnd=rnd)
        assert out.tolist() == [[0.0], [0.5]]
        assert gr["p"].tolist() == [[0.0, 0.0], [4.0, 2.0]] and gr["q"].tolist() == [[2.0]]


def test_the_chain_does_not_share_the_degree_bug():
    """fp16, mean over the 70 000-edge destination: 1 / 70 000 is representable (subnormal) in fp16 though 70 000 is not. The
    library-order chain gives every hub feeder a NON-zero gradient of the expected size (R / 70 000 summed over ~1400 edges),
    and the hub row of d p the average it should be."""
    case = next(c for c in cc.HUBS if c.name == "cgconv_w-hub_dst70000-mean-K64")
    ops, ei, R = cc.inputs(case, torch.float16)
    out, gr = cc.edge_grads(case.functor, ops, ei, case.n_dst, "mean", R)
    out_r, gr_r = cc.edge_grads(case.functor, ops, ei, case.n_dst, "mean", R, rnd=torch.float16)
    feed = slice(0, cc.HUB_FEEDERS)
    want = gr["q"][feed].abs().mean()
    assert 1e-4 < float(want) < 1e-1
    assert float(gr_r["q"][feed].abs().amax(1).min()) > 0 and float(gr_r["q"][feed].abs().mean()) > 0.9 * float(want)
    assert cc.rel_err(gr_r["q"][feed], gr["q"][feed]) < 2e-2
    assert cc.rel_err(gr_r["p"][cc.HUB_DST], gr["p"][cc.HUB_DST]) < 2e-2 and float(gr["p"][cc.HUB_DST].abs().max()) > 1e-2
    hub_edges = ei[1] == cc.HUB_DST
    assert float(gr_r["w"][hub_edges].abs().max()) > 0 and cc.rel_err(gr_r["w"][hub_edges], gr["w"][hub_edges]) < 2e-2
    # the bug itself, for scale: a degree counted in fp16 is inf and the same rows come out 0
    deg16 = torch.bincount(ei[1], minlength=case.n_dst).to(torch.float16)
    assert bool(torch.isinf(deg16[cc.HUB_DST])) and float((R[cc.HUB_DST].half() / deg16[cc.HUB_DST]).abs().max()) == 0.0


# ---- the tables ----------------------------------------------------------------------------------------------------------------
def _deg(case, g=None):
    ei = cc.graph_of(case, torch.Generator().manual_seed(2024 + sum(map(ord, case.name))))
    return ei, torch.bincount(ei[1], minlength=case.n_dst), torch.bincount(ei[0], minlength=case.n_src)


def test_dispatch_table_has_its_branches():
    seen = set()
    for c in cc.DISPATCH:
        for d in c.dtypes:
            wide = not c.ragged(d) and c.layout != "misaligned"
            seen.add((c.functor, c.aggr, cc.DNAME[d], "wide" if wide else "elem", c.add, c.layout))
    for f in cc.FUNCTORS:
        for d in ("f32", "f16", "bf16"):
            for aggr in ("sum", "mean"):
                for form in ("wide", "elem"):
                    assert any(s[:4] == (f, aggr, d, form) for s in seen), (f, aggr, d, form)
            assert any(s[0] == f and s[2] == d and s[5] == "misaligned" and s[3] == "elem" for s in seen)
            assert any(s[0] == f and s[2] == d and s[5] == "block" and s[3] == "wide" for s in seen)
    assert {c.K for c in cc.DISPATCH} == {1, 4, 8, 13, 64, 200}
    assert sum(c.add for c in cc.DISPATCH) * 2 in range(len(cc.DISPATCH) - 4, len(cc.DISPATCH) + 5)
    mis = [c for c in cc.DISPATCH if c.layout == "misaligned"]
    assert all(c.K == 64 and not c.ragged(d) for c in mis for d in c.dtypes)       # wide but for the alignment
    for layout, aligned in (("block", True), ("misaligned", False)):
        for dt in cc.DTYPES:
            t = torch.zeros(5, 128, dtype=dt)
            v = cc.place(t, layout, "cpu")
            es = t.element_size()
            assert tuple(v.shape) == (5, 128) and v.stride(1) == 1 and v.stride(0) > 128
            assert ((v.storage_offset() * es) % 16 == 0 and (v.stride(0) * es) % 16 == 0) == aligned


def test_shape_table_has_its_edges():
    names = {c.name.split("-", 1)[1] for c in cc.SHAPES}
    by = {c.name: c for c in cc.SHAPES}
    assert by["copy-E0"].E == 0 and by["film-one_dst_K1_sum_of_out"].n_dst == 1 and by["film-one_dst_K1_sum_of_out"].K == 1
    for f in ("copy", "cgconv_w", "film"):      # out.sum() of a [1, 1] output: a gradient of stride 0, not re-materialised by a mean
        c1 = by[f"{f}-one_dst_K1_sum_of_out"]
        assert c1.ones and c1.aggr == "sum" and c1.K == 1 and c1.n_dst == 1 and not c1.add and c1.layout == "plain"
        assert by[f"{f}-one_dst_K8"].aggr == "mean" and by[f"{f}-one_dst_K8"].n_dst == 1
    o = torch.zeros(1, 1, requires_grad=True)
    seen = []
    y = o * 1
    y.register_hook(lambda g: seen.append(g.contiguous().stride()))
    y.sum().backward()
    assert seen == [(0, 0)]
    assert by["copy-more_sources"].n_src > by["copy-more_sources"].n_dst and by["copy-more_destinations"].n_src < by["copy-more_destinations"].n_dst
    _, din, dout = _deg(by["cgconv_w-isolated_rows"])
    assert int(din[3]) == 0 and int(dout[2]) == 0 and int((din > 0).sum()) > 30
    ei, _, _ = _deg(by["film-duplicate_edges"])
    assert torch.unique(ei, dim=1).size(1) <= ei.size(1) - 90
    sizes = sorted({c.E for c in cc.SHAPES if c.name.split("-", 1)[1].startswith("E") and c.E > 0})
    assert sizes == [1, 1023, 1024, 1025, 24576, 24577]
    assert cc.small_plan_fits(24576, 300) and not cc.small_plan_fits(24577, 300) and cc.small_plan_fits(1025, 40000)
    assert len(names) * 3 == len(cc.SHAPES)


def test_grid_wrap_and_hub_tables_have_their_sizes():
    for c in cc.GRIDWRAP:
        for d in c.dtypes:
            assert cc.GRID_PIECES < c.pieces(d) < 1.6 * cc.GRID_PIECES and not c.ragged(d)
    assert {d for c in cc.GRIDWRAP for d in c.dtypes} == set(cc.DTYPES) and {c.functor for c in cc.GRIDWRAP} == {"cgconv_w", "film"}
    for c in cc.HUBS:
        ei, din, dout = _deg(c)
        if c.graph == "hub_dst":
            assert int(din[cc.HUB_DST]) == c.hub > cc.T_HUB and int(din.sum() - din[cc.HUB_DST]) < cc.T_HUB
            feeders = ei[0][ei[1] == cc.HUB_DST].unique()
            assert int(feeders.max()) < cc.HUB_FEEDERS and not bool((ei[0][ei[1] != cc.HUB_DST] < cc.HUB_FEEDERS).any())
            if c.hub == 70000:
                assert c.hub > 65504 and math.isinf(float(torch.tensor(float(c.hub)).half()))
        else:
            assert int(dout[cc.HUB_SRC]) == c.hub > cc.T_HUB and int(din.max()) < cc.T_HUB
        assert c.bar == "self" and (c.K == 64 or all(c.ragged(d) for d in c.dtypes))
    assert {(c.graph, c.hub) for c in cc.HUBS} == {("hub_dst", 9000), ("hub_dst", 70000), ("hub_src", 9000)}
    assert {c.aggr for c in cc.HUBS} == {"sum", "mean"} and {c.K for c in cc.HUBS} == {64, 13}


def test_saturation_table_has_its_values():
    for c in cc.SATURATION:
        for d in c.dtypes:
            ops, ei, _ = cc.inputs(c, d)
            z = ops["p"][ei[1]] + ops["q"][ei[0]] + (ops["w"] if ops["w"] is not None else 0)
            zf, zs = z[:, :c.K], z[:, c.K:]
            if c.values == "spread30":
                assert float(z.max()) > 25 and float(z.min()) < -25 and float(z.abs().max()) <= 30.1
            elif c.values == "seam":
                t = torch.exp(-zs.abs())
                assert float((t < 1e-3).float().mean()) > 0.2 and float((t >= 1e-3).float().mean()) > 0.2
                assert float((t / 1e-3).log().abs().max()) < 0.2 and bool((zs > 0).any()) and bool((zs < 0).any())
            else:
                block = ei[1] < c.n_dst // 10
                assert 0.05 < float(block.float().mean()) < 0.2
                assert float(z[block].abs().min()) >= 97 and float(z[~block].abs().max()) <= 3
                for part in (zf, zs):
                    assert bool((part[block] > 0).any()) and bool((part[block] < 0).any())
                # the block's float64 gradients stay finite, and so does the library-order chain in the storage type
                _, gr, _ = cc.case_grads(c, d, rnd=d)
                assert all(bool(torch.isfinite(v).all()) for v in gr.values())


def test_self_error_table_is_the_recording(capsys):
    """The numbers the bars of the GPU tests are 4 x of: recomputed from the chain alone, equal to tests/golden/conv_self_error.json."""
    table, recorded = ch.recomputed_table(cc, capsys, "library-order float32 chain against the float64 chain, relative to max |reference|")
    for k, v in table.items():
        assert v == v and 0 <= v < 2e-2, (k, v)
        if k.startswith("layer/"):       # the layers' float32 products go through the host's BLAS, which is not bit-reproducible
            assert recorded[k] / 1.5 <= v <= recorded[k] * 1.5, (k, v, recorded[k])      # across hosts (composite_chain's window)
        else:
            assert v == recorded[k], (k, v, recorded[k])


def test_layer_cases_are_the_layer_tests_cases_in_bf16_plus_the_hub():
    kinds = {}
    for c in cc.LAYER_CASES:
        kinds.setdefault(c.kind, []).append(c.dtype)
    assert {k: len(v) for k, v in kinds.items()} == {"cgconv": 4, "gin": 2, "sage": 2, "film": 3, "hub_sage": 2, "hub_cgconv": 2}
    assert all(d == cc.BF16 for k in ("cgconv", "gin", "sage", "film") for d in kinds[k])
    assert set(kinds["hub_sage"]) == set(kinds["hub_cgconv"]) == {cc.F16, cc.BF16}
    ei = cc.hub_graph(13, 400, 60, 2000, 70000)
    deg = torch.bincount(ei[1], minlength=60)
    assert int(deg[cc.HUB_DST]) == 70000 and bool(torch.isinf(deg.half()[cc.HUB_DST])) and float(deg.bfloat16()[cc.HUB_DST]) != 70000
    assert int(ei[0][ei[1] == cc.HUB_DST].max()) < cc.HUB_FEEDERS and not bool((ei[0][ei[1] != cc.HUB_DST] < cc.HUB_FEEDERS).any())


def test_a_bf16_degree_is_below_what_bf16_storage_costs():
    """What the suite does NOT pin: a degree counted in bf16 is off by at most 2^-9 (257 -> 256: 0.39 %; 9000 -> 9024, 70 000 ->
    70 144: 0.2 - 0.3 %), and the library-order chain with such a degree stays inside the 4 x self-error bar of its case: bf16
    storage of the gradients costs more than the rounded degree. The fp16 form of the bug (inf, gradient 0) is what every hub-mean
    case resolves; in bf16 only a gradient that is nearly exact in bf16 does (d p of film over the 70 000 hub: R times a count)."""
    worst = max(abs(float(torch.tensor(float(d)).bfloat16()) - d) / d for d in range(257, 70001))
    assert worst <= 2.0 ** -8 and abs(float(torch.tensor(257.0).bfloat16()) - 257) / 257 > 3.8e-3
    case = next(c for c in cc.HUBS if c.name == "copy-hub_dst9000-mean-K64")
    ops, ei, R = cc.inputs(case, cc.BF16)
    _, gr = cc.edge_grads("copy", ops, ei, case.n_dst, "mean", R)
    deg = torch.bincount(ei[1], minlength=case.n_dst).clamp(min=1)
    assert float(deg[cc.HUB_DST].bfloat16()) == 9024.0
    g = (R.float() / deg.bfloat16().float().unsqueeze(1)).bfloat16().float()          # the parent's line in bf16
    dq = torch.zeros(case.n_src, case.K).index_add_(0, ei[0], g[ei[1]]).bfloat16().double()
    s = cc.mean_scales(ei, case.n_src, case.n_dst)["q"]
    assert cc.rel_err(dq * s, gr["q"] * s) < 4 * cc.load_self_error()[case.key(cc.BF16, "q")]
