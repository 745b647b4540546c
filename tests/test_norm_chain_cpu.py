"""The yardstick of the head_act_norm and GATv2-model GPU tests (tests/norm_chain.py) against things it shares no code with:
torch.autograd.gradcheck, a two-row example worked by hand, the library-order float32 copy against the float64 chain, the case
tables' own edges, and the committed self-error table against a fresh computation. No GPU, no library call."""
import math

import torch

import chain_harness as ch
import norm_chain as nc

F64 = torch.float64


def _small(seed=5, N=6, H=3, C=5):
    g = torch.Generator().manual_seed(seed)
    a = nc._rand(g, N, H * C).double()
    bias = nc._rand(g, C, scale=0.5).double()
    y = a.view(N, H, C).mean(1) + bias
    a.view(N, H, C)[:, 0][y.abs() < 5e-2] += 0.3 * H          # every y away from the kink of the ReLU
    k = ((torch.rand(N, C, generator=g) >= 0.3).double() / 0.7)
    k[:, 0] = 1.0 / 0.7                                          # no row fully dropped
    return {"a": a, "bias": bias, "k": k, "gamma": 1.0 + nc._rand(g, C, scale=0.5).double(), "beta": nc._rand(g, C, scale=0.5).double()}, \
        nc._rand(g, N, C).double()


def test_gradcheck():
    ops, _ = _small()
    y = ops["a"].view(6, 3, 5).mean(1) + ops["bias"]
    assert float(y.abs().min()) > 1e-3
    leaves = [ops[n].clone().requires_grad_(True) for n in ("a", "bias", "gamma", "beta")]
    fn = lambda a, bias, gamma, beta: nc.head_act_norm(a, 3, bias, True, ops["k"], gamma, beta)   # noqa: E731
    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-6)
    fn = lambda a, bias: nc.head_act_norm(a, 3, bias, True, ops["k"])   # noqa: E731
    assert torch.autograd.gradcheck(fn, leaves[:2], eps=1e-6, atol=1e-7)


def test_hand_worked_two_rows():
    """H = 2, C = 2, bias = (0.5, -0.5), gamma = (2, 3), beta = (0.1, 0.2), eps = 0, R = ((1, 2), (1, 1)).
    Row 0: a = ((1, 3), (3, -1)), k = (1, 2): y = (2, 1) + bias = (2.5, 0.5), d = (2.5, 1), mu = 1.75, var = 0.5625, rstd = 4 / 3,
    xhat = (1, -1), out = (2.1, -2.8). Row 1: a = ((-4, 1), (0, 1)), k = (1, 1): y = (-1.5, 0.5), relu -> d = (0, 0.5), mu = 0.25,
    var = 0.0625, rstd = 4, xhat = (-1, 1), out = (-1.9, 3.2)."""
    ops = {"a": torch.tensor([[1.0, 3.0, 3.0, -1.0], [-4.0, 1.0, 0.0, 1.0]], dtype=F64), "bias": torch.tensor([0.5, -0.5], dtype=F64),
           "k": torch.tensor([[1.0, 2.0], [1.0, 1.0]], dtype=F64), "gamma": torch.tensor([2.0, 3.0], dtype=F64),
           "beta": torch.tensor([0.1, 0.2], dtype=F64)}
    R = torch.tensor([[1.0, 2.0], [1.0, 1.0]], dtype=F64)
    # row 0: gx = (2, 6), mean gx = 4, mean gx * xhat = -2, dd = 4/3 * (gx - 4 + xhat * 2) = 4/3 * (0, 0) = 0
    # row 1: gx = (2, 3), mean gx = 2.5, mean gx * xhat = 0.5, dd = 4 * (gx - 2.5 - xhat * 0.5) = 4 * (0, 0) = 0: with C = 2 the
    # norm's output does not move with d (xhat is +-1 whatever d is), so d a = d bias = 0; d gamma = sum R * xhat, d beta = sum R
    want = {"out": [[2.1, -2.8], [-1.9, 3.2]], "a": [[0.0] * 4] * 2, "bias": [0.0, 0.0], "gamma": [1.0 - 1.0, -2.0 + 1.0], "beta": [2.0, 3.0]}
    for rnd, tol in ((None, 1e-12), (torch.float32, 2e-6)):
        out, gr = nc.norm_grads(ops, 2, True, R, rnd=rnd, eps=0.0)
        assert float((out - torch.tensor(want["out"], dtype=F64)).abs().max()) < tol * 10
        for n in ("a", "bias", "gamma", "beta"):
            assert float((gr[n] - torch.tensor(want[n], dtype=F64)).abs().max()) < tol * 10, (n, rnd)
    # without the norm the row itself comes out and the gate and the mask show in d a: row 1, column 0 is closed by the ReLU
    bare = dict(ops, gamma=None, beta=None)
    for rnd in (None, torch.float32):
        out, gr = nc.norm_grads(bare, 2, True, R, rnd=rnd)
        assert torch.equal(out, torch.tensor([[2.5, 1.0], [0.0, 0.5]], dtype=F64))
        assert torch.equal(gr["a"], torch.tensor([[0.5, 2.0, 0.5, 2.0], [0.0, 0.5, 0.0, 0.5]], dtype=F64))
        assert torch.equal(gr["bias"], torch.tensor([1.0, 5.0], dtype=F64))
    assert math.isclose(4.0 / 3.0, 1.0 / math.sqrt(0.5625))


def test_library_order_copy_is_the_same_mathematics():
    """``rnd=float32`` rounds nothing that float32 arithmetic does not: the hand-written steps equal autograd to 1e-5."""
    ops, R = _small(seed=9)
    ops = {n: v.float().double() for n, v in ops.items()}
    R = R.float().double()
    for drop in ((), ("gamma", "beta"), ("k",), ("bias",), ("beta",)):
        sub = {n: (None if n in drop else v) for n, v in ops.items()}
        for relu in (True, False):
            out, gr = nc.norm_grads(sub, 3, relu, R)
            out_r, gr_r = nc.norm_grads(sub, 3, relu, R, rnd=torch.float32)
            assert set(gr) == set(gr_r) == {n for n in nc.GRAD_NAMES if sub[n] is not None}
            assert nc.rel_err(out_r, out) < 1e-6
            for n in gr:
                assert nc.rel_err(gr_r[n], gr[n]) < 1e-5, (n, drop, relu)


def test_one_pass_variance_would_cancel():
    """The big_mean rows: E[d^2] - mu^2 in float32 loses the variance altogether, the two-pass form of the chain keeps it."""
    case = [c for c in nc.VALUES if c.values == "big_mean"][0]
    ops, _ = nc.inputs(case, torch.float32)
    f = {n: (v.float() if v is not None else None) for n, v in ops.items()}
    d, _, mu, rstd = nc._library_row(f, case.H, case.relu, nc.EPS)
    two_pass = 1.0 / rstd.double() ** 2 - nc.EPS
    exact = d.double().var(dim=1, unbiased=False)
    one_pass = (d * d).mean(1) - mu * mu
    assert nc.rel_err(two_pass, exact) < 1e-3
    assert nc.rel_err(one_pass.double(), exact) > 1.0


def test_case_tables_have_their_edges():
    assert {(c.H, c.C) for c in nc.SHAPES} >= {(H, C) for H in (1, 3, 4) for C in (1, 5, 8, 64, 136, 1024)}
    assert {c.H * c.C for c in nc.SHAPES if c.H in (1, 8)} >= {8192}
    assert any(c.layout == "plain" for c in nc.SHAPES)
    for flag in ("bias", "relu", "scale", "norm"):
        assert any(not getattr(c, flag) for c in nc.SHAPES) and any(getattr(c, flag) for c in nc.SHAPES)
    assert {c.N for c in nc.ROWS} == {1, 63, 64, 65, 70000}
    for case in nc.SHAPES[:6] + nc.VALUES:
        ops, _ = nc.inputs(case, torch.bfloat16)
        if case.relu:
            y = ops["a"].view(case.N, case.H, case.C).mean(1) + (ops["bias"] if ops["bias"] is not None else 0.0)
            assert float(y.abs().min()) > 1e-2, case.name
    by = {c.values: c for c in nc.VALUES}
    rows = list(nc.SPECIAL_ROWS)
    ops, _ = nc.inputs(by["constant"], torch.float32)
    d = nc.head_act_norm(ops["a"], 2, None, True, None)
    assert float(d[rows].var(dim=1, unbiased=False).max()) == 0.0 and float(d.var(dim=1, unbiased=False).min()) == 0.0
    ops, _ = nc.inputs(by["dropped"], torch.float32)
    assert float(ops["k"][rows].abs().max()) == 0.0
    _, gr = nc.norm_grads(ops, 3, True, torch.ones(70, 8, dtype=F64))
    assert all(bool(torch.isfinite(v).all()) for v in gr.values())
    ops, _ = nc.inputs(by["gamma_zero"], torch.float32)
    assert float(ops["gamma"][2]) == 0.0
    ops, _ = nc.inputs(by["big_mean"], torch.float32)
    assert float(ops["a"].mean()) > 9.9e3 and 0.1 < float(ops["a"].std()) < 1.0
    ops, _ = nc.inputs(by["negative"], torch.float32)
    y = ops["a"].view(70, 3, 8).mean(1) + ops["bias"]
    assert float(y[rows].max()) < 0.0
    out, _ = nc.norm_grads(ops, 3, True, torch.ones(70, 8, dtype=F64))
    assert nc.rel_err(out[rows], ops["beta"].expand(len(rows), -1)) < 1e-12


def test_model_restatement():
    """The float64 model against a plain composition: GATv2 layer of attention_chain (mean over heads + bias), relu, mask,
    layer_norm; the pool as a loop over the graphs."""
    import attention_chain as ac

    P, x, ei, batch, masks = nc.model_fixture()
    P = {k: v.double() for k, v in P.items()}
    x = x.double()
    assert batch.numel() == sum(nc.GRAPH_SIZES) and len(nc.GRAPH_SIZES) == 5 and all(20 <= n <= 40 for n in nc.GRAPH_SIZES)
    got = nc.gatv2_model(P, x, ei, batch, [m.double() for m in masks])
    h = x
    for k in range(2):
        sub = {n[len(f"convs.{k}."):]: v for n, v in P.items() if n.startswith(f"convs.{k}.")}
        h = torch.relu(ac.gatv2_ref(sub, ei, h.size(0), 3, 16, False, 0.2, True, h)) * masks[k].double()
        if k == 0:
            h = torch.nn.functional.layer_norm(h, (16,), P["lns.0.weight"], P["lns.0.bias"])
    pooled = torch.stack([h[batch == g].mean(0) for g in range(5)])
    want = pooled @ P["post_mp.0.weight"].t() + P["post_mp.0.bias"]
    assert got.shape == (5, 1) and nc.rel_err(got, want) < 1e-12
    assert set(nc.used_parameters()) == {n for n in P if not n.startswith("convs.2.") and not n.startswith("lns.1.")}
    out, grads, leaves = nc.model_grads(torch.float32, True)
    assert all(leaves[n].grad is None for n in leaves if n not in nc.used_parameters())
    assert all(float(v.abs().max()) > 0 for v in grads.values())


def test_self_error_table(capsys):
    """The numbers the bars of the GPU tests are 4 x of: recomputed from the chain alone, equal to the committed JSON."""
    ch.check_self_error_table(nc, 1e-1, capsys)
