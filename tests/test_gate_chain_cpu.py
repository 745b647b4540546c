"""The yardstick of the GATConv / GATEConv / AttentiveFP GPU tests (tests/gate_chain.py) against things it shares no code with: a
dense [N_dst, N_src] score matrix with a -inf mask, torch.softmax and an einsum; torch.autograd.gradcheck; a two-edge example worked
by hand with u, row_slope and edge_scale all present; GATEConv's restatement (PyG's order: lin2 per edge) against the op's chain with
lin2 moved out of the edge loop; GRUCell written out against torch's; and the committed self-error table against a fresh
computation. No GPU, no library call."""
import math

import torch

import chain_harness as ch
import gate_chain as gc

F64 = torch.float64


def _small(seed=3, n_src=7, n_dst=9, H=2, C=3):
    """A graph without repeated edges (a dense mask says it all); destination 4 has no edge."""
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(n_dst, n_src, generator=g) < 0.45
    mask[4] = False
    mask[0, 0] = True
    dst, src = mask.nonzero(as_tuple=True)
    perm = torch.randperm(dst.numel(), generator=g)
    ei = torch.stack([src[perm], dst[perm]])
    E = ei.size(1)
    ops = {"q": gc._rand(g, n_src, H * C).double(), "d": gc._rand(g, n_dst, H).double(), "att": gc._rand(g, H * C).double(),
           "u": gc._rand(g, E, H * C).double()}
    ks = (torch.rand(E, H, generator=g) >= 0.3).double() / 0.7
    return ops, ei, mask, gc._rand(g, n_dst, H * C).double(), ks


def _dense(q, d, att, u, ks, ei, mask, H, row_slope, slope):
    n_dst, n_src = mask.shape
    C = att.numel() // H
    ud = torch.zeros(n_dst, n_src, H, C, dtype=q.dtype).index_put((ei[1], ei[0]), u.view(-1, H, C))
    kd = torch.zeros(n_dst, n_src, H, dtype=q.dtype).index_put((ei[1], ei[0]), ks)
    t = q.view(1, n_src, H, C) + ud
    r = torch.where(t > 0, t, t * row_slope)
    pre = (r * att.view(1, 1, H, C)).sum(-1) + d.view(n_dst, 1, H)
    s = torch.where(pre > 0, pre, pre * slope).masked_fill(~mask.unsqueeze(-1), float("-inf"))
    a = torch.softmax(s, dim=1)
    a = torch.where(mask.any(1).view(-1, 1, 1), a, torch.zeros_like(a))                   # a row of -inf alone is nan in softmax
    out = torch.einsum("ijh,ijhc->ihc", a * kd, r).reshape(n_dst, H * C)
    return out, torch.logsumexp(s, dim=1)


def test_chain_equals_the_dense_masked_softmax():
    ops, ei, mask, R, ks = _small()
    H, rs, slope = 2, 0.01, 0.2
    out, gr = gc.attention_grads(ops, ei, 9, H, rs, slope, ks, R)
    leaf = {k: v.clone().requires_grad_(True) for k, v in ops.items()}
    want, lse = _dense(leaf["q"], leaf["d"], leaf["att"], leaf["u"], ks, ei, mask, H, rs, slope)
    (want * R).sum().backward()
    assert gc.rel_err(out, want.detach()) < 1e-13
    assert float(out[4].abs().max()) == 0.0
    for k in ops:
        assert gc.rel_err(gr[k], leaf[k].grad) < 1e-12, k
    _, lse_chain = gc.attention_v1(ops["q"], ops["d"], ops["att"], ei, 9, H, ops["u"], rs, slope, ks)
    assert torch.isneginf(lse_chain[4]).all() and torch.isneginf(lse[4]).all()
    rows = mask.any(1)
    assert gc.rel_err(lse_chain[rows], lse.detach()[rows]) < 1e-13


def test_absent_operands_are_their_neutral_values():
    """u = None is u = 0, row_slope = None is slope 1, edge_scale = None is all ones."""
    ops, ei, _, R, _ = _small(seed=5)
    a, _ = gc.attention_v1(ops["q"], ops["d"], ops["att"], ei, 9, 2)
    b, _ = gc.attention_v1(ops["q"], ops["d"], ops["att"], ei, 9, 2, torch.zeros_like(ops["u"]), 1.0, 0.2, torch.ones(ei.size(1), 2, dtype=F64))
    assert gc.rel_err(a, b) < 1e-15


def test_gradcheck():
    ops, ei, _, _, ks = _small(seed=3)
    t, r = gc.rows(ops["q"], ops["u"], ei, 2, 0.01)
    pre = (r * ops["att"].view(1, 2, 3)).sum(-1) + ops["d"][ei[1]]
    assert float(t.abs().min()) > 1e-4 and float(pre.abs().min()) > 1e-4     # every pre-activation 100 eps away from the kinks
    leaves = [ops[k].clone().requires_grad_(True) for k in ("q", "d", "att", "u")]
    fn = lambda q, d, att, u: gc.attention_v1(q, d, att, ei, 9, 2, u, 0.01, 0.2, ks)[0]   # noqa: E731
    assert torch.autograd.gradcheck(fn, leaves, eps=1e-6, atol=1e-7)


def test_library_order_chain_is_the_same_mathematics():
    ops, ei, _, R, ks = _small(seed=7)
    ops = {k: v.float().double() for k, v in ops.items()}
    for u_on, rs, mask in ((True, 0.01, ks), (False, None, None)):
        sub = {k: v for k, v in ops.items() if u_on or k != "u"}
        out, gr = gc.attention_grads(sub, ei, 9, 2, rs, 0.2, mask, R.float().double())
        out_r, gr_r = gc.attention_grads(sub, ei, 9, 2, rs, 0.2, mask, R.float().double(), rnd=torch.float32)
        assert gc.rel_err(out_r, out) < 1e-6
        assert set(gr) == set(gr_r) == set(sub)
        for k in gr:
            assert gc.rel_err(gr_r[k], gr[k]) < 1e-5, k


def test_hand_worked_two_edges():
    """One destination, edges from sources 0 and 1, H = C = 1: q = (1, -2), u = (0.5, -1), row_slope 0.1, att = 2, d = 0.4, slope 0.2,
    edge_scale = (2, 0.5), R = 3.  t = (1.5, -3), r = (1.5, -0.3), pre = (3.4, -0.2), s = (3.4, -0.04), a0 = 1 / (1 + exp(-3.44)),
    out = 2 a0 * 1.5 + 0.5 a1 * (-0.3)."""
    ei = torch.tensor([[0, 1], [0, 0]])
    ops = {"q": torch.tensor([[1.0], [-2.0]], dtype=F64), "d": torch.tensor([[0.4]], dtype=F64), "att": torch.tensor([2.0], dtype=F64),
           "u": torch.tensor([[0.5], [-1.0]], dtype=F64)}
    ks = torch.tensor([[2.0], [0.5]], dtype=F64)
    R = torch.tensor([[3.0]], dtype=F64)
    a0 = 1.0 / (1.0 + math.exp(-3.44))
    a1 = 1.0 - a0
    K = a0 * a1 * (2 * 1.5 - 0.5 * (-0.3))         # d out / d s0 = -d out / d s1
    dpre0, dpre1 = K, -K * 0.2                     # pre0 > 0, pre1 < 0
    dt0 = (2 * a0 + dpre0 * 2.0) * 1.0             # t0 > 0
    dt1 = (0.5 * a1 + dpre1 * 2.0) * 0.1           # t1 < 0: row_slope
    want = {"q": [[3 * dt0], [3 * dt1]], "u": [[3 * dt0], [3 * dt1]], "d": [[3 * (dpre0 + dpre1)]], "att": [3 * (dpre0 * 1.5 + dpre1 * (-0.3))]}
    for rnd, tol in ((None, 1e-14), (torch.float32, 1e-6)):
        out, gr = gc.attention_grads(ops, ei, 1, 1, 0.1, 0.2, ks, R, rnd=rnd)
        assert abs(float(out) - (3 * a0 - 0.15 * a1)) < tol
        for name, w in want.items():
            assert gc.rel_err(gr[name], torch.tensor(w, dtype=F64)) < tol, (name, rnd)
    _, lse = gc.attention_v1(ops["q"], ops["d"], ops["att"], ei, 1, 1, ops["u"], 0.1, 0.2, ks)
    assert abs(float(lse) - math.log(math.exp(3.4) + math.exp(-0.04))) < 1e-14


def test_layer_restatements_reduce_to_the_op():
    g = torch.Generator().manual_seed(1)
    n, cin, cout, ed, e = 12, 5, 6, 3, 40
    ei = torch.randint(0, n, (2, e), generator=g)
    x, ea = gc._rand(g, n, cin).double(), gc._rand(g, e, ed).double()
    P = {"att_l": gc._rand(g, 1, cout).double(), "att_r": gc._rand(g, 1, cin).double(), "lin1.weight": gc._rand(g, cout, cin + ed).double(),
         "lin2.weight": gc._rand(g, cout, cout).double(), "bias": gc._rand(g, cout).double()}
    W1 = P["lin1.weight"]
    agg, _ = gc.attention_v1(x @ W1[:, :cin].t(), x @ P["att_r"].t(), P["att_l"].reshape(-1), ei, n, 1, ea @ W1[:, cin:].t(), 0.01, 0.01)
    assert gc.rel_err(gc.gate_ref(P, ei, x, ea), agg @ P["lin2.weight"].t() + P["bias"]) < 1e-13
    # GATConv: H = 2, the shared projection, self loops by the rule attention_chain pins
    H, C = 2, 3
    Q = {"lin_src.weight": gc._rand(g, H * C, cin).double(), "att_src": gc._rand(g, 1, H, C).double(), "att_dst": gc._rand(g, 1, H, C).double(),
         "bias": gc._rand(g, C).double()}
    q = x @ Q["lin_src.weight"].t()
    d = (q.view(n, H, C) * Q["att_dst"]).sum(-1)
    out, _ = gc.attention_v1(q, d, Q["att_src"].reshape(-1), gc.with_self_loops(ei, n), n, H)
    assert gc.rel_err(gc.gat_ref(Q, ei, n, H, C, False, 0.2, True, x), out.view(n, H, C).mean(1) + Q["bias"]) < 1e-14
    # the score of GAT: alpha = softmax(leaky_relu(att_src . W x_j + att_dst . W x_i)), written with a loop for one destination
    lp = gc.with_self_loops(ei, n)
    into0 = [int(s) for s, t in lp.t() if int(t) == 0]
    sc = torch.stack([torch.nn.functional.leaky_relu((q[j].view(H, C) * Q["att_src"][0]).sum(-1) + d[0], 0.2) for j in into0])
    row0 = (torch.softmax(sc, 0).unsqueeze(-1) * torch.stack([q[j].view(H, C) for j in into0])).sum(0)
    assert gc.rel_err(out[0].view(H, C), row0) < 1e-13


def test_gru_cell_written_out_is_torch_s():
    torch.manual_seed(0)
    cell = torch.nn.GRUCell(5, 7).double()
    P = {f"c.{k}": v.detach() for k, v in cell.named_parameters()}
    x, h = torch.rand(4, 5, dtype=F64), torch.rand(4, 7, dtype=F64)
    assert gc.rel_err(gc.gru_cell(P, "c", x, h), cell(x, h).detach()) < 1e-14


def test_attentive_fp_restatement_runs_and_reaches_every_parameter():
    from gnnops import conv

    torch.manual_seed(3)
    model = conv.AttentiveFP(8, 16, 3, edge_dim=1, num_layers=3, num_timesteps=2)
    assert [type(c).__name__ for c in model.atom_convs] == ["GATEConv", "GATConv", "GATConv"]
    x, ei, ea, batch = gc.molecules()
    assert x.size(0) == 31 and int(batch.max()) == 4 and all(4 <= int(c) <= 9 for c in torch.bincount(batch))
    P = {k: v.detach().double().requires_grad_(True) for k, v in model.named_parameters()}
    out = gc.attentive_fp_ref(P, 3, 2, x.double(), ei, ea.double(), batch, 5)
    assert out.shape == (5, 3)
    out.square().sum().backward()
    for k, v in P.items():
        assert v.grad is not None and float(v.grad.abs().max()) > 0, k


def test_case_tables_have_their_edges():
    for case in gc.SEAMS:
        _, ei, _, _ = gc.inputs(case, torch.float32)
        deg = torch.bincount(ei[1], minlength=case.n_dst)
        assert tuple(int(d) for d in deg[:len(gc.SEAM_DEGREES)]) == gc.SEAM_DEGREES
    for U in (1, 2, 4, 8):        # every unroll of the new kernels: U - 1, U, U + 1
        assert {U - 1, U, U + 1} <= set(gc.SEAM_DEGREES)
    for case in gc.HEAVY:
        _, ei, _, _ = gc.inputs(case, torch.float32)
        deg = torch.bincount(ei[1], minlength=case.n_dst)
        assert int(deg[5]) == gc.T_HUB + 1 and int(deg[9]) == 20000 and ei.size(1) < 60000
    for case in gc.RANGE:
        for dt in case.dtypes:
            ops, ei, _, _ = gc.inputs(case, dt)
            _, r = gc.rows(ops["q"], ops.get("u"), ei, case.H, case.row_slope)
            pre = (r * ops["att"].view(1, case.H, case.C)).sum(-1) + ops["d"][ei[1]]
            s = torch.nn.functional.leaky_relu(pre, case.slope)
            span = [s[ei[1] == d] for d in range(case.n_dst)]
            assert any(r_.numel() and float(r_.max() - r_.min()) > 100 for r_ in span)       # exp(89) overflows float32
            up, down, same = (s[ei[1] == gc.RANGE_ROWS[k]] for k in ("ascending", "descending", "equal"))
            assert up.size(0) == down.size(0) == same.size(0) == gc.SPECIAL
            assert bool((up[1:] > up[:-1]).all()) and bool((down[1:] < down[:-1]).all()) and bool((same == same[0]).all())
    for case in gc.MASK:
        _, ei, _, ks = gc.inputs(case, torch.float32)
        dead = ei[1] == gc.MASK_DEAD_DST
        assert int(dead.sum()) >= 2 and float(ks[dead].abs().max()) == 0.0 and set(ks.unique().tolist()) == {0.0, 2.0}
    assert gc.small_plan_fits(24576, 300) and not gc.small_plan_fits(24577, 300)
    assert {(c.H, c.C, c.variant) for c in gc.SHAPES} >= {(H, C, v) for H in (1, 3, 4) for C in (1, 5, 8, 64, 136) for v in gc.VARIANTS}
    _, ei, _, _ = gc.inputs(gc.EDGES[0], torch.float32)
    pairs = [(int(s), int(d)) for s, d in ei.t()]
    assert len(set(pairs)) < len(pairs) and any(s == d for s, d in pairs)


def test_self_error_table(capsys):
    """The numbers the bars of the GPU tests are 4 x of: recomputed from the chain alone, equal to the committed JSON, and every one
    below 8e-2, so that no bar reaches 1/3: a gradient of zeros (error 1) fails every case."""
    ch.check_self_error_table(gc, 8e-2, capsys)
