"""The yardstick of the edge-feature attention GPU tests (tests/attention_edge_chain.py) against things it shares no code with: the
two older chains at a zero edge term (bit for bit), a dense [N_dst, N_src] score matrix with a -inf mask and torch.softmax,
torch.autograd.gradcheck, a 4-node self-loop fill worked by hand, and the committed self-error table against a fresh computation.
No GPU, no library call."""
import torch

import attention_chain as ac
import attention_edge_chain as ec
import chain_harness as ch
import gate_chain as gc

F64 = torch.float64


def _small(seed=3, n_src=7, n_dst=9, H=2, C=3):
    """A graph without repeated edges (a dense mask says it all), about 28 edges; destination 4 has no edge."""
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(n_dst, n_src, generator=g) < 0.45
    mask[4] = False
    mask[0, 0] = True
    dst, src = mask.nonzero(as_tuple=True)
    perm = torch.randperm(dst.numel(), generator=g)
    ei = torch.stack([src[perm], dst[perm]])
    E = ei.size(1)
    r = lambda *shape: ac._rand(g, *shape).double()   # noqa: E731
    v2 = {"q": r(n_src, H * C), "p": r(n_dst, H * C), "att": r(H * C), "u": r(E, H * C)}
    v1 = {"q": r(n_src, H * C), "d": r(n_dst, H), "att": r(H * C), "c": r(E, H)}
    return v2, v1, ei, mask, r(n_dst, H * C)


def _dense_edge(ei, rows, n_dst, n_src):
    """Per-edge rows [E, ...] laid out as [n_dst, n_src, ...] (no repeated edges)."""
    out = torch.zeros((n_dst, n_src) + tuple(rows.shape[1:]), dtype=rows.dtype)
    return out.index_put((ei[1], ei[0]), rows)


def _softmax_rows(s, mask):
    s = s.masked_fill(~mask.unsqueeze(-1), float("-inf"))
    a = torch.softmax(s, dim=1)
    return torch.where(mask.any(1).view(-1, 1, 1), a, torch.zeros_like(a)), torch.logsumexp(s, dim=1)


def test_zero_edge_term_is_the_older_chain_exactly():
    for case in (ac.SHAPES[7], ac.RANGE[0]):
        for dtype, rnd in ((torch.float32, None), (torch.bfloat16, torch.bfloat16)):
            ops, ei, R = ec.inputs_u(case, dtype)
            ops["u"] = torch.zeros_like(ops["u"])
            out, gr = ec.attention_u_grads(ops, ei, case.n_dst, case.H, case.slope, R, rnd=rnd)
            old = {k: ops[k] for k in ("q", "p", "att")}
            want_out, want = ac.attention_grads(old, ei, case.n_dst, case.H, case.slope, R, rnd=rnd)
            assert torch.equal(out, want_out)
            for k in want:
                assert torch.equal(gr[k], want[k]), k
    for case in (ec.V1["shape"][7], ec.V1["range"][0]):
        for dtype, rnd in ((torch.float32, None), (torch.bfloat16, torch.bfloat16)):
            ops, ei, R = ec.inputs_c(case, dtype)
            ops["c"] = torch.zeros_like(ops["c"])
            out, gr = ec.attention_c_grads(ops, ei, case.n_dst, case.H, case.slope, R, rnd=rnd)
            old = {k: ops[k] for k in ("q", "d", "att")}
            want_out, want = gc.attention_grads(old, ei, case.n_dst, case.H, None, case.slope, None, R, rnd=rnd)
            assert torch.equal(out, want_out)
            for k in want:
                assert torch.equal(gr[k], want[k]), k


def test_chains_equal_the_dense_masked_softmax():
    v2, v1, ei, mask, R = _small()
    n_dst, n_src = mask.shape
    H, C, slope = 2, 3, 0.2
    # v2
    out, gr = ec.attention_u_grads(v2, ei, n_dst, H, slope, R)
    leaf = {k: v.clone().requires_grad_(True) for k, v in v2.items()}
    z = leaf["p"].view(n_dst, 1, H, C) + leaf["q"].view(1, n_src, H, C) + _dense_edge(ei, leaf["u"].view(-1, H, C), n_dst, n_src)
    s = (torch.where(z > 0, z, z * slope) * leaf["att"].view(1, 1, H, C)).sum(-1)
    a, lse = _softmax_rows(s, mask)
    want = torch.einsum("ijh,jhc->ihc", a, leaf["q"].view(n_src, H, C)).reshape(n_dst, H * C)
    (want * R).sum().backward()
    assert ec.rel_err(out, want.detach()) < 1e-13 and float(out[4].abs().max()) == 0.0
    for k in v2:
        assert ec.rel_err(gr[k], leaf[k].grad) < 1e-12, k
    _, lse_chain = ec.attention_u(v2["q"], v2["p"], v2["att"], v2["u"], ei, n_dst, H, slope)
    rows = mask.any(1)
    assert torch.isneginf(lse_chain[4]).all() and ec.rel_err(lse_chain[rows], lse.detach()[rows]) < 1e-13
    # v1
    out, gr = ec.attention_c_grads(v1, ei, n_dst, H, slope, R)
    leaf = {k: v.clone().requires_grad_(True) for k, v in v1.items()}
    pre = (leaf["q"].view(1, n_src, H, C) * leaf["att"].view(1, 1, H, C)).sum(-1) + leaf["d"].view(n_dst, 1, H) + _dense_edge(ei, leaf["c"], n_dst, n_src)
    a, lse = _softmax_rows(torch.where(pre > 0, pre, pre * slope), mask)
    want = torch.einsum("ijh,jhc->ihc", a, leaf["q"].view(n_src, H, C)).reshape(n_dst, H * C)
    (want * R).sum().backward()
    assert ec.rel_err(out, want.detach()) < 1e-13 and float(out[4].abs().max()) == 0.0
    for k in v1:
        assert ec.rel_err(gr[k], leaf[k].grad) < 1e-12, k
    _, lse_chain = ec.attention_c(v1["q"], v1["d"], v1["att"], v1["c"], ei, n_dst, H, slope)
    assert torch.isneginf(lse_chain[4]).all() and ec.rel_err(lse_chain[rows], lse.detach()[rows]) < 1e-13


def test_gradcheck():
    """On a graph of about ten edges, every pre-activation away from the kinks of the leaky ReLUs."""
    v2, v1, ei, _, _ = _small(seed=4)
    keep = torch.arange(ei.size(1)) < 10
    ei = ei[:, keep]
    v2["u"], v1["c"] = v2["u"][keep], v1["c"][keep]
    assert ei.size(1) == 10
    z, _, _ = ec.scores_u(v2["q"], v2["p"], v2["att"], v2["u"], ei, 2, 0.2)
    assert float(z.abs().min()) > 1e-3
    leaves = [v2[k].clone().requires_grad_(True) for k in ("q", "p", "att", "u")]
    assert torch.autograd.gradcheck(lambda q, p, att, u: ec.attention_u(q, p, att, u, ei, 9, 2, 0.2)[0], leaves, eps=1e-6, atol=1e-7)
    pre = (v1["q"][ei[0]].view(-1, 2, 3) * v1["att"].view(1, 2, 3)).sum(-1) + v1["d"][ei[1]] + v1["c"]
    assert float(pre.abs().min()) > 1e-3
    leaves = [v1[k].clone().requires_grad_(True) for k in ("q", "d", "att", "c")]
    assert torch.autograd.gradcheck(lambda q, d, att, c: ec.attention_c(q, d, att, c, ei, 9, 2, 0.2)[0], leaves, eps=1e-6, atol=1e-7)


def test_library_order_chains_are_the_same_mathematics():
    """``rnd=float32`` rounds nothing that float32 arithmetic does not: the hand-written backward steps equal autograd to 1e-5."""
    v2, v1, ei, _, R = _small(seed=7)
    R = R.float().double()
    for ops, grads in ((v2, ec.attention_u_grads), (v1, ec.attention_c_grads)):
        ops = {k: v.float().double() for k, v in ops.items()}
        out, gr = grads(ops, ei, 9, 2, 0.2, R)
        out_r, gr_r = grads(ops, ei, 9, 2, 0.2, R, rnd=torch.float32)
        assert ec.rel_err(out_r, out) < 1e-6
        for k in gr:
            assert ec.rel_err(gr_r[k], gr[k]) < 1e-5, k


def test_self_loop_fill_on_a_hand_worked_graph():
    """4 nodes; edges (0->1) a, (2->1) b, (1->1) c [a self loop: removed with its attribute], (3->0) d, (1->2) e. After removal node 0
    has in-edge d, node 1 has a and b, node 2 has e, node 3 none."""
    ei = torch.tensor([[0, 2, 1, 3, 1], [1, 1, 1, 0, 2]])
    ea = torch.tensor([[1.0, 10.0], [3.0, 30.0], [100.0, 100.0], [5.0, 7.0], [-2.0, 4.0]], dtype=F64)
    kept = [[1.0, 10.0], [3.0, 30.0], [5.0, 7.0], [-2.0, 4.0]]
    got = ec.looped_attr(ei, ea, 4, "mean")
    assert got.tolist() == kept + [[5.0, 7.0], [2.0, 20.0], [-2.0, 4.0], [0.0, 0.0]]
    got = ec.looped_attr(ei, ea, 4, 0.5)
    assert got.tolist() == kept + [[0.5, 0.5]] * 4
    aug = ec.with_self_loops(ei, 4)
    assert aug.t().tolist() == [[0, 1], [2, 1], [3, 0], [1, 2], [0, 0], [1, 1], [2, 2], [3, 3]]
    # the layer restatements apply it: the same output as the op on the hand-built lists
    g = torch.Generator().manual_seed(1)
    H, C, cin = 2, 3, 4
    r = lambda *shape: ac._rand(g, *shape).double()   # noqa: E731
    x = r(4, cin)
    P = {"lin_l.weight": r(H * C, cin), "lin_l.bias": r(H * C), "lin_r.weight": r(H * C, cin), "lin_r.bias": r(H * C), "att": r(1, H, C),
         "bias": r(C), "lin_edge.weight": r(H * C, 2)}
    got = ec.gatv2_edge_ref(P, ei, 4, H, C, False, 0.2, True, "mean", x, ea)
    q, p = x @ P["lin_l.weight"].t() + P["lin_l.bias"], x @ P["lin_r.weight"].t() + P["lin_r.bias"]
    rows = torch.tensor(kept + [[5.0, 7.0], [2.0, 20.0], [-2.0, 4.0], [0.0, 0.0]], dtype=F64)
    out, _ = ec.attention_u(q, p, P["att"].reshape(-1), rows @ P["lin_edge.weight"].t(), aug, 4, H, 0.2)
    assert ec.rel_err(got, out.view(4, H, C).mean(1) + P["bias"]) < 1e-14
    P = {"lin_src.weight": r(H * C, cin), "att_src": r(1, H, C), "att_dst": r(1, H, C), "att_edge": r(1, H, C), "lin_edge.weight": r(H * C, 2)}
    got = ec.gat_edge_ref(P, ei, 4, H, C, True, 0.2, True, 0.5, x, ea)
    q = x @ P["lin_src.weight"].t()
    d = (q.view(4, H, C) * P["att_dst"]).sum(-1)
    rows = torch.tensor(kept + [[0.5, 0.5]] * 4, dtype=F64)
    c = ((rows @ P["lin_edge.weight"].t()).view(-1, H, C) * P["att_edge"]).sum(-1)
    out, _ = ec.attention_c(q, d, P["att_src"].reshape(-1), c, aug, 4, H, 0.2)
    assert ec.rel_err(got, out) < 1e-14
    # the folded weight of the layer gives the same c: edge_attr @ fold(att_edge, W_e)^T
    fold = torch.einsum("hc,hci->hi", P["att_edge"].view(H, C), P["lin_edge.weight"].view(H, C, 2))
    assert ec.rel_err(rows @ fold.t(), c) < 1e-14


def test_case_tables_have_their_edges():
    for fam, inputs in (("v2", ec.inputs_u), ("v1", ec.inputs_c)):
        tables = ec.FAMILIES[fam]
        assert {(c.H, c.C, c.layout) for c in tables["shape"]} == {(c.H, c.C, c.layout) for c in ac.SHAPES}
        for case in tables["seams"]:
            _, ei, _ = inputs(case, torch.float32)
            deg = torch.bincount(ei[1], minlength=case.n_dst)
            assert tuple(int(d) for d in deg[:len(ec.SEAM_DEGREES)]) == (0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 129)
            assert not bool((ei[1][1:] >= ei[1][:-1]).all())                       # shuffled: the plan's perm is no identity
            ops, es, _ = inputs(case, torch.float32, sorted_edges=True)
            assert bool((es[1][1:] >= es[1][:-1]).all()) and es.size(1) == ei.size(1)
        for case in tables["heavy"]:
            _, ei, _ = inputs(case, torch.float32)
            deg = torch.bincount(ei[1], minlength=case.n_dst)
            assert int(deg[5]) == ac.T_HUB + 1 and int(deg[9]) == 20000
        assert [c.E for c in tables["edges"]] == [600, 0]
    ops, ei, _ = ec.inputs_u(ec.V2["range"][0], torch.float32)
    _, _, s = ec.scores_u(ops["q"], ops["p"], ops["att"], ops["u"], ei, 3, 0.2)
    assert any(float(s[ei[1] == d].max()) > 100 and float(s[ei[1] == d].min()) < -100 for d in range(3, 100) if bool((ei[1] == d).any()))
    # sorting moves the per-edge operand with its edge: the same function, the same value
    case = ec.V2["seams"][0]
    a, _ = ec.case_grads("v2", case, torch.float32)
    b, _ = ec.case_grads("v2", case, torch.float32, sorted_edges=True)
    assert ec.rel_err(a, b) < 1e-13


def test_self_error_table(capsys):
    """The numbers the bars of the GPU tests are 4 x of: recomputed from the chain alone, equal to the committed JSON."""
    ch.check_self_error_table(ec, 0.25, capsys)      # a bar of 4 x this must stay below 1, or it would admit a zero gradient
