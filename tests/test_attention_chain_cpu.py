"""The yardstick of the attention GPU tests (tests/attention_chain.py) against things it shares no code with: a dense
[N_dst, N_src] score matrix with a -inf mask, torch.softmax and a matmul; torch.autograd.gradcheck; a two-edge example worked by
hand; the self-loop rule of the layer restatement written as a plain loop; and the committed self-error table against a fresh
computation. No GPU, no library call."""
import math

import pytest
import torch

import attention_chain as ac
import chain_harness as ch

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
    ops = {"q": ac._rand(g, n_src, H * C).double(), "p": ac._rand(g, n_dst, H * C).double(), "att": ac._rand(g, H * C).double()}
    return ops, ei, mask, ac._rand(g, n_dst, H * C).double()


def _dense(q, p, att, mask, H, slope):
    n_dst, n_src = mask.shape
    C = att.numel() // H
    z = p.view(n_dst, 1, H, C) + q.view(1, n_src, H, C)
    s = (torch.where(z > 0, z, z * slope) * att.view(1, 1, H, C)).sum(-1)                 # [n_dst, n_src, H]
    s = s.masked_fill(~mask.unsqueeze(-1), float("-inf"))
    a = torch.softmax(s, dim=1)
    a = torch.where(mask.any(1).view(-1, 1, 1), a, torch.zeros_like(a))                   # a row of -inf alone is nan in softmax
    out = torch.einsum("ijh,jhc->ihc", a, q.view(n_src, H, C)).reshape(n_dst, H * C)
    return out, torch.logsumexp(s, dim=1)


def test_chain_equals_the_dense_masked_softmax():
    ops, ei, mask, R = _small()
    H, slope = 2, 0.2
    out, gr = ac.attention_grads(ops, ei, 9, H, slope, R)
    leaf = {k: v.clone().requires_grad_(True) for k, v in ops.items()}
    want, lse = _dense(leaf["q"], leaf["p"], leaf["att"], mask, H, slope)
    (want * R).sum().backward()
    assert ac.rel_err(out, want.detach()) < 1e-13
    assert float(out[4].abs().max()) == 0.0
    for k in ops:
        assert ac.rel_err(gr[k], leaf[k].grad) < 1e-12, k
    _, lse_chain = ac.attention(ops["q"], ops["p"], ops["att"], ei, 9, H, slope)
    assert torch.isneginf(lse_chain[4]).all() and torch.isneginf(lse[4]).all()
    rows = mask.any(1)
    assert ac.rel_err(lse_chain[rows], lse.detach()[rows]) < 1e-13


def test_gradcheck():
    ops, ei, _, _ = _small(seed=3)
    z, _, _ = ac.scores(ops["q"], ops["p"], ops["att"], ei, 2, 0.2)
    assert float(z.abs().min()) > 1e-3            # every pre-activation away from the kink of leaky_relu
    leaves = [ops[k].clone().requires_grad_(True) for k in ("q", "p", "att")]
    assert torch.autograd.gradcheck(lambda q, p, att: ac.attention(q, p, att, ei, 9, 2, 0.2)[0], leaves, eps=1e-6, atol=1e-7)


def test_library_order_chain_is_the_same_mathematics():
    """``rnd=float32`` rounds nothing that float32 arithmetic does not: the hand-written backward steps equal autograd to 1e-5."""
    ops, ei, _, R = _small(seed=7)
    ops = {k: v.float().double() for k, v in ops.items()}
    out, gr = ac.attention_grads(ops, ei, 9, 2, 0.2, R.float().double())
    out_r, gr_r = ac.attention_grads(ops, ei, 9, 2, 0.2, R.float().double(), rnd=torch.float32)
    assert ac.rel_err(out_r, out) < 1e-6
    for k in gr:
        assert ac.rel_err(gr_r[k], gr[k]) < 1e-5, k


def test_hand_worked_two_edges():
    """One destination, edges from sources 0 and 1, H = C = 1: p = 0.5, q = (1, -2), att = 2, slope 0.2, R = 3.
    z = (1.5, -1.5), leaky = (1.5, -0.3), s = (3, -0.6), a0 = 1 / (1 + exp(-3.6)), out = a0 * 1 + a1 * (-2)."""
    ei = torch.tensor([[0, 1], [0, 0]])
    ops = {"q": torch.tensor([[1.0], [-2.0]], dtype=F64), "p": torch.tensor([[0.5]], dtype=F64), "att": torch.tensor([2.0], dtype=F64)}
    R = torch.tensor([[3.0]], dtype=F64)
    a0 = 1.0 / (1.0 + math.exp(-3.6))
    a1 = 1.0 - a0
    k = a0 * a1 * (1.0 - (-2.0))                  # d out / d s0 = -d out / d s1
    want = {"q": [[3 * (a0 + k * 2.0)], [3 * (a1 - k * 2.0 * 0.2)]], "p": [[3 * k * 2.0 * (1 - 0.2)]], "att": [3 * k * (1.5 + 0.3)]}
    for rnd, tol in ((None, 1e-14), (torch.float32, 1e-6)):
        out, gr = ac.attention_grads(ops, ei, 1, 1, 0.2, R, rnd=rnd)
        assert abs(float(out) - (a0 - 2 * a1)) < tol
        for name, w in want.items():
            assert ac.rel_err(gr[name], torch.tensor(w, dtype=F64)) < tol, (name, rnd)
    _, lse = ac.attention(ops["q"], ops["p"], ops["att"], ei, 1, 1, 0.2)
    assert abs(float(lse) - math.log(math.exp(3.0) + math.exp(-0.6))) < 1e-14


def test_self_loop_rule_on_a_graph_with_self_loops_and_repeated_edges():
    """Existing self loops go (however often they occur), one per node comes, repeated edges stay repeated and count twice."""
    ei = torch.tensor([[0, 1, 1, 2, 2, 2, 3, 0], [1, 1, 2, 2, 0, 0, 3, 1]])     # (1,1), (2,2), (3,3) loops; (2,0) and (0,1) twice
    n = 5
    pairs = [(int(s), int(d)) for s, d in ei.t() if int(s) != int(d)] + [(k, k) for k in range(n)]
    got = ac.with_self_loops(ei, n)
    assert [(int(s), int(d)) for s, d in got.t()] == pairs
    assert pairs.count((2, 0)) == 2 and pairs.count((1, 1)) == 1 and pairs.count((4, 4)) == 1
    # the layer restatement applies it: the same output as the op on the hand-built list
    g = torch.Generator().manual_seed(1)
    H, C, cin = 2, 3, 4
    P = {"lin_l.weight": ac._rand(g, H * C, cin).double(), "lin_l.bias": ac._rand(g, H * C).double(), "lin_r.weight": ac._rand(g, H * C, cin).double(),
         "lin_r.bias": ac._rand(g, H * C).double(), "att": ac._rand(g, 1, H, C).double(), "bias": ac._rand(g, C).double()}
    x = ac._rand(g, n, cin).double()
    got = ac.gatv2_ref(P, ei, n, H, C, False, 0.2, True, x)
    q, p = x @ P["lin_l.weight"].t() + P["lin_l.bias"], x @ P["lin_r.weight"].t() + P["lin_r.bias"]
    out, _ = ac.attention(q, p, P["att"].reshape(-1), torch.tensor(pairs).t(), n, H, 0.2)
    assert ac.rel_err(got, out.view(n, H, C).mean(1) + P["bias"]) < 1e-14
    # a repeated edge weighs twice: dropping one copy of (2 -> 0) changes row 0
    fewer = [pr for i, pr in enumerate(pairs) if i != pairs.index((2, 0))]
    out2, _ = ac.attention(q, p, P["att"].reshape(-1), torch.tensor(fewer).t(), n, H, 0.2)
    assert float((out2[0] - out[0]).abs().max()) > 1e-3 and ac.rel_err(out2[1:], out[1:]) < 1e-14


def test_case_tables_have_their_edges():
    ops, ei, _ = ac.inputs(ac.SEAMS[0], torch.float32)
    deg = torch.bincount(ei[1], minlength=ac.SEAMS[0].n_dst)
    assert tuple(int(d) for d in deg[:len(ac.SEAM_DEGREES)]) == ac.SEAM_DEGREES
    for case in ac.HEAVY:
        _, ei, _ = ac.inputs(case, torch.float32)
        deg = torch.bincount(ei[1], minlength=case.n_dst)
        assert int(deg[5]) == ac.T_HUB + 1 and int(deg[9]) == 20000 and ei.size(1) < 60000
    for case in ac.RANGE:
        for dt in case.dtypes:
            ops, ei, _ = ac.inputs(case, dt)
            _, _, s = ac.scores(ops["q"], ops["p"], ops["att"], ei, case.H, case.slope)
            assert bool(torch.isfinite(ops["q"]).all())
            span = [s[ei[1] == d] for d in range(case.n_dst)]
            assert any(r.numel() and float(r.max()) > 100 and float(r.min()) < -100 for r in span)    # exp(100) overflows float32
            up, down, same = (s[ei[1] == ac.RANGE_ROWS[k]] for k in ("ascending", "descending", "equal"))
            assert up.size(0) == down.size(0) == same.size(0) == ac.SPECIAL
            assert bool((up[1:] > up[:-1]).all()) and bool((down[1:] < down[:-1]).all()) and bool((same == same[0]).all())
    assert ac.small_plan_fits(24576, 300) and not ac.small_plan_fits(24577, 300)
    assert {(c.H, c.C) for c in ac.SHAPES} >= {(H, C) for H in (1, 3, 4) for C in (1, 5, 8, 64, 136)}
    _, ei, _ = ac.inputs(ac.EDGES[0], torch.float32)
    pairs = [(int(s), int(d)) for s, d in ei.t()]
    assert len(set(pairs)) < len(pairs) and any(s == d for s, d in pairs)
    assert max(pairs.count(pr) for pr in set(pairs) if pr[0] == pr[1]) >= 2          # a self loop that occurs twice


def test_self_error_table(capsys):
    """The numbers the bars of the GPU tests are 4 x of: recomputed from the chain alone, equal to the committed JSON."""
    ch.check_self_error_table(ac, 5e-2, capsys)
