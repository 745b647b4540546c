"""The yardstick of the TransformerConv GPU tests (tests/transformer_chain.py) against things it shares no code with: a dense
[N_dst, N_src] score matrix with a -inf mask, torch.softmax and a matmul; torch.autograd.gradcheck; a two-edge example worked by
hand; and the committed self-error table against a fresh computation. No GPU, no library call."""
import math

import torch

import chain_harness as ch
import transformer_chain as tc

F64 = torch.float64


def _small(seed=3, n_src=7, n_dst=9, H=2, C=3, with_u=False):
    """A graph without repeated edges (a dense mask says it all); destination 4 has no edge."""
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(n_dst, n_src, generator=g) < 0.45
    mask[4] = False
    mask[0, 0] = True
    dst, src = mask.nonzero(as_tuple=True)
    perm = torch.randperm(dst.numel(), generator=g)
    ei = torch.stack([src[perm], dst[perm]])
    ops = {"qry": tc._rand(g, n_dst, H * C).double(), "k": tc._rand(g, n_src, H * C).double(), "v": tc._rand(g, n_src, H * C).double()}
    if with_u:
        ops["u"] = tc._rand(g, ei.size(1), H * C).double()
    return ops, ei, mask, tc._rand(g, n_dst, H * C).double()


def _dense(qry, k, v, u, ei, mask, H, scale, ks=None):
    """Dense masked softmax; u [E, H * C] and ks [E, H] are spread over the [n_dst, n_src] grid (no repeated edges)."""
    n_dst, n_src = mask.shape
    C = qry.size(1) // H
    kk = k.view(1, n_src, H, C).expand(n_dst, n_src, H, C)
    vv = v.view(1, n_src, H, C).expand(n_dst, n_src, H, C)
    if u is not None:
        grid = torch.zeros(n_dst, n_src, H, C, dtype=qry.dtype).index_put((ei[1], ei[0]), u.view(-1, H, C))
        kk, vv = kk + grid, vv + grid
    s = scale * (qry.view(n_dst, 1, H, C) * kk).sum(-1)                                   # [n_dst, n_src, H]
    s = s.masked_fill(~mask.unsqueeze(-1), float("-inf"))
    a = torch.softmax(s, dim=1)
    a = torch.where(mask.any(1).view(-1, 1, 1), a, torch.zeros_like(a))                   # a row of -inf alone is nan in softmax
    if ks is not None:
        a = a * torch.zeros(n_dst, n_src, H, dtype=qry.dtype).index_put((ei[1], ei[0]), ks)
    out = (a.unsqueeze(-1) * vv).sum(1).reshape(n_dst, H * C)
    return out, torch.logsumexp(s, dim=1)


def _against_dense(with_u, with_ks):
    ops, ei, mask, R = _small(with_u=with_u)
    H, scale = 2, 1.0 / math.sqrt(3)
    ks = (torch.rand(ei.size(1), H, generator=torch.Generator().manual_seed(8)) >= 0.5).double() * 2.0 if with_ks else None
    out, gr = tc.dot_grads(ops, ei, 9, H, scale, R, ks=ks)
    leaf = {name: t.clone().requires_grad_(True) for name, t in ops.items()}
    want, lse = _dense(leaf["qry"], leaf["k"], leaf["v"], leaf.get("u"), ei, mask, H, scale, ks)
    (want * R).sum().backward()
    assert tc.rel_err(out, want.detach()) < 1e-13
    assert float(out[4].abs().max()) == 0.0
    for name in ops:
        assert tc.rel_err(gr[name], leaf[name].grad) < 1e-12, name
    _, lse_chain = tc.attention(ops["qry"], ops["k"], ops["v"], ei, 9, H, scale, ops.get("u"), ks)
    assert torch.isneginf(lse_chain[4]).all() and torch.isneginf(lse[4]).all()
    have = mask.any(1)
    assert tc.rel_err(lse_chain[have], lse.detach()[have]) < 1e-13            # the dropout scale never enters lse


def test_chain_equals_the_dense_masked_softmax():
    _against_dense(False, False)


def test_chain_with_u_and_dropout_scale_equals_the_dense_masked_softmax():
    _against_dense(True, False)
    _against_dense(True, True)
    _against_dense(False, True)


def test_gradcheck():
    """5 destinations, 4 sources, every operand including u."""
    ops, ei, _, _ = _small(seed=5, n_src=4, n_dst=5, with_u=True)
    leaves = [ops[name].clone().requires_grad_(True) for name in ("qry", "k", "v", "u")]
    assert torch.autograd.gradcheck(lambda qry, k, v, u: tc.attention(qry, k, v, ei, 5, 2, 0.7, u)[0], leaves, eps=1e-6, atol=1e-7)
    ks = (torch.rand(ei.size(1), 2, generator=torch.Generator().manual_seed(8)) >= 0.5).double() * 2.0
    assert torch.autograd.gradcheck(lambda qry, k, v: tc.attention(qry, k, v, ei, 5, 2, 0.7, None, ks)[0], leaves[:3], eps=1e-6, atol=1e-7)


def test_library_order_chain_is_the_same_mathematics():
    """``rnd=float32`` rounds nothing that float32 arithmetic does not: the hand-written backward steps equal autograd to 1e-5."""
    for with_u in (False, True):
        ops, ei, _, R = _small(seed=7, with_u=with_u)
        ops = {name: t.float().double() for name, t in ops.items()}
        ks = (torch.rand(ei.size(1), 2, generator=torch.Generator().manual_seed(8)) >= 0.5).double() * 2.0
        for scale_rows in (None, ks):
            out, gr = tc.dot_grads(ops, ei, 9, 2, 0.6, R.float().double(), ks=scale_rows)
            out_r, gr_r = tc.dot_grads(ops, ei, 9, 2, 0.6, R.float().double(), rnd=torch.float32, ks=scale_rows)
            assert tc.rel_err(out_r, out) < 1e-6
            assert set(gr) == set(gr_r) == set(ops)
            for name in gr:
                assert tc.rel_err(gr_r[name], gr[name]) < 1e-5, name


def test_hand_worked_two_edges():
    """One destination, edges from sources 0 and 1, H = 1, C = 2, scale = 0.5, R = (3, -1):
    qry = (2, 1); k0 = (1, 2), k1 = (-1, 1); v0 = (1, 0), v1 = (0, 4).
    s0 = 0.5 * (2 + 2) = 2, s1 = 0.5 * (-2 + 1) = -0.5, a0 = 1 / (1 + exp(-2.5)), a1 = 1 - a0, out = a0 * v0 + a1 * v1 = (a0, 4 a1).
    With L = R . out: dL/da0 = R . v0 = 3, dL/da1 = R . v1 = -4, so dL/ds0 = a0 a1 (3 - (-4)) = 7 a0 a1 = -dL/ds1.
    d qry = 0.5 * 7 a0 a1 * (k0 - k1) = 3.5 a0 a1 * (2, 1);  d k0 = 0.5 * 7 a0 a1 * qry = -d k1;  d v0 = a0 R, d v1 = a1 R."""
    ei = torch.tensor([[0, 1], [0, 0]])
    ops = {"qry": torch.tensor([[2.0, 1.0]], dtype=F64), "k": torch.tensor([[1.0, 2.0], [-1.0, 1.0]], dtype=F64),
           "v": torch.tensor([[1.0, 0.0], [0.0, 4.0]], dtype=F64)}
    R = torch.tensor([[3.0, -1.0]], dtype=F64)
    a0 = 1.0 / (1.0 + math.exp(-2.5))
    a1 = 1.0 - a0
    t = 7.0 * a0 * a1
    want = {"qry": [[0.5 * t * 2.0, 0.5 * t * 1.0]], "k": [[0.5 * t * 2.0, 0.5 * t * 1.0], [-0.5 * t * 2.0, -0.5 * t * 1.0]],
            "v": [[3 * a0, -a0], [3 * a1, -a1]]}
    for rnd, tol in ((None, 1e-14), (torch.float32, 1e-6)):
        out, gr = tc.dot_grads(ops, ei, 1, 1, 0.5, R, rnd=rnd)
        assert tc.rel_err(out, torch.tensor([[a0, 4 * a1]], dtype=F64)) < tol
        for name, w in want.items():
            assert tc.rel_err(gr[name], torch.tensor(w, dtype=F64)) < tol, (name, rnd)
    _, lse = tc.attention(ops["qry"], ops["k"], ops["v"], ei, 1, 1, 0.5)
    assert abs(float(lse) - math.log(math.exp(2.0) + math.exp(-0.5))) < 1e-14
    # a per-edge row on edge 1 only, u1 = (1, -1): kk1 = (0, 0), s1 = 0; vv1 = (1, 3)
    ops_u = dict(ops, u=torch.tensor([[0.0, 0.0], [1.0, -1.0]], dtype=F64))
    b0 = 1.0 / (1.0 + math.exp(-2.0))
    out, gr = tc.dot_grads(ops_u, ei, 1, 1, 0.5, R)
    assert tc.rel_err(out, torch.tensor([[b0 + (1 - b0), 3 * (1 - b0)]], dtype=F64)) < 1e-14
    assert tc.rel_err(gr["u"], gr["k"] + gr["v"]) < 1e-14                     # one edge per source: d u = d k + d v row by row


def test_case_tables_have_their_edges():
    case = tc.SEAMS[0]
    _, ei, _ = tc.inputs(case, torch.float32)
    deg = torch.bincount(ei[1], minlength=case.n_dst)
    assert tuple(int(d) for d in deg[:len(tc.SEAM_DEGREES)]) == tc.SEAM_DEGREES
    for step in (4, 2, 1):                                       # DotUnroll of csrc/attention.hip: forward 4 / 2 / 1, backward 2 / 1
        assert {step - 1, step, step + 1} <= set(tc.SEAM_DEGREES)
    assert {0, 63, 64, 65, 129} <= set(tc.SEAM_DEGREES)
    for case in tc.HEAVY:
        _, ei, _ = tc.inputs(case, torch.float32)
        deg = torch.bincount(ei[1], minlength=case.n_dst)
        assert int(deg[5]) == tc.ac.T_HUB + 1 and int(deg[9]) == 20000 and ei.size(1) < 60000
    for case in tc.RANGE:
        for dt in case.dtypes:
            ops, ei, _ = tc.inputs(case, dt)
            qi, kk, _ = tc.rows(ops["qry"], ops["k"], ops["v"], None, ei, case.H)
            s = tc.scale_of(case) * (qi * kk).sum(-1)
            span = [s[ei[1] == d] for d in range(case.n_dst)]
            assert any(r.numel() and float(r.max()) > 100 and float(r.min()) < -100 for r in span)    # exp(100) overflows float32
            up, down, same = (s[ei[1] == tc.RANGE_ROWS[name]] for name in ("ascending", "descending", "equal"))
            assert up.size(0) == down.size(0) == same.size(0) == tc.SPECIAL
            assert bool((up[1:] > up[:-1]).all()) and bool((down[1:] < down[:-1]).all()) and bool((same == same[0]).all())
    assert {(c.H, c.C) for c in tc.SHAPES} >= {(H, C) for H in (1, 3, 4) for C in (1, 5, 8, 64, 136)}
    assert {(c.H, c.C) for c in tc.SHAPES if tc.has_u(c)} == set(tc.U_SHAPES)
    _, ei, _ = tc.inputs(tc.EDGES[0], torch.float32)
    pairs = [(int(s), int(d)) for s, d in ei.t()]
    assert len(set(pairs)) < len(pairs) and any(s == d for s, d in pairs)


def test_self_error_table(capsys):
    """The numbers the bars of the GPU tests are 4 x of: recomputed from the chain alone, equal to the committed JSON."""
    ch.check_self_error_table(tc, 5e-2, capsys)
