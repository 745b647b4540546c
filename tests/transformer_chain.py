"""The yardstick of the TransformerConv tests: gnnops.conv.edge_attention_dot (csrc/attention.hip, dot_fwd_kernel / dot_bwd_kernel) and
gnnops.conv.TransformerConv restated per edge in propagate order in torch float64 on the CPU, so that torch's own autograd
differentiates them:

    gather qry[i], k[j], v[j] -> kk = k[j] (+ u[e]), vv = v[j] (+ u[e]) -> s[e, h] = scale * sum_c qry[i, h, c] * kk[e, h, c]
    -> per-destination softmax by an explicit maximum (scatter amax), exp, index_add_ of the denominators, a division
    -> out = index_add_ by destination of a[e, h] * ks[e, h] * vv[e, h, :]          (ks: the attention dropout scale, after the softmax)

No running maximum, no rescaling, no log-sum-exp: the kernel's online softmax shares none of it. test_transformer_chain_cpu.py ties
this chain to a dense masked torch.softmax formulation, to torch.autograd.gradcheck and to a two-edge example worked by hand.

``rnd`` (a torch dtype) runs the library's own steps in float32 with every tensor the library materialises rounded to the storage
type, as attention_chain.library_backward does: ``out``; on the way back ``delta = sum_c g * out`` from that ROUNDED out, the scores
recomputed, a = exp(s - lse), ds = a * (ks * (g . vv) - delta), the per-edge rows ``gkv = [ds * scale * qry[i] | a * ks * g[i]]`` rounded,
their ONE segment sum by source ([d k | d v]) rounded, ``gu`` = the sum of the two unrounded halves rounded once, ``d qry`` = scale * the
float32 sum of ds * kk rounded once. ``self_error`` is the distance between the two chains, per tensor max |got - want| / max |want|:
the reference against itself, never the kernels. It is recorded in tests/golden/transformer_self_error.json
(``write_self_error_table`` regenerates it); the GPU bars of bf16 and of the range and heavy tables are 4 x that distance, fp32 and
fp16 in the shape / seams / plan / edges tables and the layers keep PROJECT_BAR — the rule of attention_chain.py.

Before the kernel was written, 4 x the self error of every fp32 / fp16 case of the PROJECT_BAR group was computed on the CPU
(``project_group_check``): none exceeds its PROJECT_BAR (the largest is 0.30 of it), so no case moved to the self-error group.

Case, the graphs, the random draws and the bars are attention_chain's and conv_chain's, imported; the seams graph is built here from
gate_chain.SEAM_DEGREES, which has every step of this pass's unrolls (4 forward; 2 and 1 backward) and its neighbours. The layer
restatement follows torch_geometric's TransformerConv (lin_key / lin_query / lin_value with biases, lin_edge without, lin_skip,
lin_beta on [out, x_r, out - x_r]; no self loops added; mean over heads when concat=False). PyG is not available to compare
against: parity unpinned."""
import functools
import math
import os
from dataclasses import dataclass

import torch

import attention_chain as ac
import chain_harness as ch
from attention_chain import Case, SPECIAL, _amax, _dot, _exp, _log  # noqa: F401
from chain_harness import BF16, DNAME, DTYPES, F16, F32, PROJECT_BAR, rel_err  # noqa: F401
from conv_chain import _lin, _q, _rand, _straight_through, place  # noqa: F401
from gate_chain import SEAM_DEGREES

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transformer_self_error.json")


# ---- the op -----------------------------------------------------------------------------------------------------------------
def rows(qry, k, v, u, edge_index, H):
    """(qi, kk, vv) [E, H, C]: the destination's query row and the edge's key and value rows."""
    src, dst = edge_index[0], edge_index[1]
    C = qry.size(1) // H
    qi, kk, vv = qry[dst].view(-1, H, C), k[src].view(-1, H, C), v[src].view(-1, H, C)
    if u is not None:
        kk, vv = kk + u.view(-1, H, C), vv + u.view(-1, H, C)
    return qi, kk, vv


def attention(qry, k, v, edge_index, n_dst, H, scale, u=None, ks=None):
    """(out [n_dst, H * C], lse [n_dst, H]); the dtype of qry is the arithmetic. ks [E, H] multiplies the weighted sum only."""
    dst = edge_index[1]
    C = qry.size(1) // H
    qi, kk, vv = rows(qry, k, v, u, edge_index, H)
    s = scale * _dot(qi, kk)
    mx = _amax(s.detach(), dst, n_dst)
    ex = _exp(s - mx[dst])
    den = torch.zeros((n_dst, H), dtype=qry.dtype).index_add_(0, dst, ex)
    a = ex / den[dst]
    if ks is not None:
        a = a * ks
    out = torch.zeros((n_dst, H, C), dtype=qry.dtype).index_add_(0, dst, a.unsqueeze(-1) * vv)
    return out.view(n_dst, H * C), mx + _log(den.detach())


def library_backward(f, out_r, lse, edge_index, n_dst, H, scale, g, rnd, ks=None):
    """The steps of gnnops_edge_attention_dot_backward + the segment sum of `_EdgeAttentionDot.backward` on float32 operands ``f``;
    ``out_r`` is the rounded forward output."""
    src, dst = edge_index[0], edge_index[1]
    qry, k, v, u = f["qry"], f["k"], f["v"], f.get("u")
    HC = qry.size(1)
    C = HC // H
    r = lambda t: _q(t, rnd)   # noqa: E731
    E = src.numel()
    if E == 0:
        return {name: torch.zeros_like(t) for name, t in f.items()}
    scale = torch.tensor(scale, dtype=torch.float32)
    gh, oh = g.view(n_dst, H, C), out_r.view(n_dst, H, C)
    delta = _dot(gh, oh)
    qi, kk, vv = rows(qry, k, v, u, edge_index, H)
    s = scale * _dot(qi, kk)
    a = _exp(s - lse[dst])
    da = _dot(gh[dst], vv)
    wk = a
    if ks is not None:
        da, wk = ks * da, a * ks
    ds = a * (da - delta[dst])
    k_half = (ds * scale).unsqueeze(-1) * qi
    v_half = wk.unsqueeze(-1) * gh[dst]
    seg = lambda rows_, index, n: torch.zeros((n, HC), dtype=torch.float32).index_add_(0, index, rows_.reshape(E, HC))   # noqa: E731
    grads = {"qry": r(scale * seg(ds.unsqueeze(-1) * kk, dst, n_dst)), "k": r(seg(r(k_half), src, k.size(0))), "v": r(seg(r(v_half), src, v.size(0)))}
    if u is not None:
        grads["u"] = r(k_half + v_half).reshape(E, HC)
    return grads


def dot_grads(ops, edge_index, n_dst, H, scale, R, rnd=None, ks=None):
    """ops: {"qry", "k", "v"} (and "u") float64 tensors of storage-rounded values. (out, {name: d sum(out * R)}) as float64: torch
    autograd of the float64 chain, or with ``rnd`` the library's own steps in float32 with storage rounding."""
    if rnd is None:
        leaf = {name: t.detach().clone().requires_grad_(True) for name, t in ops.items()}
        out, _ = attention(leaf["qry"], leaf["k"], leaf["v"], edge_index, n_dst, H, scale, leaf.get("u"), ks)
        (out * R).sum().backward()
        return out.detach(), {name: (t.grad if t.grad is not None else torch.zeros_like(t)) for name, t in leaf.items()}
    f = {name: t.float() for name, t in ops.items()}
    ksf = None if ks is None else ks.float()
    out, lse = attention(f["qry"], f["k"], f["v"], edge_index, n_dst, H, float(torch.tensor(scale, dtype=torch.float32)), f.get("u"), ksf)
    out = _q(out, rnd)
    grads = library_backward(f, out, lse, edge_index, n_dst, H, scale, R.float(), rnd, ksf)
    return out.double(), {name: t.double() for name, t in grads.items()}


# ---- cases ------------------------------------------------------------------------------------------------------------------
# a case whose name ends in "-u" runs with the per-edge row u
U_SHAPES = ((3, 8), (1, 136), (4, 64))
SHAPES = [Case("shape", f"H{H}-C{C}", H, C) for H in (1, 3, 4) for C in (1, 5, 8, 64, 136)] + [Case("shape", "H4-C8-dense", 4, 8, layout="plain")]
SHAPES += [Case("shape", f"H{H}-C{C}-u", H, C) for H, C in U_SHAPES]
SEAMS = [Case("seams", f"H{H}-C{C}{sfx}", H, C, graph="seams", n_src=140, n_dst=len(SEAM_DEGREES) + 3) for H, C, sfx in ((3, 8, ""), (1, 136, ""), (3, 8, "-u"))]
RANGE = [Case("range", f"H{H}-C{C}", H, C, graph="range", E=700, n_src=120, n_dst=100, bar="self") for H, C in ((3, 8), (1, 64))]
HEAVY = [Case("heavy", f"H{H}-C{C}{sfx}", H, C, graph="heavy", E=1500, n_src=400, n_dst=60, bar="self") for H, C, sfx in ((3, 8, ""), (1, 136, ""), (3, 8, "-u"))]
PLAN = [Case("plan", f"E{E}", 2, 8, E=E, n_src=300, n_dst=300) for E in (24576, 24577)]
EDGES = [Case("edges", "dup_and_self_loops", 3, 5, graph="dup", E=600, n_src=50, n_dst=50),
         Case("edges", "dup_and_self_loops-u", 3, 5, graph="dup", E=600, n_src=50, n_dst=50),
         Case("edges", "E0", 3, 8, graph="empty", E=0, n_src=5, n_dst=4),
         Case("edges", "E0-u", 3, 8, graph="empty", E=0, n_src=5, n_dst=4)]
TABLES = {"shape": SHAPES, "seams": SEAMS, "range": RANGE, "heavy": HEAVY, "plan": PLAN, "edges": EDGES}
RANGE_ROWS = ac.RANGE_ROWS
HEAVY_DEGREES = ac.HEAVY_DEGREES


def has_u(case):
    return case.name.endswith("-u")


def scale_of(case):
    return 1.0 / math.sqrt(case.C)


def graph_of(case, g):
    if case.graph != "seams":
        return ac.graph_of(case, g)
    # destination k has SEAM_DEGREES[k] edges; three ordinary rows follow
    dst = torch.cat([torch.full((d,), k, dtype=torch.int64) for k, d in enumerate(SEAM_DEGREES)]
                    + [torch.randint(len(SEAM_DEGREES), case.n_dst, (20,), generator=g)])
    src = torch.randint(0, case.n_src, (dst.numel(),), generator=g)
    perm = torch.randperm(dst.numel(), generator=g)
    return torch.stack([src[perm], dst[perm]])


def inputs(case, dtype, seed=2121):
    """({"qry", "k", "v"} (and "u"): float64 tensors of storage-rounded values, edge_index, R float64 storage-rounded)."""
    g = torch.Generator().manual_seed(seed + sum(map(ord, case.table + case.name)))
    ei = graph_of(case, g)
    HC = case.H * case.C
    rd = lambda t: t.to(dtype).double()   # noqa: E731
    qry, k, v = _rand(g, case.n_dst, HC), _rand(g, case.n_src, HC), _rand(g, case.n_src, HC)
    if case.graph == "range":
        # the ordinary rows: qry and k over +-20, so scale * qry . k has a deviation past a hundred and the scores of a destination lie
        # hundreds apart (a softmax without a running maximum overflows float32 past 88). Rows 0 / 1 / 2: qry = t with entries +-1 and
        # k[j] = level * t, so every head's score is level * sqrt(C): levels ascending, descending, all equal.
        qry, k = qry * 20, k * 20
        t = torch.sign(_rand(g, HC))
        t[t == 0] = 1.0
        levels = torch.linspace(-60.0, 60.0, SPECIAL)
        qry[:3] = t
        k[:SPECIAL] = levels.unsqueeze(1) * t
        k[SPECIAL:2 * SPECIAL] = levels.flip(0).unsqueeze(1) * t
        k[2 * SPECIAL:3 * SPECIAL] = 17.0 * t
    R = _rand(g, case.n_dst, HC)
    ops = {"qry": rd(qry), "k": rd(k), "v": rd(v)}
    if has_u(case):
        ops["u"] = rd(_rand(g, ei.size(1), HC))
    return ops, ei, rd(R)


def case_grads(case, dtype, rnd=None):
    ops, ei, R = inputs(case, dtype)
    return dot_grads(ops, ei, case.n_dst, case.H, scale_of(case), R, rnd=rnd)


self_error = functools.partial(ch.self_error, case_grads)


def self_error_cases():
    return ch.self_bar_cases(TABLES)


def project_group_check():
    """[(case id, tensor, 4 x self error, PROJECT_BAR)] of the fp32 / fp16 cases judged by PROJECT_BAR whose 4 x self error exceeds
    it: empty. The largest: fp16 shape/H3-C8 d k, self error 7.4e-4 (4 x = 0.30 of 1e-2); fp32 plan/E24577 d qry, 5.8e-7 (0.08 of 3e-5)."""
    over = []
    for t in TABLES.values():
        for c in t:
            for d in c.dtypes:
                if c.self_bar(d):
                    continue
                for name, e in self_error(c, d).items():
                    if 4 * e > PROJECT_BAR[d]:
                        over.append((c.id(d), name, 4 * e, PROJECT_BAR[d]))
    return over


def dropout_mask(case, p=0.5, seed=31):
    """edge_scale [E, H] of zeros and 1 / (1 - p) entries for a case, float64."""
    _, ei, _ = inputs(case, torch.float32)
    keep = torch.rand((ei.size(1), case.H), generator=torch.Generator().manual_seed(seed)) >= p
    return keep.double() / (1.0 - p)


# ---- the layer ----------------------------------------------------------------------------------------------------------------
def transformer_ref(P, ei, n_dst, H, C, concat, x, xd=None, ea=None, edge_scale=None, rd=None):
    """TransformerConv.forward of torch_geometric on the parameters P, in the dtype of x. root_weight / beta / edge features are read
    off the keys of P. ``rd`` (16-bit storage): rounds the projections straight-through, as the device stores them."""
    rd = rd or (lambda t: t)
    xt = x if xd is None else xd
    qry = rd(_lin(xt, P["lin_query.weight"], P.get("lin_query.bias")))
    k = rd(_lin(x, P["lin_key.weight"], P.get("lin_key.bias")))
    v = rd(_lin(x, P["lin_value.weight"], P.get("lin_value.bias")))
    u = rd(_lin(ea, P["lin_edge.weight"])) if "lin_edge.weight" in P else None
    out, _ = attention(qry, k, v, ei, n_dst, H, 1.0 / math.sqrt(C), u, edge_scale)
    if not concat:
        out = out.view(n_dst, H, C).mean(dim=1)
    if "lin_skip.weight" in P:
        x_r = rd(_lin(xt, P["lin_skip.weight"], P.get("lin_skip.bias")))
        if "lin_beta.weight" in P:
            beta = torch.sigmoid(torch.cat([out, x_r, out - x_r], dim=-1) @ P["lin_beta.weight"].t())
            out = beta * x_r + (1 - beta) * out
        else:
            out = out + x_r
    return out


@dataclass(frozen=True)
class LayerCase:
    name: str
    cin: int
    cout: int
    heads: int
    concat: bool = True
    beta: bool = False
    edge_dim: int = None
    root_weight: bool = True
    bipartite: bool = False

    def setup(self, dtype, dropout=0.0):
        """(layer on the CPU, {input name: float32 tensor}, edge_index, run_dev, run_ref, output shape)."""
        from gnnops import conv

        torch.manual_seed(11)
        n_src, n_dst, e = (140, 90, 900) if self.bipartite else (200, 200, 1500)
        layer = conv.TransformerConv((self.cin, self.cin + 3) if self.bipartite else self.cin, self.cout, heads=self.heads, concat=self.concat,
                                     beta=self.beta, dropout=dropout, edge_dim=self.edge_dim, root_weight=self.root_weight).to(dtype)
        g = torch.Generator().manual_seed(13)
        ei = torch.stack([torch.randint(0, n_src, (e,), generator=g), torch.randint(0, n_dst, (e,), generator=g)])
        if not self.bipartite:
            ei[:, :30] = torch.randint(0, n_dst, (30,), generator=g)        # 30 self loops in the input: they stay
            ei[:, 30:60] = ei[:, 60:90]                                       # 30 repeated edges
        inputs_ = {"x": _rand(g, n_src, self.cin)}
        if self.bipartite:
            inputs_["xd"] = _rand(g, n_dst, self.cin + 3)
        if self.edge_dim is not None:
            inputs_["ea"] = _rand(g, e, self.edge_dim)
        H, C = self.heads, self.cout

        def run_dev(layer, x, xd=None, ea=None):
            return layer((x, xd) if self.bipartite else x, ei.cuda(), ea)

        def run_ref(P, x, xd=None, ea=None, edge_scale=None):
            return transformer_ref(P, ei, n_dst, H, C, self.concat, x, xd, ea, edge_scale, rd=_straight_through(dtype))

        return layer, inputs_, ei, run_dev, run_ref, (n_dst, H * C if self.concat else C)


LAYER_CASES = [LayerCase("concat", 16, 8, 4), LayerCase("mean_heads", 16, 32, 4, concat=False), LayerCase("beta", 12, 8, 3, beta=True),
               LayerCase("edge_dim", 12, 8, 3, edge_dim=8), LayerCase("no_root", 12, 5, 2, root_weight=False),
               LayerCase("bipartite", 10, 8, 3, bipartite=True)]
# TransformerConv(16, 32, heads=4, concat=False, beta=True, edge_dim=8)
PYG_STATE = {"lin_key.weight": (128, 16), "lin_key.bias": (128,), "lin_query.weight": (128, 16), "lin_query.bias": (128,),
             "lin_value.weight": (128, 16), "lin_value.bias": (128,), "lin_edge.weight": (128, 8), "lin_skip.weight": (32, 16),
             "lin_skip.bias": (32,), "lin_beta.weight": (1, 96)}


# ---- the table ----------------------------------------------------------------------------------------------------------------
def self_error_table():
    return ch.build_table(self_error_cases(), self_error)


def write_self_error_table(path=GOLDEN_FILE):
    """Regenerates tests/golden/transformer_self_error.json (python -c "import transformer_chain as tc; tc.write_self_error_table()")."""
    return ch.write_table(self_error_table(), path)


def load_self_error():
    return ch.load_table(GOLDEN_FILE)
