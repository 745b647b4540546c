"""The yardstick of the attention tests with edge features: gnnops.conv.edge_attention(..., u=) and
gnnops.conv.edge_attention_v1(..., edge_score=) (csrc/attention.hip) and the layers GATv2Conv / GATConv with edge_dim, restated per
edge in propagate order in torch float64 on the CPU, so that torch's own autograd differentiates them:

    v2   z = p[i] + q[j] + u[e] -> leaky_relu -> s[e, h] = sum_c att[h, c] * leaky(z)[e, h, c]        the message stays q[j]
    v1   pre[e, h] = att[h] . q[j, h] + d[i, h] + c[e, h] -> s = leaky_relu(pre)                       the message stays q[j]
    -> per-destination softmax by an explicit maximum (scatter amax), exp, index_add_ of the denominators, a division
    -> out = index_add_ by destination of a[e, h] * q[j, h, :]

No running maximum, no rescaling, no log-sum-exp. With u = 0 / c = 0 the two chains ARE attention_chain.attention / gate_chain.attention_v1
(test_attention_edge_chain_cpu.py pins that bit for bit, and ties them to a dense masked torch.softmax and to gradcheck).

``rnd`` (a torch dtype) runs the library's own steps in float32 with storage rounding, as the two older chains do: out rounded, delta
from the rounded out, a = exp(s - lse), ds = a (da - delta); v2: t = ds att leaky'(z), gq = a g + t rounded, ``gu = t`` rounded once;
v1: dpre = ds leaky'(pre), gq = a g + dpre att rounded, ``gc = dpre`` rounded once. ``self_error`` is the distance between the two
chains per tensor, recorded in tests/golden/attention_edge_self_error.json (``write_self_error_table`` regenerates it); the GPU bars are
PROJECT_BAR for fp32 / fp16 in the shape, seams and edges tables and the layers, 4 x the recorded self error for bf16 and for the range
and heavy tables — the rule of attention_chain.py.

The case tables, graphs, random draws and bars are those of attention_chain.py, gate_chain.py and conv_chain.py, imported; this module
adds the edge operand to their inputs (its own generator, so the older operands keep their values). The layer restatements follow
torch_geometric's GATv2Conv / GATConv with edge_dim: lin_edge without a bias, remove_self_loops then add_self_loops with fill_value
("mean": the mean of the attributes of a node's remaining in-edges, zero for a node without any). PyG is not available to compare
against: parity unpinned."""
import functools
import os

import torch

import attention_chain as ac
import chain_harness as ch
import gate_chain as gc
from attention_chain import SPECIAL, _amax, _dot, _exp, _log, with_self_loops  # noqa: F401
from chain_harness import BF16, DNAME, DTYPES, F16, F32, PROJECT_BAR, rel_err  # noqa: F401
from conv_chain import _q, _rand, _straight_through, place  # noqa: F401

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_edge_self_error.json")
SEAM_DEGREES = gc.SEAM_DEGREES      # 0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 129: every step of the halved unrolls, and the run of 64 ids


# ---- v2: a per-edge row u in the score ------------------------------------------------------------------------------------------
def scores_u(q, p, att, u, edge_index, H, slope):
    src, dst = edge_index[0], edge_index[1]
    C = att.numel() // H
    qj, pi = q[src].view(-1, H, C), p[dst].view(-1, H, C)
    z = pi + qj
    z = z + u.view(-1, H, C)
    return z, qj, _dot(torch.nn.functional.leaky_relu(z, slope), att.view(1, H, C))


def attention_u(q, p, att, u, edge_index, n_dst, H, slope=0.2):
    """(out [n_dst, H * C], lse [n_dst, H]); the dtype of q is the arithmetic."""
    dst = edge_index[1]
    C = att.numel() // H
    _, qj, s = scores_u(q, p, att, u, edge_index, H, slope)
    mx = _amax(s.detach(), dst, n_dst)
    ex = _exp(s - mx[dst])
    den = torch.zeros((n_dst, H), dtype=q.dtype).index_add_(0, dst, ex)
    a = ex / den[dst]
    out = torch.zeros((n_dst, H, C), dtype=q.dtype).index_add_(0, dst, a.unsqueeze(-1) * qj)
    return out.view(n_dst, H * C), mx + _log(den.detach())


def library_backward_u(f, out_r, lse, edge_index, n_dst, H, slope, g, rnd):
    """The steps of gnnops_edge_attention_backward (with u) + the segment sum of the autograd function, on float32 operands ``f``."""
    src, dst = edge_index[0], edge_index[1]
    q, p, att, u = f["q"], f["p"], f["att"], f["u"]
    C = att.numel() // H
    r = lambda t: _q(t, rnd)   # noqa: E731
    E = src.numel()
    if E == 0:
        return {k: torch.zeros_like(v) for k, v in f.items()}
    gh, oh = g.view(n_dst, H, C), out_r.view(n_dst, H, C)
    delta = _dot(gh, oh)
    z, qj, s = scores_u(q, p, att, u, edge_index, H, slope)
    a = _exp(s - lse[dst])
    ds = a * (_dot(gh[dst], qj) - delta[dst])
    t = ds.unsqueeze(-1) * att.view(1, H, C) * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    gq = r(a.unsqueeze(-1) * gh[dst] + t).reshape(E, H * C)
    rows = (ds.unsqueeze(-1) * torch.nn.functional.leaky_relu(z, slope)).reshape(E, H * C)
    seg = lambda rows_, index, n: torch.zeros((n, H * C), dtype=torch.float32).index_add_(0, index, rows_)   # noqa: E731
    return {"q": r(seg(gq, src, q.size(0))), "p": r(seg(t.reshape(E, H * C), dst, n_dst)),
            "att": r(seg(rows, torch.zeros(E, dtype=torch.int64), 1)).view(att.shape), "u": r(t).reshape(E, H * C)}


def attention_u_grads(ops, edge_index, n_dst, H, slope, R, rnd=None):
    """ops: {"q", "p", "att", "u"} float64 tensors of storage-rounded values. (out, {name: d sum(out * R)}) as float64."""
    if rnd is None:
        leaf = {k: v.detach().clone().requires_grad_(True) for k, v in ops.items()}
        out, _ = attention_u(leaf["q"], leaf["p"], leaf["att"], leaf["u"], edge_index, n_dst, H, slope)
        (out * R).sum().backward()
        return out.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}
    f = {k: v.float() for k, v in ops.items()}
    out, lse = attention_u(f["q"], f["p"], f["att"], f["u"], edge_index, n_dst, H, slope)
    out = _q(out, rnd)
    grads = library_backward_u(f, out, lse, edge_index, n_dst, H, slope, R.float(), rnd)
    return out.double(), {k: v.double() for k, v in grads.items()}


# ---- v1: a per-edge scalar c in the pre-activation ------------------------------------------------------------------------------
def attention_c(q, d, att, c, edge_index, n_dst, H, slope=0.2):
    """(out [n_dst, H * C], lse [n_dst, H]) of GATConv's pass with the edge term; the dtype of q is the arithmetic."""
    dst = edge_index[1]
    C = att.numel() // H
    _, r = gc.rows(q, None, edge_index, H, None)
    pre = _dot(r, att.view(1, H, C)) + d[dst]
    pre = pre + c
    s = torch.nn.functional.leaky_relu(pre, slope)
    mx = _amax(s.detach(), dst, n_dst)
    ex = _exp(s - mx[dst])
    den = torch.zeros((n_dst, H), dtype=q.dtype).index_add_(0, dst, ex)
    a = ex / den[dst]
    out = torch.zeros((n_dst, H, C), dtype=q.dtype).index_add_(0, dst, a.unsqueeze(-1) * r)
    return out.view(n_dst, H * C), mx + _log(den.detach())


def library_backward_c(f, out_r, lse, edge_index, n_dst, H, slope, g, rnd):
    """The steps of gnnops_edge_attention_v1_backward (with c) + the segment sum of the autograd function, on float32 operands ``f``."""
    src, dst = edge_index[0], edge_index[1]
    q, d, att, c = f["q"], f["d"], f["att"], f["c"]
    C = att.numel() // H
    r_ = lambda t: _q(t, rnd)   # noqa: E731
    E = src.numel()
    if E == 0:
        return {k: torch.zeros_like(v) for k, v in f.items()}
    gh, oh = g.view(n_dst, H, C), out_r.view(n_dst, H, C)
    delta = _dot(gh, oh)
    _, r = gc.rows(q, None, edge_index, H, None)
    pre = _dot(r, att.view(1, H, C)) + d[dst]
    pre = pre + c
    a = _exp(torch.nn.functional.leaky_relu(pre, slope) - lse[dst])
    ds = a * (_dot(gh[dst], r) - delta[dst])
    dpre = ds * gc._dleaky(pre, slope)
    gq = r_(a.unsqueeze(-1) * gh[dst] + dpre.unsqueeze(-1) * att.view(1, H, C)).reshape(E, H * C)
    seg = lambda rows_, index, n: torch.zeros((n, rows_.size(1)), dtype=torch.float32).index_add_(0, index, rows_)   # noqa: E731
    return {"q": r_(seg(gq, src, q.size(0))), "d": r_(seg(dpre, dst, n_dst)),
            "att": r_(seg((dpre.unsqueeze(-1) * r).reshape(E, H * C), torch.zeros(E, dtype=torch.int64), 1)).view(att.shape),
            "c": r_(dpre)}


def attention_c_grads(ops, edge_index, n_dst, H, slope, R, rnd=None):
    """ops: {"q", "d", "att", "c"} float64 tensors of storage-rounded values. (out, {name: d sum(out * R)}) as float64."""
    if rnd is None:
        leaf = {k: v.detach().clone().requires_grad_(True) for k, v in ops.items()}
        out, _ = attention_c(leaf["q"], leaf["d"], leaf["att"], leaf["c"], edge_index, n_dst, H, slope)
        (out * R).sum().backward()
        return out.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}
    f = {k: v.float() for k, v in ops.items()}
    out, lse = attention_c(f["q"], f["d"], f["att"], f["c"], edge_index, n_dst, H, slope)
    out = _q(out, rnd)
    grads = library_backward_c(f, out, lse, edge_index, n_dst, H, slope, R.float(), rnd)
    return out.double(), {k: v.double() for k, v in grads.items()}


# ---- cases: the tables of the two older chains, with the edge operand added -------------------------------------------------------
SEAM_SHAPES = ((3, 8), (1, 136), (1, 264))      # one, one and (fp32) two pieces per lane
V2 = {"shape": ac.SHAPES,
      "seams": [ac.Case("seams", f"H{H}-C{C}", H, C, graph="seams", n_src=140, n_dst=len(SEAM_DEGREES) + 3) for H, C in SEAM_SHAPES],
      "range": ac.RANGE, "heavy": ac.HEAVY, "edges": ac.EDGES}
_gat = lambda table: [c for c in table if c.variant == "gat"]   # noqa: E731
V1 = {"shape": [gc.Case("shape", c.name, c.H, c.C, variant="gat", layout=c.layout) for c in ac.SHAPES],
      "seams": _gat(gc.SEAMS), "range": _gat(gc.RANGE), "heavy": _gat(gc.HEAVY),
      "edges": [gc.Case("edges", c.name, c.H, c.C, variant="gat", graph=c.graph, E=c.E, n_src=c.n_src, n_dst=c.n_dst) for c in ac.EDGES]}
FAMILIES = {"v2": V2, "v1": V1}


def _edge_generator(case, salt):
    return torch.Generator().manual_seed(salt + sum(map(ord, case.table + case.name)))


def sort_by_destination(ei, *per_edge):
    """The same edges ordered by destination (stable), and their per-edge operands: the plan's perm is then the identity."""
    order = torch.sort(ei[1], stable=True).indices
    return (ei[:, order].contiguous(),) + tuple(t[order].contiguous() for t in per_edge)


def inputs_u(case, dtype, sorted_edges=False):
    """({"q", "p", "att", "u"}: float64 tensors of storage-rounded values, edge_index, R float64 storage-rounded)."""
    rd = lambda t: t.to(dtype).double()   # noqa: E731
    HC = case.H * case.C
    if case.graph == "seams":       # the degrees of gate_chain.SEAM_DEGREES, which attention_chain's own seams graph lacks
        g = _edge_generator(case, 1717)
        ei = gc.graph_of(case, g)
        ops = {"q": rd(_rand(g, case.n_src, HC)), "p": rd(_rand(g, case.n_dst, HC)), "att": rd(_rand(g, HC))}
        R = rd(_rand(g, case.n_dst, HC))
    else:
        ops, ei, R = ac.inputs(case, dtype)
    u = _rand(_edge_generator(case, 9191), ei.size(1), HC)
    if case.graph == "range":       # the ascending / descending / equal rows keep their scores: their edges are the last 3 * SPECIAL
        u[-3 * SPECIAL:] = 0
    ops = dict(ops, u=rd(u))
    if sorted_edges:
        ei, ops["u"] = sort_by_destination(ei, ops["u"])
    return ops, ei, R


def inputs_c(case, dtype, sorted_edges=False):
    """({"q", "d", "att", "c"}: float64 tensors of storage-rounded values, edge_index, R float64 storage-rounded)."""
    ops, ei, R, ks = gc.inputs(case, dtype)
    assert ks is None and "u" not in ops
    c = _rand(_edge_generator(case, 9292), ei.size(1), case.H)
    if case.graph == "range":       # as gate_chain scales its u there: the near-ties of a level survive
        c = c * 0.01
        c[-3 * SPECIAL:] = 0
    ops = dict(ops, c=c.to(dtype).double())
    if sorted_edges:
        ei, ops["c"] = sort_by_destination(ei, ops["c"])
    return ops, ei, R


def case_grads(family, case, dtype, rnd=None, sorted_edges=False):
    if family == "v2":
        ops, ei, R = inputs_u(case, dtype, sorted_edges)
        return attention_u_grads(ops, ei, case.n_dst, case.H, case.slope, R, rnd=rnd)
    ops, ei, R = inputs_c(case, dtype, sorted_edges)
    return attention_c_grads(ops, ei, case.n_dst, case.H, case.slope, R, rnd=rnd)


def key(family, case, dtype, tensor):
    return f"{family}/{case.key(dtype, tensor)}"


def self_error(family, case, dtype):
    return ch.self_error(functools.partial(case_grads, family), case, dtype)


def self_error_cases():
    return [(f, c, d) for f, tables in FAMILIES.items() for c, d in ch.self_bar_cases(tables) if c.E > 0]


def self_error_table():
    return ch.build_table(self_error_cases(), self_error, key)


def write_self_error_table(path=GOLDEN_FILE):
    """Regenerates tests/golden/attention_edge_self_error.json
    (python -c "import attention_edge_chain as ec; ec.write_self_error_table()")."""
    return ch.write_table(self_error_table(), path)


def load_self_error():
    return ch.load_table(GOLDEN_FILE)


# ---- the layers -----------------------------------------------------------------------------------------------------------------
def looped_attr(edge_index, edge_attr, n, fill_value):
    """The attributes of with_self_loops(edge_index, n): those of the edges with src != dst in their order, then one row per node —
    the mean of the attributes of its remaining in-edges (zero without any), or the constant."""
    keep = edge_index[0] != edge_index[1]
    kept = edge_attr[keep]
    if fill_value == "mean":
        dst = edge_index[1][keep]
        total = torch.zeros((n, edge_attr.size(1)), dtype=edge_attr.dtype).index_add_(0, dst, kept)
        loops = total / torch.bincount(dst, minlength=n).clamp(min=1).to(edge_attr.dtype).unsqueeze(1)
    else:
        loops = torch.full((n, edge_attr.size(1)), float(fill_value), dtype=edge_attr.dtype)
    return torch.cat([kept, loops], dim=0)


def gatv2_edge_ref(P, ei, n_dst, H, C, concat, slope, add_self_loops, fill_value, x, ea, xd=None, rd=None):
    """GATv2Conv(edge_dim).forward of torch_geometric on the parameters P. ``rd`` rounds, straight-through, what the device stores in
    16 bits and a leaky ReLU then gates on (q, p, u) and the self loops' attribute rows."""
    rd = rd or (lambda t: t)
    xt = x if xd is None else xd
    q = rd(x @ P["lin_l.weight"].t() + (P["lin_l.bias"] if "lin_l.bias" in P else 0))
    p = rd(xt @ P["lin_r.weight"].t() + (P["lin_r.bias"] if "lin_r.bias" in P else 0))
    if add_self_loops:
        n_kept = int((ei[0] != ei[1]).sum())
        ea = looped_attr(ei, ea, n_dst, fill_value)
        ea = torch.cat([ea[:n_kept], rd(ea[n_kept:])], dim=0)
        ei = with_self_loops(ei, n_dst)
    u = rd(ea @ P["lin_edge.weight"].t())
    out, _ = attention_u(q, p, P["att"].reshape(-1), u, ei, n_dst, H, slope)
    if not concat:
        out = out.view(n_dst, H, C).mean(dim=1)
    return out if "bias" not in P else out + P["bias"]


def _fold(att, W, H, C):
    """[H, in]: att[h] . W[h * C:(h + 1) * C, :] — x @ fold^T is att[h] . (x W^T)[h], the same sum in another order."""
    return torch.einsum("hc,hci->hi", att.view(H, C), W.view(H, C, W.size(1)))


def gat_edge_ref(P, ei, n_dst, H, C, concat, slope, add_self_loops, fill_value, x, ea, xd=None, rd=None, folded=True):
    """GATConv(edge_dim).forward of torch_geometric on the parameters P (lin_dst.weight absent: the shared lin_src). ``rd`` rounds,
    straight-through, what the device stores in 16 bits and a leaky ReLU then gates on. ``folded``: the two score terms as the layer
    forms them, d = x_i @ fold(att_dst, W_dst)^T and c = e @ fold(att_edge, W_e)^T with the folded weight stored (rounded) too — in
    exact arithmetic PyG's (x_i W_dst^T)[h] . att_dst[h], and in 16 bits the number the device's leaky ReLU gates on, where rounding
    PyG's order instead flips the gate of a pre-activation within an ulp of zero (a whole term of d x: 1.2e-2 of scale in the
    mean-over-heads fp16 case, against 5e-4 everywhere else). False keeps PyG's order for comparison."""
    rd = rd or (lambda t: t)
    Ws = P["lin_src.weight"]
    Wd = P.get("lin_dst.weight", Ws)
    xt = x if xd is None else xd
    q = rd(x @ Ws.t())
    if folded:
        d = rd(xt @ rd(_fold(P["att_dst"], Wd, H, C)).t())
    else:
        d = rd(((xt @ Wd.t()).view(-1, H, C) * P["att_dst"].view(1, H, C)).sum(-1))
    if add_self_loops:
        n_kept = int((ei[0] != ei[1]).sum())
        ea = looped_attr(ei, ea, n_dst, fill_value)
        ea = torch.cat([ea[:n_kept], rd(ea[n_kept:])], dim=0)
        ei = with_self_loops(ei, n_dst)
    if folded:
        c = rd(ea @ rd(_fold(P["att_edge"], P["lin_edge.weight"], H, C)).t())
    else:
        c = rd(((ea @ P["lin_edge.weight"].t()).view(-1, H, C) * P["att_edge"].view(1, H, C)).sum(-1))
    out, _ = attention_c(q, d, P["att_src"].reshape(-1), c, ei, n_dst, H, slope)
    if not concat:
        out = out.view(n_dst, H, C).mean(dim=1)
    return out if "bias" not in P else out + P["bias"]


class LayerCase:
    """One layer test with edge_dim = 3: ``setup`` builds the layer on the CPU from the test's own seeds, the inputs and the two ways
    to run it (the graph of attention_chain.LayerCase: 30 self loops and 30 repeated edges in the input, unless bipartite)."""

    def __init__(self, name, kind, cin, cout, heads, concat=True, share=False, bipartite=False, fill_value="mean", edge_dim=3):
        self.name, self.kind, self.cin, self.cout, self.heads, self.concat = name, kind, cin, cout, heads, concat
        self.share, self.bipartite, self.fill_value, self.edge_dim = share, bipartite, fill_value, edge_dim

    def setup(self, dtype):
        """(layer on the CPU, {input name: float32 tensor}, edge_index, run_dev, run_ref, output shape)."""
        from gnnops import conv

        torch.manual_seed(11)
        n_src, n_dst, e = (140, 90, 900) if self.bipartite else (200, 200, 1500)
        kw = dict(heads=self.heads, concat=self.concat, add_self_loops=not self.bipartite, edge_dim=self.edge_dim, fill_value=self.fill_value)
        if self.kind == "gatv2":
            layer = conv.GATv2Conv(self.cin, self.cout, share_weights=self.share, **kw)
        else:
            layer = conv.GATConv(self.cin, self.cout, **kw)
        layer = layer.to(dtype)
        with torch.no_grad():      # PyG starts the biases at zero: give them values
            for name, prm in layer.named_parameters():
                if name.endswith("bias"):
                    prm.copy_(_rand(torch.Generator().manual_seed(12), *prm.shape, scale=0.5))
        g = torch.Generator().manual_seed(13)
        ei = torch.stack([torch.randint(0, n_src, (e,), generator=g), torch.randint(0, n_dst, (e,), generator=g)])
        if not self.bipartite:
            ei[:, :30] = torch.randint(0, n_dst, (30,), generator=g)        # 30 self loops in the input
            ei[:, 30:60] = ei[:, 60:90]                                       # 30 repeated edges
            ei[1][ei[1] == 7] = 8                                             # node 7 keeps no in-edge: its loop's mean fill is a zero row
            ei[:, 0] = 7                                                      # ... but for a self loop, which is removed
        cs, cd = (self.cin, self.cin) if isinstance(self.cin, int) else self.cin
        inputs_ = {"x": _rand(g, n_src, cs)}
        if self.bipartite:
            inputs_["xd"] = _rand(g, n_dst, cd)
        inputs_["ea"] = _rand(g, e, self.edge_dim)
        H, C, rd = self.heads, self.cout, _straight_through(dtype)
        ref = gatv2_edge_ref if self.kind == "gatv2" else gat_edge_ref

        def run_dev(layer, x, ea, xd=None):
            return layer((x, xd) if self.bipartite else x, ei.cuda(), ea)

        def run_ref(P, x, ea, xd=None):
            P = dict(P)
            if self.share:
                P["lin_r.weight"] = P["lin_l.weight"]
                if "lin_l.bias" in P:
                    P["lin_r.bias"] = P["lin_l.bias"]
            return ref(P, ei, n_dst, H, C, self.concat, 0.2, not self.bipartite, self.fill_value, x, ea, xd, rd=rd)

        return layer, inputs_, ei, run_dev, run_ref, (n_dst, H * C if self.concat else C)


LAYER_CASES = [LayerCase("gatv2-concat", "gatv2", 16, 8, 4), LayerCase("gatv2-mean_heads", "gatv2", 16, 32, 4, concat=False),
               LayerCase("gatv2-share_weights", "gatv2", 12, 8, 3, share=True), LayerCase("gatv2-fill_0.5", "gatv2", 12, 5, 2, fill_value=0.5),
               LayerCase("gatv2-bipartite", "gatv2", 10, 8, 3, bipartite=True),
               LayerCase("gat-concat", "gat", 16, 8, 4), LayerCase("gat-mean_heads", "gat", 16, 32, 4, concat=False),
               LayerCase("gat-fill_0.5", "gat", 12, 5, 2, fill_value=0.5), LayerCase("gat-bipartite", "gat", (10, 7), 8, 3, bipartite=True)]
GATV2_EDGE_STATE = dict(ac.PYG_STATE, **{"lin_edge.weight": (128, 3)})
GAT_EDGE_STATE = dict(gc.GAT_STATE, **{"lin_edge.weight": (128, 3), "att_edge": (1, 4, 32)})
