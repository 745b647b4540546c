"""The yardstick of the second attention family: gnnops.conv.edge_attention_v1 (csrc/attention.hip, gate_fwd_kernel /
gate_bwd_kernel) and the layers on it — GATConv, GATEConv, AttentiveFP — restated per edge in propagate order in torch float64 on
the CPU, so that torch's own autograd differentiates them:

    gather q[j] -> t = q[j] + u[e] -> r = t or leaky_relu(t, row_slope) -> pre[e, h] = sum_c att[h, c] * r[e, h, c] + d[i, h]
    -> s = leaky_relu(pre, slope) -> per-destination softmax by an explicit maximum (scatter amax), exp, index_add_ of the
    denominators, a division -> times edge_scale[e, h] (after the softmax: the denominator never sees it)
    -> out = index_add_ by destination of the weighted r

No running maximum, no rescaling, no log-sum-exp. test_gate_chain_cpu.py ties this chain to a dense masked torch.softmax
formulation, to torch.autograd.gradcheck and to a two-edge example worked by hand.

``rnd`` (a torch dtype) runs the library's own steps in float32 with every tensor the library materialises rounded to the storage
type, exactly as attention_chain.py does for the first family: ``out``; ``delta = sum_c g * out`` from the ROUNDED out; the scores
recomputed; a = exp(s - lse); da = k (g . r); ds = a (da - delta); dpre = ds leaky'(pre); the per-edge rows
``gq = (a k g + dpre att) f'(t)`` rounded (d u), their segment sum by source (d q) rounded, d d (float32 sum, rounded once) and d att
(float32 partial sums, rounded once). ``self_error`` is the distance between the two chains per tensor, max |got - want| / max |want|,
recorded in tests/golden/gate_attention_self_error.json (``write_self_error_table`` regenerates it). The GPU bars: PROJECT_BAR of
conv_chain.py for fp32 / fp16 in the shape, seams, plan and edges tables and for the layers; 4 x the recorded self error, per case and
tensor, for bf16 and for the range, heavy and mask tables — the rule of test_attention_gpu.py.

The layer restatements follow torch_geometric 2.0.x (GATConv: lin_src / lin_dst / att_src / att_dst; models.attentive_fp: GATEConv
and AttentiveFP). Where the device stores a tensor in 16 bits that a leaky ReLU then gates on (q, d, u), the float64 chain rounds it
straight-through, for the reason attention_chain.py gives. PyG is not available to compare against: parity unpinned."""
import functools
import os
from dataclasses import dataclass

import torch

import attention_chain as ac
import chain_harness as ch
from attention_chain import HEAVY_DEGREES, RANGE_ROWS, SPECIAL, T_HUB, _amax, _dot, _exp, _log, with_self_loops  # noqa: F401
from chain_harness import BF16, DNAME, DTYPES, F16, F32, PROJECT_BAR, rel_err  # noqa: F401
from conv_chain import _q, _rand, _straight_through, place, small_plan_fits  # noqa: F401

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gate_attention_self_error.json")
# the unrolls of the new kernels are 8, 4, 2, 1 forward and 4, 2, 1 backward (halved with u): U - 1, U, U + 1 of each, and the id run of 64
SEAM_DEGREES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 129)
VARIANTS = {"gat": (False, None), "u": (True, None), "row": (False, 0.01), "gate": (True, 0.01)}     # name -> (u present, row_slope)
MASK_DEAD_DST = 5     # the destination whose edges are all dropped in the mask cases


def _leaky(t, slope):
    return t if slope is None else torch.nn.functional.leaky_relu(t, slope)


def _dleaky(t, slope):
    return torch.ones_like(t) if slope is None else torch.where(t > 0, torch.ones_like(t), torch.full_like(t, slope))


# ---- the op -----------------------------------------------------------------------------------------------------------------
def rows(q, u, edge_index, H, row_slope):
    """(t, r) [E, H, C] of every edge."""
    t = q[edge_index[0]].view(edge_index.size(1), H, -1)
    if u is not None:
        t = t + u.view(t.shape)
    return t, _leaky(t, row_slope)


def attention_v1(q, d, att, edge_index, n_dst, H, u=None, row_slope=None, slope=0.2, edge_scale=None):
    """(out [n_dst, H * C], lse [n_dst, H]); the dtype of q is the arithmetic."""
    dst = edge_index[1]
    C = att.numel() // H
    _, r = rows(q, u, edge_index, H, row_slope)
    pre = _dot(r, att.view(1, H, C)) + d[dst]
    s = torch.nn.functional.leaky_relu(pre, slope)
    mx = _amax(s.detach(), dst, n_dst)
    ex = _exp(s - mx[dst])
    den = torch.zeros((n_dst, H), dtype=q.dtype).index_add_(0, dst, ex)
    a = ex / den[dst]
    if edge_scale is not None:
        a = a * edge_scale
    out = torch.zeros((n_dst, H, C), dtype=q.dtype).index_add_(0, dst, a.unsqueeze(-1) * r)
    return out.view(n_dst, H * C), mx + _log(den.detach())


def library_backward(f, out_r, lse, edge_index, n_dst, H, row_slope, slope, edge_scale, g, rnd):
    """The steps of gnnops_edge_attention_v1_backward + the segment sum of the autograd function, on float32 operands ``f``."""
    src, dst = edge_index[0], edge_index[1]
    q, d, att, u = f["q"], f["d"], f["att"], f.get("u")
    C = att.numel() // H
    r_ = lambda t: _q(t, rnd)   # noqa: E731
    E = src.numel()
    if E == 0:
        return {k: torch.zeros_like(v) for k, v in f.items()}
    gh, oh = g.view(n_dst, H, C), out_r.view(n_dst, H, C)
    delta = _dot(gh, oh)
    t, r = rows(q, u, edge_index, H, row_slope)
    pre = _dot(r, att.view(1, H, C)) + d[dst]
    a = _exp(torch.nn.functional.leaky_relu(pre, slope) - lse[dst])
    da = _dot(gh[dst], r)
    ak = a
    if edge_scale is not None:
        da, ak = edge_scale * da, a * edge_scale
    ds = a * (da - delta[dst])
    dpre = ds * _dleaky(pre, slope)
    gq = r_((ak.unsqueeze(-1) * gh[dst] + dpre.unsqueeze(-1) * att.view(1, H, C)) * _dleaky(t, row_slope)).reshape(E, H * C)
    seg = lambda rows_, index, n: torch.zeros((n, rows_.size(1)), dtype=torch.float32).index_add_(0, index, rows_)   # noqa: E731
    grads = {"q": r_(seg(gq, src, q.size(0))), "d": r_(seg(dpre, dst, n_dst)),
             "att": r_(seg((dpre.unsqueeze(-1) * r).reshape(E, H * C), torch.zeros(E, dtype=torch.int64), 1)).view(att.shape)}
    if u is not None:
        grads["u"] = gq
    return grads


def attention_grads(ops, edge_index, n_dst, H, row_slope, slope, edge_scale, R, rnd=None):
    """ops: {"q", "d", "att"[, "u"]} float64 tensors of storage-rounded values. (out, {name: d sum(out * R)}) as float64: torch
    autograd of the float64 chain, or with ``rnd`` the library's own steps in float32 with storage rounding."""
    if rnd is None:
        leaf = {k: v.detach().clone().requires_grad_(True) for k, v in ops.items()}
        out, _ = attention_v1(leaf["q"], leaf["d"], leaf["att"], edge_index, n_dst, H, leaf.get("u"), row_slope, slope, edge_scale)
        (out * R).sum().backward()
        return out.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}
    f = {k: v.float() for k, v in ops.items()}
    ks = None if edge_scale is None else edge_scale.float()
    out, lse = attention_v1(f["q"], f["d"], f["att"], edge_index, n_dst, H, f.get("u"), row_slope, slope, ks)
    out = _q(out, rnd)
    grads = library_backward(f, out, lse, edge_index, n_dst, H, row_slope, slope, ks, R.float(), rnd)
    return out.double(), {k: v.double() for k, v in grads.items()}


# ---- cases ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case(ch.CaseBars):
    table: str
    name: str
    H: int
    C: int
    variant: str = "gat"         # VARIANTS
    graph: str = "random"        # random | seams | range | heavy | dup | empty
    E: int = 2000
    n_src: int = 257
    n_dst: int = 300
    layout: str = "block"        # block: q and d column blocks of a wider matrix; plain: dense
    bar: str = "project"         # project: PROJECT_BAR for fp32 / fp16, 4 x self error for bf16; self: 4 x self error for all
    mask: bool = False           # edge_scale: Bernoulli(1/2) / (1/2), every edge of destination MASK_DEAD_DST dropped
    dtypes: tuple = tuple(DTYPES)
    slope: float = 0.2

    @property
    def has_u(self):
        return VARIANTS[self.variant][0]

    @property
    def row_slope(self):
        return VARIANTS[self.variant][1]


def _both(table, shapes, **kw):
    return [Case(table, f"H{H}-C{C}-{v}", H, C, variant=v, **kw) for H, C in shapes for v in ("gat", "gate")]


SHAPES = [Case("shape", f"H{H}-C{C}-{v}", H, C, variant=v) for H in (1, 3, 4) for C in (1, 5, 8, 64, 136) for v in VARIANTS]
SHAPES += [Case("shape", "H4-C8-gate-dense", 4, 8, variant="gate", layout="plain")]
# one column in and an odd pitch: single-element accesses, so 136 / 100 pieces per head = the 4- and 2-pieces-per-lane instances
SHAPES += [Case("shape", f"H{H}-C{C}-{v}-misaligned", H, C, variant=v, layout="misaligned") for H, C in ((2, 136), (3, 100)) for v in ("gat", "gate")]
SEAMS = _both("seams", ((3, 8), (1, 136), (1, 264)), graph="seams", n_src=140, n_dst=len(SEAM_DEGREES) + 3)
RANGE = _both("range", ((3, 8), (1, 64)), graph="range", E=700, n_src=120, n_dst=100, bar="self")
HEAVY = _both("heavy", ((3, 8), (1, 136)), graph="heavy", E=1500, n_src=400, n_dst=60, bar="self")
MASK = _both("mask", ((3, 8), (1, 136)), E=900, n_src=120, n_dst=100, bar="self", mask=True)
PLAN = [Case("plan", f"E{E}", 2, 8, variant="gate", E=E, n_src=300, n_dst=300) for E in (24576, 24577)]
EDGES = [Case("edges", "dup_and_self_loops", 3, 5, variant="gate", graph="dup", E=600, n_src=50, n_dst=50),
         Case("edges", "E0", 3, 8, variant="gate", graph="empty", E=0, n_src=5, n_dst=4)]
TABLES = {"shape": SHAPES, "seams": SEAMS, "range": RANGE, "heavy": HEAVY, "mask": MASK, "plan": PLAN, "edges": EDGES}


def graph_of(case, g):
    if case.graph != "seams":
        return ac.graph_of(case, g)
    dst = torch.cat([torch.full((d,), k, dtype=torch.int64) for k, d in enumerate(SEAM_DEGREES)]
                    + [torch.randint(len(SEAM_DEGREES), case.n_dst, (20,), generator=g)])
    src = torch.randint(0, case.n_src, (dst.numel(),), generator=g)
    perm = torch.randperm(dst.numel(), generator=g)
    return torch.stack([src[perm], dst[perm]])


def inputs(case, dtype, seed=777):
    """({"q", "d", "att"[, "u"]}: float64 tensors of storage-rounded values, edge_index, R, edge_scale or None — all float64,
    storage-rounded)."""
    g = torch.Generator().manual_seed(seed + sum(map(ord, case.table + case.name)))
    ei = graph_of(case, g)
    E, H, HC = ei.size(1), case.H, case.H * case.C
    rd = lambda t: t.to(dtype).double()   # noqa: E731
    q, d, att = _rand(g, case.n_src, HC), _rand(g, case.n_dst, H), _rand(g, HC)
    u = _rand(g, E, HC) if case.has_u else None
    if case.graph == "range":
        # ordinary rows: att . r up to hundreds, so the scores of a destination lie hundreds apart (a softmax without a running maximum
        # overflows float32 past 88). Rows 0 / 1 / 2 (their edges are the last 3 * SPECIAL, from sources kept for them): d = 0, u = 0
        # and q[j] = level * w with att[c] * w[c] > 0, so every head's score is strictly increasing in the level (both leaky ReLUs
        # are): levels ascending, descending, all equal.
        # Scores hundreds apart from rows of ordinary size: att is scaled so that sum_c |att[h, c]| = 160 in every head, and an ordinary
        # source is  level * sign(att) + w  with w (up to 1 an element) made orthogonal, head by head, to att times the slope each
        # element meets in the row's leaky ReLU, so w does not move the score. A fifth of the sources have level +1 (att . r about
        # +160), a fifth -1, the rest a level within +-0.01 (scores within a few units of zero, on both sides of the kink, which is
        # what gives d d its size). Sources of one level nearly TIE although their rows differ by their whole size, so a
        # destination's leading edges share an ordinary softmax hundreds above the rest, and every gradient is as large as the rows.
        # That matters for the bar: the backward reads delta = g . out from the output stored in 16 bits, an error of 2^-9 of the
        # ROW's size. Rows of size 60 that differ only where the scores differ (scores one apart: rows 1 / 150 apart) leave an error
        # there that swamps every gradient — self error above 1 in bf16, a bar that would admit a zero gradient.
        att = att * (160.0 / att.view(H, case.C).abs().sum(1)).repeat_interleave(case.C)
        first = 3 * SPECIAL
        nb = case.n_src - first
        pick = torch.rand(nb, H, 1, generator=g)
        level = torch.where(pick < 0.2, 1.0, torch.where(pick < 0.4, -1.0, 0.0)) + _rand(g, nb, H, 1) * 0.01
        base = level * torch.sign(att).view(1, H, case.C)                                        # [nb, H, C]
        w = _rand(g, nb, H, case.C)
        eff = att.view(1, H, case.C) * (torch.ones_like(base) if case.row_slope is None else torch.where(base + w > 0, 1.0, case.row_slope))
        w = w - eff * ((w * eff).sum(-1, keepdim=True) / (eff * eff).sum(-1, keepdim=True).clamp(min=1e-30))
        q[first:] = (base + w).reshape(nb, HC)
        if u is not None:
            u = u * 0.01
        w = torch.sign(att) * 0.5
        w[w == 0] = 0.5
        levels = torch.linspace(-60.0, 60.0, SPECIAL)
        d[:3] = 0
        q[:SPECIAL] = levels.unsqueeze(1) * w
        q[SPECIAL:2 * SPECIAL] = levels.flip(0).unsqueeze(1) * w
        q[2 * SPECIAL:3 * SPECIAL] = 17.0 * w
        if u is not None:
            u[-3 * SPECIAL:] = 0
    ks = None
    if case.mask:
        ks = (torch.rand(E, H, generator=g) >= 0.5).double() * 2.0
        ks[ei[1] == MASK_DEAD_DST] = 0
    R = _rand(g, case.n_dst, HC)
    ops = {"q": rd(q), "d": rd(d), "att": rd(att)}
    if u is not None:
        ops["u"] = rd(u)
    return ops, ei, rd(R), ks


def case_grads(case, dtype, rnd=None):
    ops, ei, R, ks = inputs(case, dtype)
    return attention_grads(ops, ei, case.n_dst, case.H, case.row_slope, case.slope, ks, R, rnd=rnd)


self_error = functools.partial(ch.self_error, case_grads)


def self_error_cases():
    return [(c, d) for c, d in ch.self_bar_cases(TABLES) if c.E > 0]


def self_error_table():
    return ch.build_table(self_error_cases(), self_error)


def write_self_error_table(path=GOLDEN_FILE):
    """Regenerates tests/golden/gate_attention_self_error.json (python -c "import gate_chain as gc; gc.write_self_error_table()")."""
    return ch.write_table(self_error_table(), path)


def load_self_error():
    return ch.load_table(GOLDEN_FILE)


# ---- the layers ---------------------------------------------------------------------------------------------------------------
def gat_ref(P, ei, n_dst, H, C, concat, slope, add_self_loops, x, xd=None, rd=None, edge_scale=None):
    """GATConv.forward of torch_geometric 2.0.x on the parameters P (lin_dst.weight absent: the shared lin_src). ``rd``: rounds q and d
    straight-through where the device keeps them in 16 bits. ``edge_scale``: the attention dropout mask, already divided by 1 - p."""
    rd = rd or (lambda t: t)
    Ws = P["lin_src.weight"]
    Wd = P.get("lin_dst.weight", Ws)
    xt = x if xd is None else xd
    q = rd(x @ Ws.t())
    d = rd(((xt @ Wd.t()).view(-1, H, C) * P["att_dst"].view(1, H, C)).sum(-1))
    if add_self_loops:
        ei = with_self_loops(ei, n_dst)
    out, _ = attention_v1(q, d, P["att_src"].reshape(-1), ei, n_dst, H, None, None, slope, edge_scale)
    if not concat:
        out = out.view(n_dst, H, C).mean(dim=1)
    return out if "bias" not in P else out + P["bias"]


def gate_ref(P, ei, x, edge_attr, rd=None, edge_scale=None):
    """GATEConv of torch_geometric.nn.models.attentive_fp in its own order: lin1 on cat([x_j, e]), lin2 per edge before the sum."""
    rd = rd or (lambda t: t)
    src, dst = ei[0], ei[1]
    n, cin = x.size(0), x.size(1)
    W1 = P["lin1.weight"]
    t = rd(x @ W1[:, :cin].t())[src] + rd(edge_attr @ W1[:, cin:].t())      # = lin1(cat([x_j, e])), the two parts stored by the device
    xj = torch.nn.functional.leaky_relu(t, 0.01)
    alpha = torch.nn.functional.leaky_relu((xj * P["att_l"]).sum(-1) + rd(x @ P["att_r"].t())[dst, 0], 0.01)
    mx = torch.full((n,), float("-inf"), dtype=x.dtype).scatter_reduce_(0, dst, alpha.detach(), "amax", include_self=True)
    ex = torch.exp(alpha - mx[dst])
    a = ex / torch.zeros(n, dtype=x.dtype).index_add_(0, dst, ex)[dst]
    if edge_scale is not None:
        a = a * edge_scale.view(-1)
    msg = (xj @ P["lin2.weight"].t()) * a.unsqueeze(-1)
    return torch.zeros((n, W1.size(0)), dtype=x.dtype).index_add_(0, dst, msg) + P["bias"]


def gru_cell(P, prefix, x, h):
    """torch.nn.GRUCell written out (gates in the order r, z, n)."""
    gi = x @ P[f"{prefix}.weight_ih"].t() + P[f"{prefix}.bias_ih"]
    gh = h @ P[f"{prefix}.weight_hh"].t() + P[f"{prefix}.bias_hh"]
    ir, iz, in_ = gi.chunk(3, dim=1)
    hr, hz, hn = gh.chunk(3, dim=1)
    r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
    n = torch.tanh(in_ + r * hn)
    return (1 - z) * n + z * h


def _sub(P, prefix):
    return {k[len(prefix) + 1:]: v for k, v in P.items() if k.startswith(prefix + ".")}


def attentive_fp_ref(P, num_layers, num_timesteps, x, ei, edge_attr, batch, n_graphs):
    """torch_geometric.nn.models.AttentiveFP.forward in eval mode / with dropout 0, on the parameters P of the module."""
    F = torch.nn.functional
    hidden = P["lin1.weight"].size(0)
    x = F.leaky_relu(x @ P["lin1.weight"].t() + P["lin1.bias"])
    h = F.elu(gate_ref(_sub(P, "atom_convs.0"), ei, x, edge_attr))
    x = gru_cell(P, "atom_grus.0", h, x).relu()
    for k in range(1, num_layers):
        h = F.elu(gat_ref(_sub(P, f"atom_convs.{k}"), ei, x.size(0), 1, hidden, True, 0.01, False, x))
        x = gru_cell(P, f"atom_grus.{k}", h, x).relu()
    n = x.size(0)
    out = torch.zeros((n_graphs, hidden), dtype=x.dtype).index_add_(0, batch, x).relu()
    to_mol = torch.stack([torch.arange(n), batch])
    for _ in range(num_timesteps):
        h = F.elu(gat_ref(_sub(P, "mol_conv"), to_mol, n_graphs, 1, hidden, True, 0.01, False, x, out))
        out = gru_cell(P, "mol_gru", h, out).relu()
    return out @ P["lin2.weight"].t() + P["lin2.bias"]


@dataclass(frozen=True)
class LayerCase:
    name: str
    kind: str                    # gat | gate
    cin: object
    cout: int
    heads: int = 1
    concat: bool = True
    self_loops: bool = True
    bipartite: bool = False
    edge_dim: int = 1

    def setup(self, dtype):
        """(layer on the CPU, {input name: float32 tensor}, edge_index, run_dev, run_ref)."""
        from gnnops import conv

        torch.manual_seed(11)
        n_src, n_dst, e = (140, 90, 900) if self.bipartite else (200, 200, 1500)
        if self.kind == "gat":
            layer = conv.GATConv(self.cin, self.cout, heads=self.heads, concat=self.concat, add_self_loops=self.self_loops)
        else:
            layer = conv.GATEConv(self.cin, self.cout, self.edge_dim)
        layer = layer.to(dtype)
        with torch.no_grad():      # the biases start at zero: give them values
            layer.bias.copy_(_rand(torch.Generator().manual_seed(12), *layer.bias.shape, scale=0.5))
        g = torch.Generator().manual_seed(13)
        ei = torch.stack([torch.randint(0, n_src, (e,), generator=g), torch.randint(0, n_dst, (e,), generator=g)])
        if not self.bipartite:
            ei[:, :30] = torch.randint(0, n_dst, (30,), generator=g)        # 30 self loops in the input
            ei[:, 30:60] = ei[:, 60:90]                                       # 30 repeated edges
        cs, cd = (self.cin, self.cin) if isinstance(self.cin, int) else self.cin
        inputs_ = {"x": _rand(g, n_src, cs)}
        if self.bipartite:
            inputs_["xd"] = _rand(g, n_dst, cd)
        if self.kind == "gate":
            inputs_["ea"] = _rand(g, e, self.edge_dim)
        H, C, rd = self.heads, self.cout, _straight_through(dtype)
        if self.kind == "gat":
            run_dev = lambda layer, x, xd=None: layer((x, xd) if self.bipartite else x, ei.cuda())   # noqa: E731
            run_ref = lambda P, x, xd=None, edge_scale=None: gat_ref(P, ei, n_dst, H, C, self.concat, 0.2, self.self_loops, x, xd, rd=rd,   # noqa: E731
                                                                     edge_scale=edge_scale)
        else:
            run_dev = lambda layer, x, ea: layer(x, ei.cuda(), ea)   # noqa: E731
            run_ref = lambda P, x, ea: gate_ref(P, ei, x, ea, rd=rd)   # noqa: E731
        return layer, inputs_, ei, run_dev, run_ref


LAYER_CASES = [LayerCase("gat-concat", "gat", 16, 8, 4), LayerCase("gat-mean_heads", "gat", 16, 32, 4, concat=False),
               LayerCase("gat-no_self_loops", "gat", 12, 5, 2, self_loops=False),
               LayerCase("gat-bipartite", "gat", (10, 7), 8, 3, self_loops=False, bipartite=True),
               LayerCase("gat-bipartite-shared", "gat", 10, 8, 1, self_loops=False, bipartite=True),
               LayerCase("gate-edge_dim1", "gate", 12, 16, edge_dim=1), LayerCase("gate-edge_dim3", "gate", 9, 12, edge_dim=3)]
GAT_STATE = {"att_src": (1, 4, 32), "att_dst": (1, 4, 32), "bias": (32,), "lin_src.weight": (128, 16), "lin_dst.weight": (128, 16)}
GATE_STATE = {"att_l": (1, 16), "att_r": (1, 12), "lin1.weight": (16, 15), "lin2.weight": (16, 16), "bias": (16,)}


def molecules(seed=21, sizes=(4, 9, 5, 7, 6), in_channels=8, edge_dim=1):
    """5 small molecules: a chain through every molecule's atoms plus a few chords, both directions; (x, edge_index, edge_attr, batch)."""
    g = torch.Generator().manual_seed(seed)
    pairs, start = [], 0
    for n in sizes:
        pairs += [(start + k, start + k + 1) for k in range(n - 1)]
        pairs += [(start + int(a), start + int(b)) for a, b in torch.randint(0, n, (2, 2), generator=g).t() if int(a) != int(b)]
        start += n
    und = torch.tensor(pairs).t()
    ei = torch.cat([und, und.flip(0)], dim=1)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    return _rand(g, start, in_channels), ei, _rand(g, ei.size(1), edge_dim), batch
