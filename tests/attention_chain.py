"""The yardstick of the attention tests: gnnops.conv.edge_attention (csrc/attention.hip) and gnnops.conv.GATv2Conv restated per
edge in propagate order in torch float64 on the CPU, so that torch's own autograd differentiates them:

    gather p[i], q[j] -> z = p[i] + q[j] -> torch.nn.functional.leaky_relu -> s[e, h] = sum_c att[h, c] * leaky(z)[e, h, c]
    -> per-destination softmax by an explicit maximum (scatter amax), exp, index_add_ of the denominators, a division
    -> out = index_add_ by destination of a[e, h] * q[j, h, :]

No running maximum, no rescaling, no log-sum-exp: the kernel's online softmax shares none of it. test_attention_chain_cpu.py ties
this chain to a dense masked torch.softmax formulation, to torch.autograd.gradcheck and to a two-edge example worked by hand.

``rnd`` (a torch dtype) runs the library's own steps in float32 with every tensor the library materialises rounded to the storage
type: ``out``; on the way back ``delta = sum_c g * out`` from that ROUNDED out (the kernel reads the stored output), the scores
recomputed, a = exp(s - lse) with lse = max + log(denominator) in float32, ds = a * (da - delta), the per-edge rows
``gq = a * g + t`` rounded, their segment sum by source (d q) rounded, ``d p`` (summed in float32, rounded once) and ``d att``
(float32 partial sums, rounded once). exp and log are evaluated in float64 and rounded to float32, and every dot product over the
channels is an explicit loop of float32 additions, so the figures are the same on every host. ``self_error`` is the distance
between the two chains, per tensor max |got - want| / max |want|: the reference against itself, never the kernels. It is recorded
in tests/golden/attention_self_error.json (``write_self_error_table`` regenerates it); the GPU bars of everything without
precedent in the project (bf16, heavy destinations, wide-range scores) are 4 x that distance, the factor of conv_chain.py and
composite_chain.py. fp32 and fp16 cases of the kind the conv tests cover keep PROJECT_BAR of conv_chain.py.

The fp16 LAYER keeps the project's bar too, against the float64 restatement with the two projections rounded to the storage type
(straight-through for the gradient), as conv_chain.film_ref does for relu: the device keeps q and p in the storage type, and d p
— hence d lin_r — lives on the kinks of leaky_relu alone (a softmax does not move when all scores of a destination shift together,
so where every z of a head is positive sum_e ds[e] = 0 and d p = 0). With unrounded projections in the reference the few
pre-activations that 2^-11 moves across zero each flip a whole term of that small sum: the library-order chain is then 2e-2 .. 9e-2
of scale from the float64 one in d lin_r / d xd, and 5e-4 once the reference gates on the same numbers. (Where delta comes from —
the stored out or a first loop over the edges — does not move these figures: both forms were run through this chain.)

The layer restatement follows torch_geometric 2.0.2's GATv2Conv (x_l = lin_l(x) is the source side and the message, x_r = lin_r(x)
the destination side; existing self loops removed, one added per node; mean over heads when concat=False; bias last). PyG is not
available to compare against: parity unpinned."""
import functools
import os
from dataclasses import dataclass

import torch

import chain_harness as ch
from chain_harness import BF16, DNAME, DTYPES, F16, F32, PROJECT_BAR, rel_err  # noqa: F401
from conv_chain import _lin, _q, _r, _rand, _straight_through, place, small_plan_fits  # noqa: F401

T_HUB = 8192          # csrc/hub.h: the degree past which the other edge passes go piecewise (this one does not yet)
GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_self_error.json")
SEAM_DEGREES = (0, 1, 7, 8, 9, 63, 64, 65, 129)     # the unroll steps (4 backward, 8 forward) and the run of 64 edge ids
SPECIAL = 12          # edges of each of the ascending / descending / equal destinations of the wide-range cases


def _exp(t):
    return torch.exp(t) if t.dtype == torch.float64 else torch.exp(t.double()).to(t.dtype)


def _log(t):
    return torch.log(t) if t.dtype == torch.float64 else torch.log(t.double()).to(t.dtype)


def _dot(a, b):
    """sum over the last dimension of a * b; in float32 an explicit loop, so that no host's vectorised reduction order enters."""
    if a.dtype == torch.float64:
        return (a * b).sum(-1)
    acc = torch.zeros(torch.broadcast_shapes(a.shape, b.shape)[:-1], dtype=a.dtype)
    for c in range(a.size(-1)):
        acc = acc + a[..., c] * b[..., c]
    return acc


def _amax(s, dst, n):
    H = s.size(1)
    return torch.full((n, H), float("-inf"), dtype=s.dtype).scatter_reduce_(0, dst.unsqueeze(1).expand(-1, H), s, "amax", include_self=True)


# ---- the op -----------------------------------------------------------------------------------------------------------------
def scores(q, p, att, edge_index, H, slope):
    src, dst = edge_index[0], edge_index[1]
    C = att.numel() // H
    qj, pi = q[src].view(-1, H, C), p[dst].view(-1, H, C)
    z = pi + qj
    return z, qj, _dot(torch.nn.functional.leaky_relu(z, slope), att.view(1, H, C))


def attention(q, p, att, edge_index, n_dst, H, slope=0.2):
    """(out [n_dst, H * C], lse [n_dst, H]); the dtype of q is the arithmetic."""
    dst = edge_index[1]
    C = att.numel() // H
    _, qj, s = scores(q, p, att, edge_index, H, slope)
    mx = _amax(s.detach(), dst, n_dst)
    ex = _exp(s - mx[dst])
    den = torch.zeros((n_dst, H), dtype=q.dtype).index_add_(0, dst, ex)
    a = ex / den[dst]
    out = torch.zeros((n_dst, H, C), dtype=q.dtype).index_add_(0, dst, a.unsqueeze(-1) * qj)
    return out.view(n_dst, H * C), mx + _log(den.detach())


def library_backward(f, out_r, lse, edge_index, n_dst, H, slope, g, rnd):
    """The steps of gnnops_edge_attention_backward + the segment sum of `_EdgeAttention.backward` on float32 operands ``f``;
    ``out_r`` is the rounded forward output."""
    src, dst = edge_index[0], edge_index[1]
    q, p, att = f["q"], f["p"], f["att"]
    C = att.numel() // H
    r = lambda t: _q(t, rnd)   # noqa: E731
    E = src.numel()
    if E == 0:
        return {"q": torch.zeros_like(q), "p": torch.zeros_like(p), "att": torch.zeros_like(att)}
    gh, oh = g.view(n_dst, H, C), out_r.view(n_dst, H, C)
    delta = _dot(gh, oh)
    z, qj, s = scores(q, p, att, edge_index, H, slope)
    a = _exp(s - lse[dst])
    ds = a * (_dot(gh[dst], qj) - delta[dst])
    t = ds.unsqueeze(-1) * att.view(1, H, C) * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    gq = r(a.unsqueeze(-1) * gh[dst] + t).reshape(E, H * C)
    rows = (ds.unsqueeze(-1) * torch.nn.functional.leaky_relu(z, slope)).reshape(E, H * C)
    seg = lambda rows_, index, n: torch.zeros((n, H * C), dtype=torch.float32).index_add_(0, index, rows_)   # noqa: E731
    return {"q": r(seg(gq, src, q.size(0))), "p": r(seg(t.reshape(E, H * C), dst, n_dst)),
            "att": r(seg(rows, torch.zeros(E, dtype=torch.int64), 1)).view(att.shape)}


def attention_grads(ops, edge_index, n_dst, H, slope, R, rnd=None):
    """ops: {"q", "p", "att"} float64 tensors of storage-rounded values. (out, {name: d sum(out * R)}) as float64: torch autograd of
    the float64 chain, or with ``rnd`` the library's own steps in float32 with storage rounding."""
    if rnd is None:
        leaf = {k: v.detach().clone().requires_grad_(True) for k, v in ops.items()}
        out, _ = attention(leaf["q"], leaf["p"], leaf["att"], edge_index, n_dst, H, slope)
        (out * R).sum().backward()
        return out.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}
    f = {k: v.float() for k, v in ops.items()}
    out, lse = attention(f["q"], f["p"], f["att"], edge_index, n_dst, H, slope)
    out = _q(out, rnd)
    grads = library_backward(f, out, lse, edge_index, n_dst, H, slope, R.float(), rnd)
    return out.double(), {k: v.double() for k, v in grads.items()}


class _LibraryAttention(torch.autograd.Function):
    """attention inside a float32 layer chain the way the library runs it: output rounded once, backward = library_backward."""

    @staticmethod
    def forward(ctx, edge_index, n_dst, H, slope, rnd, q, p, att):
        out, lse = attention(q, p, att, edge_index, n_dst, H, slope)
        out = _q(out, rnd)
        ctx.meta = (edge_index, n_dst, H, slope, rnd)
        ctx.save_for_backward(q, p, att, out, lse)
        return out

    @staticmethod
    def backward(ctx, g):
        edge_index, n_dst, H, slope, rnd = ctx.meta
        q, p, att, out, lse = ctx.saved_tensors
        gr = library_backward({"q": q, "p": p, "att": att}, out, lse, edge_index, n_dst, H, slope, _q(g, rnd), rnd)
        return (None,) * 5 + (gr["q"], gr["p"], gr["att"])


# ---- cases ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case(ch.CaseBars):
    table: str
    name: str
    H: int
    C: int
    graph: str = "random"        # random | seams | range | heavy | dup | empty
    E: int = 2000
    n_src: int = 257
    n_dst: int = 300
    layout: str = "block"        # block: q, p column blocks of a wider matrix (pitch != H * C); plain: dense; misaligned: off 16 B by elements
    bar: str = "project"         # project: PROJECT_BAR for fp32 / fp16, 4 x self error for bf16; self: 4 x self error for all
    dtypes: tuple = tuple(DTYPES)
    slope: float = 0.2


SHAPES = [Case("shape", f"H{H}-C{C}", H, C) for H in (1, 3, 4) for C in (1, 5, 8, 64, 136)] + [Case("shape", "H4-C8-dense", 4, 8, layout="plain")]
# one column in and an odd pitch: single-element accesses, so 136 / 100 pieces per head = the 4- and 2-pieces-per-lane instances
SHAPES += [Case("shape", f"H{H}-C{C}-misaligned", H, C, layout="misaligned") for H, C in ((2, 136), (3, 100))]
SEAMS = [Case("seams", f"H{H}-C{C}", H, C, graph="seams", n_src=140, n_dst=len(SEAM_DEGREES) + 3) for H, C in ((3, 8), (1, 136))]
RANGE = [Case("range", f"H{H}-C{C}", H, C, graph="range", E=700, n_src=120, n_dst=100, bar="self") for H, C in ((3, 8), (1, 64))]
HEAVY = [Case("heavy", f"H{H}-C{C}", H, C, graph="heavy", E=1500, n_src=400, n_dst=60, bar="self") for H, C in ((3, 8), (1, 136))]
PLAN = [Case("plan", f"E{E}", 2, 8, E=E, n_src=300, n_dst=300) for E in (24576, 24577)]
EDGES = [Case("edges", "dup_and_self_loops", 3, 5, graph="dup", E=600, n_src=50, n_dst=50),
         Case("edges", "E0", 3, 8, graph="empty", E=0, n_src=5, n_dst=4)]
TABLES = {"shape": SHAPES, "seams": SEAMS, "range": RANGE, "heavy": HEAVY, "plan": PLAN, "edges": EDGES}
HEAVY_DEGREES = {5: T_HUB + 1, 9: 20000}        # destination -> edges, among ordinary rows
RANGE_ROWS = {"ascending": 0, "descending": 1, "equal": 2}


def graph_of(case, g):
    E, n_src, n_dst = case.E, case.n_src, case.n_dst
    if case.graph == "empty":
        return torch.zeros((2, 0), dtype=torch.int64)
    if case.graph == "seams":       # destination k has SEAM_DEGREES[k] edges; three ordinary rows follow
        dst = torch.cat([torch.full((d,), k, dtype=torch.int64) for k, d in enumerate(SEAM_DEGREES)]
                        + [torch.randint(len(SEAM_DEGREES), n_dst, (20,), generator=g)])
        src = torch.randint(0, n_src, (dst.numel(),), generator=g)
        perm = torch.randperm(dst.numel(), generator=g)
        return torch.stack([src[perm], dst[perm]])
    src = torch.randint(0, n_src, (E,), generator=g)
    dst = torch.randint(0, n_dst, (E,), generator=g)
    if case.graph == "range":       # destinations 0, 1, 2 take SPECIAL edges each, in this order, from sources kept for them
        dst = 3 + dst % (n_dst - 3)
        src = 3 * SPECIAL + src % (n_src - 3 * SPECIAL)
        sp_src = torch.arange(3 * SPECIAL)
        sp_dst = torch.arange(3).repeat_interleave(SPECIAL)
        return torch.stack([torch.cat([src, sp_src]), torch.cat([dst, sp_dst])])
    if case.graph == "heavy":
        for d in HEAVY_DEGREES:
            dst[dst == d] = d + 1
        extra = [(torch.randint(0, n_src, (k,), generator=g), torch.full((k,), d, dtype=torch.int64)) for d, k in HEAVY_DEGREES.items()]
        src, dst = torch.cat([src] + [e[0] for e in extra]), torch.cat([dst] + [e[1] for e in extra])
        perm = torch.randperm(dst.numel(), generator=g)
        return torch.stack([src[perm], dst[perm]])
    if case.graph == "dup":         # a fifth of the edges twice, and a self loop at every third node (some of them twice)
        src[E // 2:E // 2 + E // 5], dst[E // 2:E // 2 + E // 5] = src[:E // 5], dst[:E // 5]
        loops = torch.arange(0, n_dst, 3)
        src[-loops.numel():], dst[-loops.numel():] = loops, loops
        src[-2 * loops.numel():-loops.numel():2], dst[-2 * loops.numel():-loops.numel():2] = loops[::2], loops[::2]
    if n_dst > 8:
        dst[dst == 3] = 4            # destination 3 has no incoming edge
    return torch.stack([src, dst])


def inputs(case, dtype, seed=4242):
    """({"q", "p", "att"}: float64 tensors of storage-rounded values, edge_index, R float64 storage-rounded)."""
    g = torch.Generator().manual_seed(seed + sum(map(ord, case.table + case.name)))
    ei = graph_of(case, g)
    HC = case.H * case.C
    rd = lambda t: t.to(dtype).double()   # noqa: E731
    q, p, att = _rand(g, case.n_src, HC), _rand(g, case.n_dst, HC), _rand(g, HC)
    if case.graph == "range":
        # the ordinary rows: z = p + q over +-120, so the scores of a destination lie hundreds apart (a softmax without a running
        # maximum overflows float32 past 88). Rows 0 / 1 / 2: p = 0 and q[j] = level * u with att[c] * u[c] > 0, so every head's
        # score is strictly increasing in the level (leaky_relu is): levels ascending, descending, all equal.
        q, p = q * 60, p * 60
        u = torch.sign(att) * 0.5
        u[u == 0] = 0.5
        levels = torch.linspace(-60.0, 60.0, SPECIAL)
        p[:3] = 0
        q[:SPECIAL] = levels.unsqueeze(1) * u
        q[SPECIAL:2 * SPECIAL] = levels.flip(0).unsqueeze(1) * u
        q[2 * SPECIAL:3 * SPECIAL] = 17.0 * u
    R = _rand(g, case.n_dst, HC)
    return {"q": rd(q), "p": rd(p), "att": rd(att)}, ei, rd(R)


def case_grads(case, dtype, rnd=None):
    ops, ei, R = inputs(case, dtype)
    return attention_grads(ops, ei, case.n_dst, case.H, case.slope, R, rnd=rnd)


self_error = functools.partial(ch.self_error, case_grads)


def self_error_cases():
    return ch.self_bar_cases(TABLES)


# ---- the layer ----------------------------------------------------------------------------------------------------------------
def with_self_loops(edge_index, n):
    """PyG's remove_self_loops followed by add_self_loops: the edges with src != dst in their order, then (k, k) for k < n."""
    keep = edge_index[0] != edge_index[1]
    loops = torch.arange(n, dtype=edge_index.dtype)
    return torch.cat([edge_index[:, keep], torch.stack([loops, loops])], dim=1)


def gatv2_ref(P, ei, n_dst, H, C, concat, slope, add_self_loops, x, xd=None, rnd=None, rd=None):
    """GATv2Conv.forward of torch_geometric 2.0.2 on the parameters P. ``rnd``: the layer as the library runs it — the two
    projections rounded, one library attention pass, the mean over heads and the bias as elementwise ops in the storage type.
    ``rd`` (float64 chain, 16-bit storage): rounds the two projections straight-through, so that leaky_relu gates on the numbers
    the device gates on (module docstring)."""
    xt = x if xd is None else xd
    q = _lin(x, P["lin_l.weight"], P.get("lin_l.bias"), rnd)
    p = _lin(xt, P["lin_r.weight"], P.get("lin_r.bias"), rnd)
    if rd is not None and rnd is None:
        q, p = rd(q), rd(p)
    if add_self_loops:
        ei = with_self_loops(ei, n_dst)
    att = P["att"].reshape(-1)
    if rnd is None:
        out, _ = attention(q, p, att, ei, n_dst, H, slope)
    else:
        out = _LibraryAttention.apply(ei, n_dst, H, slope, rnd, q, p, att)
    if not concat:
        out = _r(out.view(n_dst, H, C).mean(dim=1), rnd)
    return out if "bias" not in P else _r(out + P["bias"], rnd)


@dataclass(frozen=True)
class LayerCase:
    name: str
    cin: int
    cout: int
    heads: int
    concat: bool = True
    share: bool = False
    bias: bool = True
    bipartite: bool = False

    def setup(self, dtype):
        """(layer on the CPU, {input name: float32 tensor}, edge_index, run_dev, run_ref, output shape)."""
        from gnnops import conv

        torch.manual_seed(11)
        n_src, n_dst, e = (140, 90, 900) if self.bipartite else (200, 200, 1500)
        layer = conv.GATv2Conv(self.cin, self.cout, heads=self.heads, concat=self.concat, share_weights=self.share, bias=self.bias,
                               add_self_loops=not self.bipartite).to(dtype)
        with torch.no_grad():      # PyG starts the biases at zero: give them values, or their gradients' paths go untested forward
            for name, prm in layer.named_parameters():
                if name.endswith("bias"):
                    prm.copy_(_rand(torch.Generator().manual_seed(12), *prm.shape, scale=0.5))
        g = torch.Generator().manual_seed(13)
        ei = torch.stack([torch.randint(0, n_src, (e,), generator=g), torch.randint(0, n_dst, (e,), generator=g)])
        if not self.bipartite:
            ei[:, :30] = torch.randint(0, n_dst, (30,), generator=g)        # 30 self loops in the input
            ei[:, 30:60] = ei[:, 60:90]                                       # 30 repeated edges
        inputs_ = {"x": _rand(g, n_src, self.cin)}
        if self.bipartite:
            inputs_["xd"] = _rand(g, n_dst, self.cin)
        H, C = self.heads, self.cout
        run_dev = lambda layer, x, xd=None: layer((x, xd) if self.bipartite else x, ei.cuda())   # noqa: E731

        def run_ref(P, x, xd=None, rnd=None):
            P = dict(P)
            if self.share:
                P["lin_r.weight"] = P["lin_l.weight"]
                if self.bias:
                    P["lin_r.bias"] = P["lin_l.bias"]
            return gatv2_ref(P, ei, n_dst, H, C, self.concat, 0.2, not self.bipartite, x, xd, rnd=rnd, rd=_straight_through(dtype))

        return layer, inputs_, ei, run_dev, run_ref, (n_dst, H * C if self.concat else C)


LAYER_CASES = [LayerCase("concat", 16, 8, 4), LayerCase("mean_heads", 16, 32, 4, concat=False), LayerCase("share_weights", 12, 8, 3, share=True),
               LayerCase("no_bias", 12, 5, 2, bias=False), LayerCase("bipartite", 10, 8, 3, bipartite=True)]
PYG_STATE = {"att": (1, 4, 32), "bias": (32,), "lin_l.weight": (128, 16), "lin_l.bias": (128,), "lin_r.weight": (128, 16), "lin_r.bias": (128,)}


# ---- the table ----------------------------------------------------------------------------------------------------------------
def self_error_table():
    return ch.build_table(self_error_cases(), self_error)


def write_self_error_table(path=GOLDEN_FILE):
    """Regenerates tests/golden/attention_self_error.json (python -c "import attention_chain as ac; ac.write_self_error_table()")."""
    return ch.write_table(self_error_table(), path)


def load_self_error():
    return ch.load_table(GOLDEN_FILE)
