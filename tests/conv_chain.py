"""The yardstick of the conv training tests: the edge pass of gnnops.conv (csrc/conv.hip: copy / cgconv / film messages, sum /
mean by destination, + add) restated per edge in propagate order in torch float64 on the CPU — gather p[i], q[j], w[e]; message;
index_add_ by destination; a mean divides by max(deg, 1); + add — so that torch's own autograd differentiates it. The messages
use torch.sigmoid / softplus / relu, not the kernel's exp2 / rcp forms. test_conv_chain_cpu.py ties the forward to
oracle/conv_oracle.py and the gradients to torch.autograd.gradcheck and to hand-worked values.

``rnd`` (a torch dtype) runs the same chain the way the library has to for that storage type: float32 arithmetic (torch's
sequential CPU index_add_ stands for the fp32 accumulators; sigmoid / softplus are evaluated in float64 and rounded to float32,
which makes the figures the same on every host), the output rounded once, and on the way back the steps of
gnnops.conv._EdgeReduce.backward with every tensor it materialises rounded to the storage type: g / deg (the degree and the
division in float32), the per-edge rows gp / gq of gnnops_edge_grad, the segment sums by destination and by source.
``self_error`` is the distance between that chain and the float64 one: the reference against itself, never the kernels. The
bars of the GPU tests that have no precedent in the project (bf16, hubs, saturated pre-activations) are 4 x that distance (the
factor of spline_chain.py and composite_chain.py: device exp / log / rcp a few ulp from torch's, another summation order),
recorded per case and tensor in tests/golden/conv_self_error.json (``write_self_error_table`` regenerates it).

Distances are per tensor, max |got - want| / max |want|. A mean's gradients are first multiplied by the degree they were
divided by (``mean_scales``): a member of a 70 000-edge destination has 1 / 70 000 of the gradient of the rest and would
disappear under a max-relative measure.

film inputs lie on a grid of 1 / 16: gamma * q + beta is then exact in float32 and in float64, so the relu gate falls on the same
side in the kernel and in the chain (a pre-activation of exactly 0 occurs, and has gradient 0 in both, like torch.relu); with
continuous inputs one gate in ~1e7 would flip on rounding and move a whole gradient term.

The four layer restatements of test_conv_train_gpu.py (CGConv follows the reference's layer text, groq_script.py:91-109; GIN /
SAGE / FiLM restate PyG 2.0.2: parity unpinned) and its comparison helpers live here too, with the same ``rnd`` option."""
import os
from dataclasses import dataclass

import torch

import chain_harness as ch
from chain_harness import BF16, DNAME, DTYPES, F16, F32, PROJECT_BAR, rel_err  # noqa: F401  (these names were first defined here, and stay importable from here)

VEC = {F32: 4, F16: 8, BF16: 8}            # Elem<T>::VEC: elements of a 16-byte piece
T_HUB = 8192                               # csrc/hub.h: more edges than this and a row is reduced piecewise
GRID_PIECES = 8192 * 256                   # edge_grad_kernel: 8192 workgroups of 256 pieces; more pieces and the grid-stride loop iterates
SMALL_MAX_E, SMALL_MAX_N = 24576, 40000    # gnnops_plan_small_fits (include/gnnops.h)
SOFTPLUS_SEAM = 6.907755278982137          # exp(-|z|) = 1e-3: the series / log seam of softplus_f
FILM_F16_BAR = 3e-2
FUNCTORS = ("copy", "cgconv", "cgconv_w", "film")
PARTS = {"copy": (1, 0, 0), "cgconv": (2, 2, 0), "cgconv_w": (2, 2, 2), "film": (1, 2, 0)}   # K-wide parts of q, p, w
GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_self_error.json")


def _q(t, rnd):
    return t if rnd is None else t.to(rnd).to(t.dtype)


def _sigmoid(t):
    return torch.sigmoid(t) if t.dtype == torch.float64 else torch.sigmoid(t.double()).to(t.dtype)


def _softplus(t):
    sp = torch.nn.functional.softplus
    return sp(t) if t.dtype == torch.float64 else sp(t.double()).to(t.dtype)


def small_plan_fits(E, N):
    return 0 < E <= SMALL_MAX_E and 0 < N <= SMALL_MAX_N


# ---- the edge pass --------------------------------------------------------------------------------------------------------
def message(functor, pi, qj, we):
    """Rows per edge: pi = p[dst], qj = q[src], we = w (or None)."""
    if functor == "copy":
        return qj
    K = pi.size(1) // 2
    if functor == "film":                     # p = [beta | gamma]
        return torch.relu(pi[:, K:] * qj + pi[:, :K])
    z = pi + qj
    if we is not None:
        z = z + we
    return _sigmoid(z[:, :K]) * _softplus(z[:, K:])


def edge_pass(functor, q, p, w, add, edge_index, n_dst, aggr):
    """functor: copy | cgconv | film (cgconv_w = cgconv with w). The dtype of q is the arithmetic."""
    functor = "cgconv" if functor == "cgconv_w" else functor
    src, dst = edge_index[0], edge_index[1]
    m = message(functor, p[dst] if p is not None else None, q[src], w)
    out = torch.zeros((n_dst, m.size(1)), dtype=q.dtype).index_add_(0, dst, m)
    if aggr == "mean":
        out = out / torch.bincount(dst, minlength=n_dst).clamp(min=1).to(q.dtype).unsqueeze(1)
    return out if add is None else out + add


def edge_grads(functor, ops, edge_index, n_dst, aggr, R, rnd=None):
    """ops: {"q", "p", "w", "add": float64 tensor of storage-rounded values, or None}. Returns (out, {name: d sum(out * R)}) as
    float64: torch autograd of the float64 chain, or with ``rnd`` the library's own steps in float32 with storage rounding."""
    src, dst = edge_index[0], edge_index[1]
    if rnd is None:
        leaf = {k: (v.detach().clone().requires_grad_(True) if v is not None else None) for k, v in ops.items()}
        out = edge_pass(functor, leaf["q"], leaf["p"], leaf["w"], leaf["add"], edge_index, n_dst, aggr)
        (out * R).sum().backward()
        return out.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items() if v is not None}
    f = {k: (v.float() if v is not None else None) for k, v in ops.items()}
    out = _q(edge_pass(functor, f["q"], f["p"], f["w"], f["add"], edge_index, n_dst, aggr), rnd)
    grads = library_backward(functor, f, edge_index, n_dst, aggr, R.float(), rnd)
    return out.double(), {k: v.double() for k, v in grads.items()}


def library_backward(functor, f, edge_index, n_dst, aggr, g, rnd):
    """The steps of gnnops.conv._EdgeReduce.backward on float32 operands ``f``, every tensor it materialises rounded to ``rnd``."""
    src, dst = edge_index[0], edge_index[1]
    q, p, w = f["q"], f["p"], f["w"]
    r = lambda t: _q(t, rnd)   # noqa: E731
    grads = {}
    if f["add"] is not None:
        grads["add"] = g
    if aggr == "mean":        # the degree and the division in float32, one rounding
        g = r(g / torch.bincount(dst, minlength=n_dst).clamp(min=1).float().unsqueeze(1))
    seg = lambda rows, index, n: r(torch.zeros((n, rows.size(1)), dtype=torch.float32).index_add_(0, index, rows))   # noqa: E731
    ge = g[dst]
    if functor == "copy":
        grads["q"] = seg(ge, src, q.size(0))
    elif functor == "film":
        K = q.size(1)
        be, ga, qv = p[dst][:, :K], p[dst][:, K:], q[src]
        gm = torch.where(ga * qv + be > 0, ge, torch.zeros_like(ge))
        grads["p"] = seg(torch.cat([gm, r(gm * qv)], 1), dst, n_dst)
        grads["q"] = seg(r(gm * ga), src, q.size(0))
    else:
        K = q.size(1) // 2
        z = p[dst] + q[src]
        if w is not None:
            z = z + w
        sg, sp = _sigmoid(z[:, :K]), _softplus(z[:, K:])
        gp = torch.cat([r(ge * sp * (sg * (1 - sg))), r(ge * sg * _sigmoid(z[:, K:]))], 1)
        grads["p"] = seg(gp, dst, n_dst)
        grads["q"] = seg(gp, src, q.size(0))
        if w is not None:
            grads["w"] = gp
    return grads


class _LibraryEdgePass(torch.autograd.Function):
    """edge_pass inside a float32 layer chain the way the library runs it: output rounded once, backward = library_backward."""

    @staticmethod
    def forward(ctx, functor, aggr, edge_index, n_dst, rnd, q, p, w, add):
        ctx.meta = (functor, aggr, edge_index, n_dst, rnd)
        ctx.save_for_backward(*(t if t is not None else torch.empty(0) for t in (q, p, w, add)))
        ctx.has = tuple(t is not None for t in (q, p, w, add))
        return _q(edge_pass(functor, q, p, w, add, edge_index, n_dst, aggr), rnd)

    @staticmethod
    def backward(ctx, g):
        functor, aggr, edge_index, n_dst, rnd = ctx.meta
        f = {k: (t.detach() if h else None) for k, t, h in zip(("q", "p", "w", "add"), ctx.saved_tensors, ctx.has)}
        gr = library_backward("cgconv" if functor == "cgconv_w" else functor, f, edge_index, n_dst, aggr, _q(g, rnd), rnd)
        return (None,) * 5 + tuple(gr.get(k) for k in ("q", "p", "w", "add"))


def mean_scales(edge_index, n_src, n_dst):
    """Per-row factors that put a mean's gradients back on the scale of R: d p[i] * deg_i, d w[e] * deg of its destination,
    d q[j] * the smallest degree among the destinations j feeds (a source that feeds only a hub: the hub's degree)."""
    src, dst = edge_index[0], edge_index[1]
    deg = torch.bincount(dst, minlength=n_dst).clamp(min=1).double()
    big = float(deg.max()) if deg.numel() else 1.0
    sq = torch.full((n_src,), big, dtype=torch.float64).scatter_reduce_(0, src, deg[dst], "amin", include_self=True)
    sq[torch.bincount(src, minlength=n_src) == 0] = 1.0
    return {"p": deg.unsqueeze(1), "w": deg[dst].unsqueeze(1), "q": sq.unsqueeze(1)}


def scaled(name, t, scales):
    return t * scales[name] if scales is not None and name in scales else t


# ---- case tables ----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case(ch.CaseBars):
    table: str
    name: str
    functor: str
    aggr: str
    K: int
    E: int
    n_src: int
    n_dst: int
    add: bool = False
    layout: str = "plain"        # plain | block (column blocks of a wider matrix, 16-B aligned) | misaligned (by whole elements)
    graph: str = "random"        # random | dup | hub_dst | hub_src
    hub: int = 0
    values: str = "unit"         # unit | quarter | spread30 | seam | pm100 (a block of +-100 rows among unit ones)
    dtypes: tuple = tuple(DTYPES)
    bar: str = "project"         # project: PROJECT_BAR for fp32 / fp16, 4 x self error for bf16; self: 4 x self error for all
    ones: bool = False           # the functional is out.sum(): an expanded gradient of stride 0

    def project_bar(self, dtype):
        return FILM_F16_BAR if (self.functor == "film" and dtype == F16) else PROJECT_BAR[dtype]

    def pieces(self, dtype):
        """Pieces edge_grad_kernel walks: E * K / VEC when K and the layout allow 16-byte pieces, E * K otherwise."""
        wide = self.K % VEC[dtype] == 0 and self.layout != "misaligned"
        return self.E * (self.K // VEC[dtype] if wide else self.K)

    def ragged(self, dtype):
        return self.K % VEC[dtype] != 0


def _dispatch():
    cases, n = [], 0
    for fi, f in enumerate(FUNCTORS):
        for aggr in ("sum", "mean"):
            for K in (1, 4, 8, 13, 64, 200):
                n += 1
                cases.append(Case("dispatch", f"{f}-{aggr}-K{K}" + ("-add" if n % 2 else "") + ("-block" if (n // 2) % 2 else ""), f, aggr, K,
                                  600, 90, 70, add=bool(n % 2), layout="block" if (n // 2) % 2 else "plain"))
        cases.append(Case("dispatch", f"{f}-sum-K64-misaligned", f, "sum", 64, 600, 90, 70, add=fi % 2 == 0, layout="misaligned"))
    return cases


def _shapes():
    cases = []
    for f in ("copy", "cgconv_w", "film"):
        def c(name, K, E, n_src, n_dst, aggr="mean", **kw):
            cases.append(Case("shape", f"{f}-{name}", f, aggr, K, E, n_src, n_dst, **kw))
        c("E0", 8, 0, 5, 4, add=True)
        c("one_dst_K1_sum_of_out", 1, 9, 6, 1, aggr="sum", ones=True)     # sum: the expanded gradient reaches edge_grad as it came
        c("one_dst_K8", 8, 9, 6, 1, add=True)
        c("more_sources", 8, 400, 50, 20)
        c("more_destinations", 8, 400, 20, 50, add=True)
        c("isolated_rows", 13, 500, 40, 40, aggr="sum")
        c("duplicate_edges", 8, 500, 40, 40, graph="dup")
        for E, N in ((1, 1), (1023, 7), (1024, 1024), (1025, 40000), (24576, 300), (24577, 300)):
            c(f"E{E}_N{N}", 8, E, N, N, add=E % 2 == 0)
    return cases


def _gridwrap():
    return [Case("gridwrap", f"{f}-E{E}-K64", f, "sum", 64, E, 2000, 2000, dtypes=(dt,))
            for dt, E in ((F32, 200_000), (F16, 270_000), (BF16, 270_000)) for f in ("cgconv_w", "film")]


def _hubs():
    cases = []
    for f in ("copy", "cgconv_w", "film"):
        for graph, hub, E in (("hub_dst", 9000, 12000), ("hub_dst", 70000, 72000), ("hub_src", 9000, 12000)):
            for aggr in ("sum", "mean"):
                for K in (64, 13):
                    cases.append(Case("hub", f"{f}-{graph}{hub}-{aggr}-K{K}", f, aggr, K, E, 400, 40, graph=graph, hub=hub, values="quarter", bar="self"))
    return cases


def _saturation():
    return [Case("saturation", f"{f}-{v}", f, "sum", 16, 2000, 200, 200, values=v, dtypes=(F32, F16), bar="self")
            for f in ("cgconv", "cgconv_w") for v in ("spread30", "seam", "pm100")]


DISPATCH, SHAPES, GRIDWRAP, HUBS, SATURATION = _dispatch(), _shapes(), _gridwrap(), _hubs(), _saturation()
TABLES = {"dispatch": DISPATCH, "shape": SHAPES, "gridwrap": GRIDWRAP, "hub": HUBS, "saturation": SATURATION}
HUB_DST, HUB_SRC, HUB_FEEDERS = 5, 7, 50     # the hub destination / source; sources 0 .. 49 feed only the hub destination


def graph_of(case, g):
    E, n_src, n_dst = case.E, case.n_src, case.n_dst
    src = torch.randint(0, n_src, (E,), generator=g)
    dst = torch.randint(0, n_dst, (E,), generator=g)
    if case.graph == "hub_dst":
        src = HUB_FEEDERS + src % (n_src - HUB_FEEDERS)
        dst[dst == HUB_DST] = HUB_DST + 1
        src[:case.hub] = torch.randint(0, HUB_FEEDERS, (case.hub,), generator=g)
        dst[:case.hub] = HUB_DST
    elif case.graph == "hub_src":
        src[src == HUB_SRC] = HUB_SRC + 1
        src[:case.hub] = HUB_SRC
    elif case.graph == "dup":
        src[E // 2:E // 2 + E // 5], dst[E // 2:E // 2 + E // 5] = src[:E // 5], dst[:E // 5]
    if n_dst > 8 and n_src > 8 and E > 50:
        dst[dst == 3] = 4                       # destination 3 has no incoming edge
        if case.graph != "hub_dst":
            src[src == 2] = 1                   # source 2 has no outgoing edge
    if case.graph.startswith("hub") or case.graph == "dup":
        perm = torch.randperm(E, generator=g)
        src, dst = src[perm], dst[perm]
    return torch.stack([src, dst])


def _unit(g, *shape):
    return torch.rand(*shape, generator=g) * 2 - 1


def inputs(case, dtype, seed=2024):
    """({"q", "p", "w", "add"}: float64 tensors of storage-rounded values or None, edge_index, R float64 storage-rounded)."""
    g = torch.Generator().manual_seed(seed + sum(map(ord, case.name)))
    ei = graph_of(case, g)
    nq, np_, nw = PARTS[case.functor]
    K, E = case.K, case.E
    rd = lambda t: t.to(dtype).double()   # noqa: E731
    if case.functor == "film":            # a grid of 1 / 16 (module docstring)
        top = 4 if case.values == "quarter" else 16
        draw = lambda *s: torch.randint(-top, top + 1, s, generator=g).float() / 16   # noqa: E731
    else:      # quarter: [-0.25, 0.25], so that an fp16 sum over 70 000 messages stays below 65 504
        draw = lambda *s: _unit(g, *s) * (0.25 if case.values == "quarter" else 1.0)   # noqa: E731
    q = draw(case.n_src, nq * K)
    p = draw(case.n_dst, np_ * K) if np_ else None
    w = draw(E, nw * K) if nw else None
    if case.values == "spread30":         # z = p + q (+ w) spans [-30, 30]
        s = 10.0 if w is not None else 15.0
        q, p, w = q * s, p * s, (w * s if w is not None else None)
    elif case.values == "seam":           # z_s within 0.15 of +-SOFTPLUS_SEAM, on both sides of it
        sign = (torch.randint(0, 2, (case.n_dst, K), generator=g) * 2 - 1).float()
        p[:, K:] = sign * SOFTPLUS_SEAM + p[:, K:] * 0.05
        q[:, K:] *= 0.05
        if w is not None:
            w[:, K:] *= 0.05
    elif case.values == "pm100":          # the first tenth of the destinations: z = +-100 +- 2 in both parts (PM100_ROWS)
        nb = case.n_dst // 10
        p[:nb] = (torch.randint(0, 2, (nb, 2 * K), generator=g) * 2 - 1).float() * 100
    add = _unit(g, case.n_dst, K) if case.add else None
    R = torch.ones(case.n_dst, K) if case.ones else _unit(g, case.n_dst, K)
    if case.values == "quarter" and case.aggr == "sum":   # d p of a sum over the hub is R times up to 70 000 open gates: fp16 again
        R = R * 0.25
    ops = {"q": rd(q), "p": rd(p) if p is not None else None, "w": rd(w) if w is not None else None,
           "add": rd(add) if add is not None else None}
    return ops, ei, rd(R)


def case_grads(case, dtype, rnd=None):
    ops, ei, R = inputs(case, dtype)
    out, grads = edge_grads(case.functor, ops, ei, case.n_dst, case.aggr, R, rnd=rnd)
    return out, grads, (mean_scales(ei, case.n_src, case.n_dst) if case.aggr == "mean" else None)


def self_error(case, dtype):
    """{"out" | operand: rel_err of the rounded chain against the float64 one (a mean's gradients degree-scaled)}."""
    out, grads, scales = case_grads(case, dtype)
    out_r, grads_r, _ = case_grads(case, dtype, rnd=dtype)
    err = {"out": rel_err(out_r, out)}
    for k in grads:
        err[k] = rel_err(scaled(k, grads_r[k], scales), scaled(k, grads[k], scales))
    return err


def self_error_cases():
    return ch.self_bar_cases(TABLES)


def self_error_table():
    return {**ch.build_table(self_error_cases(), self_error), **layer_self_error_table()}


def write_self_error_table(path=GOLDEN_FILE):
    """Regenerates tests/golden/conv_self_error.json (python -c "import conv_chain; conv_chain.write_self_error_table()")."""
    return ch.write_table(self_error_table(), path)


def load_self_error():
    return ch.load_table(GOLDEN_FILE)


def place(t, layout, device="cuda"):
    """A differentiable view of the leaf ``t`` [rows, cols] on its device: itself, or a column block of a wider matrix —
    ``block``: 8 columns in, the pitch a multiple of 8 elements (every row start 16-byte aligned for 2- and 4-byte types);
    ``misaligned``: 1 column in and an odd pitch, so row starts are off 16 bytes by whole elements."""
    if layout == "plain" or t is None:
        return t
    cols = t.size(1)
    lead, pitch = (8, 8 + (cols + 7) // 8 * 8 + 8) if layout == "block" else (1, cols + 2 + (cols % 2))
    return torch.nn.functional.pad(t, (lead, pitch - lead - cols))[:, lead:lead + cols]


# ---- the layers of test_conv_train_gpu.py ---------------------------------------------------------------------------------
class _RoundBothWays(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, dtype):
        ctx.dtype = dtype
        return t.to(dtype).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dtype).to(g.dtype), None


def _r(t, rnd):
    """A tensor the library materialises in the storage type: rounded on the way forward and its gradient on the way back."""
    return t if rnd is None else _RoundBothWays.apply(t, rnd)


def _graph(seed, n_dst, e, n_src=None):
    g = torch.Generator().manual_seed(seed)
    n_src = n_dst if n_src is None else n_src
    src = torch.randint(0, n_src, (e,), generator=g)
    dst = torch.randint(0, n_dst, (e,), generator=g)
    if n_dst > 8 and e > 50:
        dst[dst == 3] = 4          # node 3 has no incoming edge
        dst[:40] = 5               # node 5 is a (small) hub
    return torch.stack([src, dst])


def hub_graph(seed, n_src, n_dst, e, hub):
    """_graph with destination HUB_DST receiving ``hub`` more edges from sources 0 .. HUB_FEEDERS - 1, which feed nothing else."""
    g = torch.Generator().manual_seed(seed)
    src = HUB_FEEDERS + torch.randint(0, n_src - HUB_FEEDERS, (e,), generator=g)
    dst = torch.randint(0, n_dst, (e,), generator=g)
    dst[dst == HUB_DST] = HUB_DST + 1
    ei = torch.stack([torch.cat([src, torch.randint(0, HUB_FEEDERS, (hub,), generator=g)]),
                      torch.cat([dst, torch.full((hub,), HUB_DST)])])
    return ei[:, torch.randperm(e + hub, generator=g)].contiguous()


def _rand(g, *shape, scale=1.0):
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def _scatter64(m, dst, n, reduce):
    out = torch.zeros((n,) + tuple(m.shape[1:]), dtype=m.dtype).index_add_(0, dst, m)
    if reduce == "mean":
        out = out / torch.bincount(dst, minlength=n).clamp(min=1).to(m.dtype).unsqueeze(1)
    return out


def _lin(z, W, b=None, rnd=None):
    y = z @ W.t()
    return _r(y if b is None else y + b, rnd)


def cgconv_ref(P, ei, n_dst, aggr, bip, x, xd=None, ea=None, rnd=None):
    """groq_script.py:91-109. ``rnd``: the layer as the library runs it — the per-node products p, q, w rounded, the message and
    the sum in float32, the output rounded once."""
    src, dst = ei
    xt = xd if bip else x
    if rnd is None:
        z = torch.cat([xt[dst], x[src]] + ([ea] if ea is not None else []), dim=-1)
        zf, zs = z @ P["lin_f.weight"].t() + P["lin_f.bias"], z @ P["lin_s.weight"].t() + P["lin_s.bias"]
    else:
        cd, cs = xt.size(1), x.size(1)
        W = torch.cat([P["lin_f.weight"], P["lin_s.weight"]], 0)
        p = _lin(xt, W[:, :cd], torch.cat([P["lin_f.bias"], P["lin_s.bias"]]), rnd)
        q = _lin(x, W[:, cd:cd + cs], None, rnd)
        w = _lin(ea, W[:, cd + cs:], None, rnd) if ea is not None else None
        return _LibraryEdgePass.apply("cgconv", "sum" if aggr == "add" else aggr, ei, n_dst, rnd, q, p, w, xt)
    m = _sigmoid(zf) * _softplus(zs)
    return _r(_scatter64(m, dst, n_dst, "sum" if aggr == "add" else aggr) + xt, rnd)


def gin_ref(P, ei, n, eps, x, xd=None, rnd=None):
    """``rnd``: the root (1 + eps) * x is an elementwise op in the storage type (1 + eps too when eps is a tensor), the sum + root
    one library edge pass, the product's output rounded."""
    src, dst = ei
    xt = x if xd is None else xd
    if rnd is None:
        h = _scatter64(x[src], dst, n, "sum") + (1.0 + eps) * xt
    else:
        root = _r((_r(1.0 + eps, rnd) if torch.is_tensor(eps) else 1.0 + eps) * xt, rnd)
        h = _LibraryEdgePass.apply("copy", "sum", ei, n, rnd, x, None, None, root)
    return _lin(h, P["nn.weight"], P["nn.bias"], rnd)


def sage_ref(P, ei, n_dst, root_weight, x, xd=None, rnd=None):
    src, dst = ei
    xt = x if xd is None else xd
    mean = _scatter64(x[src], dst, n_dst, "mean") if rnd is None else _LibraryEdgePass.apply("copy", "mean", ei, n_dst, rnd, x, None, None, None)
    out = mean @ P["lin_l.weight"].t() + P["lin_l.bias"]
    return _r(out + xt[:n_dst] @ P["lin_r.weight"].t() if root_weight else out, rnd)


def film_ref(P, ei, et, n, o, relations, aggr, x, rd):
    """relu gates: which side of zero a pre-activation falls on must be decided from the SAME numbers. The device keeps the
    per-node projections in the storage type, so for 16-bit types the restatement rounds them too (``rd``: straight-through for
    the gradient); otherwise a handful of near-zero pre-activations gate differently and each flips a whole gradient term."""
    e = ei.size(1)
    fs = rd(x @ P["film_skip.weight"].t())
    # the skip term is two elementwise ops in the storage type on the device (product rounded, then the sum): same here
    out = torch.relu(rd(rd(fs[:, o:] * rd(x @ P["lin_skip.weight"].t())) + fs[:, :o]))
    for r in range(relations):
        sel = et == r if relations > 1 else torch.ones(e, dtype=torch.bool)
        src, dst = ei[0][sel], ei[1][sel]
        f = rd(x @ P[f"films.{r}.weight"].t() + P[f"films.{r}.bias"])
        m = torch.relu(f[dst][:, o:] * rd(x @ P[f"lins.{r}.weight"].t())[src] + f[dst][:, :o])
        out = out + _scatter64(m, dst, n, "sum" if aggr == "add" else aggr)
    return out


def _check(got, want, tol, what, scale_rows=None):
    assert got is not None, f"{what}: no gradient"
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if scale_rows is not None:
        got, want = got * scale_rows, want * scale_rows
    scale = max(float(want.abs().max()), 1e-6)
    err = float((got - want).abs().max()) / scale
    print(f"{what}: {err:.3e} (bar {tol:.3e})")
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    assert err <= tol, f"{what}: gradient error {err:.3e} of scale exceeds {tol:.1e}"


def _compare(layer, run_dev, run_ref, inputs, tol, scale_rows=None):
    """inputs: {name: CPU fp32 tensor}; run_dev(layer, **device tensors) -> out; run_ref(P, **float64 tensors) -> out.
    tol: one bar, or {"forward" | "d <name>": bar}; scale_rows: {input name: per-row factors applied to both sides}."""
    dev = {k: v.clone().to(next(layer.parameters()).dtype).cuda().requires_grad_(True) for k, v in inputs.items()}
    out = run_dev(layer, **dev)
    g = torch.Generator().manual_seed(99)
    coef = _rand(g, *out.shape)
    (out.float() * coef.cuda()).sum().backward()
    P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in layer.named_parameters()}
    ref_in = {k: dev[k].detach().double().cpu().requires_grad_(True) for k in inputs}
    ref = run_ref(P, **ref_in)
    bar = (lambda k: tol[k]) if isinstance(tol, dict) else (lambda k: tol)
    _check(out, ref.detach(), bar("forward"), "forward")
    (ref * coef.double()).sum().backward()
    for k in inputs:
        _check(dev[k].grad, ref_in[k].grad, bar(f"d {k}"), f"d {k}", (scale_rows or {}).get(k))
    for k, p in layer.named_parameters():
        _check(p.grad, P[k].grad if P[k].grad is not None else torch.zeros_like(P[k]), bar(f"d {k}"), f"d {k}")


def layer_errors(params, run_ref, inputs, out_shape, dtype, scale_rows=None):
    """Self error of a layer restatement: ``run_ref(P, rnd=..., **inputs)`` in float32 with storage rounding against itself in
    float64, on storage-rounded parameters and inputs, for the functional _compare draws. {"forward" | "d <name>": rel_err}."""
    coef = _rand(torch.Generator().manual_seed(99), *out_shape)
    res = []
    for rnd in (None, dtype):
        cdt = torch.float64 if rnd is None else torch.float32
        P = {k: v.to(dtype).to(cdt).requires_grad_(True) for k, v in params.items()}
        xin = {k: v.to(dtype).to(cdt).requires_grad_(True) for k, v in inputs.items()}
        out = run_ref(P, rnd=rnd, **xin)
        (out * coef.to(cdt)).sum().backward()
        d = {"forward": out.detach().double()}
        for k, v in list(xin.items()) + list(P.items()):
            gr = (v.grad if v.grad is not None else torch.zeros_like(v)).double()
            d[f"d {k}"] = gr * scale_rows[k] if scale_rows and k in scale_rows else gr
        res.append(d)
    return {k: rel_err(res[1][k], res[0][k]) for k in res[0]}


def film_lib(P, ei, et, n, o, relations, aggr, x, rnd):
    """FiLMConv as the library runs it: every per-node projection rounded, the skip term two elementwise ops, one library edge
    pass per relation that adds to the running output."""
    fs = _lin(x, P["film_skip.weight"], None, rnd)
    out = torch.relu(_r(_r(fs[:, o:] * _lin(x, P["lin_skip.weight"], None, rnd), rnd) + fs[:, :o], rnd))
    for r in range(relations):
        sub = ei if relations == 1 else ei[:, et == r]
        f = _lin(x, P[f"films.{r}.weight"], P[f"films.{r}.bias"], rnd)
        out = _LibraryEdgePass.apply("film", "sum" if aggr == "add" else aggr, sub, n, rnd, _lin(x, P[f"lins.{r}.weight"], None, rnd), f, None, out)
    return out


def _straight_through(dtype):
    return lambda t: t if dtype == torch.float32 else t + (t.to(dtype).to(t.dtype) - t).detach()


@dataclass(frozen=True)
class LayerCase:
    """One layer test: ``setup`` builds the layer on the CPU from the test's own seeds, the inputs, the two ways to run it, the
    output's shape and the per-row scales of a mean over a hub."""
    name: str
    kind: str           # cgconv | gin | sage | film | hub_sage | hub_cgconv
    cfg: tuple
    dtype: torch.dtype

    def key(self, tensor):
        return f"layer/{self.name}/{DNAME[self.dtype]}/{tensor}"

    def setup(self):
        from gnnops import conv

        dtype, kind, scale = self.dtype, self.kind, None
        if kind == "cgconv":
            channels, dim, aggr = self.cfg
            torch.manual_seed(1)
            c_src, c_dst = (channels, channels) if isinstance(channels, int) else channels
            bip = not isinstance(channels, int)
            n_src, n_dst, e = (29, 29, 56) if channels == 11 else (300, 300 if not bip else 210, 2500)
            layer = conv.CGConv(channels, dim, aggr=aggr).to(dtype)
            ei = _graph(2, n_dst, e, n_src=n_src)
            g = torch.Generator().manual_seed(5)
            inputs = {"x": _rand(g, n_src, c_src)}
            if bip:
                inputs["xd"] = _rand(g, n_dst, c_dst)
            if dim:
                inputs["ea"] = _rand(g, e, dim)
            run_dev = lambda layer, x, xd=None, ea=None: layer((x, xd) if bip else x, ei.cuda(), ea)   # noqa: E731
            run_ref = lambda P, x, xd=None, ea=None, rnd=None: cgconv_ref(P, ei, n_dst, aggr, bip, x, xd, ea, rnd=rnd)   # noqa: E731
            shape = (n_dst, c_dst)
        elif kind == "gin":
            (train_eps,) = self.cfg
            torch.manual_seed(2)
            layer = conv.GINConv(torch.nn.Linear(24, 40), eps=0.3, train_eps=train_eps).to(dtype)
            ei = _graph(3, 250, 2000)
            inputs = {"x": _rand(torch.Generator().manual_seed(6), 250, 24)}
            run_dev = lambda layer, x: layer(x, ei.cuda())   # noqa: E731
            run_ref = lambda P, x, rnd=None: gin_ref(P, ei, 250, P["eps"] if train_eps else 0.3, x, rnd=rnd)   # noqa: E731
            shape = (250, 40)
        elif kind == "sage":
            (root_weight,) = self.cfg
            torch.manual_seed(3)
            layer = conv.SAGEConv(20, 36, root_weight=root_weight).to(dtype)
            ei = _graph(4, 250, 2000)
            inputs = {"x": _rand(torch.Generator().manual_seed(7), 250, 20)}
            run_dev = lambda layer, x: layer(x, ei.cuda())   # noqa: E731
            run_ref = lambda P, x, rnd=None: sage_ref(P, ei, 250, root_weight, x, rnd=rnd)   # noqa: E731
            shape = (250, 36)
        elif kind == "film":
            relations, aggr = self.cfg
            torch.manual_seed(4)
            o, n, e = 24, 220, 1800
            layer = conv.FiLMConv(12, o, num_relations=relations, aggr=aggr).to(dtype)
            ei = _graph(5, n, e)
            et = torch.randint(0, relations, (e,), generator=torch.Generator().manual_seed(8))
            inputs = {"x": _rand(torch.Generator().manual_seed(9), n, 12)}
            run_dev = lambda layer, x: layer(x, ei.cuda(), et.cuda() if relations > 1 else None)   # noqa: E731
            rd = _straight_through(dtype)
            run_ref = lambda P, x, rnd=None: (film_ref(P, ei, et, n, o, relations, aggr, x, rd) if rnd is None   # noqa: E731
                                              else film_lib(P, ei, et, n, o, relations, aggr, x, rnd))
            shape = (n, o)
        else:               # a 70 000-edge destination fed by sources 0 .. 49 alone; bipartite: d x holds only what the mean sent
            torch.manual_seed(8)
            n_src, n_dst, c = 400, 60, 16
            ei = hub_graph(13, n_src, n_dst, 2000, 70000)
            g = torch.Generator().manual_seed(14)
            inputs = {"x": _rand(g, n_src, c), "xd": _rand(g, n_dst, c)}
            scale = {"x": mean_scales(ei, n_src, n_dst)["q"]}
            run_dev = lambda layer, x, xd: layer((x, xd), ei.cuda())   # noqa: E731
            if kind == "hub_sage":
                layer = conv.SAGEConv((c, c), 24, root_weight=True).to(dtype)
                run_ref = lambda P, x, xd, rnd=None: sage_ref(P, ei, n_dst, True, x, xd, rnd=rnd)   # noqa: E731
                shape = (n_dst, 24)
            else:
                layer = conv.CGConv((c, c), 0, aggr="mean").to(dtype)
                run_ref = lambda P, x, xd, rnd=None: cgconv_ref(P, ei, n_dst, "mean", True, x, xd, rnd=rnd)   # noqa: E731
                shape = (n_dst, c)
        return layer, inputs, run_dev, run_ref, shape, scale, ei

    def self_error(self):
        layer, inputs, _, run_ref, shape, scale, _ = self.setup()
        return layer_errors({k: v.detach() for k, v in layer.named_parameters()}, run_ref, inputs, shape, self.dtype, scale)


CGCONV_CFGS = [(16, 0, "add"), (32, 5, "add"), ((24, 16), 3, "mean"), (11, 0, "add")]
FILM_CFGS = [(1, "mean"), (3, "mean"), (1, "add")]
LAYER_CASES = ([LayerCase(f"cgconv-{c}-{d}-{a}".replace(" ", ""), "cgconv", (c, d, a), BF16) for c, d, a in CGCONV_CFGS]
               + [LayerCase(f"gin-train_eps{t}", "gin", (t,), BF16) for t in (False, True)]
               + [LayerCase(f"sage-root{r}", "sage", (r,), BF16) for r in (True, False)]
               + [LayerCase(f"film-{r}-{a}", "film", (r, a), BF16) for r, a in FILM_CFGS]
               + [LayerCase(k, k, (), d) for k in ("hub_sage", "hub_cgconv") for d in (F16, BF16)])


def layer_self_error_table():
    return {c.key(k): v for c in LAYER_CASES for k, v in c.self_error().items()}
