"""The yardstick of the GraphUNet tests: torch_geometric 2.0.2's `topk` (dense pad + sort), `filter_adj`,
`add_remaining_self_loops` + `gcn_norm` + propagate, `TopKPooling`, `augment_adj` and the `GraphUNet` forward, restated in plain torch
on the CPU. The dtype of the operands is the arithmetic: float64 is the reference; autograd differentiates it. torch_geometric is not
available to compare against: parity unpinned. test_unet_chain_cpu.py ties the pieces to independent formulations.

``rnd`` (a torch dtype) runs the same chain the way the library has to for that storage type: float32 arithmetic, and every tensor
the library materialises (the dense product, the propagate output, the gathered and scaled rows) rounded to the storage type by a
cast pair, whose backward rounds the gradient at the same place. ``self_error`` is the distance between that chain and the float64
one, per tensor, max |got - want| / max |want| — the reference against itself, never the kernels — recorded in
tests/golden/unet_self_error.json (``write_self_error_table`` regenerates it). The GPU bars: PROJECT_BAR of conv_chain.py for
fp32 / fp16; 4 x the recorded self error for bf16 and for the heavy table, the project's rule.

Selections must be reproduced exactly, so every layer case keeps the scores inside a graph apart (``min_gap``): at least 1e-3 in
fp32 cases and 0.05 in 16-bit cases — test_unet_chain_cpu.py checks it. Random inputs cannot do that for 130 nodes under a tanh,
so the inputs are built: `pool_inputs` places the scores on a shuffled grid, `model_case` builds the model cases (see there)."""
import functools
import math
import os
from dataclasses import dataclass

import numpy as np
import torch

import chain_harness as ch
from chain_harness import BF16, DNAME, DTYPES, F16, F32, PROJECT_BAR, rel_err  # noqa: F401
from conv_chain import _q

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet_self_error.json")
SEAM_DEGREES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 129)
HEAVY_DEGREES = (8193, 20000)
TOPK_RATIOS = (0.5, 0.8, 1.0, 1e-5)      # the float ratios the GPU tests use (1e-5: k = 1 everywhere)
GAP = {F32: 1e-3, F16: 0.05, BF16: 0.05}


# ---- selection ------------------------------------------------------------------------------------------------------------
def k_of(num_nodes, ratio):
    """int64 k per graph: PyG's (ratio * num_nodes.to(torch.float)).ceil() in float32, or min(k, n) for an integer ratio."""
    if isinstance(ratio, int):
        return num_nodes.clamp(max=ratio)
    return (ratio * num_nodes.to(torch.float)).ceil().to(torch.long)


def k_of_numpy(n, ratio):
    """The same formula restated in numpy float32 for one n."""
    return int(np.ceil(np.float32(ratio) * np.float32(n)))


def topk(x, ratio, batch, num_graphs):
    """torch_geometric.nn.pool.topk_pool.topk without min_score; the sort is stable, so ties go to the lower id."""
    num_nodes = torch.bincount(batch, minlength=num_graphs)
    max_n = int(num_nodes.max()) if num_graphs else 0
    cum = torch.cat([num_nodes.new_zeros(1), num_nodes.cumsum(0)[:-1]])
    index = torch.arange(batch.numel()) - cum[batch] + batch * max_n
    dense = x.new_full((num_graphs * max_n,), torch.finfo(x.dtype).min)
    dense[index] = x
    _, perm = dense.view(num_graphs, max_n).sort(dim=-1, descending=True, stable=True)
    perm = (perm + cum.view(-1, 1)).view(-1)
    k = k_of(num_nodes, ratio)
    mask = [torch.arange(int(k[i])) + i * max_n for i in range(num_graphs)]
    out_ptr = torch.cat([k.new_zeros(1), k.cumsum(0)])
    return perm[torch.cat(mask)] if mask else perm[:0], out_ptr


def filter_adj(edge_index, edge_attr, perm, num_nodes):
    mask = perm.new_full((num_nodes,), -1)
    mask[perm] = torch.arange(perm.numel())
    row, col = mask[edge_index[0]], mask[edge_index[1]]
    keep = (row >= 0) & (col >= 0)
    return torch.stack([row[keep], col[keep]]), (edge_attr[keep] if edge_attr is not None else None)


def remove_self_loops(edge_index, edge_attr=None):
    keep = edge_index[0] != edge_index[1]
    return edge_index[:, keep], (edge_attr[keep] if edge_attr is not None else None)


def min_gap(score, batch, num_graphs):
    """The smallest distance between two adjacent scores of one graph (inf without a pair)."""
    gap = math.inf
    for g in range(num_graphs):
        s = score[batch == g].double().sort().values
        if s.numel() > 1:
            gap = min(gap, float((s[1:] - s[:-1]).min()))
    return gap


# ---- GCN ------------------------------------------------------------------------------------------------------------------
def gcn_norm(edge_index, w, n, fill_value, dtype):
    """add_remaining_self_loops + gcn_norm: (edge_index with one loop per node, its normalised weights)."""
    row, col = edge_index[0], edge_index[1]
    w = torch.ones(row.numel(), dtype=dtype) if w is None else w.to(dtype)
    keep = row != col
    loop_w = torch.full((n,), float(fill_value), dtype=dtype)
    for e in torch.nonzero(~keep).view(-1).tolist():      # the CPU implementation: in edge order, the last one wins
        loop_w[row[e]] = w[e]
    loops = torch.arange(n)
    ei = torch.cat([edge_index[:, keep], torch.stack([loops, loops])], dim=1)
    w = torch.cat([w[keep], loop_w])
    deg = torch.zeros(n, dtype=dtype).index_add_(0, ei[1], w)
    dis = torch.where(deg > 0, deg.clamp(min=1e-300 if dtype == torch.float64 else 1e-38).pow(-0.5), torch.zeros_like(deg))
    return ei, dis[ei[0]] * w * dis[ei[1]]


def gcn_propagate(h, edge_index, w, n, fill_value, bias=None, rnd=None):
    ei, norm = gcn_norm(edge_index, w, n, fill_value, h.dtype)
    out = torch.zeros((n, h.size(1)), dtype=h.dtype).index_add_(0, ei[1], norm.unsqueeze(1) * h[ei[0]])
    return _q(out if bias is None else out + bias, rnd)


def gcn_conv(P, prefix, x, edge_index, w, improved, rnd=None):
    h = _q(x @ P[prefix + "lin.weight"].t(), rnd)
    return gcn_propagate(h, edge_index, w, x.size(0), 2.0 if improved else 1.0, P.get(prefix + "bias"), rnd)


def _leaves(ops, dtype):
    return {k: (v.to(dtype).detach().clone().requires_grad_(True) if v is not None else None) for k, v in ops.items()}


def _run(fn, ops, R, rnd):
    """(out, grads of sum(out * R)) as float64 of fn(leaves) in float64, or with ``rnd`` in float32 with storage rounding."""
    leaf = _leaves(ops, torch.float64 if rnd is None else torch.float32)
    out = fn(leaf)
    (out * R.to(out.dtype)).sum().backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).double() for k, v in leaf.items() if v is not None}
    if rnd is not None:
        grads = {k: _q(v, rnd) for k, v in grads.items()}
    return out.detach().double(), grads


def propagate_grads(ops, edge_index, w, n, fill_value, R, rnd=None):
    """ops: {"h", "bias"}."""
    return _run(lambda f: gcn_propagate(f["h"], edge_index, w, n, fill_value, f["bias"], rnd), ops, R, rnd)


def conv_grads(ops, edge_index, w, improved, R, rnd=None):
    """ops: {"x", "lin.weight", "bias"}."""
    return _run(lambda f: gcn_conv(f, "", f["x"], edge_index, w, improved, rnd), ops, R, rnd)


# ---- TopKPooling / GraphUNet ----------------------------------------------------------------------------------------------
def pool_score(x, weight, nonlinearity):
    return nonlinearity((x * weight).sum(dim=-1) / weight.norm(p=2, dim=-1))


def topk_pooling(x, weight, edge_index, edge_attr, batch, num_graphs, ratio, nonlinearity=torch.tanh, multiplier=1.0, rnd=None):
    score = pool_score(x, weight, nonlinearity)
    perm, _ = topk(score.detach(), ratio, batch, num_graphs)
    kept = _q(score, rnd)[perm]
    out = _q(x[perm] * kept.view(-1, 1), rnd)
    if multiplier != 1:
        out = _q(multiplier * out, rnd)
    ei, ea = filter_adj(edge_index, edge_attr, perm, x.size(0))
    return out, ei, ea, batch[perm], perm, kept, score.detach()


def pooling_grads(ops, edge_index, edge_attr, batch, num_graphs, ratio, nonlinearity, R, rnd=None):
    """ops: {"x", "weight"}. Returns (out, grads, the forward's other results)."""
    keep = {}

    def fn(f):
        res = topk_pooling(f["x"], f["weight"], edge_index, edge_attr, batch, num_graphs, ratio, nonlinearity, rnd=rnd)
        keep["rest"] = res[1:]
        return res[0]

    out, grads = _run(fn, ops, R, rnd)
    return out, grads, keep["rest"]


def augment_adj(edge_index, edge_weight, n):
    """remove_self_loops, a unit loop per node, A @ A (dense: test sizes), remove_self_loops; row-major like a coalesced result."""
    ei, ew = remove_self_loops(edge_index, edge_weight)
    a = torch.zeros((n, n), dtype=edge_weight.dtype).index_put_((ei[0], ei[1]), ew, accumulate=True)
    a = a + torch.eye(n, dtype=edge_weight.dtype)
    pattern = ((a != 0).double() @ (a != 0).double()) > 0      # structural nonzeros, as the sparse product keeps them
    a2 = a @ a
    idx = torch.nonzero(pattern).t()
    return remove_self_loops(idx, a2[idx[0], idx[1]])


def graph_unet(P, depth, x, edge_index, batch, num_graphs, sum_res=True, ratio=0.5):
    """torch_geometric.nn.models.GraphUNet.forward (2.0.2): (out, perms, [(score, batch) the pool of each level saw])."""
    act = torch.relu
    ew = torch.ones(edge_index.size(1), dtype=x.dtype)
    x = act(gcn_conv(P, "down_convs.0.", x, edge_index, ew, True))
    xs, eis, ews, perms, scores = [x], [edge_index], [ew], [], []
    ei = edge_index
    for i in range(1, depth + 1):
        ei, ew = augment_adj(ei, ew, x.size(0))
        seen = batch
        x, ei, ew, batch, perm, _, score = topk_pooling(x, P[f"pools.{i - 1}.weight"], ei, ew, batch, num_graphs, ratio)
        scores.append((score, seen))
        x = act(gcn_conv(P, f"down_convs.{i}.", x, ei, ew, True))
        if i < depth:
            xs.append(x)
            eis.append(ei)
            ews.append(ew)
        perms.append(perm)
    for i in range(depth):
        j = depth - 1 - i
        up = torch.zeros_like(xs[j]).index_add(0, perms[j], x)
        x = xs[j] + up if sum_res else torch.cat((xs[j], up), dim=-1)
        x = gcn_conv(P, f"up_convs.{i}.", x, eis[j], ews[j], True)
        x = act(x) if i < depth - 1 else x
    return x, perms, scores


# ---- model cases ----------------------------------------------------------------------------------------------------------
# Scores inside a graph must stay 1e-3 apart at every level. Random inputs cannot do that (300 values under a tanh: one chance
# in e^45), so the inputs are BUILT. Every graph is a directed ring i -> i + 1 whose size is a multiple of 4. On such a ring the
# improved normalised adjacency is (2 I + S) / 3, and when every other node is kept, the squared, filtered ring is again a directed
# ring with unit weights. Hidden channel 0 of down conv l is the score channel of pool l + 1 (its weight row is a unit vector, its
# bias 0, the pool's weight is e_0); the value it must take — a grid of well separated positive numbers, the upper half on every
# other node — is carried there from input channel l through unit rows, and the input channel is found by solving the linear
# maps backwards (`_dense_norm` of the graphs the chain itself produces). Values that pass a relu are kept >= 0: score grids of
# levels >= 2 lie in [0.65, 1.15], where the inverse of (2 I + S) / 3 stays positive, and carriers are zero off the kept nodes.
# The other channels, rows and parameters are random.
UNET_SHAPES = {"in": 6, "hidden": 16, "out": 3}
MODEL_GRAPHS = {"molecules": (24, 32, 40, 28), "ring": (300,)}
MODEL_CASES = [(graph, depth, sum_res) for graph in MODEL_GRAPHS for depth in (1, 3) for sum_res in (True, False)]


def unet_state_shapes(depth, sum_res):
    c, up_in = UNET_SHAPES["hidden"], UNET_SHAPES["hidden"] * (1 if sum_res else 2)
    shapes = {"down_convs.0.lin.weight": (c, UNET_SHAPES["in"]), "down_convs.0.bias": (c,)}
    for i in range(depth):
        shapes[f"pools.{i}.weight"] = (1, c)
        shapes[f"down_convs.{i + 1}.lin.weight"] = (c, c)
        shapes[f"down_convs.{i + 1}.bias"] = (c,)
        out = c if i < depth - 1 else UNET_SHAPES["out"]
        shapes[f"up_convs.{i}.lin.weight"] = (out, up_in)
        shapes[f"up_convs.{i}.bias"] = (out,)
    return shapes


def _dense_norm(ei, ew, n):
    """The improved normalised adjacency as a dense matrix: out = M @ h."""
    full, norm = gcn_norm(ei, ew, n, 2.0, torch.float64)
    return torch.zeros((n, n), dtype=torch.float64).index_put_((full[1], full[0]), norm, accumulate=True)


def _grid(n, lo, hi, high, g):
    """n values evenly spaced in [lo, hi], shuffled, the upper half on the nodes of the bool mask ``high``."""
    vals = lo + (hi - lo) * torch.arange(n, dtype=torch.float64) / max(n - 1, 1)
    k = int(high.sum())
    t = torch.empty(n, dtype=torch.float64)
    t[high] = vals[n - k:][torch.randperm(k, generator=g)]
    t[~high] = vals[:n - k][torch.randperm(n - k, generator=g)]
    return t


def model_case(graph, depth, sum_res, seed=3):
    """(P, x, edge_index, batch, G): float64 tensors of float32 values."""
    g = torch.Generator().manual_seed(seed)
    sizes = MODEL_GRAPHS[graph]
    G, N = len(sizes), sum(sizes)
    start = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    batch = torch.cat([torch.full((n,), b, dtype=torch.long) for b, n in enumerate(sizes)])
    pos = torch.cat([torch.arange(n) for n in sizes])                       # place on its ring
    src = torch.arange(N)
    dst = torch.cat([torch.as_tensor(start[b]) + (torch.arange(n) + 1) % n for b, n in enumerate(sizes)])
    ei = torch.stack([src, dst])[:, torch.randperm(N, generator=g)]
    # structure pass: the graphs, the kept nodes and the score grids of every level follow from the grids alone
    mats, targets, perms, sc = [], [], [], []
    e, w, b_l, pos_l = ei, torch.ones(N, dtype=torch.float64), batch, pos
    for l in range(depth):
        n_l = b_l.numel()
        mats.append(_dense_norm(e, w, n_l))
        high = (pos_l % (2 ** (l + 1))) == 0
        t = torch.empty(n_l, dtype=torch.float64)
        for b in range(G):
            m = b_l == b
            t[m] = _grid(int(m.sum()), 0.05 if l == 0 else 0.65, 1.15, high[m], g)
        perm, _ = topk(torch.tanh(t), 0.5, b_l, G)
        targets.append(t); perms.append(perm); sc.append(torch.tanh(t))
        e, w = augment_adj(e, w, n_l)
        e, w = filter_adj(e, w, perm, n_l)
        b_l, pos_l = b_l[perm], pos_l[perm]
    # solve backwards: input channel l carries the score grid of level l + 1
    x = torch.randn(N, UNET_SHAPES["in"], generator=g, dtype=torch.float64)
    for l in range(depth):
        need = torch.linalg.solve(mats[l], targets[l])            # what the conv of level l must read in its carrier channel
        for k in range(l - 1, -1, -1):                            # down through pool k + 1 and conv k
            kept = perms[k]
            v = need / sc[k][kept]                                # the conv output on the kept nodes (>= 0), zero elsewhere
            sub = mats[k][kept][:, kept]
            need = torch.zeros(mats[k].size(0), dtype=torch.float64)
            if k > 0:
                need[kept] = torch.linalg.solve(sub, v)           # kept nodes are never neighbours: sub is diagonal
            else:
                full = torch.zeros(mats[0].size(0), dtype=torch.float64)
                full[kept] = v
                need = torch.linalg.solve(mats[0], full)          # the raw input may have any sign
        x[:, l] = need
    x = x.float().double()
    P = {k: (torch.randn(s, generator=g, dtype=torch.float64) * (0.1 if k.endswith("bias") else 0.5))
         for k, s in unet_state_shapes(depth, sum_res).items()}
    for l in range(depth):
        P[f"pools.{l}.weight"].zero_()
        P[f"pools.{l}.weight"][0, 0] = 1.0
        for j in range(l, depth):                                 # conv l: out channel 0 <- carrier l, out channel j <- carrier j
            row = 0 if j == l else j
            W = P[f"down_convs.{l}.lin.weight"]
            W[row].zero_()
            W[row, j if (l == 0 or j > l) else l] = 1.0
            P[f"down_convs.{l}.bias"][row] = 0.0
    return {k: v.float().double() for k, v in P.items()}, x, ei, batch, G


def model_gap(graph, depth, sum_res):
    P, x, ei, batch, G = model_case(graph, depth, sum_res)
    _, _, scores = graph_unet(P, depth, x, ei, batch, G, sum_res)
    return min(min_gap(s, b, G) for s, b in scores)


def model_grads(graph, depth, sum_res):
    """(out, perms, {parameter or "x": gradient of sum(out * R)}, R) of the float64 chain."""
    P, x, ei, batch, G = model_case(graph, depth, sum_res)
    leaf = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    xl = x.clone().requires_grad_(True)
    out, perms, _ = graph_unet(leaf, depth, xl, ei, batch, G, sum_res)
    R = torch.randn(out.shape, generator=torch.Generator().manual_seed(17), dtype=torch.float64)
    (out * R).sum().backward()
    grads = {k: v.grad for k, v in leaf.items()}
    grads["x"] = xl.grad
    return out.detach(), perms, grads, R


# ---- graphs and case tables -----------------------------------------------------------------------------------------------
def degree_graph(degrees, n_extra, g):
    """A graph whose first len(degrees) nodes have exactly those numbers of non-loop in-edges, from random other nodes."""
    n = len(degrees) + n_extra
    src, dst = [], []
    for i, d in enumerate(degrees):
        s = torch.randint(0, n - 1, (d,), generator=g)
        s = s + (s >= i).long()          # never i itself
        src.append(s); dst.append(torch.full((d,), i, dtype=torch.long))
    extra = torch.randint(0, n, (2, 3 * n_extra), generator=g)
    extra = extra[:, extra[0] != extra[1]]
    ei = torch.cat([torch.stack([torch.cat(src), torch.cat(dst)]), extra], dim=1)
    return ei[:, torch.randperm(ei.size(1), generator=g)], n


@dataclass(frozen=True)
class GcnCase(ch.CaseBars):
    table: str
    name: str
    K: int = 8
    graph: str = "random"        # random | seams | loops | heavy | empty | dup
    weights: str = "random"      # none | random
    layout: str = "dense"        # dense | aligned (a 16-byte aligned column block) | misaligned
    improved: bool = False
    bias: bool = True
    ones: bool = False           # the functional is out.sum(): an expanded gradient
    dtypes: tuple = tuple(DTYPES)

    def id(self, dtype):
        return f"{self.table}-{self.name}-{DNAME[dtype]}"

    def self_bar(self, dtype):
        return dtype == BF16 or self.table == "heavy"


SHAPES = [GcnCase("shape", f"K{K}-{lay}", K=K, layout=lay) for K in (1, 5, 8, 64, 136) for lay in ("dense", "aligned", "misaligned")]
SEAMS = [GcnCase("seams", f"K{K}", K=K, graph="seams") for K in (8, 5)]
LOOPS = [GcnCase("loops", f"improved{int(i)}", K=8, graph="loops", improved=i) for i in (False, True)]
WEIGHTS = [GcnCase("weights", "none", weights="none"), GcnCase("weights", "random"), GcnCase("weights", "dup", graph="dup"),
           GcnCase("weights", "ones-nobias", bias=False, ones=True)]
HEAVY = [GcnCase("heavy", "K8", K=8, graph="heavy")]
EMPTY = [GcnCase("plan", "E0", graph="empty")]
TABLES = {"shape": SHAPES, "seams": SEAMS, "loops": LOOPS, "weights": WEIGHTS, "heavy": HEAVY, "plan": EMPTY}
LOOP_NODES = {"none": 0, "one": 1, "two": 2, "dead": 3}     # loops graph: node 3's only edge is a self loop of weight 0


def gcn_inputs(case, dtype, seed=4242):
    """(ops {"h", "bias"} float64 of storage-rounded values, edge_index, w or None (fp32 values), n, fill, R)."""
    g = torch.Generator().manual_seed(seed)
    if case.graph == "seams":
        ei, n = degree_graph(SEAM_DEGREES, 140, g)
    elif case.graph == "heavy":
        ei, n = degree_graph(HEAVY_DEGREES, 300, g)
    elif case.graph == "empty":
        ei, n = torch.zeros((2, 0), dtype=torch.long), 37
    elif case.graph == "loops":
        n = 40
        ei = torch.randint(4, n, (2, 150), generator=g)
        ei = ei[:, ei[0] != ei[1]]
        ei = torch.cat([ei, torch.tensor([[5, 9, 1, 2, 7, 2, 3], [0, 0, 1, 2, 1, 2, 3]])], dim=1)   # loops: 1 once, 2 twice, 3 (dead)
    elif case.graph == "dup":
        n = 50
        ei = torch.randint(0, n, (2, 120), generator=g)
        ei = torch.cat([ei, ei[:, :60], ei[:, :20]], dim=1)
    else:
        n = 203
        ei = torch.randint(0, n, (2, 1100), generator=g)
    E = ei.size(1)
    w = None
    if case.weights == "random":
        w = (torch.rand(E, generator=g) + 0.25).float()
        if case.graph == "loops":
            w[-1] = 0.0                                                  # node 3: deg = 0
    rd = lambda t: t.to(dtype).double()   # noqa: E731
    ops = {"h": rd(torch.randn(n, case.K, generator=g, dtype=torch.float64)),
           "bias": rd(torch.randn(case.K, generator=g, dtype=torch.float64)) if case.bias else None}
    R = torch.ones(n, case.K, dtype=torch.float64) if case.ones else rd(torch.randn(n, case.K, generator=g, dtype=torch.float64))
    return ops, ei, w, n, (2.0 if case.improved else 1.0), R


def gcn_case_grads(case, dtype, rnd=None):
    ops, ei, w, n, fill, R = gcn_inputs(case, dtype)
    return propagate_grads(ops, ei, w, n, fill, R, rnd=rnd)


def pool_inputs(sizes, C, dtype, seed=99):
    """x, weight (storage-rounded float64), edge_index, edge_attr, batch for TopKPooling: the pre-activation scores of every graph
    lie on a shuffled grid, spaced so that the gap bar of the dtype holds after the nonlinearity the case uses (tanh for fp32,
    the identity for 16 bits: no 130 values 0.05 apart fit under a tanh)."""
    g = torch.Generator().manual_seed(seed)
    rd = lambda t: t.to(dtype).double()   # noqa: E731
    weight = rd(torch.randn(1, C, generator=g, dtype=torch.float64))
    unit = weight / weight.norm()
    step = 0.023 if dtype == F32 else 0.125
    xs, batch = [], []
    for b, n in enumerate(sizes):
        target = (torch.arange(n, dtype=torch.float64) - (n - 1) / 2) * step
        target = target[torch.randperm(n, generator=g)]
        noise = torch.randn(n, C, generator=g, dtype=torch.float64)
        noise = noise - (noise * unit).sum(-1, keepdim=True) * unit if C > 1 else noise * 0
        xs.append(target.view(-1, 1) * unit + noise)
        batch.append(torch.full((n,), b, dtype=torch.long))
    x, batch = rd(torch.cat(xs)), torch.cat(batch)
    N = x.size(0)
    start = torch.tensor([0] + list(np.cumsum(sizes)[:-1]))
    src = torch.randint(0, 10 ** 6, (4 * N,), generator=g)
    dst = torch.randint(0, 10 ** 6, (4 * N,), generator=g)
    eb = torch.randint(0, len(sizes), (4 * N,), generator=g)
    size_t = torch.tensor(sizes)
    ei = torch.stack([start[eb] + src % size_t[eb], start[eb] + dst % size_t[eb]])
    ea = rd(torch.randn(4 * N, 3, generator=g, dtype=torch.float64))
    return x, weight, ei, ea, batch


POOL_NONLINEARITY = {F32: torch.tanh, F16: torch.nn.Identity(), BF16: torch.nn.Identity()}
POOL_CASES = [(C, d) for C in (5, 64) for d in DTYPES]
POOL_SIZES = (7, 64, 130)


def pool_case_grads(C, dtype, rnd=None):
    x, weight, ei, ea, batch = pool_inputs(POOL_SIZES, C, dtype)
    g = torch.Generator().manual_seed(5)
    k = int(k_of(torch.tensor(POOL_SIZES), 0.5).sum())
    R = torch.randn(k, C, generator=g, dtype=torch.float64).to(dtype).double()
    return pooling_grads({"x": x, "weight": weight}, ei, ea, batch, len(POOL_SIZES), 0.5, POOL_NONLINEARITY[dtype], R, rnd=rnd)


# ---- the chain against itself ---------------------------------------------------------------------------------------------
def self_error_table():
    """One host thread: torch's float32 index_add_ then adds in edge order, so the figures are the same on every host."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _self_error_table()
    finally:
        torch.set_num_threads(threads)


def _self_error_table():
    table = ch.build_table(ch.self_bar_cases(TABLES), functools.partial(ch.self_error, gcn_case_grads))
    for C, d in POOL_CASES:
        if d != BF16:
            continue
        out, grads, _ = pool_case_grads(C, d)
        out_r, grads_r, _ = pool_case_grads(C, d, rnd=d)
        table[f"pool/C{C}/{DNAME[d]}/out"] = rel_err(out_r, out)
        for k in grads:
            table[f"pool/C{C}/{DNAME[d]}/{k}"] = rel_err(grads_r[k], grads[k])
    for improved in (False, True):
        ops, ei, w, R = conv_inputs(BF16, improved)
        out, grads = conv_grads(ops, ei, w, improved, R)
        out_r, grads_r = conv_grads(ops, ei, w, improved, R, rnd=BF16)
        table[f"conv/improved{int(improved)}/bf16/out"] = rel_err(out_r, out)
        for k in grads:
            table[f"conv/improved{int(improved)}/bf16/{k}"] = rel_err(grads_r[k], grads[k])
    return table


def conv_inputs(dtype, improved, seed=31):
    """A GCNConv layer case: 24 -> 40 channels on the loops graph with random weights."""
    g = torch.Generator().manual_seed(seed)
    case = GcnCase("conv", "layer", graph="loops", improved=improved)
    _, ei, w, n, _, _ = gcn_inputs(case, dtype)
    rd = lambda t: t.to(dtype).double()   # noqa: E731
    ops = {"x": rd(torch.randn(n, 24, generator=g, dtype=torch.float64)),
           "lin.weight": rd(torch.randn(40, 24, generator=g, dtype=torch.float64) * 0.3),
           "bias": rd(torch.randn(40, generator=g, dtype=torch.float64))}
    return ops, ei, w, rd(torch.randn(n, 40, generator=g, dtype=torch.float64))


def write_self_error_table(path=GOLDEN_FILE):
    """Regenerates tests/golden/unet_self_error.json (python -c "import unet_chain as uc; uc.write_self_error_table()")."""
    return ch.write_table(self_error_table(), path)


def load_self_error():
    return ch.load_table(GOLDEN_FILE)
