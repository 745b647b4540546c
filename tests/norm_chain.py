"""The yardstick of the head_act_norm and GATv2-model tests: gnnops.conv.head_act_norm (csrc/norm.hip) restated in torch float64 on
the CPU from stock ops, so that torch's own autograd differentiates it:

    a.view(N, H, C).mean(1) -> + bias -> torch.relu -> * k -> torch.nn.functional.layer_norm

``rnd`` (a torch dtype) runs the library's own steps in float32: the heads added in ascending order and divided by H, the mean and
the biased variance as TWO passes over the row, rstd = 1 / sqrt(var + eps), ``out`` rounded to the storage type; on the way back
y, the gate and xhat recomputed, d a = d y / H rounded, and d bias / d gamma / d beta as float32 partial sums (group w of W takes
the rows w, w + W, ...; the W partials are then added in order) rounded once. Every sum over the channels or the rows is an explicit
loop of float32 additions, so the figures are the same on every host. ``self_error`` is the distance between the two chains, per
tensor max |got - want| / max |want|: the reference against itself, never the kernels. It is recorded in
tests/golden/head_act_norm_self_error.json (``write_self_error_table`` regenerates it); the GPU bars of bf16 and of the values
table are 4 x that distance, the factor of attention_chain.py and conv_chain.py. fp32 and fp16 keep PROJECT_BAR of conv_chain.py.

The inputs keep every y at least 1e-2 from the kink of the ReLU (``inputs`` moves the few that are not), as the attention tests
keep their pre-activations off the kink of leaky_relu: float32 and float64 must gate alike for a bar of 3e-5 to mean anything.

The model (gnnops.conv.GATv2, the reference's GATv2REG) restated in float64: per layer the GATv2 attention of attention_chain
(imported, not edited), this file's epilogue, then the mean over each graph's nodes and a Linear."""
import functools
import os
from dataclasses import dataclass

import torch

import attention_chain as ac
import chain_harness as ch
from chain_harness import BF16, DNAME, DTYPES, F16, F32, PROJECT_BAR, rel_err  # noqa: F401
from conv_chain import _lin, _q, _r, _rand, _straight_through, place  # noqa: F401

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_act_norm_self_error.json")
EPS = 1e-5
PARTIAL_GROUPS = 256
P_DROP = 0.3


# ---- the op -----------------------------------------------------------------------------------------------------------------
def head_act_norm(a, H, bias=None, relu=True, k=None, gamma=None, beta=None, eps=EPS):
    """Stock torch ops; the dtype of a is the arithmetic."""
    N, C = a.size(0), a.size(1) // H
    y = a.view(N, H, C).mean(dim=1)
    if bias is not None:
        y = y + bias
    d = torch.relu(y) if relu else y
    if k is not None:
        d = d * k
    if gamma is None:
        return d
    return torch.nn.functional.layer_norm(d, (C,), gamma, beta, eps)


def _row_sum(t):
    """sum over the last dimension as an explicit loop of additions"""
    acc = torch.zeros(t.shape[:-1], dtype=t.dtype)
    for c in range(t.size(-1)):
        acc = acc + t[..., c]
    return acc


def _col_sum(t):
    """sum over the rows as the library adds them: PARTIAL_GROUPS running sums over strided rows, then added in order"""
    N, C = t.shape
    W = max(1, min(PARTIAL_GROUPS, N))
    steps = (N + W - 1) // W
    padded = torch.zeros((steps * W, C), dtype=t.dtype)
    padded[:N] = t
    part = torch.zeros((W, C), dtype=t.dtype)
    for s in range(steps):
        part = part + padded[s * W:(s + 1) * W]
    acc = torch.zeros(C, dtype=t.dtype)
    for w in range(W):
        acc = acc + part[w]
    return acc


def _library_row(f, H, relu, eps):
    """(d, m, mu, rstd): the value the norm sees, d d / d y, and the row statistics, in float32"""
    a = f["a"]
    N, C = a.size(0), a.size(1) // H
    ah = a.view(N, H, C)
    y = ah[:, 0]
    for h in range(1, H):
        y = y + ah[:, h]
    y = y / torch.tensor(float(H), dtype=a.dtype)
    if f.get("bias") is not None:
        y = y + f["bias"]
    k = f["k"] if f.get("k") is not None else torch.ones_like(y)
    r = torch.where(y < 0, torch.zeros_like(y), y) if relu else y
    m = torch.where(y > 0, k, torch.zeros_like(k)) if relu else k
    d = r * k
    if f.get("gamma") is None:
        return d, m, None, None
    Cf = torch.tensor(float(C), dtype=a.dtype)
    mu = _row_sum(d) / Cf
    e = d - mu.unsqueeze(1)
    var = _row_sum(e * e) / Cf
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=a.dtype))
    return d, m, mu, rstd


def library_forward(f, H, relu, eps, rnd):
    d, _, mu, rstd = _library_row(f, H, relu, eps)
    if mu is None:
        return _q(d, rnd)
    out = (d - mu.unsqueeze(1)) * rstd.unsqueeze(1) * f["gamma"]
    if f.get("beta") is not None:
        out = out + f["beta"]
    return _q(out, rnd)


def library_backward(f, H, relu, eps, g, rnd):
    """The steps of gnnops_head_act_norm_backward on float32 operands ``f``: {name: gradient} for a, bias, gamma, beta."""
    a = f["a"]
    N, C = a.size(0), a.size(1) // H
    d, m, mu, rstd = _library_row(f, H, relu, eps)
    r = lambda t: _q(t, rnd)   # noqa: E731
    grads = {}
    if mu is None:
        dd = g
    else:
        Cf = torch.tensor(float(C), dtype=a.dtype)
        xh = (d - mu.unsqueeze(1)) * rstd.unsqueeze(1)
        gx = g * f["gamma"]
        s1 = _row_sum(gx) / Cf
        s2 = _row_sum(gx * xh) / Cf
        dd = rstd.unsqueeze(1) * (gx - s1.unsqueeze(1) - xh * s2.unsqueeze(1))
        grads["gamma"] = r(_col_sum(g * xh))
        if f.get("beta") is not None:
            grads["beta"] = r(_col_sum(g))
    dy = dd * m
    grads["a"] = r(dy / torch.tensor(float(H), dtype=a.dtype)).unsqueeze(1).expand(N, H, C).reshape(N, H * C)
    if f.get("bias") is not None:
        grads["bias"] = r(_col_sum(dy))
    return grads


class _LibraryNorm(torch.autograd.Function):
    """head_act_norm inside a float32 model chain the way the library runs it: output rounded once, backward = library_backward."""

    @staticmethod
    def forward(ctx, H, relu, eps, rnd, k, a, bias, gamma, beta):
        f = {"a": a, "bias": bias, "k": k, "gamma": gamma, "beta": beta}
        ctx.meta = (H, relu, eps, rnd, k)
        ctx.save_for_backward(a, bias, gamma, beta)
        return library_forward(f, H, relu, eps, rnd)

    @staticmethod
    def backward(ctx, g):
        H, relu, eps, rnd, k = ctx.meta
        a, bias, gamma, beta = ctx.saved_tensors
        gr = library_backward({"a": a, "bias": bias, "k": k, "gamma": gamma, "beta": beta}, H, relu, eps, _q(g, rnd), rnd)
        return (None,) * 5 + (gr["a"], gr.get("bias"), gr.get("gamma"), gr.get("beta"))


GRAD_NAMES = ("a", "bias", "gamma", "beta")


def norm_grads(ops, H, relu, R, rnd=None, eps=EPS):
    """ops: {"a", "bias", "k", "gamma", "beta"} float64 tensors of storage-rounded values (None = absent).
    (out, {name: d sum(out * R)}) as float64: torch autograd of the float64 chain, or with ``rnd`` the library's own steps."""
    if rnd is None:
        leaf = {n: (v.detach().clone().requires_grad_(n != "k") if v is not None else None) for n, v in ops.items()}
        out = head_act_norm(leaf["a"], H, leaf["bias"], relu, leaf["k"], leaf["gamma"], leaf["beta"], eps)
        (out * R).sum().backward()
        return out.detach(), {n: (leaf[n].grad if leaf[n].grad is not None else torch.zeros_like(leaf[n]))
                              for n in GRAD_NAMES if leaf[n] is not None}
    f = {n: (v.float() if v is not None else None) for n, v in ops.items()}
    out = library_forward(f, H, relu, eps, rnd)
    grads = library_backward(f, H, relu, eps, R.float(), rnd)
    return out.double(), {n: v.double() for n, v in grads.items()}


# ---- cases ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case(ch.CaseBars):
    table: str
    name: str
    H: int
    C: int
    N: int = 257
    layout: str = "block"        # block: a is a column block of a wider matrix (pitch != H * C); plain: dense
    bias: bool = True
    relu: bool = True
    scale: bool = True
    norm: bool = True
    values: str = "random"       # random | constant | dropped | gamma_zero | big_mean | negative
    bar: str = "project"         # project: PROJECT_BAR for fp32 / fp16, 4 x self error for bf16; self: 4 x self error for all
    dtypes: tuple = tuple(DTYPES)


SHAPES = [Case("shape", f"H{H}-C{C}", H, C) for H in (1, 3, 4) for C in (1, 5, 8, 64, 136, 1024)]
SHAPES += [Case("shape", "H4-C8-dense", 4, 8, layout="plain"),
           Case("shape", "H3-C40-no_bias", 3, 40, bias=False), Case("shape", "H3-C40-no_relu", 3, 40, relu=False),
           Case("shape", "H3-C40-no_scale", 3, 40, scale=False), Case("shape", "H3-C40-no_norm", 3, 40, norm=False),
           Case("shape", "H2-C136-bare", 2, 136, bias=False, relu=False, scale=False, norm=False),
           Case("shape", "H1-C8192", 1, 8192, N=33), Case("shape", "H8-C1024", 8, 1024, N=33)]
# C = 4 is one 16-byte (fp32) or 8-byte (16-bit) piece: one lane per row, 64 rows per wave in every type
ROWS = [Case("rows", f"N{N}", 3, 4, N=N) for N in (1, 63, 64, 65)] + [Case("rows", "N70000", 2, 8, N=70000)]
VALUES = [Case("values", "constant_rows", 2, 8, N=70, bias=False, scale=False, values="constant", bar="self"),
          Case("values", "dropped_rows", 3, 8, N=70, values="dropped", bar="self"),
          Case("values", "gamma_zero", 3, 8, N=70, values="gamma_zero", bar="self"),
          Case("values", "big_mean", 2, 64, N=70, bias=False, scale=False, values="big_mean", bar="self"),
          Case("values", "all_negative", 3, 8, N=70, values="negative", bar="self")]
TABLES = {"shape": SHAPES, "rows": ROWS, "values": VALUES}
SPECIAL_ROWS = (0, 5, 64, 69)      # the rows the constant / dropped / negative cases set


def inputs(case, dtype, seed=777):
    """({"a", "bias", "k", "gamma", "beta"}: float64 tensors of storage-rounded values or None, R float64 storage-rounded)."""
    g = torch.Generator().manual_seed(seed + sum(map(ord, case.table + case.name)))
    N, H, C = case.N, case.H, case.C
    rd = lambda t: t.to(dtype).double()   # noqa: E731
    a = _rand(g, N, H * C)
    bias = _rand(g, C, scale=0.5) if case.bias else None
    k = ((torch.rand(N, C, generator=g) >= P_DROP).float() / (1.0 - P_DROP)) if case.scale else None
    gamma = 1.0 + _rand(g, C, scale=0.5) if case.norm else None
    beta = _rand(g, C, scale=0.5) if case.norm else None
    R = _rand(g, N, C)
    rows = [r for r in SPECIAL_ROWS if r < N]
    if case.values == "constant":           # every entry of the row the same power of two: sums exact in any order, var = 0
        for j, r_ in enumerate(rows):
            a[r_] = 0.5 / (1 << j)
    elif case.values == "dropped":
        k[rows] = 0.0
    elif case.values == "gamma_zero":
        gamma[2] = 0.0
    elif case.values == "big_mean":
        a = 1.0e4 + a
    elif case.values == "negative":
        a[rows] = -a[rows].abs() - 1.0
    a = rd(a)
    if case.relu:                           # keep y off the kink: move the few entries within 1e-2 of it
        y = a.view(N, H, C).mean(1) + (rd(bias) if bias is not None else 0.0)
        near = y.abs() < 1e-2
        step = torch.where(y >= 0, torch.ones_like(y), -torch.ones_like(y)) * 0.0625 * H
        a.view(N, H, C)[:, 0][near] += step[near]
        a = rd(a)
    opt = lambda t: None if t is None else rd(t)   # noqa: E731
    return {"a": a, "bias": opt(bias), "k": opt(k), "gamma": opt(gamma), "beta": opt(beta)}, rd(R)


def case_grads(case, dtype, rnd=None, ones=False):
    ops, R = inputs(case, dtype)
    return norm_grads(ops, case.H, case.relu, torch.ones_like(R) if ones else R, rnd=rnd)


self_error = functools.partial(ch.self_error, case_grads)


def self_error_cases():
    return ch.self_bar_cases(TABLES)


# ---- the model ----------------------------------------------------------------------------------------------------------------
MODEL = {"input_dim": 7, "hidden_dim": 16, "dropout": P_DROP, "num_conv_layers": 2, "heads": 3}
GRAPH_SIZES = (20, 33, 40, 27, 36)


def model_state_shapes(input_dim, hidden_dim, num_conv_layers, heads):
    """The key set and shapes of the reference model's state_dict, from the names of the issue (PyG 2.0.2 GATv2Conv, LayerNorm)."""
    st = {}
    for k in range(num_conv_layers + 1):
        cin = input_dim if k == 0 else hidden_dim
        st.update({f"convs.{k}.att": (1, heads, hidden_dim), f"convs.{k}.bias": (hidden_dim,),
                   f"convs.{k}.lin_l.weight": (heads * hidden_dim, cin), f"convs.{k}.lin_l.bias": (heads * hidden_dim,),
                   f"convs.{k}.lin_r.weight": (heads * hidden_dim, cin), f"convs.{k}.lin_r.bias": (heads * hidden_dim,)})
    for k in range(num_conv_layers):
        st.update({f"lns.{k}.weight": (hidden_dim,), f"lns.{k}.bias": (hidden_dim,)})
    st.update({"post_mp.0.weight": (1, hidden_dim), "post_mp.0.bias": (1,)})
    return st


def model_fixture(seed=31):
    """(params {name: float32}, x, edge_index, batch, masks [layers x [N, hidden]] float32): 5 graphs of 20 to 40 nodes, edges
    inside each graph, some self loops and repeated edges."""
    g = torch.Generator().manual_seed(seed)
    shapes = model_state_shapes(MODEL["input_dim"], MODEL["hidden_dim"], MODEL["num_conv_layers"], MODEL["heads"])
    params = {}
    for name, shape in shapes.items():
        scale = 0.5 if name.endswith("bias") else 0.7
        params[name] = _rand(g, *shape, scale=scale)
        if name.startswith("lns.") and name.endswith("weight"):
            params[name] = params[name] + 1.0
    batch = torch.cat([torch.full((n,), i, dtype=torch.int64) for i, n in enumerate(GRAPH_SIZES)])
    N = batch.numel()
    edges, start = [], 0
    for n in GRAPH_SIZES:
        e = 4 * n
        edges.append(torch.randint(0, n, (2, e), generator=g) + start)
        start += n
    ei = torch.cat(edges, dim=1)
    ei = ei[:, torch.randperm(ei.size(1), generator=g)]
    x = _rand(g, N, MODEL["input_dim"])
    masks = [(torch.rand(N, MODEL["hidden_dim"], generator=g) >= P_DROP).float() / (1.0 - P_DROP) for _ in range(MODEL["num_conv_layers"])]
    return params, x, ei, batch, masks


def used_parameters():
    L = MODEL["num_conv_layers"]
    shapes = model_state_shapes(MODEL["input_dim"], MODEL["hidden_dim"], L, MODEL["heads"])
    return [n for n in shapes if not n.startswith(f"convs.{L}.") and not n.startswith(f"lns.{L - 1}.")]


def mean_pool(x, batch, G):
    out = torch.zeros((G, x.size(1)), dtype=x.dtype).index_add_(0, batch, x)
    return out / torch.bincount(batch, minlength=G).clamp(min=1).to(x.dtype).unsqueeze(1)


def gatv2_model(P, x, ei, batch, masks=None, rnd=None, rd=None):
    """The model's forward on the parameters P. masks: per layer the [N, hidden] feature mask (train mode) or None (eval).
    ``rnd``: as the library runs it in float32 (projections and attention output rounded, the library-order epilogue, the pool
    and the Linear rounded). ``rd`` (float64, 16-bit storage): rounds straight-through what the device keeps in the storage type
    ahead of a kink (the projections, the attention output, a layer's output), so that both sides gate on the same numbers."""
    L, H, C = MODEL["num_conv_layers"], MODEL["heads"], MODEL["hidden_dim"]
    n = x.size(0)
    looped = ac.with_self_loops(ei, n)
    for k in range(L):
        pre = f"convs.{k}."
        q = _lin(x, P[pre + "lin_l.weight"], P[pre + "lin_l.bias"], rnd)
        p = _lin(x, P[pre + "lin_r.weight"], P[pre + "lin_r.bias"], rnd)
        if rd is not None and rnd is None:
            q, p = rd(q), rd(p)
        att = P[pre + "att"].reshape(-1)
        last = k == L - 1
        gamma, beta = (None, None) if last else (P[f"lns.{k}.weight"], P[f"lns.{k}.bias"])
        mask = None if masks is None else masks[k].to(x.dtype)
        if rnd is None:
            a, _ = ac.attention(q, p, att, looped, n, H, 0.2)
            if rd is not None:
                a = rd(a)
            x = head_act_norm(a, H, P[pre + "bias"], True, mask, gamma, beta)
            if rd is not None:
                x = rd(x)
        else:
            a = ac._LibraryAttention.apply(looped, n, H, 0.2, rnd, q, p, att)
            x = _LibraryNorm.apply(H, True, EPS, rnd, mask, a, P[pre + "bias"], gamma, beta)
    G = len(GRAPH_SIZES)
    pooled = _r(mean_pool(x, batch, G), rnd)
    return _lin(pooled, P["post_mp.0.weight"], P["post_mp.0.bias"], rnd)


def model_grads(dtype, train, rnd=None, params=None):
    """(out [G, 1], {used parameter: d sum(out * coef)}) as float64 on storage-rounded parameters and input."""
    P0, x, ei, batch, masks = model_fixture()
    if params is not None:
        P0 = params
    cdt = torch.float64 if rnd is None else torch.float32
    P = {k: v.to(dtype).to(cdt).requires_grad_(True) for k, v in P0.items()}
    xin = x.to(dtype).to(cdt)
    mk = [m.to(dtype).to(cdt) for m in masks] if train else None
    out = gatv2_model(P, xin, ei, batch, mk, rnd=rnd, rd=_straight_through(dtype))
    coef = _rand(torch.Generator().manual_seed(99), *out.shape)
    (out * coef.to(cdt)).sum().backward()
    # the device holds a parameter's gradient in the storage type: whatever produced it (a kernel of this package or torch's own
    # Linear backward), it is rounded once more on the way into .grad
    return out.detach().double(), {k: _q(P[k].grad if P[k].grad is not None else torch.zeros_like(P[k]), rnd).double()
                                   for k in used_parameters()}, P


def model_self_error(dtype, train):
    out, grads, _ = model_grads(dtype, train)
    out_r, grads_r, _ = model_grads(dtype, train, rnd=dtype)
    err = {"forward": rel_err(out_r, out)}
    for k in grads:
        err[f"d {k}"] = rel_err(grads_r[k], grads[k])
    return err


def model_key(mode, dtype, tensor):
    return f"model/{mode}/{DNAME[dtype]}/{tensor}"


# ---- the table ----------------------------------------------------------------------------------------------------------------
def self_error_table():
    table = ch.build_table(self_error_cases(), self_error)
    for mode, train in (("eval", False), ("train", True)):
        for k, v in model_self_error(BF16, train).items():
            table[model_key(mode, BF16, k)] = v
    return table


def write_self_error_table(path=GOLDEN_FILE):
    """Regenerates tests/golden/head_act_norm_self_error.json (python -c "import norm_chain as nc; nc.write_self_error_table()")."""
    return ch.write_table(self_error_table(), path)


def load_self_error():
    return ch.load_table(GOLDEN_FILE)
