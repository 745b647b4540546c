"""Single message-passing layers, forward pass: the five layers the reference's app benchmarks time
(app_bm/benchmark_convs.py:146-246: FiLMConv, GINConv, CGConv, PNAConv, SAGEConv; app_bm/groq_script.py:15-111 holds the
text of CGConv itself) — SURVEY.md §8(f) rank 4.

Constructor arguments, parameter names and shapes follow torch_geometric.nn.conv (2.0.2, requirements.txt:211), so a
state_dict moves between the two; the forward is NOT MessagePassing.propagate. A layer here is
    one dense product  x @ [all the layer's per-node weight blocks]      (gemm.hip, MFMA)
    one edge pass      gnnops_edge_reduce (csrc/conv.hip): message + aggregation(s) + degree scalers + residual
    (PNA / GIN / SAGE) one dense product on the aggregate                (gemm.hip)
because every Linear a message applies to cat([x_i, x_j, e]) splits into per-node products: z W = x_i W_i + x_j W_j + e W_e.
The [E, .] tensors of propagate (x_i, x_j, z, the messages) never exist.

Training (the reference's OpProfiler.py:259-292 profiles a train loop): GINConv, SAGEConv, CGConv and FiLMConv are
differentiable — the dense products through gnnops.autograd.addmm, the edge pass through `_EdgeReduce` below, whose backward
is the forward's own machinery run the other way: the output gradient gathered along the TRANSPOSED plan (copy messages), or
one streaming kernel that writes the per-edge gradient of the message (gnnops_edge_grad: cgconv / film) followed by two
segment sums over the plans the forward already holds (by destination for the p side, by source for the q side). Packed
weight operands are cached only while nothing requires grad. PNAConv (min / max / std aggregators with degree scalers) trains
through `edge_aggregate`: the same fused multi-aggregator pass forward, and ONE kernel backward (gnnops_edge_multi_grad: each
destination's edges walked twice, nothing saved from the forward) that writes the per-edge gradient of the message and d p;
d q is a segment sum over the source plan as above. `edge_reduce` itself keeps refusing a gradient for those forms.

Attention: `GATv2Conv` (the reference's model zoo, graph_benchmark/models/ptg_models.py:208-236) is one dense product and one
attention pass, `edge_attention` (csrc/attention.hip: online softmax per destination and head, trainable) — SURVEY.md §8(f) rank 1.
`GATConv` (the original GAT), `GATEConv` and the `AttentiveFP` model on them (the reference's AttentiveFPREG, ptg_models.py:91-120) run
on the second member of that family, `edge_attention_v1`: per-edge rows, a leaky ReLU on the row, attention dropout after the softmax.
Edge features: `GATv2Conv(edge_dim=)` adds u = lin_edge(edge_attr) to the score's pre-activation (`edge_attention(..., u=)`), `GATConv(edge_dim=)`
adds the scalar att_edge . lin_edge(edge_attr) per head from one product with the folded weight (`edge_attention_v1(..., edge_score=)`); both
are compile-time instances of the same two passes and train through them.
`TransformerConv` (scaled dot-product attention, PyG's layer of UniMP) runs on the third member, `edge_attention_dot`: the score is
qry[i] . k[j], the message a second gathered row v[j], per-edge rows add to both, attention dropout after the softmax.

The GATv2 MODEL (the reference's GATv2REG) is `GATv2`: per layer the product, the attention pass and ONE `head_act_norm` pass
(csrc/norm.hip: mean over heads + bias + ReLU + feature-dropout mask + LayerNorm, trainable), then gnnops.pool.global_mean_pool.

GraphUNet's layers (the reference's GraphUNetREG): `GCNConv` is one product and `gcn_propagate` (csrc/gcn.hip: symmetric normalisation
with edge weights, trainable), `TopKPooling` selects with `gnnops.pool.topk` / `filter_adj` (csrc/pool.hip), `GraphUNet` is the model.
"""
import ctypes

import torch

from . import _lib, ops
from ._lib import check
from .ops import _dtype_code, _hub_workspace, _on, _ptr, _require_gpu, _stream, get_plan
from .sparse import _coo_rows_cols, _csr_arrays

FUNCTORS = {"copy": 0, "add": 1, "cgconv": 2, "film": 3}
_PARTS = {"copy": (1, 0, 0), "add": (1, 1, 1), "cgconv": (2, 2, 2), "film": (1, 2, 0)}   # K-wide parts per row of q, p, w
AGGREGATORS = {"sum": 0, "add": 0, "mean": 1, "min": 2, "max": 3, "std": 4}
SCALERS = {"identity": 0, "amplification": 1, "attenuation": 2, "linear": 3, "inverse_linear": 4}


def _rows(t, what, parts, K, op="edge_reduce"):
    """A [rows, >= parts*K] operand whose rows are contiguous runs (column blocks of a wider matrix are fine)."""
    if t is None:
        return None, 0
    if t.dim() != 2 or (t.size(1) > 1 and t.stride(1) != 1) or t.size(1) < parts * K:
        raise RuntimeError(f"{op}: {what} must be 2-D with unit column stride and at least {parts * K} columns")
    return t, (t.stride(0) if t.size(0) > 1 else t.size(1))


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def edge_reduce(functor, q, edge_index, num_dst, p=None, w=None, add=None, aggr=("sum",), scalers=(), avg_deg=None, out=None,
                flip=False):
    """out[i] = [scaler_s(deg_i) * AGGR_a_{(j -> i) in edge_index} f(p[i], q[j], w[e])  for s in scalers for a in aggr].

    edge_index int64 [2, E] = (source j, destination i), PyG's flow="source_to_target" (``flip=True``: the transposed graph,
    row 0 = destinations — what the backward of a copy message runs). See include/gnnops.h (gnnops_edge_reduce) for the
    functors. ``out`` may be a column block of a wider buffer (what the layer would cat into). The destination plan
    (rowptr, perm) and the plan-ordered source ids are cached under the edge_index tensor. Differentiable in q, p, w and
    add for one sum / mean aggregator without scalers and ``out=None`` (copy / cgconv / film messages)."""
    if _wants_grad(q, p, w, add):
        if len(aggr) != 1 or aggr[0] not in ("sum", "add", "mean") or scalers or out is not None or flip or functor == "add":
            raise NotImplementedError("gnnops.conv.edge_reduce: an operand requires grad, but only one sum / mean aggregator "
                                      "without scalers of a copy / cgconv / film message has a backward (several aggregators, scalers or "
                                      "the add message: gnnops.conv.edge_aggregate)")
        return _EdgeReduce.apply(functor, "mean" if aggr[0] == "mean" else "sum", edge_index, num_dst, q, p, w, add)
    _require_gpu(q, edge_index, p, w, add, out)
    edge_index, src_rows, dst_rows = _coo_rows_cols(edge_index, "edge_reduce")
    if flip:
        src_rows, dst_rows = dst_rows, src_rows
    nq, np_, nw = _PARTS[functor]
    if q.dim() != 2 or q.size(1) % nq:
        raise RuntimeError(f"edge_reduce: q must be [rows, {nq} * K]")
    K = q.size(1) // nq
    dt = _dtype_code(q, "edge_reduce")
    for t in (p, w, add, out):
        if t is not None and t.dtype != q.dtype:
            raise RuntimeError("edge_reduce: operands must have the same dtype")
    if functor != "copy" and p is None:
        raise RuntimeError(f"edge_reduce: the {functor} message needs the per-destination rows p")
    q, ldq = _rows(q, "q", nq, K)
    p, ldp = _rows(p, "p", np_, K)
    w, ldw = _rows(w, "w", nw, K)
    add, ldadd = _rows(add, "add", 1, K)
    E = edge_index.size(1)
    if p is not None and p.size(0) != num_dst or add is not None and add.size(0) != num_dst:
        raise RuntimeError("edge_reduce: p and add have one row per destination")
    if w is not None and w.size(0) != E:
        raise RuntimeError("edge_reduce: w has one row per edge")
    aggr_ids = [AGGREGATORS[a] for a in aggr]
    scal_ids = [SCALERS[s] for s in scalers]
    width = max(len(scal_ids), 1) * len(aggr_ids) * K
    if out is None:
        out = torch.empty((num_dst, width), dtype=q.dtype, device=q.device)
    elif out.size(0) != num_dst:
        raise RuntimeError("edge_reduce: out has one row per destination")
    out, ldo = _rows(out, "out", 1, width)
    avg_log, avg_lin = (1.0, 1.0) if avg_deg is None else (float(avg_deg["log"]), float(avg_deg["lin"]))
    # plans are cached under the [2, E] tensor: tag 1 = plan of row 1 (destinations), tag 0 = plan of row 0 (the flipped graph)
    plan = get_plan(dst_rows, num_dst, owner=edge_index, tag=0 if flip else 1, companion=src_rows)   # small graphs: col comes with the plan
    if plan.col is not None or E == 0:
        col = plan.col if E else src_rows
    else:
        col, _ = _csr_arrays(plan, src_rows, None, owner=edge_index, tag=1 if flip else 0)
    c_aggr = (ctypes.c_int * len(aggr_ids))(*aggr_ids)
    c_scal = (ctypes.c_int * max(len(scal_ids), 1))(*scal_ids)
    L = _lib.load()
    # destinations with more than 8192 edges: reduced piecewise
    hub_ws, hub_ptr, hub_bytes = _hub_workspace(L.gnnops_edge_reduce_hub_workspace_bytes(E, K), q.device)
    with _on(q.device):
        rc = L.gnnops_edge_reduce_hubs(FUNCTORS[functor], _ptr(q), ldq, _ptr(p), ldp, _ptr(w), ldw, _ptr(add), ldadd,
                                       plan.rowptr.data_ptr(), plan.perm.data_ptr(), col.data_ptr(), out.data_ptr(), ldo,
                                       num_dst, E, K, c_aggr, len(aggr_ids), c_scal, len(scal_ids), avg_log, avg_lin, dt,
                                       hub_ptr, hub_bytes, _stream())
    check(rc, "edge_reduce")
    return out


class _EdgeReduce(torch.autograd.Function):
    """One sum / mean edge pass, differentiable in q [N_src, .], p [N_dst, .], w [E, .] and add [N_dst, K].

    backward, with g = grad_out (for mean: divided by max(deg, 1) per destination):
      copy    d q[j] = sum over the edges OUT of j of g[i]        = the same edge pass over the transposed graph
      cgconv  gz[e] = g[i] * d message / d z (gnnops_edge_grad), z = p[i] + q[j] + w[e]:
              d p = segment sum of gz by destination, d q = segment sum by source, d w = gz
      film    gp[e], gq[e] from the same kernel; d p = sum of gp by destination, d q = sum of gq by source
      d add = grad_out."""

    @staticmethod
    def forward(ctx, functor, aggr, edge_index, num_dst, q, p, w, add):
        out = edge_reduce(functor, q, edge_index, num_dst, p=p, w=w, add=add, aggr=(aggr,))
        ctx.functor, ctx.aggr, ctx.num_dst, ctx.n_src = functor, aggr, num_dst, q.size(0)
        ctx.has = (p is not None, w is not None, add is not None)
        ctx.save_for_backward(edge_index, q, *(t for t in (p, w) if t is not None))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        edge_index, q, *rest = ctx.saved_tensors
        has_p, has_w, has_add = ctx.has
        p = rest.pop(0) if has_p else None
        w = rest.pop(0) if has_w else None
        need_q, need_p, need_w, need_add = ctx.needs_input_grad[4:8]
        g = grad_out.contiguous()
        d_add = g if (has_add and need_add) else None
        index, src_rows, dst_rows = _coo_rows_cols(edge_index, "edge_reduce")
        E = index.size(1)
        plan_dst = get_plan(dst_rows, ctx.num_dst, owner=edge_index, tag=1, companion=src_rows)
        if ctx.aggr == "mean":
            # counted and divided in float32, rounded once: an fp16 degree above 65504 is inf (gradient 0), a bf16 one above 256 inexact
            deg = (plan_dst.rowptr[1:] - plan_dst.rowptr[:-1]).clamp(min=1).to(torch.float32)
            g = (g / deg.unsqueeze(1)).to(g.dtype)
        d_q = d_p = d_w = None
        K = g.size(1)
        if ctx.functor == "copy":
            if need_q:
                d_q = edge_reduce("copy", g, edge_index, ctx.n_src, flip=True)
            return None, None, None, None, d_q, None, None, d_add
        if E == 0:
            d_q = torch.zeros_like(q) if need_q else None
            d_p = torch.zeros_like(p) if need_p else None
            d_w = torch.zeros_like(w) if (has_w and need_w) else None
            return None, None, None, None, d_q, d_p, d_w, d_add
        q_, ldq = _rows(q, "q", _PARTS[ctx.functor][0], K)
        p_, ldp = _rows(p, "p", 2, K)
        w_, ldw = _rows(w, "w", 2, K) if has_w else (None, 0)
        g, ldg = _rows(g, "the output gradient", 1, K)     # one expanded row (out.sum().backward()) has stride 0
        gp = torch.empty((E, 2 * K), dtype=g.dtype, device=g.device)
        gq = torch.empty((E, K), dtype=g.dtype, device=g.device) if ctx.functor == "film" else None
        with _on(g.device):
            check(_lib.load().gnnops_edge_grad(FUNCTORS[ctx.functor], _ptr(p_), ldp, _ptr(q_), ldq, _ptr(w_), ldw, g.data_ptr(), ldg,
                                               src_rows.data_ptr(), dst_rows.data_ptr(), gp.data_ptr(), _ptr(gq), E, K,
                                               _dtype_code(g, "edge_grad"), _stream()), "edge_grad")
        if need_p:
            d_p = ops.scatter(gp, plan_dst, 0, None, None, "sum")
            if p.size(1) != 2 * K:       # p was a column block wider than its 2K parts (never the case for the layers here)
                d_p = torch.nn.functional.pad(d_p, (0, p.size(1) - 2 * K))
        if need_q:
            plan_src = get_plan(src_rows, ctx.n_src, owner=edge_index, tag=0)
            d_q = ops.scatter(gq if gq is not None else gp, plan_src, 0, None, None, "sum")
        if has_w and need_w:
            d_w = gp
        return None, None, None, None, d_q, d_p, d_w, d_add


def edge_aggregate(functor, q, edge_index, num_dst, p=None, w=None, aggr=("mean", "min", "max", "std"), scalers=(), avg_deg=None):
    """`edge_reduce` for the messages that are affine in their operands — "copy" (q[j]) and "add" (p[i] + q[j] (+ w[e])) — with any
    ordered subset of sum / mean / min / max / std and PNA's degree scalers, differentiable in q, p and w: PNAConv's edge pass in a
    training loop. The forward is the launch of `edge_reduce` (the same bits); the backward is one launch of
    gnnops_edge_multi_grad (csrc/conv.hip), which walks every destination's edges twice and saves nothing from the forward.
    min / max send their gradient to one edge per destination and column, the smallest edge id among those that attain the value
    (the arg rule of gnnops.scatter); std passes nothing where the variance is 0 (torch's relu)."""
    if functor not in ("copy", "add"):
        raise NotImplementedError(f"gnnops.conv.edge_aggregate: the {functor} message is not affine in its operands (copy / add)")
    if functor == "copy":
        p = w = None
    if _wants_grad(q, p, w):
        return _EdgeAggregate.apply(functor, tuple(aggr), tuple(scalers), avg_deg, edge_index, num_dst, q, p, w)
    return _aggregate_forward(functor, tuple(aggr), tuple(scalers), avg_deg, edge_index, num_dst, q, p, w)


def _aggregate_forward(functor, aggr, scalers, avg_deg, edge_index, num_dst, q, p, w):
    if num_dst == 0:
        return q.new_zeros((0, max(len(scalers), 1) * len(aggr) * q.size(1)))
    return edge_reduce(functor, q, edge_index, num_dst, p=p, w=w, aggr=aggr, scalers=scalers, avg_deg=avg_deg)


class _EdgeAggregate(torch.autograd.Function):
    """The multi-aggregator edge pass, differentiable in q [N_src, .], p [N_dst, .] and w [E, .]; saves its operands only.

    backward: gnnops_edge_multi_grad writes gm [E, K] = d message per edge, in edge order, and d p (its sums by destination);
    d w = gm, d q = the segment sum of gm over the plan of the source ids — as `_EdgeReduce` and `_EdgeAttention`."""

    @staticmethod
    def forward(ctx, functor, aggr, scalers, avg_deg, edge_index, num_dst, q, p, w):
        out = _aggregate_forward(functor, aggr, scalers, avg_deg, edge_index, num_dst, q, p, w)
        ctx.meta = (functor, aggr, scalers, avg_deg, num_dst)
        ctx.has = (p is not None, w is not None)
        ctx.save_for_backward(edge_index, q, *(t for t in (p, w) if t is not None))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        edge_index, q0, *rest = ctx.saved_tensors
        functor, aggr, scalers, avg_deg, num_dst = ctx.meta
        has_p, has_w = ctx.has
        p0 = rest.pop(0) if has_p else None
        w0 = rest.pop(0) if has_w else None
        need_q, need_p, need_w = ctx.needs_input_grad[6:9]
        index, src_rows, dst_rows = _coo_rows_cols(edge_index, "edge_aggregate")
        E, K = index.size(1), q0.size(1)
        zeros = lambda t, need: torch.zeros_like(t) if (t is not None and need) else None   # noqa: E731
        if E == 0 or num_dst == 0 or K == 0:
            return (None,) * 6 + (zeros(q0, need_q), zeros(p0, need_p), zeros(w0, need_w))
        q, ldq = _rows(q0, "q", 1, K, op="edge_aggregate")
        p, ldp = _rows(p0, "p", 1, K, op="edge_aggregate")
        w, ldw = _rows(w0, "w", 1, K, op="edge_aggregate")
        # autograd hands over whatever layout the consumer made (`_EdgeAttention.backward`): rows of unit column stride are read
        # in place (pitch 0 = one expanded row for all), anything else is copied
        g = grad_out if grad_out.stride(1) == 1 or grad_out.size(1) == 1 else grad_out.contiguous()
        g, ldg = _rows(g, "the output gradient", 1, g.size(1), op="edge_aggregate")
        if g.size(0) > 1 and g.stride(0) == 0:
            ldg = 0
        plan = get_plan(dst_rows, num_dst, owner=edge_index, tag=1, companion=src_rows)   # cached by the forward
        col = plan.col if plan.col is not None else _csr_arrays(plan, src_rows, None, owner=edge_index, tag=0)[0]
        gm = torch.empty((E, K), dtype=q.dtype, device=q.device)
        d_p = torch.empty((num_dst, K), dtype=q.dtype, device=q.device) if has_p else None
        aggr_ids = [AGGREGATORS[a] for a in aggr]
        scal_ids = [SCALERS[s] for s in scalers]
        c_aggr = (ctypes.c_int * len(aggr_ids))(*aggr_ids)
        c_scal = (ctypes.c_int * max(len(scal_ids), 1))(*scal_ids)
        avg_log, avg_lin = (1.0, 1.0) if avg_deg is None else (float(avg_deg["log"]), float(avg_deg["lin"]))
        with _on(q.device):
            check(_lib.load().gnnops_edge_multi_grad(FUNCTORS[functor], q.data_ptr(), ldq, _ptr(p), ldp, _ptr(w), ldw, g.data_ptr(), ldg,
                                                     plan.rowptr.data_ptr(), plan.perm.data_ptr(), col.data_ptr(), gm.data_ptr(),
                                                     _ptr(d_p), num_dst, E, K, c_aggr, len(aggr_ids), c_scal, len(scal_ids), avg_log,
                                                     avg_lin, _dtype_code(q, "edge_aggregate"), _stream()), "edge_multi_grad")
        pad = lambda d, t: d if t.size(1) == K else torch.nn.functional.pad(d, (0, t.size(1) - K))   # noqa: E731  (column blocks wider than K)
        d_q = None
        if need_q:
            plan_src = get_plan(src_rows, q0.size(0), owner=edge_index, tag=0)
            d_q = pad(ops.scatter(gm, plan_src, 0, None, None, "sum"), q0)
        d_p = pad(d_p, p0) if (has_p and need_p) else None
        d_w = pad(gm, w0) if (has_w and need_w) else None
        return (None,) * 6 + (d_q, d_p, d_w)


# ---- dense side: every weight block a layer applies per node, as ONE operand of the MFMA product ------------------------
class _Packed:
    """Weights of several nn.Linear maps packed for one product, rebuilt only when a parameter changes (identity + version
    counter of the parameters named in ``params``), so transposes and concatenation are paid once per set of weights.

    side by side (default): x @ [W_0^T | W_1^T | ...] — one input, several maps; bias = the concatenated bias rows
    stacked  (stack=True) : [h_0 | h_1 | ...] @ [W_0^T ; W_1^T ; ...] — several inputs summed into one output"""

    def __init__(self):
        self.key = self.weight = self.bias = self._alive = None

    def get(self, params, blocks, stack=False):
        """params: the Parameters the blocks are cut from; blocks: [(weight or a column slice of it [out, in], bias or None)], or a
        callable that returns that list."""
        # Module.to() / .half() swap a parameter's data without touching its version counter: the pointer and dtype are in the key
        # tensors created under torch.inference_mode() have no version counter: nothing derived from them is cached
        if _wants_grad(*params):     # training: the packed operand is part of the graph (cat / t are differentiable) and never cached
            return self._pack(blocks, stack)
        cacheable = all(ops._version_of(t) is not None for t in params if t is not None)
        key = tuple((id(t), t._version, t.data_ptr(), t.dtype) for t in params if t is not None) if cacheable else None
        if key is None or key != self.key:
            with torch.no_grad():
                self.weight, self.bias = self._pack(blocks, stack)
            self.key = key
            self._alive = list(params)   # the key holds ids: keep the tensors they name alive so that no id is handed out again
        return self.weight, self.bias

    @staticmethod
    def _pack(blocks, stack):
        if callable(blocks):     # blocks that cost weight-sized work to cut (a fold, a pad) are made only when the cache misses
            blocks = blocks()
        if stack:
            weight = torch.cat([wt.t() for wt, _ in blocks], dim=0).contiguous()
            biases = [b for _, b in blocks if b is not None]
            bias = sum(biases[1:], biases[0]).contiguous() if biases else None
        else:
            weight = torch.cat([wt.t() for wt, _ in blocks], dim=1).contiguous()
            if any(b is not None for _, b in blocks):
                bias = torch.cat([b if b is not None else wt.new_zeros(wt.size(0)) for wt, b in blocks]).contiguous()
            else:
                bias = None
        return weight, bias


def _dense(x, packed):
    """x [N, D_in] @ weight [D_in, W] (+ bias row) on the MFMA kernels (gemm.hip)."""
    from . import autograd

    weight, bias = packed
    return autograd.addmm(bias, x, weight) if bias is not None else autograd.matmul(x, weight)


def _linear(x, lin, cache):
    return _dense(x, cache.get([lin.weight, lin.bias], [(lin.weight, lin.bias)]))


def _pair(x):
    return x if isinstance(x, (tuple, list)) else (x, x)


class _Layer(torch.nn.Module):
    """Every layer is trainable (module docstring); `_freeze` / `_forward_only` remain for callers that want an inference-only copy."""

    def _freeze(self):
        self.requires_grad_(False)

    def _forward_only(self, *tensors):
        if torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters()) or
                                        any(t is not None and t.requires_grad for t in tensors)):
            raise RuntimeError(f"gnnops.conv.{type(self).__name__} is forward-only: freeze its parameters / call it under "
                               "torch.no_grad() (trainable: GINConv, SAGEConv, CGConv, FiLMConv)")


class GINConv(_Layer):
    """x'_i = nn((1 + eps) * x_i + sum_j x_j)  (torch_geometric GINConv; benchmark_convs.py:163 GINConv(Linear(11, 2048)))."""

    def __init__(self, nn, eps=0.0, train_eps=False):
        super().__init__()
        self.nn = nn
        self.initial_eps = eps
        if train_eps:
            self.eps = torch.nn.Parameter(torch.tensor([float(eps)]))
        else:
            self.register_buffer("eps", torch.tensor([float(eps)]))
        self._packed = _Packed()
        self._eps_key, self._eps_host = None, float(eps)

    def _eps_value(self):
        """eps as a host number, read back from the device only when the tensor changed (a read-back per forward would
        synchronise every call and cannot be captured into a graph)."""
        t = self.eps
        key = (ops._version_of(t), t.data_ptr())
        if key[0] is None or key != self._eps_key:
            self._eps_host = float(t)
            self._eps_key = key
        return self._eps_host

    def forward(self, x, edge_index, size=None):
        x_src, x_dst = _pair(x)
        n_dst = x_dst.size(0) if size is None else size[1]
        if _wants_grad(self.eps):       # train_eps: eps is part of the graph
            root = x_dst * (1.0 + self.eps)
        else:
            eps = self._eps_value()
            root = x_dst if eps == 0.0 else x_dst * (1.0 + eps)
        h = edge_reduce("copy", x_src.contiguous(), edge_index, n_dst, add=root.contiguous())
        return _linear(h, self.nn, self._packed) if isinstance(self.nn, torch.nn.Linear) else self.nn(h)


class SAGEConv(_Layer):
    """x'_i = W_l mean_j x_j + W_r x_i  (torch_geometric SAGEConv; benchmark_convs.py:231 SAGEConv(-1, 2048)).
    One edge pass writes the mean into the left block of [mean | x]; one product with [W_l^T ; W_r^T] finishes the layer."""

    def __init__(self, in_channels, out_channels, normalize=False, root_weight=True, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.normalize, self.root_weight, self._bias = normalize, root_weight, bias
        self.lin_l = self.lin_r = None
        if not (isinstance(in_channels, int) and in_channels < 0):
            self._build(*((in_channels, in_channels) if isinstance(in_channels, int) else in_channels))
        self._packed = _Packed()

    def _build(self, in_src, in_dst, like=None):
        kw = {} if like is None else {"device": like.device, "dtype": like.dtype}
        self.lin_l = torch.nn.Linear(in_src, self.out_channels, bias=self._bias, **kw)
        if self.root_weight:
            self.lin_r = torch.nn.Linear(in_dst, self.out_channels, bias=False, **kw)

    def forward(self, x, edge_index, size=None):
        x_src, x_dst = _pair(x)
        if self.lin_l is None:   # in_channels = -1: sized by the first input, like PyG's lazy Linear
            self._build(x_src.size(1), x_dst.size(1), like=x_src)
        n_dst = x_dst.size(0) if size is None else size[1]
        d_src = x_src.size(1)
        if self.root_weight:
            if _wants_grad(x_src, x_dst):     # in a graph the mean is a tensor of its own (the out= form has no backward)
                h = torch.cat([edge_reduce("copy", x_src.contiguous(), edge_index, n_dst, aggr=("mean",)), x_dst[:n_dst]], dim=1)
            else:
                h = torch.empty((n_dst, d_src + x_dst.size(1)), dtype=x_src.dtype, device=x_src.device)
                h[:, d_src:] = x_dst[:n_dst]
                edge_reduce("copy", x_src.contiguous(), edge_index, n_dst, aggr=("mean",), out=h[:, :d_src])
            packed = self._packed.get([self.lin_l.weight, self.lin_r.weight, self.lin_l.bias],
                                      [(self.lin_l.weight, self.lin_l.bias), (self.lin_r.weight, None)], stack=True)
        else:
            h = edge_reduce("copy", x_src.contiguous(), edge_index, n_dst, aggr=("mean",))
            packed = self._packed.get([self.lin_l.weight, self.lin_l.bias], [(self.lin_l.weight, self.lin_l.bias)])
        out = _dense(h, packed)
        return torch.nn.functional.normalize(out, p=2.0, dim=-1) if self.normalize else out


class CGConv(_Layer):
    """x'_i = x_i + sum_j sigmoid(z_ij W_f + b_f) * softplus(z_ij W_s + b_s),  z_ij = [x_i, x_j, e_ij]
    (app_bm/groq_script.py:15-111; forward :91-102, message :104-109)."""

    def __init__(self, channels, dim=0, aggr="add", batch_norm=False, bias=True):
        super().__init__()
        self.channels, self.dim, self.aggr, self.batch_norm = channels, dim, aggr, batch_norm
        self._ch = (channels, channels) if isinstance(channels, int) else tuple(channels)
        self.lin_f = torch.nn.Linear(sum(self._ch) + dim, self._ch[1], bias=bias)
        self.lin_s = torch.nn.Linear(sum(self._ch) + dim, self._ch[1], bias=bias)
        self.bn = torch.nn.BatchNorm1d(self._ch[1]) if batch_norm else None
        self._pk_both, self._pk_dst, self._pk_src, self._pk_edge = _Packed(), _Packed(), _Packed(), _Packed()

    def forward(self, x, edge_index, edge_attr=None):
        x_src, x_dst = _pair(x)
        c_src, c_dst = self._ch
        K = c_dst
        Wf, Ws, bf, bs = self.lin_f.weight, self.lin_s.weight, self.lin_f.bias, self.lin_s.bias
        params = [Wf, Ws, bf, bs]
        # the weight columns follow cat([x_i, x_j, e]) (groq_script.py:105-108)
        dst_blocks = [(Wf[:, :c_dst], bf), (Ws[:, :c_dst], bs)]                                # -> p = [f | s], biases included
        src_blocks = [(Wf[:, c_dst:c_dst + c_src], None), (Ws[:, c_dst:c_dst + c_src], None)]  # -> q = [f | s]
        n_dst = x_dst.size(0)
        if x_src is x_dst:   # one product for both sides: [p | q] = x @ [W_f,i | W_s,i | W_f,j | W_s,j]
            pq = _dense(x_dst.contiguous(), self._pk_both.get(params, dst_blocks + src_blocks))   # its own cache: 4K columns, not 2K
            p, q = pq[:, :2 * K], pq[:, 2 * K:]
        else:
            p = _dense(x_dst.contiguous(), self._pk_dst.get(params, dst_blocks))
            q = _dense(x_src.contiguous(), self._pk_src.get(params, src_blocks))
        w = None
        if edge_attr is not None:
            if edge_attr.dim() == 1:
                edge_attr = edge_attr.unsqueeze(-1)
            w = _dense(edge_attr.contiguous(), self._pk_edge.get(params, [(Wf[:, c_dst + c_src:], None), (Ws[:, c_dst + c_src:], None)]))
        aggr = "sum" if self.aggr == "add" else self.aggr
        if self.bn is None:
            return edge_reduce("cgconv", q, edge_index, n_dst, p=p, w=w, add=x_dst.contiguous(), aggr=(aggr,))
        out = self.bn(edge_reduce("cgconv", q, edge_index, n_dst, p=p, w=w, aggr=(aggr,)))
        out += x_dst
        return out


class FiLMConv(_Layer):
    """x'_i = sum_r mean_{j in N_r(i)} relu(gamma_r,i * W_r x_j + beta_r,i) + relu(gamma_s,i * W_s x_i + beta_s,i)
    (torch_geometric FiLMConv, aggr="mean", act=ReLU; benchmark_convs.py:146 FiLMConv(in_channels=11, out_channels=2048)).
    One product gives [beta_s | gamma_s | W_s x | (beta_r | gamma_r | W_r x) for every relation] per node."""

    def __init__(self, in_channels, out_channels, num_relations=1, nn=None, act=torch.nn.ReLU(), aggr="mean"):
        super().__init__()
        if nn is not None:
            raise NotImplementedError("gnnops.conv.FiLMConv: a custom film network is not fused; pass nn=None")
        if not isinstance(act, torch.nn.ReLU):
            raise NotImplementedError("gnnops.conv.FiLMConv: act must be ReLU (the edge pass applies it)")
        if isinstance(in_channels, (tuple, list)):
            raise NotImplementedError("gnnops.conv.FiLMConv: bipartite input")
        self.in_channels, self.out_channels, self.num_relations = in_channels, out_channels, max(num_relations, 1)
        self.act, self.aggr = act, aggr
        R = self.num_relations
        self.lins = torch.nn.ModuleList([torch.nn.Linear(in_channels, out_channels, bias=False) for _ in range(R)])
        self.films = torch.nn.ModuleList([torch.nn.Linear(in_channels, 2 * out_channels) for _ in range(R)])
        self.lin_skip = torch.nn.Linear(in_channels, out_channels, bias=False)
        self.film_skip = torch.nn.Linear(in_channels, 2 * out_channels, bias=False)
        self._packed = _Packed()

    def forward(self, x, edge_index, edge_type=None):
        if isinstance(x, (tuple, list)):
            raise NotImplementedError("gnnops.conv.FiLMConv: bipartite input")
        o, R = self.out_channels, self.num_relations
        blocks = [(self.film_skip.weight, None), (self.lin_skip.weight, None)]
        for r in range(R):
            blocks += [(self.films[r].weight, self.films[r].bias), (self.lins[r].weight, None)]
        y = _dense(x.contiguous(), self._packed.get(list(self.parameters()), blocks))   # [N, 3 o (1 + R)]
        beta_s, gamma_s, xs = y[:, :o], y[:, o:2 * o], y[:, 2 * o:3 * o]
        out = torch.relu_(gamma_s * xs + beta_s)
        aggr = "sum" if self.aggr == "add" else self.aggr
        n = x.size(0)
        for r in range(R):
            base = 3 * o * (1 + r)     # film(x) = [beta | gamma] (FiLMConv.forward: .split(out_channels, dim=-1)), then W_r x
            ei = edge_index if R == 1 else edge_index[:, edge_type == r].contiguous()
            out = edge_reduce("film", y[:, base + 2 * o:base + 3 * o], ei, n, p=y[:, base:base + 2 * o], add=out, aggr=(aggr,))
        return out


class PNAConv(_Layer):
    """Principal neighbourhood aggregation (torch_geometric PNAConv; benchmark_convs.py:197-206: in 1, out 2048,
    aggregators mean/min/max/std, scalers identity/amplification/attenuation, deg = in-degree histogram).
    message = pre_nn([x_i, x_j (, enc(e))]) with ONE pre-layer is p_i + q_j (+ w_e); the aggregators and scalers come out of
    one edge pass, written next to x into the [N, (1 + A S) F] operand of the post layer (inference; when a gradient is needed
    the same route runs on `edge_aggregate` and a cat). pre_layers > 1: the first layer is
    still split per node, the rest of the MLP runs on per-edge rows (see forward); post_layers > 1: more node-row products."""

    def __init__(self, in_channels, out_channels, aggregators, scalers, deg, edge_dim=None, towers=1, pre_layers=1,
                 post_layers=1, divide_input=False):
        super().__init__()
        if pre_layers < 1 or post_layers < 1:
            raise ValueError("PNAConv: pre_layers and post_layers must be >= 1")
        self.pre_layers, self.post_layers = pre_layers, post_layers
        if divide_input and in_channels % towers or out_channels % towers:
            raise ValueError("PNAConv: channels must divide by towers")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.aggregators, self.scalers = list(aggregators), list(scalers)
        self.edge_dim, self.towers, self.divide_input = edge_dim, towers, divide_input
        self.F_in = in_channels // towers if divide_input else in_channels
        self.F_out = out_channels // towers
        deg = deg.to(torch.float)
        total = deg.sum()
        bins = torch.arange(deg.numel(), dtype=torch.float)
        self.avg_deg = {"lin": float((bins * deg).sum() / total), "log": float(((bins + 1).log() * deg).sum() / total),
                        "exp": float((bins.exp() * deg).sum() / total)}
        F = self.F_in
        if edge_dim is not None:
            self.edge_encoder = torch.nn.Linear(edge_dim, F)
        def mlp(first_in, width_out, layers):   # PyG's PNAConv: Linear, then (ReLU, Linear) per extra layer
            mods = [torch.nn.Linear(first_in, width_out)]
            for _ in range(layers - 1):
                mods += [torch.nn.ReLU(), torch.nn.Linear(width_out, width_out)]
            return torch.nn.Sequential(*mods)

        self.pre_nns = torch.nn.ModuleList([mlp((3 if edge_dim else 2) * F, F, pre_layers) for _ in range(towers)])
        width = (len(self.aggregators) * len(self.scalers) + 1) * F
        self.post_nns = torch.nn.ModuleList([mlp(width, self.F_out, post_layers) for _ in range(towers)])
        self.lin = torch.nn.Linear(out_channels, out_channels)
        self._pk = {}

    def _cache(self, name):
        if name not in self._pk:
            self._pk[name] = _Packed()
        return self._pk[name]

    def forward(self, x, edge_index, edge_attr=None):
        if self.edge_dim is not None and edge_attr is None:
            raise RuntimeError("PNAConv: edge_attr is required when edge_dim is set")
        # in a graph that needs gradients the same route on the differentiable front ends: `edge_aggregate` for the edge pass, a
        # cat for the post layer's operand (an out= view has no backward), out-of-place ReLU
        train = _wants_grad(x, edge_attr, *self.parameters())
        relu = torch.relu if train else torch.relu_
        F, T = self.F_in, self.towers
        n = x.size(0)
        xt = x.view(n, T, F) if self.divide_input else x.view(n, 1, F).expand(n, T, F)
        A, S = len(self.aggregators), len(self.scalers)
        e = None
        if self.edge_dim is not None:
            e = _linear(edge_attr.contiguous(), self.edge_encoder, self._cache("enc"))
        outs = []
        for t in range(T):
            pre, post = self.pre_nns[t][0], self.post_nns[t][0]
            xin = xt[:, t].contiguous()
            Wp = pre.weight                                              # [F, 2F or 3F]: columns follow cat([x_i, x_j, e])
            pq = _dense(xin, self._cache(f"pre{t}").get([Wp, pre.bias], [(Wp[:, :F], pre.bias), (Wp[:, F:2 * F], None)]))
            w = _dense(e, self._cache(f"edge{t}").get([Wp], [(Wp[:, 2 * F:], None)])) if e is not None else None
            if train:
                reduce, h = edge_aggregate, None
            else:
                h = torch.empty((n, (1 + A * S) * F), dtype=x.dtype, device=x.device)
                h[:, :F] = xin
                reduce = lambda *a, **kw: edge_reduce(*a, out=h[:, F:], **kw)   # noqa: E731
            if self.pre_layers == 1:
                agg = reduce("add", pq[:, F:], edge_index, n, p=pq[:, :F], w=w, aggr=self.aggregators, scalers=self.scalers,
                             avg_deg=self.avg_deg)
            else:
                # a deeper pre-MLP is not linear in [x_i, x_j]: only its FIRST layer leaves the edge loop (the split product
                # above); its output is materialised per edge, the remaining (ReLU, Linear) pairs run as [E, F] products, and
                # the aggregators take the finished messages as "copy" rows of a graph whose sources are the edges themselves
                from . import autograd as ad

                select = ad.index_select if train else ops.index_select
                src_rows, dst_rows = edge_index[0].contiguous(), edge_index[1].contiguous()
                m = select(pq[:, :F].contiguous(), 0, dst_rows) + select(pq[:, F:].contiguous(), 0, src_rows)
                if w is not None:
                    m = m + w
                for li in range(1, self.pre_layers):
                    m = _linear(relu(m), self.pre_nns[t][2 * li], self._cache(f"pre{t}.{li}"))
                per_edge = torch.stack([torch.arange(m.size(0), device=m.device), dst_rows])
                agg = reduce("copy", m, per_edge, n, aggr=self.aggregators, scalers=self.scalers, avg_deg=self.avg_deg)
            if train:
                h = torch.cat([xin, agg], dim=1)
            o = _linear(h, post, self._cache(f"post{t}"))
            for li in range(1, self.post_layers):
                o = _linear(relu(o), self.post_nns[t][2 * li], self._cache(f"post{t}.{li}"))
            outs.append(o)
        out = outs[0] if T == 1 else torch.cat(outs, dim=1)
        return _linear(out, self.lin, self._cache("lin"))


class SplineConv(_Layer):
    """x'_i = 1/|N(i)| sum_j x_j . h(e_ij) + x_i . root + bias, h = the B-spline kernel over the K = kernel_size^dim table
    ``weight`` [K, in, out] (SplineCNN, Fey et al. 2018; torch_geometric SplineConv). Not one of the reference's five layers: it is
    the trainable front end of torch_spline_conv.spline_conv (gnnops/spatial.py) — one fused forward kernel, backward in
    gnnops.autograd._SplineConv. ``aggr`` "mean" divides by the in-degree (norm=True), "add" does not.

    ``edge_index`` follows PyG's source_to_target flow: row 0 holds the sources, messages are summed at ``edge_index[1]``.
    spline_conv sums at row 0 of ITS index, so the layer hands it the flipped index; the flipped copy is kept per edge_index
    object, which keeps the edge plans cached across steps. torch_geometric is not available to compare against: the parameter
    names ``weight``, ``root``, ``bias`` and the uniform initialisation are this package's choice (name parity unpinned)."""

    def __init__(self, in_channels, out_channels, dim, kernel_size, is_open_spline=True, degree=1, aggr="mean", root_weight=True,
                 bias=True):
        super().__init__()
        if aggr not in ("mean", "add", "sum"):
            raise ValueError("SplineConv: aggr must be 'mean' or 'add'")
        as_list = lambda v: [v] * dim if isinstance(v, (int, bool)) else list(v)   # noqa: E731
        ks, op = as_list(kernel_size), as_list(is_open_spline)
        if len(ks) != dim or len(op) != dim:
            raise ValueError("SplineConv: kernel_size and is_open_spline need one entry per dimension")
        self.in_channels, self.out_channels, self.dim, self.degree, self.aggr = in_channels, out_channels, dim, degree, aggr
        self.register_buffer("kernel_size", torch.tensor(ks, dtype=torch.int64), persistent=False)
        self.register_buffer("is_open_spline", torch.tensor([1 if o else 0 for o in op], dtype=torch.uint8), persistent=False)
        K = 1
        for k in ks:
            K *= k
        bound = 1.0 / float(in_channels * (degree + 1) ** dim) ** 0.5
        self.weight = torch.nn.Parameter(torch.empty(K, in_channels, out_channels).uniform_(-bound, bound))
        rb = 1.0 / float(in_channels) ** 0.5
        self.root = torch.nn.Parameter(torch.empty(in_channels, out_channels).uniform_(-rb, rb)) if root_weight else None
        self.bias = torch.nn.Parameter(torch.zeros(out_channels)) if bias else None
        self._flipped = None   # (weakref to edge_index, its version, flipped copy)

    def _flip(self, edge_index):
        import weakref

        hit = self._flipped
        if hit is not None and hit[0]() is edge_index and hit[1] == edge_index._version:
            return hit[2]
        flipped = edge_index.flip(0).contiguous()
        if not edge_index.is_inference():
            self._flipped = (weakref.ref(edge_index), edge_index._version, flipped)
        return flipped

    def forward(self, x, edge_index, edge_attr):
        from .spatial import spline_conv

        return spline_conv(x, self._flip(edge_index), edge_attr, self.weight, self.kernel_size, self.is_open_spline, self.degree,
                           self.aggr == "mean", self.root, self.bias)


# ---- attention: GATv2 (csrc/attention.hip) ---------------------------------------------------------------------------------
def _attention_prepare(op, q, att, edge_index, num_dst, heads, dst, per_edge):
    """What both attention passes do with their operands before a launch. dst = (tensor, name, width, what it has): the operand with
    one row per destination; per_edge = [(tensor or None, name, width)]: the operands with one row per edge, in the order of
    edge_index; a width is "heads * channels" or "heads". Returns (q, ldq, dst, ld_dst, att [H * C], the per-edge operands made
    contiguous, edge_index, src_rows, the destination plan, col = the source row of each sorted position, E, H * C)."""
    HC = att.numel()
    if heads < 1 or HC == 0 or HC % heads:
        raise RuntimeError(f"{op}: heads = {heads} does not divide the row width {HC} (att has one entry per head and channel)")
    widths = {"heads * channels": HC, "heads": heads}
    t_dst, name, width, has = dst
    if any(t is not None and t.dtype != q.dtype for t in (t_dst, att, *(t for t, _, _ in per_edge))):
        raise RuntimeError(f"{op}: operands must have the same dtype")
    q, ldq = _rows(q, "q", 1, HC, op=op)
    t_dst, ld_dst = _rows(t_dst, name, 1, widths[width], op=op)
    if t_dst.size(0) != num_dst:
        raise RuntimeError(f"{op}: {name} has {has}")
    if q.size(0) >= 2 ** 31:
        raise NotImplementedError(f"{op}: 2^31 or more source rows")
    edge_index, src_rows, dst_rows = _coo_rows_cols(edge_index, op)
    E = edge_index.size(1)
    rows = []
    for t, name, width in per_edge:
        if t is not None:
            if t.dim() != 2 or tuple(t.shape) != (E, widths[width]):
                raise RuntimeError(f"{op}: {name} must be [E, {width}] = [{E}, {widths[width]}], in the order of edge_index")
            t = t.contiguous()
        rows.append(t)
    plan = get_plan(dst_rows, num_dst, owner=edge_index, tag=1, companion=src_rows)   # the plans of edge_reduce: nothing new on a warm call
    if plan.col is not None or E == 0:
        col = plan.col if E else src_rows
    else:
        col, _ = _csr_arrays(plan, src_rows, None, owner=edge_index, tag=0)
    return q, ldq, t_dst, ld_dst, att.contiguous().view(-1), rows, edge_index, src_rows, plan, col, E, HC


def _grad_rows(grad_out, HC, op):
    """(g, ldg) for the kernels. autograd hands over whatever layout the consumer made: out.sum() an expanded scalar (strides 0, 0),
    W @ out.t() a transposed one. Rows of unit column stride are read in place (pitch 0 = one row for all); anything else is copied."""
    g = grad_out if grad_out.dim() == 2 and (grad_out.stride(1) == 1 or grad_out.size(1) == 1) else grad_out.contiguous()
    g, ldg = _rows(g, "the output gradient", 1, HC, op=op)
    if g.size(0) > 1 and g.stride(0) == 0:
        ldg = 0
    return g, ldg


def _attention_tail(gq, d_dst, src_rows, edge_index, q0, dst0, need_q, need_dst):
    """(d q, d of the per-destination operand) as autograd wants them: d q = the segment sum of gq over the plan of the source ids,
    and either one padded with zero columns where the operand was a column block wider than what the pass reads."""
    d_q = None
    if need_q:
        plan_src = get_plan(src_rows, q0.size(0), owner=edge_index, tag=0)
        d_q = ops.scatter(gq, plan_src, 0, None, None, "sum")
        if q0.size(1) != gq.size(1):
            d_q = torch.nn.functional.pad(d_q, (0, q0.size(1) - gq.size(1)))
    if need_dst and dst0.size(1) != d_dst.size(1):
        d_dst = torch.nn.functional.pad(d_dst, (0, dst0.size(1) - d_dst.size(1)))
    return d_q, (d_dst if need_dst else None)


def _attention_operands(q, p, att, edge_index, num_dst, heads, u=None):
    _require_gpu(q, p, att, edge_index, u)
    if u is not None and u.device != q.device:
        raise RuntimeError("edge_attention: u must be on the device of q")
    q, ldq, p, ldp, att, (u,), edge_index, src_rows, plan, col, E, HC = _attention_prepare(
        "edge_attention", q, att, edge_index, num_dst, heads, (p, "p", "heads * channels", "one row per destination"),
        [(u, "u", "heads * channels")])
    return q, ldq, p, ldp, att, u, edge_index, src_rows, plan, col, E, HC


def _attention_forward(q, p, att, edge_index, num_dst, heads, negative_slope, u=None, identity_perm=False):
    """(out [num_dst, H * C], lse fp32 [num_dst, H]) of one launch of gnnops_edge_attention.
    identity_perm: the caller knows the edge list to be sorted by destination already, and u is read without the plan's perm."""
    q, ldq, p, ldp, att, u, edge_index, _, plan, col, E, HC = _attention_operands(q, p, att, edge_index, num_dst, heads, u)
    out = torch.empty((num_dst, HC), dtype=q.dtype, device=q.device)
    lse = torch.empty((num_dst, heads), dtype=torch.float32, device=q.device)
    perm = None if identity_perm or u is None else plan.perm.data_ptr()   # only u is read through it
    with _on(q.device):
        check(_lib.load().gnnops_edge_attention(q.data_ptr(), ldq, p.data_ptr(), ldp, att.data_ptr(), _ptr(u), plan.rowptr.data_ptr(), perm,
                                                col.data_ptr(), out.data_ptr(), HC, lse.data_ptr(), num_dst, E, heads, HC // heads,
                                                float(negative_slope), _dtype_code(q, "edge_attention"), _stream()), "edge_attention")
    return out, lse


def _attention_backward(q0, p0, att0, u0, edge_index, out, lse, grad_out, num_dst, heads, slope, identity_perm=False):
    """(gq [E, H * C] or None, d p [num_dst, H * C], d att [H * C], d u [E, H * C] or None, src_rows, edge_index) of one launch of
    gnnops_edge_attention_backward; None where there is no edge."""
    q, ldq, p, ldp, att, u, edge_index, src_rows, plan, col, E, HC = _attention_operands(q0, p0, att0, edge_index, num_dst, heads, u0)
    if E == 0 or num_dst == 0:
        return None, None, None, None, src_rows, edge_index
    g, ldg = _grad_rows(grad_out, HC, "edge_attention")
    d_p = torch.empty((num_dst, HC), dtype=q.dtype, device=q.device)
    gq = torch.empty((E, HC), dtype=q.dtype, device=q.device)
    d_att = torch.empty(HC, dtype=q.dtype, device=q.device)
    d_u = None if u is None else torch.empty((E, HC), dtype=q.dtype, device=q.device)
    L = _lib.load()
    perm = None if identity_perm else plan.perm.data_ptr()
    with _on(q.device):
        ws_bytes = L.gnnops_edge_attention_backward_workspace_bytes(num_dst, heads, HC // heads)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device)
        check(L.gnnops_edge_attention_backward(q.data_ptr(), ldq, p.data_ptr(), ldp, att.data_ptr(), _ptr(u), out.data_ptr(), HC,
                                               lse.data_ptr(), g.data_ptr(), ldg, plan.rowptr.data_ptr(), perm, col.data_ptr(),
                                               d_p.data_ptr(), gq.data_ptr(), _ptr(d_u), d_att.data_ptr(), num_dst, E, heads, HC // heads,
                                               slope, _dtype_code(q, "edge_attention"), ws.data_ptr(), ws_bytes, _stream()),
              "edge_attention_backward")
    return gq, d_p, d_att, d_u, src_rows, edge_index


def edge_attention(q, p, att, edge_index, num_dst, heads, negative_slope=0.2, u=None):
    """out[i, h, :] = sum over the edges (j -> i) of softmax_e(s[e, h]) * q[j, h, :],  s[e, h] = att[h] . leaky_relu(p[i, h] + q[j, h] + u[e, h])
    — GATv2's message and aggregation in one pass with an online softmax (csrc/attention.hip). q [N_src, H * C] and p [num_dst, H * C]
    may be column blocks of one product; att holds H * C entries (any shape); edge_index int64 [2, E] = (source, destination); u, when
    given, is [E, H * C] in the order of edge_index (GATv2Conv's lin_edge(edge_attr)) and enters the score only, never the message. A
    destination without edges gets a zero row. Differentiable in q, p, att and u."""
    if _wants_grad(q, p, att, u):
        return _EdgeAttention.apply(q, p, att, u, edge_index, num_dst, heads, float(negative_slope))
    return _attention_forward(q, p, att, edge_index, num_dst, heads, negative_slope, u)[0]


class _EdgeAttention(torch.autograd.Function):
    """backward (gnnops_edge_attention_backward, destination-ordered like the forward): d p and d att from the kernel, and one
    per-edge tensor gq [E, H * C] in edge order whose segment sum over the plan of the source ids is d q — as `_EdgeReduce`. With u
    a second per-edge tensor in edge order is d u."""

    @staticmethod
    def forward(ctx, q, p, att, u, edge_index, num_dst, heads, negative_slope):
        out, lse = _attention_forward(q, p, att, edge_index, num_dst, heads, negative_slope, u)
        ctx.meta = (num_dst, heads, negative_slope, u is not None)
        ctx.save_for_backward(q, p, att, edge_index, out, lse, *(() if u is None else (u,)))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q0, p0, att0, edge_index, out, lse, *rest = ctx.saved_tensors
        num_dst, heads, slope, has_u = ctx.meta
        u0 = rest[0] if has_u else None
        need_q, need_p, need_att, need_u = ctx.needs_input_grad[:4]
        gq, d_p, d_att, d_u, src_rows, edge_index = _attention_backward(q0, p0, att0, u0, edge_index, out, lse, grad_out, num_dst, heads, slope)
        if gq is None:
            return (torch.zeros_like(q0) if need_q else None, torch.zeros_like(p0) if need_p else None,
                    torch.zeros_like(att0) if need_att else None, torch.zeros_like(u0) if has_u and need_u else None, None, None, None, None)
        d_q, d_p = _attention_tail(gq, d_p, src_rows, edge_index, q0, p0, need_q, need_p)
        return (d_q, d_p, (d_att.view(att0.shape) if need_att else None), (d_u if has_u and need_u else None), None, None, None, None)


def _checked_fill_value(fill_value, who):
    """The attribute of an added self loop (PyG's add_self_loops): "mean", or a constant."""
    if isinstance(fill_value, str):
        if fill_value != "mean":
            raise ValueError(f"{who}: fill_value must be 'mean' or a number, got {fill_value!r}")
        return fill_value
    if isinstance(fill_value, bool) or not isinstance(fill_value, (int, float)):
        raise ValueError(f"{who}: fill_value must be 'mean' or a number, got {fill_value!r}")
    return float(fill_value)


class GATv2Conv(_Layer):
    """x'_i = sum_j alpha_ij W_l x_j (+ bias),  alpha_ij = softmax_j(att . leaky_relu(W_l x_j + W_r x_i))  per head
    (torch_geometric 2.0.2 GATv2Conv, Brody et al. 2021; the reference's GATv2REG, graph_benchmark/models/ptg_models.py:208-236,
    calls GATv2Conv(in, hidden, heads=heads, concat=False)). One product x @ [W_l^T | W_r^T] (one block when the weights are
    shared), one attention pass (`edge_attention`), then the mean over heads (concat=False) and the bias. Parameter names and shapes
    follow PyG so a state_dict moves across; torch_geometric is not available to compare against: parity unpinned. Self loops:
    existing ones are removed, then one is added per node, and the augmented index is kept per edge_index object so that its
    plans stay cached. Attention dropout is not implemented (the reference uses the default 0).
    Edge features (edge_dim set): alpha_ij = softmax_j(att . leaky_relu(W_l x_j + W_r x_i + W_e e_ij)), lin_edge without a bias as in
    PyG; u = edge_attr @ W_e^T is one more product, read by the same attention pass (the message stays W_l x_j). The self loops'
    attributes follow PyG's add_self_loops: fill_value "mean" = the mean of the attributes of a node's remaining in-edges (this
    package's scatter; a zero row for a node without any), or a constant; they are rebuilt per call, differentiable in edge_attr."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True,
                 bias=True, share_weights=False, edge_dim=None, fill_value="mean"):
        super().__init__()
        self.in_channels, self.out_channels, self.heads, self.concat = in_channels, out_channels, heads, concat
        self.negative_slope, self.dropout, self.add_self_loops, self.share_weights = negative_slope, dropout, add_self_loops, share_weights
        self.edge_dim, self.fill_value = edge_dim, _checked_fill_value(fill_value, "GATv2Conv")
        in_l, in_r = (in_channels, in_channels) if isinstance(in_channels, int) else in_channels
        self.lin_l = torch.nn.Linear(in_l, heads * out_channels, bias=bias)
        self.lin_r = self.lin_l if share_weights else torch.nn.Linear(in_r, heads * out_channels, bias=bias)
        self.att = torch.nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = torch.nn.Parameter(torch.zeros(heads * out_channels if concat else out_channels)) if bias else None
        for w in (self.lin_l.weight, self.lin_r.weight, self.att):      # glorot, as PyG
            torch.nn.init.xavier_uniform_(w)
        for lin in (self.lin_l, self.lin_r):
            if lin.bias is not None:
                torch.nn.init.zeros_(lin.bias)
        if edge_dim is not None:       # present only with edge features, so that a state_dict without them keeps PyG's keys
            self.lin_edge = torch.nn.Linear(edge_dim, heads * out_channels, bias=False)
            torch.nn.init.xavier_uniform_(self.lin_edge.weight)
        self._pk_both, self._pk_l, self._pk_r, self._pk_e = _Packed(), _Packed(), _Packed(), _Packed()
        self._looped = None   # (weakref to edge_index, its version, number of nodes, augmented copy)
        self._kept = None     # (weakref to edge_index, its version, positions of the edges that are no self loops)

    def _with_self_loops(self, edge_index, n):
        import weakref

        cacheable = ops._plan_cache_enabled and ops._version_of(edge_index) is not None
        hit = self._looped if cacheable else None
        if hit is not None and hit[0]() is edge_index and hit[1] == ops._version_of(edge_index) and hit[2] == n:
            return hit[3]
        keep = edge_index[0] != edge_index[1]
        loops = torch.arange(n, dtype=edge_index.dtype, device=edge_index.device)
        looped = torch.cat([edge_index[:, keep], torch.stack([loops, loops])], dim=1).contiguous()
        self._looped = (weakref.ref(edge_index), edge_index._version, n, looped) if cacheable else None
        return looped

    def _kept_edges(self, edge_index):
        """Positions in edge_index of the edges `_with_self_loops` keeps, in their order; kept per edge_index object like the
        augmented index, so that a warm call reads nothing back from the device."""
        import weakref

        cacheable = ops._plan_cache_enabled and ops._version_of(edge_index) is not None
        hit = self._kept if cacheable else None
        if hit is not None and hit[0]() is edge_index and hit[1] == ops._version_of(edge_index):
            return hit[2]
        kept = (edge_index[0] != edge_index[1]).nonzero().view(-1)
        self._kept = (weakref.ref(edge_index), edge_index._version, kept) if cacheable else None
        return kept

    def _edge_rows(self, edge_attr, edge_index, n_dst, looped):
        """edge_attr [E, edge_dim] checked against the layer and the edge list, and — with self loops — carried over to the
        augmented list of `_with_self_loops`: the kept edges' rows in their order, then one row per node (fill_value)."""
        who = type(self).__name__
        if self.edge_dim is None:
            if edge_attr is not None:
                raise RuntimeError(f"{who}: edge_attr given, but the layer was built without edge_dim")
            return None
        if edge_attr is None:
            raise RuntimeError(f"{who}: the layer was built with edge_dim = {self.edge_dim} and needs edge_attr")
        if edge_attr.dim() == 1:
            edge_attr = edge_attr.view(-1, 1)
        if edge_attr.dim() != 2 or edge_attr.size(0) != edge_index.size(1) or edge_attr.size(1) != self.edge_dim:
            raise RuntimeError(f"{who}: edge_attr must be [E, edge_dim] = [{edge_index.size(1)}, {self.edge_dim}], got {tuple(edge_attr.shape)}")
        _require_gpu(edge_attr)
        if not looped:
            return edge_attr.contiguous()
        from . import autograd

        kept = self._kept_edges(edge_index)
        rows = autograd.index_select(edge_attr.contiguous(), 0, kept)
        if self.fill_value == "mean":      # of the in-edges that remain; a node without any gets a zero row
            loops = autograd.scatter(rows, edge_index[1].index_select(0, kept), 0, None, n_dst, "mean")
        else:
            loops = rows.new_full((n_dst, self.edge_dim), self.fill_value)
        return torch.cat([rows, loops], dim=0)

    def _attend(self, x, edge_index, size=None, edge_attr=None):
        """The attention output [n_dst, H * C] before the head mean / bias of `forward` (`GATv2` fuses those into `head_act_norm`)."""
        if self.dropout > 0.0 and self.training:
            raise NotImplementedError("gnnops.conv.GATv2Conv: attention dropout is not implemented in the fused pass; construct the "
                                      "layer with dropout=0.0 (the reference's default) or call it in eval mode")
        H, C = self.heads, self.out_channels
        HC = H * C
        ll, lr = self.lin_l, self.lin_r
        if isinstance(x, (tuple, list)):
            if self.add_self_loops:
                raise RuntimeError("GATv2Conv: a bipartite pair needs add_self_loops=False")
            x_src, x_dst = x
            q = _dense(x_src.contiguous(), self._pk_l.get([ll.weight, ll.bias], [(ll.weight, ll.bias)]))
            p = _dense(x_dst.contiguous(), self._pk_r.get([lr.weight, lr.bias], [(lr.weight, lr.bias)]))
            n_dst = x_dst.size(0) if size is None else size[1]
            rows = self._edge_rows(edge_attr, edge_index, n_dst, False)
        else:
            n_dst = x.size(0)
            if self.share_weights:
                q = p = _dense(x.contiguous(), self._pk_l.get([ll.weight, ll.bias], [(ll.weight, ll.bias)]))
            else:       # [q | p] = x @ [W_l^T | W_r^T]: the two projections reach the kernel as column blocks
                qp = _dense(x.contiguous(), self._pk_both.get([ll.weight, lr.weight, ll.bias, lr.bias], [(ll.weight, ll.bias), (lr.weight, lr.bias)]))
                q, p = qp[:, :HC], qp[:, HC:]
            rows = self._edge_rows(edge_attr, edge_index, n_dst, self.add_self_loops)
            if self.add_self_loops:
                edge_index = self._with_self_loops(edge_index, n_dst)
        u = None
        if rows is not None:            # u = lin_edge(edge_attr) of the augmented list: one product
            we = self.lin_edge.weight
            u = _edge_dense(rows, self._pk_e.get([we], [(we, None)]))
        return edge_attention(q, p, self.att, edge_index, n_dst, H, self.negative_slope, u=u)

    def forward(self, x, edge_index, edge_attr=None, size=None):
        out = self._attend(x, edge_index, size, edge_attr)
        if not self.concat:
            out = out.view(out.size(0), self.heads, self.out_channels).mean(dim=1)
        return out if self.bias is None else out + self.bias


# ---- the epilogue between two attention passes (csrc/norm.hip) and the GATv2 model ------------------------------------------------
def _norm_operands(a, heads, bias, scale, norm_weight, norm_bias):
    op = "head_act_norm"
    _require_gpu(a, bias, scale, norm_weight, norm_bias)
    if a.dim() != 2 or heads < 1 or a.size(1) % heads:
        raise RuntimeError(f"{op}: a must be 2-D with heads = {heads} dividing its columns")
    HC = a.size(1)
    C = HC // heads
    if HC > 8192:
        raise RuntimeError(f"{op}: heads * channels = {HC} is past the 8192 the row pass holds")
    if norm_bias is not None and norm_weight is None:
        raise RuntimeError(f"{op}: norm_bias without norm_weight")
    if HC > 1 and a.stride(1) != 1:
        a = a.contiguous()
    a, lda = _rows(a, "a", 1, HC, op=op) if HC else (a, 0)
    vecs = []
    for t, what in ((bias, "bias"), (norm_weight, "norm_weight"), (norm_bias, "norm_bias")):
        if t is not None and (t.numel() != C or t.dtype != a.dtype):
            raise RuntimeError(f"{op}: {what} must hold {C} values of a's dtype")
        vecs.append(None if t is None else t.contiguous().view(-1))
    if scale is not None:
        if tuple(scale.shape) != (a.size(0), C) or scale.dtype != a.dtype:
            raise RuntimeError(f"{op}: scale must be [{a.size(0)}, {C}] of a's dtype")
        scale = scale.contiguous()
    return a, lda, vecs[0], scale, vecs[1], vecs[2], HC, C


def _norm_forward(a, heads, bias, relu, scale, norm_weight, norm_bias, eps, want_stats):
    """(out [N, C], stats fp32 [N, 2] or None) of one launch of gnnops_head_act_norm: the raw call, which like every raw entry
    point refuses operands that require grad (inside `_HeadActNorm` grad mode is off)."""
    ops._refuse_grad("conv.head_act_norm", a, bias, scale, norm_weight, norm_bias)
    a, lda, bias, scale, gamma, beta, HC, C = _norm_operands(a, heads, bias, scale, norm_weight, norm_bias)
    N = a.size(0)
    out = torch.empty((N, C), dtype=a.dtype, device=a.device)
    stats = torch.empty((N, 2), dtype=torch.float32, device=a.device) if want_stats and gamma is not None else None
    if C == 0:
        return out, stats
    with _on(a.device):
        check(_lib.load().gnnops_head_act_norm(a.data_ptr(), lda, _ptr(bias), _ptr(scale), _ptr(gamma), _ptr(beta), out.data_ptr(),
                                               _ptr(stats), N, heads, C, int(bool(relu)), float(eps), _dtype_code(a, "head_act_norm"),
                                               _stream()), "head_act_norm")
    return out, stats


def head_act_norm(a, heads, bias=None, relu=True, scale=None, norm_weight=None, norm_bias=None, eps=1e-5):
    """out[i] = LayerNorm(relu(mean over heads of a[i] + bias) * scale[i]) in one row pass (csrc/norm.hip): what the GATv2 model
    runs between two attention passes. a [N, heads * C] (a column block of a wider matrix is fine), bias [C], scale [N, C] (the
    dropout mask already divided by 1 - p; not differentiated), norm_weight / norm_bias [C]; each optional: without norm_weight
    there is no normalisation. Differentiable in a, bias, norm_weight and norm_bias; the backward recomputes the row from a."""
    if _wants_grad(scale):
        raise RuntimeError("head_act_norm: scale (the dropout mask) is not differentiated; detach it")
    if _wants_grad(a, bias, norm_weight, norm_bias):
        return _HeadActNorm.apply(a, bias, scale, norm_weight, norm_bias, heads, bool(relu), float(eps))
    return _norm_forward(a, heads, bias, relu, scale, norm_weight, norm_bias, eps, False)[0]


class _HeadActNorm(torch.autograd.Function):
    """backward (gnnops_head_act_norm_backward): saves the operands and (mu, rstd) only; y, the ReLU gate and xhat are recomputed
    from a. d bias / d norm_weight / d norm_bias are fp32 partial sums added in a fixed order (no atomics)."""

    @staticmethod
    def forward(ctx, a, bias, scale, norm_weight, norm_bias, heads, relu, eps):
        out, stats = _norm_forward(a, heads, bias, relu, scale, norm_weight, norm_bias, eps, True)
        ctx.meta = (heads, relu)
        ctx.save_for_backward(a, bias, scale, norm_weight, norm_bias, stats)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        a0, bias0, scale, gamma0, beta0, stats = ctx.saved_tensors
        heads, relu = ctx.meta
        a, lda, bias, scale, gamma, _, HC, C = _norm_operands(a0, heads, bias0, scale, gamma0, None)
        N = a.size(0)
        need_a, need_bias, _, need_gamma, need_beta = ctx.needs_input_grad[:5]
        d_a = torch.empty((N, HC), dtype=a.dtype, device=a.device)
        d_bias = torch.zeros(C, dtype=a.dtype, device=a.device) if need_bias else None
        d_gamma = torch.zeros(C, dtype=a.dtype, device=a.device) if need_gamma else None
        d_beta = torch.zeros(C, dtype=a.dtype, device=a.device) if need_beta else None
        if N and C:
            # the layouts autograd hands over, as `_EdgeAttention.backward`: unit column stride in place (pitch 0 = one row for
            # all), anything else copied
            g = grad_out if grad_out.dim() == 2 and (grad_out.stride(1) == 1 or grad_out.size(1) == 1) else grad_out.contiguous()
            g, ldg = _rows(g, "the output gradient", 1, C, op="head_act_norm")
            if g.size(0) > 1 and g.stride(0) == 0:
                ldg = 0
            L = _lib.load()
            ws_bytes = L.gnnops_head_act_norm_backward_workspace_bytes(N, heads, C)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=a.device)
            with _on(a.device):
                check(L.gnnops_head_act_norm_backward(a.data_ptr(), lda, _ptr(bias), _ptr(scale), _ptr(gamma), _ptr(stats), g.data_ptr(), ldg,
                                                      d_a.data_ptr(), _ptr(d_bias), _ptr(d_gamma), _ptr(d_beta), N, heads, C, int(relu),
                                                      _dtype_code(a, "head_act_norm"), ws.data_ptr(), ws_bytes, _stream()),
                      "head_act_norm_backward")
        shaped = lambda d, like: None if d is None else d.view(like.shape)   # noqa: E731
        return (d_a if need_a else None, shaped(d_bias, bias0) if need_bias else None, None, shaped(d_gamma, gamma0) if need_gamma else None,
                shaped(d_beta, beta0) if need_beta else None, None, None, None)


def _feature_scale(n, channels, p, dtype, device):
    """The feature dropout mask of one layer of `GATv2`, [N, C]: Bernoulli(1 - p) drawn with torch, already divided by 1 - p."""
    keep = torch.rand((n, channels), device=device) >= p
    return (keep.to(torch.float32) / (1.0 - p)).to(dtype)


class GATv2(torch.nn.Module):
    """The graph regressor the reference's zoo builds from GATv2Conv (GATv2REG, graph_benchmark/models/ptg_models.py): `convs` holds
    num_conv_layers + 1 GATv2Conv(., hidden_dim, heads, concat=False), `lns` num_conv_layers LayerNorm(hidden_dim), `post_mp` one
    Linear(hidden_dim, 1); the last conv and the last norm are parameters the forward never uses, as there, so a state_dict moves
    across. A layer is one dense product, one attention pass and ONE `head_act_norm` (mean over heads + bias + ReLU + the feature
    dropout mask + LayerNorm, the norm left out after the last layer); then the mean over each graph's nodes and `post_mp`."""

    def __init__(self, input_dim, hidden_dim, dropout, num_conv_layers, heads):
        super().__init__()
        self.dropout, self.num_layers = dropout, num_conv_layers
        self.convs = torch.nn.ModuleList([GATv2Conv(input_dim if k == 0 else hidden_dim, hidden_dim, heads=heads, concat=False)
                                          for k in range(num_conv_layers + 1)])
        self.lns = torch.nn.ModuleList([torch.nn.LayerNorm(hidden_dim) for _ in range(num_conv_layers)])
        self.post_mp = torch.nn.Sequential(torch.nn.Linear(hidden_dim, 1))

    def forward(self, x, edge_index=None, batch=None, num_graphs=None):
        """forward(x, edge_index, batch), or forward(data) with data.x / data.edge_index / data.batch. num_graphs spares the read
        of batch.max() from the device."""
        from . import pool

        if edge_index is None:
            x, edge_index, batch = x.x, x.edge_index, x.batch
        _require_gpu(x, edge_index, batch)
        for k in range(self.num_layers):
            conv = self.convs[k]
            a = conv._attend(x, edge_index)
            scale = None
            if self.training and self.dropout > 0.0:
                scale = _feature_scale(a.size(0), conv.out_channels, self.dropout, a.dtype, a.device)
            ln = self.lns[k] if k != self.num_layers - 1 else None
            x = head_act_norm(a, conv.heads, conv.bias, True, scale, None if ln is None else ln.weight, None if ln is None else ln.bias,
                              1e-5 if ln is None else ln.eps)
        return self.post_mp(pool.global_mean_pool(x, batch, num_graphs))


# ---- attention: GAT (v1), GATEConv and AttentiveFP (csrc/attention.hip, gate_fwd_kernel / gate_bwd_kernel) ------------------
def _v1_operands(q, d, att, edge_index, num_dst, heads, u, edge_scale, c=None):
    op = "edge_attention_v1"
    _require_gpu(q, d, att, edge_index, u, edge_scale, c)
    if att.numel() > 8192:
        raise RuntimeError(f"{op}: heads * channels = {att.numel()} exceeds the row limit of 8192")
    q, ldq, d, ldd, att, (u, edge_scale, c), edge_index, src_rows, plan, col, E, HC = _attention_prepare(
        op, q, att, edge_index, num_dst, heads, (d, "d", "heads", "one row per destination and one column per head"),
        [(u, "u", "heads * channels"), (edge_scale, "edge_scale", "heads"), (c, "edge_score", "heads")])
    if u is not None and c is not None:
        raise NotImplementedError(f"{op}: u and edge_score together have no kernel instance")
    if edge_scale is not None:
        edge_scale = edge_scale.detach()
    return q, ldq, d, ldd, att, u, edge_scale, c, edge_index, src_rows, plan, col, E, HC


def _v1_forward(q, d, att, edge_index, num_dst, heads, u, row_slope, negative_slope, edge_scale, c=None, identity_perm=False):
    """(out [num_dst, H * C], lse fp32 [num_dst, H]) of one launch of gnnops_edge_attention_v1.
    identity_perm: the caller knows the edge list to be sorted by destination already; the per-edge operands are read without perm."""
    q, ldq, d, ldd, att, u, ks, c, edge_index, _, plan, col, E, HC = _v1_operands(q, d, att, edge_index, num_dst, heads, u, edge_scale, c)
    out = torch.empty((num_dst, HC), dtype=q.dtype, device=q.device)
    lse = torch.empty((num_dst, heads), dtype=torch.float32, device=q.device)
    perm = None if identity_perm else plan.perm.data_ptr()
    with _on(q.device):
        check(_lib.load().gnnops_edge_attention_v1(q.data_ptr(), ldq, d.data_ptr(), ldd, att.data_ptr(), _ptr(u), _ptr(c), _ptr(ks),
                                                   plan.rowptr.data_ptr(), perm, col.data_ptr(), out.data_ptr(), HC, lse.data_ptr(), num_dst, E,
                                                   heads, HC // heads, int(row_slope is not None), float(row_slope or 0.0),
                                                   float(negative_slope), _dtype_code(q, "edge_attention_v1"), _stream()), "edge_attention_v1")
    return out, lse


def edge_attention_v1(q, d, att, edge_index, num_dst, heads, u=None, row_slope=None, negative_slope=0.2, edge_scale=None, edge_score=None):
    """out[i, h, :] = sum over the edges e = (j -> i) of softmax_e(s[e, h]) * edge_scale[e, h] * r[e, h, :], with
    r = q[j, h] + u[e, h] (through leaky_relu(., row_slope) when row_slope is given) and s[e, h] = leaky_relu(att[h] . r[e, h] + d[i, h],
    negative_slope): the message and aggregation of GATConv (u, row_slope absent) and of AttentiveFP's GATEConv in one pass with an
    online softmax (csrc/attention.hip). q [N_src, H * C] and d [num_dst, H] may be column blocks of one product; att holds H * C
    entries; u [E, H * C] and edge_scale [E, H] follow the order of edge_index. edge_scale (the attention dropout mask divided by
    1 - p) multiplies the weighted sum only, never the softmax denominator, and is not differentiated. A destination without edges
    gets a zero row. edge_score [E, H], in the order of edge_index, is added to att[h] . r[e, h] + d[i, h] before the leaky ReLU
    (GATConv's att_edge . lin_edge(edge_attr)); it cannot be combined with u. Differentiable in q, d, att, u and edge_score."""
    if _wants_grad(q, d, att, u, edge_score):
        return _EdgeAttentionV1.apply(q, d, att, u, edge_score, edge_scale, edge_index, num_dst, heads, row_slope, float(negative_slope))
    return _v1_forward(q, d, att, edge_index, num_dst, heads, u, row_slope, negative_slope, edge_scale, edge_score)[0]


def _v1_backward(q0, d0, att0, u0, c0, ks0, edge_index, out, lse, grad_out, num_dst, heads, row_slope, slope, identity_perm=False):
    """(gq [E, H * C] or None, d d [num_dst, H], d att [H * C], d edge_score [E, H] or None, src_rows, edge_index) of one launch of
    gnnops_edge_attention_v1_backward; None where there is no edge."""
    q, ldq, d, ldd, att, u, ks, c, edge_index, src_rows, plan, col, E, HC = _v1_operands(q0, d0, att0, edge_index, num_dst, heads, u0, ks0, c0)
    if E == 0 or num_dst == 0:
        return None, None, None, None, src_rows, edge_index
    g, ldg = _grad_rows(grad_out, HC, "edge_attention_v1")
    d_d = torch.empty((num_dst, heads), dtype=q.dtype, device=q.device)
    gq = torch.empty((E, HC), dtype=q.dtype, device=q.device)
    d_att = torch.empty(HC, dtype=q.dtype, device=q.device)
    d_c = None if c is None else torch.empty((E, heads), dtype=q.dtype, device=q.device)
    L = _lib.load()
    perm = None if identity_perm else plan.perm.data_ptr()
    with _on(q.device):
        ws_bytes = L.gnnops_edge_attention_backward_workspace_bytes(num_dst, heads, HC // heads)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device)
        check(L.gnnops_edge_attention_v1_backward(q.data_ptr(), ldq, d.data_ptr(), ldd, att.data_ptr(), _ptr(u), _ptr(c), _ptr(ks),
                                                  out.data_ptr(), HC, lse.data_ptr(), g.data_ptr(), ldg, plan.rowptr.data_ptr(), perm,
                                                  col.data_ptr(), d_d.data_ptr(), gq.data_ptr(), _ptr(d_c), d_att.data_ptr(), num_dst, E,
                                                  heads, HC // heads, int(row_slope is not None), float(row_slope or 0.0), slope,
                                                  _dtype_code(q, "edge_attention_v1"), ws.data_ptr(), ws_bytes, _stream()),
              "edge_attention_v1_backward")
    return gq, d_d, d_att, d_c, src_rows, edge_index


class _EdgeAttentionV1(torch.autograd.Function):
    """backward (gnnops_edge_attention_v1_backward, destination-ordered like the forward): d d and d att from the kernel, and one
    per-edge tensor gq [E, H * C] in edge order: d u is gq itself, d q its segment sum over the plan of the source ids. With
    edge_score its gradient [E, H] comes from the kernel in edge order too."""

    @staticmethod
    def forward(ctx, q, d, att, u, c, edge_scale, edge_index, num_dst, heads, row_slope, negative_slope):
        out, lse = _v1_forward(q, d, att, edge_index, num_dst, heads, u, row_slope, negative_slope, edge_scale, c)
        ctx.meta = (num_dst, heads, row_slope, negative_slope, u is not None, c is not None, edge_scale is not None)
        ctx.save_for_backward(q, d, att, edge_index, out, lse, *(t for t in (u, c, edge_scale) if t is not None))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q0, d0, att0, edge_index, out, lse, *rest = ctx.saved_tensors
        num_dst, heads, row_slope, slope, has_u, has_c, has_ks = ctx.meta
        u0 = rest.pop(0) if has_u else None
        c0 = rest.pop(0) if has_c else None
        ks0 = rest.pop(0) if has_ks else None
        need_q, need_d, need_att, need_u, need_c = ctx.needs_input_grad[:5]
        tail = (None,) * 6
        gq, d_d, d_att, d_c, src_rows, edge_index = _v1_backward(q0, d0, att0, u0, c0, ks0, edge_index, out, lse, grad_out, num_dst, heads,
                                                                 row_slope, slope)
        if gq is None:
            return (torch.zeros_like(q0) if need_q else None, torch.zeros_like(d0) if need_d else None,
                    torch.zeros_like(att0) if need_att else None, torch.zeros_like(u0) if has_u and need_u else None,
                    torch.zeros_like(c0) if has_c and need_c else None) + tail
        d_q, d_d = _attention_tail(gq, d_d, src_rows, edge_index, q0, d0, need_q, need_d)
        return (d_q, d_d, d_att.view(att0.shape) if need_att else None, gq if has_u and need_u else None,
                d_c if has_c and need_c else None) + tail


def _dropout_scale(E, heads, p, dtype, device):
    """The attention dropout mask of one call, [E, H]: Bernoulli(1 - p) drawn with torch, already divided by 1 - p."""
    keep = torch.rand((E, heads), device=device) >= p
    return (keep.to(torch.float32) / (1.0 - p)).to(dtype)


def _fold(att, weight, heads):
    """[H, in]: row h = att[h, :] @ weight[h * C:(h + 1) * C, :], so that x @ row^T = att[h] . (x W^T)[h] — the per-node score term
    as H more columns of the layer's one product."""
    return torch.einsum("hc,hci->hi", att.view(heads, -1), weight.view(heads, att.numel() // heads, weight.size(1)))


def _pad8(blocks, like):
    """Zero columns up to a multiple of 8, so that every row of the product starts on a 16-byte boundary in every type."""
    width = sum(w.size(0) for w, _ in blocks)
    if width % 8:
        blocks = blocks + [(like.new_zeros((8 - width % 8, like.size(1))), None)]
    return blocks


class GATConv(_Layer):
    """x'_i = sum_j alpha_ij W x_j (+ bias),  alpha_ij = softmax_j(leaky_relu(att_src . W x_j + att_dst . W x_i))  per head
    (torch_geometric 2.0.x GATConv, Velickovic et al. 2018; AttentiveFP's atom layers after the first and its read-out). One product
    x @ [W^T | fold(att_dst, W_dst)^T]: the per-destination score term d comes out of it as H more columns (att_dst folded into the
    weight, `_fold`), then one attention pass (`edge_attention_v1`), the mean over heads (concat=False) and the bias. Parameter names
    follow PyG 2.0.x (lin_src, lin_dst, att_src, att_dst, bias); parity unpinned. Self loops and the bipartite pair as GATv2Conv.
    Attention dropout: a Bernoulli mask [E, H] drawn with torch, scaled by 1 / (1 - p), applied after the softmax (edge_scale).
    Edge features (edge_dim set; parameters lin_edge.weight and att_edge as PyG): the score gains att_edge . lin_edge(e_ij) per head.
    att_edge is folded into lin_edge's weight exactly as att_dst is into lin_dst's, so the term is ONE product edge_attr @ [H, edge_dim]^T
    (padded to 8 columns) whose [E, H] result the attention pass adds before the leaky ReLU (edge_score): no [E, H * C] tensor exists.
    Self-loop attributes (fill_value) as GATv2Conv."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True, bias=True,
                 edge_dim=None, fill_value="mean"):
        super().__init__()
        self.in_channels, self.out_channels, self.heads, self.concat = in_channels, out_channels, heads, concat
        self.negative_slope, self.dropout, self.add_self_loops = negative_slope, dropout, add_self_loops
        self.edge_dim, self.fill_value = edge_dim, _checked_fill_value(fill_value, "GATConv")
        if isinstance(in_channels, int):
            self.lin_src = torch.nn.Linear(in_channels, heads * out_channels, bias=False)
            self.lin_dst = self.lin_src
        else:
            self.lin_src = torch.nn.Linear(in_channels[0], heads * out_channels, bias=False)
            self.lin_dst = torch.nn.Linear(in_channels[1], heads * out_channels, bias=False)
        self.att_src = torch.nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = torch.nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = torch.nn.Parameter(torch.zeros(heads * out_channels if concat else out_channels)) if bias else None
        for w in (self.lin_src.weight, self.lin_dst.weight, self.att_src, self.att_dst):      # glorot, as PyG
            torch.nn.init.xavier_uniform_(w)
        if edge_dim is not None:
            self.lin_edge = torch.nn.Linear(edge_dim, heads * out_channels, bias=False)
            self.att_edge = torch.nn.Parameter(torch.empty(1, heads, out_channels))
            torch.nn.init.xavier_uniform_(self.lin_edge.weight)
            torch.nn.init.xavier_uniform_(self.att_edge)
        self._pk_both, self._pk_src, self._pk_dst, self._pk_e = _Packed(), _Packed(), _Packed(), _Packed()
        self._looped = self._kept = None

    _with_self_loops = GATv2Conv._with_self_loops
    _kept_edges = GATv2Conv._kept_edges
    _edge_rows = GATv2Conv._edge_rows

    def forward(self, x, edge_index, edge_attr=None, size=None):
        H, C = self.heads, self.out_channels
        HC = H * C
        ws, wd = self.lin_src.weight, self.lin_dst.weight
        if isinstance(x, (tuple, list)):
            if self.add_self_loops:
                raise RuntimeError("GATConv: a bipartite pair needs add_self_loops=False")
            x_src, x_dst = x
            _require_gpu(x_src, x_dst, edge_index)
            q = _dense(x_src.contiguous(), self._pk_src.get([ws], [(ws, None)]))
            d = _dense(x_dst.contiguous(), self._pk_dst.get([wd, self.att_dst], lambda: _pad8([(_fold(self.att_dst, wd, H), None)], wd)))[:, :H]
            n_dst = x_dst.size(0) if size is None else size[1]
            rows = self._edge_rows(edge_attr, edge_index, n_dst, False)
        else:
            _require_gpu(x, edge_index)
            n_dst = x.size(0)
            qd = _dense(x.contiguous(), self._pk_both.get([ws, wd, self.att_dst], lambda: _pad8([(ws, None), (_fold(self.att_dst, wd, H), None)], ws)))
            q, d = qd[:, :HC], qd[:, HC:HC + H]
            rows = self._edge_rows(edge_attr, edge_index, n_dst, self.add_self_loops)
            if self.add_self_loops:
                edge_index = self._with_self_loops(edge_index, n_dst)
        c = None
        if rows is not None:            # c[e, h] = att_edge[h] . lin_edge(edge_attr)[e, h]: one product with the folded weight
            we = self.lin_edge.weight
            c = _edge_dense(rows, self._pk_e.get([we, self.att_edge], lambda: _pad8([(_fold(self.att_edge, we, H), None)], we)))[:, :H]
        scale = None
        if self.dropout > 0.0 and self.training:
            scale = _dropout_scale(edge_index.size(1), H, self.dropout, q.dtype, q.device)
        out = edge_attention_v1(q, d, self.att_src, edge_index, n_dst, H, negative_slope=self.negative_slope, edge_scale=scale, edge_score=c)
        if not self.concat:
            out = out.view(n_dst, H, C).mean(dim=1)
        return out if self.bias is None else out + self.bias


class _EdgeLinear(torch.autograd.Function):
    """u = edge_attr @ weight_t for [E, edge_dim] edge features, edge_dim tiny. The backward of gnnops.autograd.matmul copies the
    transpose of its left operand, and that copy stops at 64 * 65535 rows; the transpose of ONE column is the same memory, so for
    edge_dim = 1 (the reference's config) d weight_t = edge_attr.view(1, E) @ g needs no copy and no limit. A wider edge_attr of more
    rows than that is transposed and multiplied in row blocks of that size, the blocks' products added in float32 in their order.
    Where ops.matmul_tn_preferred holds, d weight_t = ops.matmul_tn(edge_attr, g): no transpose, no row limit, no blocks."""

    MAX_ROWS = 64 * 65535

    @staticmethod
    def forward(ctx, edge_attr, weight_t):
        ctx.save_for_backward(edge_attr, weight_t)
        return ops.matmul(edge_attr, weight_t)

    @staticmethod
    def backward(ctx, g):
        from .sparse import transpose_contiguous

        edge_attr, weight_t = ctx.saved_tensors
        g = g.contiguous()
        d_e = d_w = None
        if ctx.needs_input_grad[0]:
            d_e = ops.matmul(g, transpose_contiguous(weight_t))
        if ctx.needs_input_grad[1]:
            if edge_attr.size(1) != 1 and ops.matmul_tn_preferred(edge_attr.size(0), edge_attr.size(1), g.size(1), g.dtype):
                d_w = ops.matmul_tn(edge_attr, g)
            elif edge_attr.size(1) == 1 or edge_attr.size(0) <= _EdgeLinear.MAX_ROWS:
                e_t = edge_attr.view(1, -1) if edge_attr.size(1) == 1 else transpose_contiguous(edge_attr)
                d_w = ops.matmul(e_t, g)
            else:
                step = _EdgeLinear.MAX_ROWS
                parts = [ops.matmul(transpose_contiguous(edge_attr[k:k + step]), g[k:k + step]).float() for k in range(0, edge_attr.size(0), step)]
                d_w = sum(parts[1:], parts[0]).to(g.dtype)
        return d_e, d_w


def _edge_dense(rows, packed):
    """rows [E, edge_dim] @ the packed weight [edge_dim, W]: `_dense` for the one product of a layer whose left operand has a row per
    EDGE (`_EdgeLinear`: no row limit in its backward)."""
    weight_t = packed[0]
    return _EdgeLinear.apply(rows, weight_t) if _wants_grad(rows, weight_t) else ops.matmul(rows, weight_t)


class GATEConv(_Layer):
    """AttentiveFP's first atom layer (torch_geometric.nn.models.attentive_fp.GATEConv, one head):
    x_j' = leaky_relu(lin1([x_j, e_ji])),  alpha_ji = softmax_j(leaky_relu(att_l . x_j' + att_r . x_i)),  x'_i = lin2(sum_j alpha_ji x_j') + bias
    (both slopes 0.01). lin1 splits into its node and its edge columns: one product x @ [W1x^T | att_r^T] gives q and d, one product
    edge_attr @ W1e^T gives the per-edge rows u, one attention pass (`edge_attention_v1` with u and row_slope), and lin2 — linear —
    is applied once to the aggregate instead of once per edge. No self loops. Attention dropout as GATConv."""

    def __init__(self, in_channels, out_channels, edge_dim, dropout=0.0):
        super().__init__()
        self.in_channels, self.out_channels, self.edge_dim, self.dropout = in_channels, out_channels, edge_dim, dropout
        self.att_l = torch.nn.Parameter(torch.empty(1, out_channels))
        self.att_r = torch.nn.Parameter(torch.empty(1, in_channels))
        self.lin1 = torch.nn.Linear(in_channels + edge_dim, out_channels, bias=False)
        self.lin2 = torch.nn.Linear(out_channels, out_channels, bias=False)
        self.bias = torch.nn.Parameter(torch.zeros(out_channels))
        for w in (self.att_l, self.att_r, self.lin1.weight, self.lin2.weight):
            torch.nn.init.xavier_uniform_(w)
        self._pk_x, self._pk_e, self._pk_2 = _Packed(), _Packed(), _Packed()

    def forward(self, x, edge_index, edge_attr):
        _require_gpu(x, edge_index, edge_attr)
        cin, cout = self.in_channels, self.out_channels
        w1 = self.lin1.weight
        qd = _dense(x.contiguous(), self._pk_x.get([w1, self.att_r], lambda: _pad8([(w1[:, :cin], None), (self.att_r, None)], self.att_r)))
        q, d = qd[:, :cout], qd[:, cout:cout + 1]
        w1e_t = self._pk_e.get([w1], lambda: [(w1[:, cin:], None)])[0]
        u = _EdgeLinear.apply(edge_attr.contiguous(), w1e_t) if _wants_grad(edge_attr, w1e_t) else ops.matmul(edge_attr.contiguous(), w1e_t)
        scale = None
        if self.dropout > 0.0 and self.training:
            scale = _dropout_scale(edge_index.size(1), 1, self.dropout, q.dtype, q.device)
        agg = edge_attention_v1(q, d, self.att_l, edge_index, x.size(0), 1, u=u, row_slope=0.01, negative_slope=0.01, edge_scale=scale)
        return _dense(agg, self._pk_2.get([self.lin2.weight, self.bias], [(self.lin2.weight, self.bias)]))


class AttentiveFP(torch.nn.Module):
    """The molecule regressor of Xiong et al. 2020 as torch_geometric.nn.models.AttentiveFP builds it (submodule names lin1,
    atom_convs, atom_grus, mol_conv, mol_gru, lin2; the reference's AttentiveFPREG, graph_benchmark/models/ptg_models.py): atom
    layers of GATEConv / GATConv each followed by a GRU cell, a read-out of num_timesteps rounds of GATConv over the bipartite
    (atom -> molecule) graph with a GRU cell, and a Linear. The attention layers are this package's fused ones, the sum over a
    molecule's atoms its scatter; GRUCell, elu and the feature dropout are torch's."""

    def __init__(self, in_channels, hidden_channels, out_channels, edge_dim, num_layers, num_timesteps, dropout=0.0):
        super().__init__()
        self.num_layers, self.num_timesteps, self.dropout = num_layers, num_timesteps, dropout
        self.lin1 = torch.nn.Linear(in_channels, hidden_channels)
        self.atom_convs = torch.nn.ModuleList([GATEConv(hidden_channels, hidden_channels, edge_dim, dropout)])
        self.atom_grus = torch.nn.ModuleList([torch.nn.GRUCell(hidden_channels, hidden_channels)])
        for _ in range(num_layers - 1):
            self.atom_convs.append(GATConv(hidden_channels, hidden_channels, dropout=dropout, add_self_loops=False, negative_slope=0.01))
            self.atom_grus.append(torch.nn.GRUCell(hidden_channels, hidden_channels))
        self.mol_conv = GATConv(hidden_channels, hidden_channels, dropout=dropout, add_self_loops=False, negative_slope=0.01)
        self.mol_gru = torch.nn.GRUCell(hidden_channels, hidden_channels)
        self.lin2 = torch.nn.Linear(hidden_channels, out_channels)

    def forward(self, x, edge_index, edge_attr, batch, num_graphs=None):
        """batch int64 [N]: the molecule of each atom; num_graphs spares the read of batch.max() from the device."""
        from . import autograd
        F = torch.nn.functional
        _require_gpu(x, edge_index, edge_attr, batch)
        x = F.leaky_relu(self.lin1(x))
        for k, (conv, gru) in enumerate(zip(self.atom_convs, self.atom_grus)):
            h = F.elu(conv(x, edge_index, edge_attr) if k == 0 else conv(x, edge_index))
            h = F.dropout(h, p=self.dropout, training=self.training)
            x = gru(h, x).relu()
        n = x.size(0)
        G = int(batch.max()) + 1 if num_graphs is None else num_graphs
        out = autograd.scatter(x, batch, 0, None, G, "sum").relu()
        to_mol = torch.stack([torch.arange(n, dtype=batch.dtype, device=batch.device), batch])   # one object: its plans serve every round
        for _ in range(self.num_timesteps):
            h = F.elu(self.mol_conv((x, out), to_mol, size=(n, G)))
            h = F.dropout(h, p=self.dropout, training=self.training)
            out = self.mol_gru(h, out).relu()
        out = F.dropout(out, p=self.dropout, training=self.training)
        return self.lin2(out)


# ---- attention: TransformerConv (csrc/attention.hip, dot_fwd_kernel / dot_bwd_kernel) ----------------------------------------
def _dot_operands(qry, k, v, edge_index, num_dst, heads, u, edge_scale):
    op = "edge_attention_dot"
    _require_gpu(qry, k, v, edge_index, u, edge_scale)
    if qry.dim() != 2 or k.dim() != 2 or v.dim() != 2:
        raise RuntimeError(f"{op}: qry, k and v must be 2-D")
    HC = qry.size(1)
    if HC > 8192:
        raise RuntimeError(f"{op}: heads * channels = {HC} exceeds the row limit of 8192")
    if v.dtype != k.dtype:
        raise RuntimeError(f"{op}: operands must have the same dtype")
    if v.size(0) != k.size(0):
        raise RuntimeError(f"{op}: k and v must have one row per source each, got {k.size(0)} and {v.size(0)}")
    width = torch.empty(HC, dtype=k.dtype, device="meta")     # this pass has no att: only its size and type are asked for
    k, ldkv, qry, ldq, _, (u, edge_scale), edge_index, src_rows, plan, col, E, HC = _attention_prepare(
        op, k, width, edge_index, num_dst, heads, (qry, "qry", "heads * channels", "one row per destination"),
        [(u, "u", "heads * channels"), (edge_scale, "edge_scale", "heads")])
    v, ldv = _rows(v, "v", 1, HC, op=op)
    if ldv != ldkv:           # the kernel reads both rows of a source from one row base: two blocks of one matrix, or two dense copies
        k, v, ldkv = k[:, :HC].contiguous(), v[:, :HC].contiguous(), HC
    if edge_scale is not None:
        edge_scale = edge_scale.detach()
    return qry, ldq, k, v, ldkv, u, edge_scale, edge_index, src_rows, plan, col, E, HC


def _dot_scale(scale, HC, heads):
    return float(scale) if scale is not None else 1.0 / float(max(HC // max(heads, 1), 1)) ** 0.5


def _dot_forward(qry, k, v, edge_index, num_dst, heads, scale=None, u=None, edge_scale=None, identity_perm=False):
    """(out [num_dst, H * C], lse fp32 [num_dst, H]) of one launch of gnnops_edge_attention_dot.
    identity_perm: the caller knows the edge list to be sorted by destination already; the per-edge operands are read without perm."""
    qry, ldq, k, v, ldkv, u, ks, edge_index, _, plan, col, E, HC = _dot_operands(qry, k, v, edge_index, num_dst, heads, u, edge_scale)
    out = torch.empty((num_dst, HC), dtype=k.dtype, device=k.device)
    lse = torch.empty((num_dst, heads), dtype=torch.float32, device=k.device)
    perm = None if identity_perm or (u is None and ks is None) else plan.perm.data_ptr()   # only u and edge_scale are read through it
    with _on(k.device):
        check(_lib.load().gnnops_edge_attention_dot(qry.data_ptr(), ldq, k.data_ptr(), v.data_ptr(), ldkv, _ptr(u), _ptr(ks), plan.rowptr.data_ptr(),
                                                    perm, col.data_ptr(), out.data_ptr(), HC, lse.data_ptr(), num_dst, E, heads, HC // heads,
                                                    _dot_scale(scale, HC, heads), _dtype_code(k, "edge_attention_dot"), _stream()),
              "edge_attention_dot")
    return out, lse


def _dot_backward(qry0, k0, v0, u0, ks0, edge_index, out, lse, grad_out, num_dst, heads, scale, identity_perm=False):
    """(gkv [E, 2 * H * C] or None, d qry [num_dst, H * C], d u [E, H * C] or None, src_rows, edge_index) of one launch of
    gnnops_edge_attention_dot_backward; None where there is no edge."""
    qry, ldq, k, v, ldkv, u, ks, edge_index, src_rows, plan, col, E, HC = _dot_operands(qry0, k0, v0, edge_index, num_dst, heads, u0, ks0)
    if E == 0 or num_dst == 0:
        return None, None, None, src_rows, edge_index
    g, ldg = _grad_rows(grad_out, HC, "edge_attention_dot")
    d_qry = torch.empty((num_dst, HC), dtype=k.dtype, device=k.device)
    gkv = torch.empty((E, 2 * HC), dtype=k.dtype, device=k.device)
    d_u = None if u is None else torch.empty((E, HC), dtype=k.dtype, device=k.device)
    perm = None if identity_perm else plan.perm.data_ptr()
    with _on(k.device):
        check(_lib.load().gnnops_edge_attention_dot_backward(qry.data_ptr(), ldq, k.data_ptr(), v.data_ptr(), ldkv, _ptr(u), _ptr(ks), out.data_ptr(),
                                                             HC, lse.data_ptr(), g.data_ptr(), ldg, plan.rowptr.data_ptr(), perm, col.data_ptr(),
                                                             d_qry.data_ptr(), gkv.data_ptr(), _ptr(d_u), num_dst, E, heads, HC // heads,
                                                             _dot_scale(scale, HC, heads), _dtype_code(k, "edge_attention_dot"), _stream()),
              "edge_attention_dot_backward")
    return gkv, d_qry, d_u, src_rows, edge_index


def edge_attention_dot(qry, k, v, edge_index, num_dst, heads, scale=None, u=None, edge_scale=None):
    """out[i, h, :] = sum over the edges e = (j -> i) of softmax_e(s[e, h]) * edge_scale[e, h] * (v[j, h] + u[e, h]), with
    s[e, h] = scale * qry[i, h] . (k[j, h] + u[e, h]): scaled dot-product attention over the edges of a destination, TransformerConv's
    message and aggregation in one pass with an online softmax (csrc/attention.hip). qry [num_dst, H * C], k and v [N_src, H * C] may be
    column blocks of wider products and are read in place (k and v of different pitches are copied: the kernel reads both from one
    row base); scale defaults to 1 / sqrt(C); u [E, H * C] and edge_scale [E, H] follow the order of edge_index. edge_scale (the
    attention dropout mask divided by 1 - p) multiplies the weighted sum only, never the softmax denominator, and is not
    differentiated. A destination without edges gets a zero row. Differentiable in qry, k, v and u."""
    if _wants_grad(qry, k, v, u):
        return _EdgeAttentionDot.apply(qry, k, v, u, edge_scale, edge_index, num_dst, heads, scale)
    return _dot_forward(qry, k, v, edge_index, num_dst, heads, scale, u, edge_scale)[0]


class _EdgeAttentionDot(torch.autograd.Function):
    """backward (gnnops_edge_attention_dot_backward, destination-ordered like the forward): d qry from the kernel, and one per-edge
    tensor gkv [E, 2 * H * C] in edge order whose ONE segment sum over the plan of the source ids is [d k | d v]. With u a second
    per-edge tensor in edge order is d u."""

    @staticmethod
    def forward(ctx, qry, k, v, u, edge_scale, edge_index, num_dst, heads, scale):
        out, lse = _dot_forward(qry, k, v, edge_index, num_dst, heads, scale, u, edge_scale)
        ctx.meta = (num_dst, heads, scale, u is not None, edge_scale is not None)
        ctx.save_for_backward(qry, k, v, edge_index, out, lse, *(t for t in (u, edge_scale) if t is not None))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        qry0, k0, v0, edge_index, out, lse, *rest = ctx.saved_tensors
        num_dst, heads, scale, has_u, has_ks = ctx.meta
        u0 = rest.pop(0) if has_u else None
        ks0 = rest.pop(0) if has_ks else None
        need_qry, need_k, need_v, need_u = ctx.needs_input_grad[:4]
        tail = (None,) * 5
        gkv, d_qry, d_u, src_rows, edge_index = _dot_backward(qry0, k0, v0, u0, ks0, edge_index, out, lse, grad_out, num_dst, heads, scale)
        if gkv is None:
            return (torch.zeros_like(qry0) if need_qry else None, torch.zeros_like(k0) if need_k else None,
                    torch.zeros_like(v0) if need_v else None, torch.zeros_like(u0) if has_u and need_u else None) + tail
        HC = d_qry.size(1)
        both = torch.empty((k0.size(0), 2 * HC), device="meta")     # the shape of [d k | d v]: one segment sum, no padding
        d_kv, d_qry = _attention_tail(gkv, d_qry, src_rows, edge_index, both, qry0, need_k or need_v, need_qry)
        pad = lambda d, t: d if t.size(1) == HC else torch.nn.functional.pad(d, (0, t.size(1) - HC))   # noqa: E731
        return (d_qry, pad(d_kv[:, :HC], k0) if need_k else None, pad(d_kv[:, HC:], v0) if need_v else None,
                d_u if has_u and need_u else None) + tail


class TransformerConv(_Layer):
    """x'_i = W_skip x_i + sum_j alpha_ij (W_v x_j + W_e e_ij),  alpha_ij = softmax_j((W_q x_i) . (W_k x_j + W_e e_ij) / sqrt(C))  per head
    (torch_geometric TransformerConv; UniMP, Shi et al. 2021). With one node set, ONE product x @ [W_k^T | W_v^T | W_q^T | W_skip^T]
    whose column blocks reach the kernel in place; with a bipartite pair (x_src, x_dst), one product per side. Then one attention pass
    (`edge_attention_dot`), the mean over heads (concat=False) and the skip: out + x_r, or with beta=True
    beta * x_r + (1 - beta) * out, beta = sigmoid(lin_beta([out, x_r, out - x_r])), composed from torch ops (not fused). Edge features
    (edge_dim set): lin_edge(edge_attr), without a bias, is one more product, added to the key AND to the value by the pass. Attention
    dropout in training: a Bernoulli mask [E, H] drawn with torch, scaled by 1 / (1 - p), applied after the softmax (edge_scale); eval
    ignores it. Parameter names and shapes follow PyG (lin_key, lin_query, lin_value, lin_edge, lin_skip, lin_beta), so a state_dict
    moves across; parity unpinned. No self loops are added, as in PyG. `return_attention_weights` is not implemented: the argument
    is absent, because the pass never writes the [E, H] weights."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, beta=False, dropout=0.0, edge_dim=None, bias=True, root_weight=True):
        super().__init__()
        self.in_channels, self.out_channels, self.heads, self.concat = in_channels, out_channels, heads, concat
        self.beta, self.dropout, self.edge_dim, self.root_weight = beta and root_weight, dropout, edge_dim, root_weight
        in_src, in_dst = _pair(in_channels)
        HC = heads * out_channels
        self.lin_key = torch.nn.Linear(in_src, HC, bias=bias)
        self.lin_query = torch.nn.Linear(in_dst, HC, bias=bias)
        self.lin_value = torch.nn.Linear(in_src, HC, bias=bias)
        if edge_dim is not None:       # present only with edge features, so that a state_dict without them keeps PyG's keys
            self.lin_edge = torch.nn.Linear(edge_dim, HC, bias=False)
        if root_weight:
            width = HC if concat else out_channels
            self.lin_skip = torch.nn.Linear(in_dst, width, bias=bias)
            if self.beta:
                self.lin_beta = torch.nn.Linear(3 * width, 1, bias=False)
        self._pk_all, self._pk_src, self._pk_dst, self._pk_e = _Packed(), _Packed(), _Packed(), _Packed()

    _edge_rows = GATv2Conv._edge_rows

    def forward(self, x, edge_index, edge_attr=None):
        H, C = self.heads, self.out_channels
        HC = H * C
        kv = [self.lin_key, self.lin_value]
        qs = [self.lin_query] + ([self.lin_skip] if self.root_weight else [])
        pack = lambda cache, lins: cache.get([m.weight for m in lins] + [m.bias for m in lins], [(m.weight, m.bias) for m in lins])   # noqa: E731
        if isinstance(x, (tuple, list)):
            x_src, x_dst = x
            _require_gpu(x_src, x_dst, edge_index)
            left = _dense(x_src.contiguous(), pack(self._pk_src, kv))
            right = _dense(x_dst.contiguous(), pack(self._pk_dst, qs))
            n_dst = x_dst.size(0)
        else:       # [key | value | query | skip] = x @ [W_k^T | W_v^T | W_q^T | W_skip^T]: the projections reach the kernel as column blocks
            _require_gpu(x, edge_index)
            both = _dense(x.contiguous(), pack(self._pk_all, kv + qs))
            left, right = both[:, :2 * HC], both[:, 2 * HC:]
            n_dst = x.size(0)
        k, v, qry = left[:, :HC], left[:, HC:], right[:, :HC]
        rows = self._edge_rows(edge_attr, edge_index, n_dst, False)
        u = None
        if rows is not None:            # u = lin_edge(edge_attr): one product
            we = self.lin_edge.weight
            u = _edge_dense(rows, self._pk_e.get([we], [(we, None)]))
        scale = None
        if self.dropout > 0.0 and self.training:
            scale = _dropout_scale(edge_index.size(1), H, self.dropout, k.dtype, k.device)
        out = edge_attention_dot(qry, k, v, edge_index, n_dst, H, u=u, edge_scale=scale)
        if not self.concat:
            out = out.view(n_dst, H, C).mean(dim=1)
        if self.root_weight:
            x_r = right[:, HC:]
            if self.beta:
                beta = torch.sigmoid(torch.nn.functional.linear(torch.cat([out, x_r, out - x_r], dim=-1), self.lin_beta.weight))
                out = beta * x_r + (1.0 - beta) * out
            else:
                out = out + x_r
        return out


# ---- GCNConv, TopKPooling and GraphUNet (csrc/gcn.hip, csrc/pool.hip) -------------------------------------------------------
def _gcn_plan(edge_index, num_nodes, flip):
    """(plan, plan-ordered column ids, E) of the destination plan (``flip``: of the source ids) — the plans of `edge_reduce`."""
    edge_index, src_rows, dst_rows = _coo_rows_cols(edge_index, "gcn_propagate")
    if flip:
        src_rows, dst_rows = dst_rows, src_rows
    E = edge_index.size(1)
    plan = get_plan(dst_rows, num_nodes, owner=edge_index, tag=0 if flip else 1, companion=src_rows)
    if plan.col is not None or E == 0:
        col = plan.col if E else src_rows
    else:
        col, _ = _csr_arrays(plan, src_rows, None, owner=edge_index, tag=1 if flip else 0)
    return plan, col, E


def _gcn_degree(edge_index, w, num_nodes, fill_value):
    """(dis, lw) fp32 [num_nodes] of gnnops_gcn_degree: D^-1/2 and the self-loop weight of every node."""
    plan, col, E = _gcn_plan(edge_index, num_nodes, False)
    dev = edge_index.device
    dis = torch.empty(num_nodes, dtype=torch.float32, device=dev)
    lw = torch.empty(num_nodes, dtype=torch.float32, device=dev)
    with _on(dev):
        check(_lib.load().gnnops_gcn_degree(plan.rowptr.data_ptr(), plan.perm.data_ptr(), col.data_ptr() if E else None,
                                            w.data_ptr() if w is not None else None, num_nodes, E, float(fill_value),
                                            dis.data_ptr(), lw.data_ptr(), _stream()), "gcn_degree")
    return dis, lw


def _gcn_launch(h, edge_index, w, dis, lw, bias, num_nodes, flip):
    plan, col, E = _gcn_plan(edge_index, num_nodes, flip)
    K = h.size(1)
    h, ldh = _rows(h, "h", 1, K, op="gcn_propagate")
    if h.size(0) > 1 and h.stride(0) == 0:
        ldh = 0
    out = torch.empty((num_nodes, K), dtype=h.dtype, device=h.device)
    with _on(h.device):
        check(_lib.load().gnnops_gcn_propagate(h.data_ptr(), ldh, plan.rowptr.data_ptr(), plan.perm.data_ptr(),
                                               col.data_ptr() if E else None, w.data_ptr() if w is not None else None,
                                               dis.data_ptr(), lw.data_ptr(), bias.data_ptr() if bias is not None else None,
                                               out.data_ptr(), K, num_nodes, E, K, _dtype_code(h, "gcn_propagate"), _stream()),
              "gcn_propagate")
    return out


class _GCNPropagate(torch.autograd.Function):
    """The normalised edge pass is a symmetric operator in h: d h is the same kernel over the plan of the source ids (tag 0 of the
    same edge_index object) with the forward's dis / lw; d bias is the column sum of the output gradient."""

    @staticmethod
    def forward(ctx, h, bias, edge_index, w, num_nodes, fill_value):
        dis, lw = _gcn_degree(edge_index, w, num_nodes, fill_value)
        out = _gcn_launch(h, edge_index, w, dis, lw, bias, num_nodes, False)
        ctx.num_nodes = num_nodes
        ctx.save_for_backward(edge_index, dis, lw, *((w,) if w is not None else ()))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        edge_index, dis, lw, *rest = ctx.saved_tensors
        w = rest[0] if rest else None
        need_h, need_bias = ctx.needs_input_grad[:2]
        # as _EdgeAttention.backward: rows of unit column stride are read in place (pitch 0 = one row for all), the rest is copied
        g = grad_out if grad_out.dim() == 2 and (grad_out.stride(1) == 1 or grad_out.size(1) == 1) else grad_out.contiguous()
        d_h = _gcn_launch(g, edge_index, w, dis, lw, None, ctx.num_nodes, True) if need_h else None
        d_bias = grad_out.sum(dim=0) if need_bias else None
        return d_h, d_bias, None, None, None, None


def gcn_propagate(h, edge_index, edge_weight, num_nodes, fill_value=1.0, bias=None):
    """out = D^-1/2 (A + L) D^-1/2 h (+ bias): GCNConv's normalised aggregation (torch_geometric's add_remaining_self_loops +
    gcn_norm + propagate) in two launches, without rewriting the edge list. L is diagonal: the weight of a node's last self loop
    in edge order, ``fill_value`` for a node without one; A holds the other edges (j -> i) = (edge_index[0], edge_index[1]) with
    ``edge_weight`` [E] (``None``: ones); D is the row sum of A + L, D^-1/2 = 0 where that is not positive. h [num_nodes, K] may be a
    column block. Differentiable in h and bias; an ``edge_weight`` that requires grad raises."""
    _require_gpu(h, edge_index, edge_weight, bias)
    if edge_weight is not None and torch.is_grad_enabled() and edge_weight.requires_grad:
        raise NotImplementedError("gnnops.conv.gcn_propagate: edge_weight requires grad, but the normalised edge pass has no backward "
                                  "for its weights (differentiable in h and bias only); detach edge_weight")
    if h.dim() != 2 or h.size(0) != num_nodes:
        raise RuntimeError("gcn_propagate: h must be [num_nodes, K]")
    if bias is not None and (bias.dtype != h.dtype or bias.numel() != h.size(1)):
        raise RuntimeError("gcn_propagate: bias must hold K entries of h's dtype")
    _dtype_code(h, "gcn_propagate")
    w = None
    if edge_weight is not None:
        if edge_weight.numel() != edge_index.size(1):
            raise RuntimeError("gcn_propagate: edge_weight has one entry per edge")
        w = edge_weight.detach().reshape(-1).to(torch.float32).contiguous()
    bias_c = bias.contiguous() if bias is not None else None
    if _wants_grad(h, bias):
        return _GCNPropagate.apply(h, bias_c, edge_index, w, num_nodes, float(fill_value))
    dis, lw = _gcn_degree(edge_index, w, num_nodes, fill_value)
    return _gcn_launch(h, edge_index, w, dis, lw, bias_c, num_nodes, False)


class GCNConv(_Layer):
    """x' = D^-1/2 (A + fill I) D^-1/2 x W^T + bias (Kipf & Welling 2017; torch_geometric 2.0.2 GCNConv — the layer the reference's
    GraphUNetREG is built from, graph_benchmark/models/ptg_models.py): one dense product and `gcn_propagate`. ``improved=True`` makes
    the self-loop weight 2. Parameter names and shapes follow PyG (``lin.weight`` [out, in], ``bias`` [out]; glorot / zeros) so a
    state_dict moves across; torch_geometric is not available to compare against: parity unpinned. ``cached=True``,
    ``normalize=False`` and ``add_self_loops=False`` are not implemented."""

    def __init__(self, in_channels, out_channels, improved=False, cached=False, add_self_loops=True, normalize=True, bias=True):
        super().__init__()
        if cached or not add_self_loops or not normalize:
            raise NotImplementedError("gnnops.conv.GCNConv: cached=True, add_self_loops=False and normalize=False are not implemented")
        self.in_channels, self.out_channels, self.improved = in_channels, out_channels, improved
        self.lin = torch.nn.Linear(in_channels, out_channels, bias=False)
        self.bias = torch.nn.Parameter(torch.zeros(out_channels)) if bias else None
        torch.nn.init.xavier_uniform_(self.lin.weight)
        self._pk = _Packed()

    def forward(self, x, edge_index, edge_weight=None):
        _require_gpu(x, edge_index, edge_weight)
        h = _dense(x.contiguous(), self._pk.get([self.lin.weight], [(self.lin.weight, None)]))
        return gcn_propagate(h, edge_index, edge_weight, x.size(0), 2.0 if self.improved else 1.0, self.bias)


class TopKPooling(torch.nn.Module):
    """torch_geometric 2.0.2 TopKPooling (Gao & Ji 2019) without ``min_score``: score = nonlinearity(x . weight / |weight|), the
    ceil(ratio * n) best nodes of every graph are kept (`gnnops.pool.topk`), x = x[perm] * score[perm] * multiplier, and the
    edge list is cut down to the kept nodes and relabelled (`gnnops.pool.filter_adj`). ``weight`` [1, in_channels] as in PyG;
    parity unpinned. The score is formed in float32 whatever x's dtype, so the selection does not hang on 16-bit rounding; the
    gather is the package's differentiable index_select, so gradients reach x and weight. Two host reads (the two result sizes)."""

    def __init__(self, in_channels, ratio=0.5, min_score=None, multiplier=1.0, nonlinearity=torch.tanh):
        super().__init__()
        if min_score is not None:
            raise NotImplementedError("gnnops.conv.TopKPooling: min_score is not supported")
        self.in_channels, self.ratio, self.multiplier, self.nonlinearity = in_channels, ratio, multiplier, nonlinearity
        self.weight = torch.nn.Parameter(torch.empty(1, in_channels))
        bound = 1.0 / (in_channels ** 0.5)
        torch.nn.init.uniform_(self.weight, -bound, bound)

    def forward(self, x, edge_index, edge_attr=None, batch=None, num_graphs=None):
        from . import autograd, pool

        _require_gpu(x, edge_index, edge_attr, batch)
        n = x.size(0)
        w = self.weight.float()
        score = self.nonlinearity((x.float() * w).sum(dim=-1) / w.norm(p=2, dim=-1))
        perm = pool.topk(score, self.ratio, batch, num_graphs)
        kept = autograd.index_select(score.to(x.dtype).view(-1, 1), 0, perm)
        out = autograd.index_select(x, 0, perm) * kept
        if self.multiplier != 1:
            out = self.multiplier * out
        if batch is None:
            batch = edge_index.new_zeros(n)
        edge_index, edge_attr = pool.filter_adj(edge_index, edge_attr, perm, num_nodes=n)
        return out, edge_index, edge_attr, batch[perm], perm, kept.view(-1)


class GraphUNet(torch.nn.Module):
    """torch_geometric.nn.models.GraphUNet (2.0.2; Gao & Ji 2019 — the reference's GraphUNetREG, graph_benchmark/models/ptg_models.py):
    ``depth`` levels of GCNConv(improved=True) + TopKPooling on the squared adjacency going down, unpooling with a residual (sum, or
    concatenation with ``sum_res=False``) going up. Submodule names ``down_convs``, ``pools``, ``up_convs`` and the forward order are
    PyG's, so a state_dict moves across; torch_geometric is not available to compare against: parity unpinned. `augment_adj` is
    remove_self_loops, one unit self loop per node, `gnnops.spspmm(..., method="auto")` of the matrix with itself (coalesced row-major, which
    is what sort_edge_index + spspmm give upstream) and remove_self_loops again; unpooling ``up[perm] = x`` is the package's
    differentiable scatter. Edge weights are float32 at every level, whatever x's dtype. The pooled levels' edge lists are new
    tensors on every forward, so only level 0's plans are cached across calls; inside one call a level's plans serve its down conv,
    its up conv and their backward. ``num_graphs`` spares the host read of ``batch.max()``."""

    def __init__(self, in_channels, hidden_channels, out_channels, depth, pool_ratios=0.5, sum_res=True, act=torch.relu):
        super().__init__()
        if depth < 1:
            raise ValueError("GraphUNet: depth >= 1")
        self.in_channels, self.hidden_channels, self.out_channels, self.depth = in_channels, hidden_channels, out_channels, depth
        self.pool_ratios = list(pool_ratios) if isinstance(pool_ratios, (list, tuple)) else [pool_ratios] * depth
        self.act, self.sum_res = act, sum_res
        channels = hidden_channels
        self.down_convs = torch.nn.ModuleList([GCNConv(in_channels, channels, improved=True)])
        self.pools = torch.nn.ModuleList()
        for i in range(depth):
            self.pools.append(TopKPooling(channels, self.pool_ratios[i]))
            self.down_convs.append(GCNConv(channels, channels, improved=True))
        up_in = channels if sum_res else 2 * channels
        self.up_convs = torch.nn.ModuleList([GCNConv(up_in, channels, improved=True) for _ in range(depth - 1)])
        self.up_convs.append(GCNConv(up_in, out_channels, improved=True))

    @staticmethod
    def augment_adj(edge_index, edge_weight, num_nodes, method="auto"):
        from . import pool
        from .sparse import spspmm

        edge_index, edge_weight = pool.remove_self_loops(edge_index, edge_weight)
        loops = torch.arange(num_nodes, dtype=edge_index.dtype, device=edge_index.device)
        edge_index = torch.cat([edge_index, torch.stack([loops, loops])], dim=1)
        edge_weight = torch.cat([edge_weight, edge_weight.new_ones(num_nodes)])
        # "auto": row-wise with on-chip accumulators when no entry is stored twice and the graphs fit the window (the pooled
        # levels always are repeat-free: a coalesced product, filtered), expand - sort - compress otherwise; same bits either way
        edge_index, edge_weight = spspmm(edge_index, edge_weight, edge_index, edge_weight, num_nodes, num_nodes, num_nodes,
                                         method=method)
        return pool.remove_self_loops(edge_index, edge_weight)

    def forward(self, x, edge_index, batch=None, num_graphs=None, return_perms=False):
        from . import autograd

        _require_gpu(x, edge_index, batch)
        if batch is None:
            batch, num_graphs = edge_index.new_zeros(x.size(0)), 1
        edge_weight = torch.ones(edge_index.size(1), dtype=torch.float32, device=x.device)
        x = self.act(self.down_convs[0](x, edge_index, edge_weight))
        xs, edge_indices, edge_weights, perms = [x], [edge_index], [edge_weight], []
        for i in range(1, self.depth + 1):
            edge_index, edge_weight = self.augment_adj(edge_index, edge_weight, x.size(0))
            x, edge_index, edge_weight, batch, perm, _ = self.pools[i - 1](x, edge_index, edge_weight, batch, num_graphs)
            edge_index, edge_weight = edge_index.contiguous(), edge_weight.contiguous()   # one object per level: its plans are built once
            x = self.act(self.down_convs[i](x, edge_index, edge_weight))
            if i < self.depth:
                xs.append(x)
                edge_indices.append(edge_index)
                edge_weights.append(edge_weight)
            perms.append(perm)
        for i in range(self.depth):
            j = self.depth - 1 - i
            res, perm = xs[j], perms[j]
            up = autograd.scatter(x, perm, 0, None, res.size(0), "sum")   # up[perm] = x: perm holds distinct ids
            x = res + up if self.sum_res else torch.cat((res, up), dim=-1)
            x = self.up_convs[i](x, edge_indices[j], edge_weights[j])
            if i < self.depth - 1:
                x = self.act(x)
        return (x, perms) if return_perms else x


# ---- per-type weights: HeteroLinear and RGCNConv on the grouped product (csrc/segment_matmul.hip) --------------------------------
def _sorted_by_type(type_vec, num_types, is_sorted):
    """(sorted types, the stable permutation that sorts them or None, int64 ptr [num_types + 1] on the device)."""
    from . import segment, sparse

    if type_vec.dtype != torch.int64 or type_vec.dim() != 1:
        raise RuntimeError(f"expected a 1-D int64 type vector, got {type_vec.dtype} with {type_vec.dim()} dims")
    perm = None
    if not is_sorted:
        type_vec, perm = sparse.sort(type_vec, stable=True)
    return type_vec, perm, segment.rowptr_from_sorted(type_vec, num_types).to(torch.int64)


class HeteroLinear(_Layer):
    """torch_geometric HeteroLinear: out_i = x_i @ weight[type_i] + bias[type_i]. ``weight`` [num_types, in, out], ``bias``
    [num_types, out], ``forward(x, type_vec)`` as in PyG (glorot / zeros). Rows are brought into type order by a stable sort
    (skipped with ``is_sorted=True``), multiplied by one grouped launch (`gnnops.segment_matmul`) and put back; the inverse
    permutation is the sort of the permutation. torch_geometric is not available to compare against: parity unpinned."""

    def __init__(self, in_channels, out_channels, num_types, is_sorted=False, bias=True):
        super().__init__()
        self.in_channels, self.out_channels, self.num_types, self.is_sorted = in_channels, out_channels, num_types, is_sorted
        self.weight = torch.nn.Parameter(torch.empty(num_types, in_channels, out_channels))
        self.bias = torch.nn.Parameter(torch.zeros(num_types, out_channels)) if bias else None
        for w in self.weight:
            torch.nn.init.xavier_uniform_(w)

    def forward(self, x, type_vec):
        from . import autograd, sparse

        _require_gpu(x, type_vec)
        if type_vec.numel() != x.size(0):
            raise RuntimeError(f"HeteroLinear: {x.size(0)} rows but {type_vec.numel()} types")
        _, perm, ptr = _sorted_by_type(type_vec, self.num_types, self.is_sorted)
        if perm is not None:
            x = autograd.index_select(x, 0, perm)
        out = autograd.segment_matmul(x.contiguous(), ptr, self.weight, self.bias)
        if perm is not None:
            out = autograd.index_select(out, 0, sparse.sort(perm)[1])
        return out


class RGCNConv(_Layer):
    """torch_geometric RGCNConv (Schlichtkrull et al. 2018): out_i = x_i @ root + bias + sum_r aggr_{j in N_r(i)} x_j @ W_r, with
    aggr = "mean" (the sum over the edges of relation r into i divided by their number) or "sum". Parameters as in PyG:
    ``weight`` [num_relations, in, out] — with ``num_bases``: ``weight`` [num_bases, in, out] and ``comp`` [num_relations,
    num_bases], W = comp @ weight (a torch op) — ``root`` [in, out], ``bias`` [out]; glorot / zeros.

    One pass of each kind: the edges are sorted by relation (stable; skipped with ``is_sorted=True``), the source rows gathered
    (`index_select`), multiplied by their relation's weight in one grouped launch (`segment_matmul`), and summed into their
    destinations by one sparse product whose values are the factors 1 / |N_r(i)| (`spmm`; the counts come from a scatter over
    the key dst * R + r). The root weight is one more relation whose edges are the self-loops i -> i, with ``bias`` as that
    type's bias row: x @ root + bias goes through the same three launches and no partial result is rounded on the way.
    ``num_blocks`` is not implemented. torch_geometric is not available to compare against: parity unpinned."""

    def __init__(self, in_channels, out_channels, num_relations, num_bases=None, aggr="mean", root_weight=True, is_sorted=False,
                 bias=True):
        super().__init__()
        if aggr not in ("mean", "sum", "add"):
            raise NotImplementedError(f"gnnops.conv.RGCNConv: aggr={aggr!r} is not implemented (mean, sum)")
        self.in_channels, self.out_channels, self.num_relations, self.num_bases = in_channels, out_channels, num_relations, num_bases
        self.aggr, self.is_sorted = "sum" if aggr == "add" else aggr, is_sorted
        self.weight = torch.nn.Parameter(torch.empty(num_bases if num_bases else num_relations, in_channels, out_channels))
        self.comp = torch.nn.Parameter(torch.empty(num_relations, num_bases)) if num_bases else None
        self.root = torch.nn.Parameter(torch.empty(in_channels, out_channels)) if root_weight else None
        self.bias = torch.nn.Parameter(torch.zeros(out_channels)) if bias else None
        for w in self.weight:
            torch.nn.init.xavier_uniform_(w)
        for w in (self.comp, self.root):
            if w is not None:
                torch.nn.init.xavier_uniform_(w)

    def forward(self, x, edge_index, edge_type):
        from . import autograd

        _require_gpu(x, edge_index, edge_type)
        if edge_index.dim() != 2 or edge_index.size(0) != 2 or edge_type.numel() != edge_index.size(1):
            raise RuntimeError("RGCNConv: edge_index must be [2, E] and edge_type [E]")
        R, N, E, dev = self.num_relations, x.size(0), edge_index.size(1), x.device
        et, perm, ptr = _sorted_by_type(edge_type, R, self.is_sorted)
        src, dst = (edge_index[0], edge_index[1]) if perm is None else (edge_index[0][perm], edge_index[1][perm])
        weight = self.weight
        if self.comp is not None:
            weight = (self.comp @ weight.reshape(self.num_bases, -1)).view(R, self.in_channels, self.out_channels)
        factor = None
        if self.aggr == "mean":
            key = dst * R + et
            count = ops.scatter(torch.ones(E, dtype=torch.float32, device=dev), key, 0, None, N * R, "sum")
            factor = ops.index_select(count, 0, key).reciprocal_().to(x.dtype)
        bias = None
        if self.root is not None:      # relation R: the self-loops, weight `root`, bias row `bias`
            loops = torch.arange(N, dtype=torch.int64, device=dev)
            src, dst = torch.cat([src, loops]), torch.cat([dst, loops])
            ptr = torch.cat([ptr, ptr.new_full((1,), E + N)])
            weight = torch.cat([weight, self.root.unsqueeze(0)])
            if self.bias is not None:
                bias = torch.cat([self.bias.new_zeros(R, self.out_channels), self.bias.unsqueeze(0)])
            if factor is not None:
                factor = torch.cat([factor, factor.new_ones(N)])
        msg = autograd.segment_matmul(autograd.index_select(x.contiguous(), 0, src), ptr, weight, bias)
        index = torch.stack([dst, torch.arange(msg.size(0), dtype=torch.int64, device=dev)])
        out = autograd.spmm(index, factor, N, msg.size(0), msg)
        if self.root is None and self.bias is not None:
            out = out + self.bias
        return out
