"""Float64 restatement of the per-type products: gnnops.segment_matmul, gnnops.conv.HeteroLinear and gnnops.conv.RGCNConv.

Plain torch on the CPU, written the way the library computes (rows in type order, one product per segment, one weighted sum into the
destinations), differentiable, so the GPU tests compare forward values and gradients against it. tests/test_hetero_chain_cpu.py pins it
against a second formulation that shares none of this code — a per-row loop x[i] @ W[type[i]] and per-relation dense adjacency
products — and pins its gradients with torch.autograd.gradcheck.

``rd``: what the library materialises in the storage type on the way (the weights combined from bases, the per-edge messages, the
root rows and the factors 1 / |N_r(i)| of RGCNConv) is passed through it; `straight_through(dtype)` rounds the value and lets the gradient pass, None keeps
everything in the chain's own precision."""
import math

import torch

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
DNAME = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
MANTISSA = {torch.float32: 23, torch.float16: 10, torch.bfloat16: 7}


def straight_through(dtype):
    return lambda t: t if dtype == torch.float32 else t + (t.to(dtype).to(t.dtype) - t).detach()


def ulp_rel(scale, dtype):
    """One unit in the last place of the dtype at |value| = scale, as a fraction of scale."""
    return 2.0 ** (math.floor(math.log2(scale)) - MANTISSA[dtype]) / scale


def metric(got, ref):
    """max |got - ref| / max |ref|."""
    if ref.numel() == 0:
        return 0.0
    return float((got.double() - ref.double()).abs().max()) / max(float(ref.abs().max()), 1e-30)


def bar(single, ref, dtype):
    """4 x the metric of `single` (the same computation in float32 on the CPU, rounded once to the dtype), at least 4 units in the
    last place of the dtype at max |ref|: the bar of tests/test_matmul_tn_gpu.py."""
    return 4 * max(metric(single, ref), ulp_rel(max(float(ref.abs().max()), 1e-30), dtype))


def ptr_of(lengths):
    ptr = [0]
    for n in lengths:
        ptr.append(ptr[-1] + n)
    return torch.tensor(ptr, dtype=torch.int64)


def segment_matmul_ref(x, ptr, weight, bias=None):
    """out[ptr[t] : ptr[t+1]] = x[ptr[t] : ptr[t+1]] @ weight[t] (+ bias[t]); ptr a list or an int64 tensor that covers every row."""
    ptr = [int(v) for v in ptr]
    pieces = []
    for t in range(weight.size(0)):
        y = x[ptr[t]:ptr[t + 1]] @ weight[t]
        pieces.append(y if bias is None else y + bias[t])
    if not pieces:
        return x.new_zeros((x.size(0), weight.size(2)))
    return torch.cat(pieces)


def _sorted_types(type_vec, num_types):
    order = torch.sort(type_vec, stable=True)[1]
    counts = torch.bincount(type_vec, minlength=num_types)
    return order, [0] + counts.cumsum(0).tolist()


def hetero_linear_ref(P, x, type_vec, num_types):
    """P: {"weight": [T, in, out], "bias": [T, out] (optional)}."""
    order, ptr = _sorted_types(type_vec, num_types)
    out_sorted = segment_matmul_ref(x[order], ptr, P["weight"], P.get("bias"))
    inverse = torch.empty_like(order)
    inverse[order] = torch.arange(order.numel())
    return out_sorted[inverse]


def rgcn_ref(P, x, edge_index, edge_type, num_relations, aggr="mean", rd=None):
    """P: {"weight": [R, in, out] or [B, in, out] with "comp" [R, B], "root" [in, out] (optional), "bias" [out] (optional)}."""
    rd = rd or (lambda t: t)
    R, n = num_relations, x.size(0)
    weight = P["weight"]
    if "comp" in P:
        weight = rd((P["comp"] @ weight.reshape(weight.size(0), -1)).view(R, weight.size(1), weight.size(2)))
    order, ptr = _sorted_types(edge_type, R)
    src, dst, et = edge_index[0][order], edge_index[1][order], edge_type[order]
    msg = rd(segment_matmul_ref(x[src], ptr, weight))
    if aggr == "mean":
        key = dst * R + et
        count = torch.bincount(key, minlength=n * R).to(x.dtype)
        msg = msg * rd(1.0 / count[key]).unsqueeze(1)
    out = torch.zeros((n, weight.size(2)), dtype=x.dtype).index_add(0, dst, msg)
    if "root" in P:
        own = x @ P["root"]
        out = out + rd(own + P["bias"] if "bias" in P else own)
    elif "bias" in P:
        out = out + P["bias"]
    return out


# ---- the second formulation: nothing above is used below ------------------------------------------------------------------------
def rowwise_matmul(x, types, weight, bias=None):
    rows = []
    for i in range(x.size(0)):
        t = int(types[i])
        y = x[i] @ weight[t]
        rows.append(y if bias is None else y + bias[t])
    return torch.stack(rows) if rows else x.new_zeros((0, weight.size(2)))


def rgcn_dense(P, x, edge_index, edge_type, num_relations, aggr="mean"):
    """sum_r A_r @ (x @ W_r) with A_r [n, n] the (multi-)adjacency of relation r, its rows divided by their sums for "mean"."""
    n = x.size(0)
    weight = P["weight"]
    if "comp" in P:
        weight = torch.einsum("rb,bio->rio", P["comp"], weight)
    out = torch.zeros((n, weight.size(2)), dtype=x.dtype)
    for r in range(num_relations):
        A = torch.zeros((n, n), dtype=x.dtype)
        for e in range(edge_index.size(1)):
            if int(edge_type[e]) == r:
                A[int(edge_index[1][e]), int(edge_index[0][e])] += 1
        if aggr == "mean":
            A = A / A.sum(1, keepdim=True).clamp(min=1)
        out = out + A @ (x @ weight[r])
    if "root" in P:
        out = out + x @ P["root"]
    if "bias" in P:
        out = out + P["bias"]
    return out


# ---- cases the CPU and the GPU tests share ----------------------------------------------------------------------------------------
def graph(seed, n, e, num_relations):
    """(edge_index [2, e], edge_type [e]) in no order, with node 3 without an incoming edge, relation 1 without an edge, and the
    first edge four times."""
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, n, (e,), generator=g)
    dst = torch.randint(0, n, (e,), generator=g)
    et = torch.randint(0, num_relations, (e,), generator=g)
    if n > 4:
        dst[dst == 3] = 4
    if num_relations > 2:
        et[et == 1] = 2
    if e > 8:
        src[1:4], dst[1:4], et[1:4] = src[0], dst[0], et[0]
    return torch.stack([src, dst]), et


def rgcn_params(seed, cin, cout, num_relations, num_bases, root_weight, bias, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)

    def rand(*shape):
        return ((torch.rand(*shape, generator=g) * 2 - 1) / math.sqrt(shape[-2] if len(shape) > 1 else 1)).to(dtype)

    P = {"weight": rand(num_bases or num_relations, cin, cout)}
    if num_bases:
        P["comp"] = rand(num_relations, num_bases)
    if root_weight:
        P["root"] = rand(cin, cout)
    if bias:
        P["bias"] = rand(cout)
    return P
