"""The yardstick of the multi-aggregator edge pass in a training loop (gnnops.conv.edge_aggregate, gnnops_edge_multi_grad in
csrc/conv.hip; PNAConv on top of it): the pass restated per edge in propagate order in torch float64 on the CPU — gather p[i],
q[j], w[e]; the message; one reduction by destination per aggregator; the degree scalers as constant factors — so that torch's
own autograd differentiates it.

  sum / mean   index_add_ by destination; a mean divides by max(deg, 1)
  std          sqrt(relu(mean(m^2) - mean(m)^2) + 1e-5), PNAConv.aggregate: torch's relu passes no gradient at 0
  min / max    torch's amin / amax backward splits a tie evenly, which is NOT the rule of this package: the whole gradient goes to
               ONE edge per destination and column, the smallest edge id among the edges that attain the value (the arg rule of
               gnnops.scatter). So they are a ``gather`` at ``arg``, with ``arg`` computed from the same operands (``first_arg``);
               a destination without edges gathers a zero row.
  scalers      identity, amplification log(deg + 1) / avg_log, attenuation avg_log / log(deg + 1), linear deg / avg_lin,
               inverse_linear avg_lin / deg, with deg clamped to >= 1; output blocks scaler-major, then aggregator.

16-bit cases hand it the operands already rounded to the storage type (as conv_chain.inputs does), in float64.
test_pna_chain_cpu.py ties the gradients to torch.autograd.gradcheck and to a hand-worked row with a tie.

Operands of the GPU tests lie on a grid of 1 / 1024 (``grid``): every message p + q + w is then exact in float32 and in float64,
so the kernel and the chain see the same numbers, pick the same arg and find the same ties (conv_chain does the same for the
relu gate of film). ``pna_ref`` is PNAConv (PyG 2.0.2 definitions: parity unpinned) on this pass."""
import torch

AGGREGATORS = ("sum", "mean", "min", "max", "std")
SCALERS = ("identity", "amplification", "attenuation", "linear", "inverse_linear")


def grid(g, *shape, top=1024):
    """Uniform on {-1, ..., 1} in steps of 1 / top, float32."""
    return torch.randint(-top, top + 1, shape, generator=g).float() / top


def first_arg(m, dst, n_dst, largest):
    """[n_dst, K] int64: per destination and column the smallest edge id among the edges whose message attains the min (max);
    E for a destination without edges."""
    E, K = m.shape
    index = dst.view(-1, 1).expand(E, K)
    init = torch.full((n_dst, K), float("-inf") if largest else float("inf"), dtype=m.dtype)
    best = init.scatter_reduce(0, index, m.detach(), "amax" if largest else "amin", include_self=True)
    ids = torch.arange(E).view(-1, 1).expand(E, K)
    ids = torch.where(m.detach() == best[dst], ids, torch.full_like(ids, E))
    return torch.full((n_dst, K), E, dtype=torch.int64).scatter_reduce(0, index, ids, "amin", include_self=True)


def scaler_factors(dst, n_dst, scalers, avg_deg, dtype=torch.float64):
    deg = torch.bincount(dst, minlength=n_dst).clamp(min=1).to(dtype).unsqueeze(1)
    logd = torch.log(deg + 1)
    avg_log, avg_lin = (1.0, 1.0) if avg_deg is None else (avg_deg["log"], avg_deg["lin"])
    fac = {"identity": torch.ones_like(deg), "amplification": logd / avg_log, "attenuation": avg_log / logd, "linear": deg / avg_lin,
           "inverse_linear": avg_lin / deg}
    return [fac[s] for s in scalers]


def aggregate_messages(m, dst, n_dst, aggr, scalers=(), avg_deg=None):
    """m [E, K] per-edge messages -> [n_dst, max(S, 1) * A * K]."""
    E, K = m.shape
    deg = torch.bincount(dst, minlength=n_dst).clamp(min=1).to(m.dtype).unsqueeze(1)
    total = torch.zeros((n_dst, K), dtype=m.dtype).index_add_(0, dst, m)
    mean = total / deg
    padded = torch.cat([m, torch.zeros((1, K), dtype=m.dtype)])     # row E: what a destination without edges gathers
    blocks = []
    for a in aggr:
        if a in ("sum", "add"):
            blocks.append(total)
        elif a == "mean":
            blocks.append(mean)
        elif a in ("min", "max"):
            blocks.append(padded.gather(0, first_arg(m, dst, n_dst, a == "max")))
        elif a == "std":
            sq = torch.zeros((n_dst, K), dtype=m.dtype).index_add_(0, dst, m * m) / deg
            blocks.append(torch.sqrt(torch.relu(sq - mean * mean) + 1e-5))
        else:
            raise ValueError(a)
    out = torch.cat(blocks, dim=1)
    if scalers:
        out = torch.cat([out * f for f in scaler_factors(dst, n_dst, scalers, avg_deg, m.dtype)], dim=1)
    return out


def edge_aggregate(functor, q, edge_index, n_dst, p=None, w=None, aggr=("mean", "min", "max", "std"), scalers=(), avg_deg=None):
    """gnnops.conv.edge_aggregate restated; the dtype of q is the arithmetic."""
    src, dst = edge_index[0], edge_index[1]
    if functor == "copy":
        m = q[src]
    else:
        m = p[dst] + q[src]
        if w is not None:
            m = m + w
    return aggregate_messages(m, dst, n_dst, aggr, scalers, avg_deg)


def aggregate_grads(functor, ops, edge_index, n_dst, aggr, scalers, avg_deg, R):
    """ops: {"q", "p", "w": float64 tensor or None}. (out, {name: d sum(out * R)}) by torch autograd of the float64 chain."""
    leaf = {k: (v.detach().double().clone().requires_grad_(True) if v is not None else None) for k, v in ops.items()}
    out = edge_aggregate(functor, leaf["q"], edge_index, n_dst, p=leaf["p"], w=leaf["w"], aggr=aggr, scalers=scalers, avg_deg=avg_deg)
    (out * R.double()).sum().backward()
    return out.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items() if v is not None}


def pna_ref(P, ei, n, cfg, aggr, scalers, avg_deg, x, ea=None):
    """PNAConv in propagate order on float64 parameters P (names of gnnops.conv.PNAConv / PyG); cfg: towers, divide, pre, post."""
    T = cfg["towers"]
    F = x.size(1) // T if cfg["divide"] else x.size(1)
    src, dst = ei

    def mlp(name, z, layers):
        z = z @ P[f"{name}.0.weight"].t() + P[f"{name}.0.bias"]
        for li in range(1, layers):
            z = torch.relu(z) @ P[f"{name}.{2 * li}.weight"].t() + P[f"{name}.{2 * li}.bias"]
        return z

    xt = x.view(n, T, F) if cfg["divide"] else x.view(n, 1, F).expand(n, T, F)
    en = ea @ P["edge_encoder.weight"].t() + P["edge_encoder.bias"] if ea is not None else None
    outs = []
    for t in range(T):
        xin = xt[:, t]
        m = mlp(f"pre_nns.{t}", torch.cat([xin[dst], xin[src]] + ([en] if en is not None else []), -1), cfg["pre"])
        out = aggregate_messages(m, dst, n, aggr, scalers, avg_deg)
        outs.append(mlp(f"post_nns.{t}", torch.cat([xin, out], -1), cfg["post"]))
    return torch.cat(outs, -1) @ P["lin.weight"].t() + P["lin.bias"]
