"""AttentiveFP and its two attention layers: the fused layers (gnnops.conv.GATConv / GATEConv: one product, one attention edge
pass, csrc/attention.hip gate_fwd_kernel / gate_bwd_kernel) against the same layers written as the unfused chain on this package's
own differentiable ops — index_select per edge, leaky ReLU and the per-head dot product, scatter_softmax, multiply, scatter_add —
with the SAME parameters, forward and forward + backward, fp32 and bf16.

  model   AttentiveFP at the reference's profiled shape: 64 graphs of about 1000 nodes, average degree 10, hidden 512, 4 layers,
          5 timesteps, edge_dim 1 (64 input channels, dropout 0 so that both sides compute the same function)
  layers  single GATConv(128, 32, heads=4) and GATEConv(128, 128, edge_dim=1) layers at N = 1M, E = 5M, uniform endpoints

The implementations alternate inside one process, every (implementation, mode) is warmed first, each sample is enough calls between
two device events to last tens of milliseconds, and the table gives the median and the spread over the samples. The unfused chain
keeps its index tensors across calls, so its plans are cached exactly as the fused layers' are. No pass bar: the record is the
deliverable. Beside each layer: the algorithmic bytes of the fused edge passes.

  python tools/time_attentive_fp.py [--samples S] [--skip-model] [--skip-layers] [--out profiles/attentive_fp.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gnn-ops-benchmark_amd")]
import torch  # noqa: E402

import gnnops  # noqa: E402
from gnnops import autograd as ad, conv  # noqa: E402

F = torch.nn.functional


def _softmax_sum(rows, s, dst, n, H):
    alpha = gnnops.scatter_softmax(s, dst, dim=0, dim_size=n)                       # [E, H]
    C = rows.size(1) // H
    return ad.scatter((rows.view(-1, H, C) * alpha.unsqueeze(-1)).view(-1, H * C), dst, 0, None, n, "sum")


def unfused_gat(layer, x, src, dst, n_dst):
    """GATConv as the chain on this package's ops; x is a tensor or the bipartite pair."""
    H, C = layer.heads, layer.out_channels
    xs, xd = x if isinstance(x, (tuple, list)) else (x, x)
    ql = ad.matmul(xs, layer.lin_src.weight.t().contiguous())
    qr = ql if xd is xs else ad.matmul(xd, layer.lin_dst.weight.t().contiguous())
    a_src = (ql.view(-1, H, C) * layer.att_src).sum(-1)                             # [N, H]
    a_dst = (qr.view(-1, H, C) * layer.att_dst).sum(-1)
    xj = ad.index_select(ql, 0, src)                                                # [E, H * C]
    s = F.leaky_relu(ad.index_select(a_src, 0, src) + ad.index_select(a_dst, 0, dst), layer.negative_slope)
    out = _softmax_sum(xj, s, dst, n_dst, H)
    out = out if layer.concat else out.view(n_dst, H, C).mean(dim=1)
    return out if layer.bias is None else out + layer.bias


def unfused_gate(layer, x, src, dst, ea):
    cin = layer.in_channels
    w1 = layer.lin1.weight
    q = ad.matmul(x, w1[:, :cin].t().contiguous())
    # not ad.matmul: its backward copies the transpose of the left operand, which stops at 64 * 65535 rows (E = 5M is past it)
    u = conv._EdgeLinear.apply(ea, w1[:, cin:].t().contiguous())
    xj = F.leaky_relu(ad.index_select(q, 0, src) + u, 0.01)                         # [E, out]
    a_i = ad.matmul(x, layer.att_r.t().contiguous())                                # [N, 1]
    s = F.leaky_relu((xj * layer.att_l).sum(-1, keepdim=True) + ad.index_select(a_i, 0, dst), 0.01)
    agg = _softmax_sum(xj, s, dst, x.size(0), 1)
    return ad.addmm(layer.bias, agg, layer.lin2.weight.t().contiguous())


def unfused_model(m, x, ei, ea, batch, G, to_mol):
    x = F.leaky_relu(m.lin1(x))
    for k, (c, gru) in enumerate(zip(m.atom_convs, m.atom_grus)):
        h = F.elu(unfused_gate(c, x, ei[0], ei[1], ea) if k == 0 else unfused_gat(c, x, ei[0], ei[1], x.size(0)))
        x = gru(h, x).relu()
    out = ad.scatter(x, batch, 0, None, G, "sum").relu()
    for _ in range(m.num_timesteps):
        h = F.elu(unfused_gat(m.mol_conv, (x, out), to_mol[0], to_mol[1], G))
        out = m.mol_gru(h, out).relu()
    return m.lin2(out)


def measure(runs, samples, window_ms):
    """runs: {key: callable}. {key: (list of ms per call, calls per sample)}; the runs alternate inside every sample."""
    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps, times = {}, {k: [] for k in runs}
    for k, fn in runs.items():      # warm every shape (code objects, plans, allocator), then size the sample's window
        fn()
        fn()
        s.record()
        fn()
        t.record()
        torch.cuda.synchronize()
        reps[k] = max(2, min(200, int(window_ms / max(s.elapsed_time(t), 1e-3)) + 1))
    for _ in range(samples):
        for k, fn in runs.items():
            s.record()
            for _ in range(reps[k]):
                fn()
            t.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(t) / reps[k])
    return {k: (times[k], reps[k]) for k in runs}


def report(lines, res):
    for mode in ("forward", "forward + backward"):
        med = {}
        for impl in ("fused", "unfused"):
            v, reps = res[(mode, impl)]
            med[impl] = statistics.median(v)
            lines.append(f"  {mode:19s} {impl:8s} {med[impl]:9.3f} ms  [{min(v):.3f} .. {max(v):.3f}]  ({reps} calls per sample)")
        lines.append(f"  {mode:19s} unfused / fused = {med['unfused'] / med['fused']:.2f}")


def pair(fused, unfused, params, x, coef):
    """The four timed callables of one (fused, unfused) pair taking the input that requires grad."""
    def fwd(fn):
        with torch.no_grad():
            fn(x)

    def fwd_bwd(fn):
        for p in params:
            p.grad = None
        xg = x.detach().requires_grad_(True)
        (fn(xg) * coef).sum().backward()

    return {("forward", "fused"): lambda: fwd(fused), ("forward", "unfused"): lambda: fwd(unfused),
            ("forward + backward", "fused"): lambda: fwd_bwd(fused), ("forward + backward", "unfused"): lambda: fwd_bwd(unfused)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=60.0, help="a sample repeats its call until about this long")
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=5_000_000)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-layers", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_attentive_fp.py needs a GPU: nothing is measured without one")
    gnnops.load_library()
    g = torch.Generator(device="cuda").manual_seed(5)
    rel = lambda a, b: float((a.float() - b.float()).abs().max() / b.float().abs().max())   # noqa: E731
    lines = [f"AttentiveFP, GATConv and GATEConv on {torch.cuda.get_device_name(0)}: fused layers against the unfused chain on the package's ops",
             f"ms per call: median [min .. max] of {args.samples} samples, each of enough calls for ~{args.window_ms:.0f} ms; the implementations "
             "alternate in one process; plans cached on both sides", ""]
    for dtype, name, es in ((torch.float32, "fp32", 4), (torch.bfloat16, "bf16", 2)):
        if not args.skip_model:
            graphs, per, deg, hidden = 64, 1000, 10, 512
            n = graphs * per
            batch = torch.arange(graphs, device="cuda").repeat_interleave(per)
            src = torch.randint(0, per, (n * deg,), generator=g, device="cuda")
            dst = torch.randint(0, n, (n * deg,), generator=g, device="cuda")
            ei = torch.stack([src + dst // per * per, dst])                          # every edge inside its graph
            ea = torch.rand(ei.size(1), 1, generator=g, device="cuda").to(dtype)
            x = (torch.rand(n, 64, generator=g, device="cuda") - 0.5).to(dtype)
            to_mol = torch.stack([torch.arange(n, device="cuda"), batch])
            torch.manual_seed(0)
            model = conv.AttentiveFP(64, hidden, 1, edge_dim=1, num_layers=4, num_timesteps=5).to(dtype).cuda()
            fused = lambda xx: model(xx, ei, ea, batch, num_graphs=graphs)   # noqa: E731
            unfused = lambda xx: unfused_model(model, xx, ei, ea, batch, graphs, to_mol)   # noqa: E731
            with torch.no_grad():
                diff = rel(fused(x), unfused(x))
            coef = (torch.rand(graphs, 1, generator=g, device="cuda") - 0.5).to(dtype)
            res = measure(pair(fused, unfused, list(model.parameters()), x, coef), args.samples, args.window_ms)
            lines.append(f"{name} model: AttentiveFP(64, 512, 1, edge_dim=1, num_layers=4, num_timesteps=5), {graphs} graphs x {per} nodes, "
                         f"E = {ei.size(1)}; fused against unfused output {diff:.2e}")
            report(lines, res)
            lines.append("")
            del model, x, ea, ei, to_mol
        if not args.skip_layers:
            n, e = args.nodes, args.edges
            ei = torch.randint(0, n, (2, e), generator=g, device="cuda")
            src, dst = ei[0].contiguous(), ei[1].contiguous()
            x = (torch.rand(n, 128, generator=g, device="cuda") - 0.5).to(dtype)
            ea = torch.rand(e, 1, generator=g, device="cuda").to(dtype)
            coef = (torch.rand(n, 128, generator=g, device="cuda") - 0.5).to(dtype)
            torch.manual_seed(0)
            gat = conv.GATConv(128, 32, heads=4, add_self_loops=False).to(dtype).cuda()
            gate = conv.GATEConv(128, 128, edge_dim=1).to(dtype).cuda()
            HC, H = 128, 4
            for label, layer, fused, unfused, fw_bytes, bw_bytes in (
                ("GATConv(128, 32, heads=4, add_self_loops=False)", gat, lambda xx: gat(xx, ei), lambda xx: unfused_gat(gat, xx, src, dst, n),
                 e * (HC * es + 8) + n * (HC * es + H * es + 4 * H),
                 e * (2 * HC * es + 12) + n * (2 * HC * es + 2 * H * es + 4 * H)),
                ("GATEConv(128, 128, edge_dim=1)", gate, lambda xx: gate(xx, ei, ea), lambda xx: unfused_gate(gate, xx, src, dst, ea),
                 e * (2 * HC * es + 12) + n * (HC * es + es + 4),
                 e * (3 * HC * es + 12) + n * (2 * HC * es + 2 * es + 4)),
            ):
                with torch.no_grad():
                    diff = rel(fused(x), unfused(x))
                res = measure(pair(fused, unfused, list(layer.parameters()), x, coef), args.samples, args.window_ms)
                lines.append(f"{name} layer: {label}, N = {n}, E = {e}; fused against unfused output {diff:.2e}")
                lines.append(f"  algorithmic bytes of the fused edge pass: forward {fw_bytes / 1e6:.0f} MB (gathered q rows, ids"
                             f"{', u rows' if layer is gate else ''}, out, d, lse), backward {bw_bytes / 1e6:.0f} MB (the same reads, g and out rows, gq written; "
                             "the segment sum of gq by source comes on top)")
                report(lines, res)
                lines.append("")
            del gat, gate, x, ea, coef, ei, src, dst
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
