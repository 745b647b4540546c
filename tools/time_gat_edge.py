"""GATv2Conv and GATConv with edge features (edge_dim): the fused layers (one product per operand, one attention edge pass,
csrc/attention.hip) against the same computation as a per-edge chain on stock torch ops — index_select of the projections per edge,
the edge product, leaky ReLU, the per-head dot product, a softmax per destination by scatter_reduce / index_add_, multiply and
index_add_ — with the SAME parameters, forward and one train step (forward + backward). Both sides rebuild the self loops'
attributes (fill_value="mean") in every call; both keep the augmented edge list across calls.

A second section times the forward of both layers WITHOUT edge_dim — the path this change must not slow — on this tree and, with
--parent-tree, on a checkout of the parent commit (its package directory with its library built): the parent is run in a fresh
process before and after this tree's run, so the two parent runs show the run-to-run spread the comparison has to be read against.

The graph and shapes are those of tools/time_gat.py (profiles/gatv2.txt): uniform random endpoints, N = 1M, E = 5M, 64 input channels,
4 heads x 32 channels, fp32 and bf16; edge_dim = 8. Every (implementation, mode) is warmed first, the implementations alternate
inside one process, each sample is enough calls between two device events to last tens of milliseconds, and the table gives the
median and the spread over the samples. No pass bar: the record is the deliverable.

  python tools/time_gat_edge.py [--nodes N] [--edges E] [--samples S] [--parent-tree DIR] [--out profiles/gat_edge.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (("fp32", "float32"), ("bf16", "bfloat16"))
EDGE_DIM = 8


def chain(layer, kind, x, src, dst, kept, kept_dst, edge_attr):
    """The layer on stock torch ops; (src, dst) hold the self loops already, kept = positions of the input edges that stay."""
    import torch

    n, H, C = x.size(0), layer.heads, layer.out_channels
    rows = edge_attr.index_select(0, kept)
    total = torch.zeros((n, edge_attr.size(1)), dtype=torch.float32, device=x.device).index_add_(0, kept_dst, rows.float())
    count = torch.zeros(n, dtype=torch.float32, device=x.device).index_add_(0, kept_dst, torch.ones_like(kept_dst, dtype=torch.float32))
    ea = torch.cat([rows, (total / count.clamp(min=1).unsqueeze(1)).to(rows.dtype)], dim=0)
    e = torch.nn.functional.linear(ea, layer.lin_edge.weight).view(-1, H, C)
    if kind == "GATv2Conv":
        xl, xr = layer.lin_l(x), layer.lin_r(x)
        xj = xl.index_select(0, src).view(-1, H, C)
        z = torch.nn.functional.leaky_relu(xr.index_select(0, dst).view(-1, H, C) + xj + e, layer.negative_slope)
        s = (z * layer.att).sum(-1)
    else:
        xs = layer.lin_src(x).view(n, H, C)
        a_src, a_dst = (xs * layer.att_src).sum(-1), (xs * layer.att_dst).sum(-1)
        xj = xs.index_select(0, src)
        s = torch.nn.functional.leaky_relu(a_src.index_select(0, src) + a_dst.index_select(0, dst) + (e * layer.att_edge).sum(-1), layer.negative_slope)
    s = s.float()
    idx = dst.unsqueeze(1).expand(-1, H)
    mx = torch.full((n, H), float("-inf"), device=x.device).scatter_reduce(0, idx, s.detach(), "amax", include_self=True)
    ex = torch.exp(s - mx.index_select(0, dst))
    den = torch.zeros((n, H), device=x.device).index_add_(0, dst, ex)
    alpha = (ex / den.index_select(0, dst)).to(x.dtype)
    out = torch.zeros((n, H, C), dtype=x.dtype, device=x.device).index_add_(0, dst, xj * alpha.unsqueeze(-1)).view(n, H * C)
    return out if layer.bias is None else out + layer.bias


def sample(runs, samples, window_ms):
    """{key: (times in ms, calls per sample)}: warm, size each sample's window, then alternate over the keys."""
    import torch

    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps, times = {}, {k: [] for k in runs}
    for k, fn in runs.items():
        fn()
        fn()
        s.record()
        fn()
        t.record()
        torch.cuda.synchronize()
        reps[k] = max(3, min(200, int(window_ms / max(s.elapsed_time(t), 1e-3)) + 1))
    for _ in range(samples):
        for k, fn in runs.items():
            s.record()
            for _ in range(reps[k]):
                fn()
            t.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(t) / reps[k])
    return {k: (times[k], reps[k]) for k in runs}


def fmt(v):
    return f"{statistics.median(v):9.3f} ms  [{min(v):.3f} .. {max(v):.3f}]"


def setup(args):
    import torch

    import gnnops

    if not torch.cuda.is_available():
        raise SystemExit("time_gat_edge.py needs a GPU: nothing is measured without one")
    gnnops.load_library()
    g = torch.Generator(device="cuda").manual_seed(5)
    ei = torch.randint(0, args.nodes, (2, args.edges), generator=g, device="cuda")
    return torch, g, ei


def plain_forward(args):
    """The no-edge_dim forward of both layers on whatever package sys.path holds: {"layer dtype": [ms per sample]}."""
    torch, g, ei = setup(args)
    from gnnops import conv

    out = {}
    for name, tname in DTYPES:
        dtype = getattr(torch, tname)
        x = (torch.rand(args.nodes, 64, generator=g, device="cuda") - 0.5).to(dtype)
        runs = {}
        for kind in ("GATv2Conv", "GATConv"):
            torch.manual_seed(0)
            layer = getattr(conv, kind)(64, 32, heads=4).to(dtype).cuda()

            def fwd(layer=layer):
                with torch.no_grad():
                    layer(x, ei)

            runs[f"{kind} {name}"] = fwd
        for k, (v, _) in sample(runs, args.samples, args.window_ms).items():
            out[k] = v
    return out


def run_parent(args):
    env = dict(os.environ, GNNOPS_TIME_TREE=os.path.abspath(args.parent_tree))
    cmd = [sys.executable, os.path.abspath(__file__), "--plain-only", "--nodes", str(args.nodes), "--edges", str(args.edges),
           "--samples", str(args.samples), "--window-ms", str(args.window_ms)]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if res.returncode != 0:
        raise SystemExit(f"the parent tree's run failed:\n{res.stdout}\n{res.stderr}")
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=5_000_000)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=60.0, help="a sample repeats its call until about this long")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--plain-only", action="store_true", help="print the no-edge_dim forward samples as one JSON line and stop")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tree = os.environ.get("GNNOPS_TIME_TREE", ROOT)
    sys.path[:0] = [os.path.join(tree, "gnn-ops-benchmark_amd")]
    if args.plain_only:
        print(json.dumps(plain_forward(args)))
        return
    before = run_parent(args) if args.parent_tree else None      # fresh processes: two versions of one package cannot share one
    torch, g, ei = setup(args)
    from gnnops import conv

    n, e = args.nodes, args.edges
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "gfx950").split(":")[0]
    lines = [f"GATv2Conv / GATConv (64, 32, heads=4, edge_dim={EDGE_DIM}, fill_value='mean') on {torch.cuda.get_device_name(0)} ({arch}): "
             f"N = {n}, E = {e} (+ {n} self loops), uniform endpoints",
             f"ms per call: median [min .. max] of {args.samples} samples, each of enough calls for ~{args.window_ms:.0f} ms; the implementations "
             "alternate in one process", "stock chain: the same computation per edge on torch's own ops, the augmented edge list kept across calls", ""]
    for name, tname in DTYPES:
        dtype = getattr(torch, tname)
        x = (torch.rand(n, 64, generator=g, device="cuda") - 0.5).to(dtype)
        ea = (torch.rand(e, EDGE_DIM, generator=g, device="cuda") - 0.5).to(dtype)
        coef = (torch.rand(n, 128, generator=g, device="cuda") - 0.5).to(dtype)
        for kind in ("GATv2Conv", "GATConv"):
            torch.manual_seed(0)
            layer = getattr(conv, kind)(64, 32, heads=4, edge_dim=EDGE_DIM).to(dtype).cuda()
            with torch.no_grad():
                looped = layer._with_self_loops(ei, n)
                src, dst = looped[0].contiguous(), looped[1].contiguous()
                kept = layer._kept_edges(ei)
                kept_dst = ei[1].index_select(0, kept)
                a, b = layer(x, ei, ea).float(), chain(layer, kind, x, src, dst, kept, kept_dst, ea).float()
                diff = float((a - b).abs().max() / b.abs().max())
                del a, b

            def fwd(fn):
                with torch.no_grad():
                    fn(x, ea)

            def step(fn, layer=layer):
                layer.zero_grad(set_to_none=True)
                xg, eg = x.detach().requires_grad_(True), ea.detach().requires_grad_(True)
                (fn(xg, eg) * coef).sum().backward()

            fused = lambda xx, ee, layer=layer: layer(xx, ei, ee)   # noqa: E731
            stock = lambda xx, ee, layer=layer, kind=kind: chain(layer, kind, xx, src, dst, kept, kept_dst, ee)   # noqa: E731
            runs = {("forward", "fused"): lambda: fwd(fused), ("forward", "stock chain"): lambda: fwd(stock),
                    ("train step", "fused"): lambda: step(fused), ("train step", "stock chain"): lambda: step(stock)}
            res = sample(runs, args.samples, args.window_ms)
            lines.append(f"{kind} {name}: fused against stock output, max |a - b| / max |b| = {diff:.2e}")
            for mode in ("forward", "train step"):
                med = {}
                for impl in ("fused", "stock chain"):
                    v, reps = res[(mode, impl)]
                    med[impl] = statistics.median(v)
                    lines.append(f"  {mode:11s} {impl:12s} {fmt(v)}  ({reps} calls per sample)")
                lines.append(f"  {mode:11s} stock / fused = {med['stock chain'] / med['fused']:.2f}")
            lines.append("")
            del layer
            torch.cuda.empty_cache()
        del x, ea, coef
    lines.append("forward WITHOUT edge_dim (the path of the parent commit), ms per call" +
                 (": the parent tree in a fresh process before and after this tree's run" if args.parent_tree else " (no parent tree given)"))
    here = plain_forward(args)
    torch.cuda.empty_cache()
    after = run_parent(args) if args.parent_tree else None
    for k, v in here.items():
        lines.append(f"  {k:15s} this tree        {fmt(v)}")
        if before is not None:
            lines.append(f"  {k:15s} parent (before)  {fmt(before[k])}")
            lines.append(f"  {k:15s} parent (after)   {fmt(after[k])}")
            lo = min(statistics.median(before[k]), statistics.median(after[k]), min(before[k]), min(after[k]))
            hi = max(statistics.median(before[k]), statistics.median(after[k]), max(before[k]), max(after[k]))
            m = statistics.median(v)
            where = "below (faster than)" if m < lo else "inside" if m <= hi else "ABOVE (slower than)"
            lines.append(f"  {k:15s} this tree's median is {where} the parent's recorded spread [{lo:.3f} .. {hi:.3f}]")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
