"""GATv2Conv: the fused layer (gnnops.conv.GATv2Conv: one product, one attention edge pass, csrc/attention.hip) against the unfused
chain a user had to write on this package's own differentiable ops — index_select of both projections per edge, leaky ReLU and
the per-head dot product, scatter_softmax, multiply and scatter_add — with the SAME parameters, forward and forward + backward.

One graph of BASELINE config 2's kind (uniform random endpoints, 5 edges per node) scaled to fit the chain's per-edge tensors:
N = 1M, E = 5M, 64 input channels, 4 heads x 32 channels (rows of 128), fp16 and fp32. The chain is timed twice: with its index
tensors kept across calls, so that its plans are cached exactly as the fused layer's are ("unfused"), and with fresh index tensors
per call, which rebuilds a destination plan in every forward and a source plan in every backward ("unfused, plans rebuilt"). The
implementations alternate inside one process, every (implementation, mode) is warmed first, each sample is enough calls between two
device events to last tens of milliseconds, and the table gives the median and the spread over the samples. No pass bar: the
record is the deliverable.

  python tools/time_gat.py [--nodes N] [--edges E] [--samples S] [--out profiles/gatv2.txt]
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


def unfused(layer, x, src, dst):
    """The chain on this package's ops; (src, dst) already hold the layer's self loops. The plans of scatter_softmax / scatter /
    the index_select backward are cached under the index tensor OBJECTS: the caller keeps src and dst alive across calls and the
    chain's plans hit like the fused layer's do; fresh objects per call rebuild them (a sort of E ids) every call."""
    n, H, C = x.size(0), layer.heads, layer.out_channels
    xl = ad.addmm(layer.lin_l.bias, x, layer.lin_l.weight.t().contiguous())
    xr = ad.addmm(layer.lin_r.bias, x, layer.lin_r.weight.t().contiguous())
    xj = ad.index_select(xl, 0, src)                                               # [E, H * C]
    z = torch.nn.functional.leaky_relu(ad.index_select(xr, 0, dst) + xj, layer.negative_slope)
    s = (z.view(-1, H, C) * layer.att).sum(-1)                                     # [E, H]
    alpha = gnnops.scatter_softmax(s, dst, dim=0, dim_size=n)                      # [E, H]
    out = ad.scatter((xj.view(-1, H, C) * alpha.unsqueeze(-1)).view(-1, H * C), dst, 0, None, n, "sum")
    out = out if layer.concat else out.view(n, H, C).mean(dim=1)
    return out if layer.bias is None else out + layer.bias


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=5_000_000)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=60.0, help="a sample repeats its call until about this long")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_gat.py needs a GPU: nothing is measured without one")
    gnnops.load_library()
    n, e = args.nodes, args.edges
    g = torch.Generator(device="cuda").manual_seed(5)
    ei = torch.randint(0, n, (2, e), generator=g, device="cuda")
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "gfx950").split(":")[0]
    lines = [f"GATv2Conv(64, 32, heads=4) on {torch.cuda.get_device_name(0)} ({arch}: the name torch reports for an MI355X): "
             f"N = {n}, E = {e} (+ {n} self loops), uniform endpoints",
             f"ms per call: median [min .. max] of {args.samples} samples, each of enough calls for ~{args.window_ms:.0f} ms; the implementations "
             "alternate in one process", "unfused: plans cached under its index tensors, like the fused layer's; unfused, plans rebuilt: "
             "fresh index tensors per call", ""]
    for dtype, name in ((torch.float16, "fp16"), (torch.float32, "fp32")):
        torch.manual_seed(0)
        layer = conv.GATv2Conv(64, 32, heads=4).to(dtype).cuda()
        x = (torch.rand(n, 64, generator=g, device="cuda") - 0.5).to(dtype)
        with torch.no_grad():
            looped = layer._with_self_loops(ei, n)
            src, dst = looped[0].contiguous(), looped[1].contiguous()
            a, b = layer(x, ei).float(), unfused(layer, x, src, dst).float()
            diff = float((a - b).abs().max() / b.abs().max())
            del a, b
        coef = (torch.rand(n, 128, generator=g, device="cuda") - 0.5).to(dtype)

        def fwd(fn):
            with torch.no_grad():
                fn()

        def fwd_bwd(fn):
            layer.zero_grad(set_to_none=True)
            xg = x.detach().requires_grad_(True)
            (fn(xg) * coef).sum().backward()

        cold = lambda xx: unfused(layer, xx, looped[0].contiguous(), looped[1].contiguous())   # noqa: E731
        IMPLS = ("fused", "unfused", "unfused, plans rebuilt")
        runs = {
            ("forward", "fused"): lambda: fwd(lambda: layer(x, ei)),
            ("forward", "unfused"): lambda: fwd(lambda: unfused(layer, x, src, dst)),
            ("forward", "unfused, plans rebuilt"): lambda: fwd(lambda: cold(x)),
            ("forward + backward", "fused"): lambda: fwd_bwd(lambda xg: layer(xg, ei)),
            ("forward + backward", "unfused"): lambda: fwd_bwd(lambda xg: unfused(layer, xg, src, dst)),
            ("forward + backward", "unfused, plans rebuilt"): lambda: fwd_bwd(cold),
        }
        times = {k: [] for k in runs}
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = {}
        for k, fn in runs.items():      # warm every shape (code objects, plans, allocator), then size the sample's window
            fn()
            fn()
            s.record()
            fn()
            t.record()
            torch.cuda.synchronize()
            reps[k] = max(3, min(200, int(args.window_ms / max(s.elapsed_time(t), 1e-3)) + 1))
        for _ in range(args.samples):
            for k, fn in runs.items():  # alternate: a drift of the box lands on every side
                s.record()
                for _ in range(reps[k]):
                    fn()
                t.record()
                torch.cuda.synchronize()
                times[k].append(s.elapsed_time(t) / reps[k])
        lines.append(f"{name}: fused against unfused output, max |a - b| / max |b| = {diff:.2e}")
        for mode in ("forward", "forward + backward"):
            med = {}
            for impl in IMPLS:
                v = times[(mode, impl)]
                med[impl] = statistics.median(v)
                lines.append(f"  {mode:19s} {impl:23s} {med[impl]:9.3f} ms  [{min(v):.3f} .. {max(v):.3f}]  ({reps[(mode, impl)]} calls per sample)")
            lines.append(f"  {mode:19s} unfused / fused = {med['unfused'] / med['fused']:.2f}  (plans rebuilt / fused = "
                         f"{med['unfused, plans rebuilt'] / med['fused']:.2f})")
        lines.append("")
        del layer, x, coef, src, dst
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
