"""The GATv2 model's epilogue (gnnops.conv.head_act_norm, csrc/norm.hip: mean over heads + bias + ReLU + dropout mask + LayerNorm in
one row pass) against the SAME computation on stock torch ops (mean, +, relu, the mask multiply, F.layer_norm), and the model
(gnnops.conv.GATv2, 2 layers, hidden 128, heads 4) against the same model with only the epilogue and the pool swapped for stock
torch ops (the attention passes are this package's on both sides).

  epilogue  N = 100 000, H in {1, 4}, C = 128, fp32 / fp16 / bf16, forward and forward + backward
  model     one graph of 100 000 nodes and 64 graphs of 1000 nodes (5 edges per node inside each graph), forward (eval) and train
            step (forward + backward, dropout 0.3, the mask drawn per call on both sides)

The implementations alternate inside one process, every (implementation, mode) is warmed first, each sample is enough calls between
two device events to last tens of milliseconds, and the table gives the median and the spread over the samples. No pass bar: the
record is the deliverable.

  python tools/time_gatv2_model.py [--rows N] [--samples S] [--out profiles/gatv2_model.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gnn-ops-benchmark_amd")]
import torch  # noqa: E402

import gnnops  # noqa: E402
from gnnops import conv  # noqa: E402

F = torch.nn.functional


def stock_epilogue(a, H, bias, k, gamma, beta):
    y = a.view(a.size(0), H, -1).mean(dim=1) + bias
    y = torch.relu(y)
    if k is not None:
        y = y * k
    return y if gamma is None else F.layer_norm(y, (y.size(1),), gamma, beta, 1e-5)


def stock_model(model, x, edge_index, batch, G):
    """gnnops.conv.GATv2.forward with the epilogue and the pool on stock torch ops."""
    for k in range(model.num_layers):
        c = model.convs[k]
        a = c._attend(x, edge_index)
        scale = conv._feature_scale(a.size(0), c.out_channels, model.dropout, a.dtype, a.device) if model.training and model.dropout > 0 else None
        ln = model.lns[k] if k != model.num_layers - 1 else None
        x = stock_epilogue(a, c.heads, c.bias, scale, None if ln is None else ln.weight, None if ln is None else ln.bias)
    pooled = torch.zeros((G, x.size(1)), dtype=x.dtype, device=x.device).index_add_(0, batch, x)
    pooled = pooled / torch.bincount(batch, minlength=G).clamp(min=1).to(x.dtype).unsqueeze(1)
    return model.post_mp(pooled)


def measure(runs, samples, window_ms):
    """{key: (median, min, max, calls per sample)} of ms per call; the keys alternate inside every sample."""
    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps, times = {}, {k: [] for k in runs}
    for k, fn in runs.items():
        fn()
        fn()
        s.record()
        fn()
        t.record()
        torch.cuda.synchronize()
        reps[k] = max(3, min(500, int(window_ms / max(s.elapsed_time(t), 1e-3)) + 1))
    for _ in range(samples):
        for k, fn in runs.items():
            s.record()
            for _ in range(reps[k]):
                fn()
            t.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(t) / reps[k])
    return {k: (statistics.median(v), min(v), max(v), reps[k]) for k, v in times.items()}


def report(lines, res, modes):
    for mode in modes:
        for impl in ("fused", "stock"):
            med, lo, hi, reps = res[(mode, impl)]
            lines.append(f"  {mode:19s} {impl:6s} {med:9.4f} ms  [{lo:.4f} .. {hi:.4f}]  ({reps} calls per sample)")
        lines.append(f"  {mode:19s} stock / fused = {res[(mode, 'stock')][0] / res[(mode, 'fused')][0]:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=40.0, help="a sample repeats its call until about this long")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_gatv2_model.py needs a GPU: nothing is measured without one")
    gnnops.load_library()
    n, C = args.rows, 128
    g = torch.Generator(device="cuda").manual_seed(5)
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "gfx950").split(":")[0]
    lines = [f"head_act_norm and gnnops.conv.GATv2 on {torch.cuda.get_device_name(0)} ({arch}: the name torch reports for an MI355X)",
             f"ms per call: median [min .. max] of {args.samples} samples, each of enough calls for ~{args.window_ms:.0f} ms; the implementations "
             "alternate in one process", "fused: gnnops.conv.head_act_norm / gnnops.pool.global_mean_pool; stock: mean, +, relu, *, F.layer_norm / index_add_", ""]
    modes = ("forward", "forward + backward")
    for dtype, name in ((torch.float32, "fp32"), (torch.float16, "fp16"), (torch.bfloat16, "bf16")):
        for H in (1, 4):
            a = (torch.rand(n, H * C, generator=g, device="cuda") - 0.5).to(dtype)
            vec = [(torch.rand(C, generator=g, device="cuda") + 0.5).to(dtype).requires_grad_(True) for _ in range(3)]
            k = conv._feature_scale(n, C, 0.3, dtype, a.device)
            coef = (torch.rand(n, C, generator=g, device="cuda") - 0.5).to(dtype)
            fused = lambda aa: conv.head_act_norm(aa, H, vec[0], True, k, vec[1], vec[2])   # noqa: E731
            stock = lambda aa: stock_epilogue(aa, H, vec[0], k, vec[1], vec[2])             # noqa: E731
            with torch.no_grad():
                x_, y_ = fused(a).float(), stock(a).float()
                diff = float((x_ - y_).abs().max() / y_.abs().max())

            def fwd(fn):
                with torch.no_grad():
                    fn(a)

            def fwd_bwd(fn):
                for v in vec:
                    v.grad = None
                ag = a.detach().requires_grad_(True)
                (fn(ag) * coef).sum().backward()

            runs = {("forward", "fused"): lambda: fwd(fused), ("forward", "stock"): lambda: fwd(stock),
                    ("forward + backward", "fused"): lambda: fwd_bwd(fused), ("forward + backward", "stock"): lambda: fwd_bwd(stock)}
            res = measure(runs, args.samples, args.window_ms)
            lines.append(f"epilogue {name} N = {n}, H = {H}, C = {C}: fused against stock output, max |a - b| / max |b| = {diff:.2e}")
            report(lines, res, modes)
            lines.append("")
    for graphs, per in ((1, n), (64, 1000)):
        N = graphs * per
        batch = torch.arange(graphs, device="cuda").repeat_interleave(per)
        ei = torch.randint(0, per, (2, 5 * N), generator=g, device="cuda") + batch.repeat_interleave(5).unsqueeze(0) * per
        for dtype, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            torch.manual_seed(0)
            model = conv.GATv2(64, C, 0.3, 2, 4).to(dtype).cuda()
            x = (torch.rand(N, 64, generator=g, device="cuda") - 0.5).to(dtype)
            coef = (torch.rand(graphs, 1, generator=g, device="cuda") - 0.5).to(dtype)
            model.eval()
            with torch.no_grad():
                x_, y_ = model(x, ei, batch, graphs).float(), stock_model(model, x, ei, batch, graphs).float()
                diff = float((x_ - y_).abs().max() / y_.abs().max())

            def fwd(fn):
                model.eval()
                with torch.no_grad():
                    fn()

            def step(fn):
                model.train()
                model.zero_grad(set_to_none=True)
                (fn() * coef).sum().backward()

            fused = lambda: model(x, ei, batch, graphs)                    # noqa: E731
            stock = lambda: stock_model(model, x, ei, batch, graphs)       # noqa: E731
            runs = {("forward", "fused"): lambda: fwd(fused), ("forward", "stock"): lambda: fwd(stock),
                    ("train step", "fused"): lambda: step(fused), ("train step", "stock"): lambda: step(stock)}
            res = measure(runs, args.samples, args.window_ms)
            lines.append(f"model {name} GATv2(64, 128, 0.3, 2, heads=4), {graphs} graph(s) x {per} nodes, E = {5 * N} (+ self loops): "
                         f"fused against stock eval output, max |a - b| / max |b| = {diff:.2e}")
            report(lines, res, ("forward", "train step"))
            lines.append("")
            del model, x
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
