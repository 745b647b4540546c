"""gnnops.conv.PNAConv, forward (no_grad) and train step (forward + backward of a linear functional, parameters and input with
gradients), at three points, each in fp32 and fp16:

  app     the app benchmark's layer (app_bm/benchmark_convs.py:197-206): in 1, out 2048, mean / min / max / std x identity /
          amplification / attenuation, so the edge pass runs at K = 1; 20 000 nodes, 10 edges per node
  F64     in 64, out 64, 4 aggregators x 3 scalers, 100 000 nodes, 10 edges per node
  batch   the same layer on 64 graphs of 1000 nodes, 5 edges per node inside each graph

The tool times whatever gnnops package sits next to it, so the same file run from a checkout of another commit gives that commit's
column (profiles/pna_train.txt holds the commit before the fused backward and the commit with it, same box). Every mode is warmed
first, each sample is enough calls between two device events to last tens of milliseconds, and the table gives the median and
the spread over the samples. No pass bar: the record is the deliverable.

  python tools/time_pna_train.py [--samples S] [--out profiles/pna_train.txt]
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

AGGR, SCAL = ["mean", "min", "max", "std"], ["identity", "amplification", "attenuation"]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=40.0, help="a sample repeats its call until about this long")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pna_train.py needs a GPU: nothing is measured without one")
    gnnops.load_library()
    g = torch.Generator(device="cuda").manual_seed(5)
    route = "fused backward (edge_aggregate)" if hasattr(conv, "edge_aggregate") else "propagate-order chain (_forward_train)"
    lines = [f"gnnops.conv.PNAConv on {torch.cuda.get_device_name(0)}; a graph that needs gradients takes: {route}",
             f"ms per call: median [min .. max] of {args.samples} samples, each of enough calls for ~{args.window_ms:.0f} ms", ""]
    points = [("app   in 1, out 2048, N = 20000, E = 200000", 1, 2048, 1, 20_000, 10),
              ("F64   in 64, out 64, N = 100000, E = 1000000", 64, 64, 1, 100_000, 10),
              ("batch in 64, out 64, 64 graphs x 1000 nodes, E = 320000", 64, 64, 64, 1000, 5)]
    for name, cin, cout, graphs, per, fan in points:
        n = graphs * per
        offset = torch.arange(graphs, device="cuda").repeat_interleave(per * fan).unsqueeze(0) * per
        ei = torch.randint(0, per, (2, fan * n), generator=g, device="cuda") + offset
        deg_hist = torch.bincount(torch.bincount(ei[1], minlength=n)).cpu()
        for dtype, dname in ((torch.float32, "fp32"), (torch.float16, "fp16")):
            torch.manual_seed(0)
            layer = conv.PNAConv(cin, cout, AGGR, SCAL, deg_hist).to(dtype).cuda()
            x = (torch.rand(n, cin, generator=g, device="cuda") - 0.5).to(dtype)
            coef = (torch.rand(n, cout, generator=g, device="cuda") - 0.5).to(dtype)

            def fwd():
                with torch.no_grad():
                    layer(x, ei)

            def step():
                layer.zero_grad(set_to_none=True)
                xg = x.detach().requires_grad_(True)
                (layer(xg, ei) * coef).sum().backward()

            res = measure({"forward": fwd, "train step": step}, args.samples, args.window_ms)
            lines.append(f"{name} {dname}")
            for mode in ("forward", "train step"):
                med, lo, hi, reps = res[mode]
                lines.append(f"  {mode:11s} {med:9.4f} ms  [{lo:.4f} .. {hi:.4f}]  ({reps} calls per sample)")
            del layer, x, coef
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
