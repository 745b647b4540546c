"""ops.matmul_tn(a, b) (csrc/gemm_tn.hip: a^T @ b split along the long dimension) against the route it replaces in the weight
gradients, ops.matmul(transpose_contiguous(a), b) (in row blocks of 64 * 65535 where the transpose copy needs them), and against torch.mm(a.t(), b).

Sweep: R in {10^4, 10^5, 10^6, 6 * 10^6} x (P, Q) in {(1, 128), (8, 8), (8, 128), (11, 2048), (64, 256), (128, 1024), (512, 512)} x
fp32 / fp16 / bf16. The three implementations alternate inside one process; every figure is the median [min .. max] of --samples
samples, each enough calls between two device events to last --window-ms (one call where a call is longer). Every (dtype, R) block
runs in a process of its own under its own time limit, so a block that hangs costs that block only. Beside the new route's time stands
the rate at which it moves its operands, R * (P + Q) elements over the whole call (both stages; stage 2 reads slabs * P * Q * 4 bytes
of partials on top), next to the copy ceiling bench.py quotes (6290 GB/s measured, 8000 GB/s specified).

ops.matmul_tn_preferred is set from the table this writes: true only where the new route's median is below the old route's minimum
at the point and at its recorded neighbours. No pass bar: the record is the deliverable.

  python tools/time_matmul_tn.py [--samples 7] [--window-ms 30] [--block-timeout 300] [--out profiles/matmul_tn.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (10_000, 100_000, 1_000_000, 6_000_000)
WIDTHS = ((1, 128), (8, 8), (8, 128), (11, 2048), (64, 256), (128, 1024), (512, 512))
DTYPES = (("fp32", "float32"), ("fp16", "float16"), ("bf16", "bfloat16"))
MAX_ROWS = 64 * 65535
COPY_CEILING_GBS, SPEC_GBS = 6290.0, 8000.0     # bench.py: HBM_PEAK_GBS and the measured copy ceiling beside it


def sample(runs, samples, window_ms):
    import torch

    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps, times = {}, {k: [] for k in runs}
    for k, fn in runs.items():
        fn()
        s.record()
        fn()
        t.record()
        torch.cuda.synchronize()
        reps[k] = max(1, min(200, int(window_ms / max(s.elapsed_time(t), 1e-3))))
    for _ in range(samples):
        for k, fn in runs.items():
            s.record()
            for _ in range(reps[k]):
                fn()
            t.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(t) / reps[k])
    return times


def block(args):
    """One (dtype, R) block: a JSON line per (P, Q)."""
    sys.path.insert(0, os.path.join(ROOT, "gnn-ops-benchmark_amd"))
    import torch

    import gnnops
    from gnnops import ops
    from gnnops.sparse import transpose_contiguous

    if not torch.cuda.is_available():
        raise SystemExit("time_matmul_tn.py needs a GPU: nothing is measured without one")
    gnnops.load_library()
    dtype, R = getattr(torch, args.dtype), args.rows
    g = torch.Generator(device="cuda").manual_seed(7)
    for P, Q in WIDTHS:
        a = (torch.rand(R, P, generator=g, device="cuda") - 0.5).to(dtype)
        b = (torch.rand(R, Q, generator=g, device="cuda") - 0.5).to(dtype)

        def old():      # the transpose copy stops at 64 * 65535 rows: beyond, row blocks added in float32 as conv._EdgeLinear adds them
            if R <= MAX_ROWS:
                return ops.matmul(transpose_contiguous(a), b)
            parts = [ops.matmul(transpose_contiguous(a[k:k + MAX_ROWS]), b[k:k + MAX_ROWS]).float() for k in range(0, R, MAX_ROWS)]
            return sum(parts[1:], parts[0]).to(dtype)

        runs = {"tn": lambda: ops.matmul_tn(a, b), "old": old, "torch": lambda: torch.mm(a.t(), b)}
        times = sample(runs, args.samples, args.window_ms)
        err = {k: float("nan") for k in runs}
        if R * (P + Q) <= 3 * 10 ** 9:      # the float64 copies of larger operands are not worth their memory
            ref = a.double().t() @ b.double()
            err = {k: float((fn().double() - ref).abs().max() / ref.abs().max()) for k, fn in runs.items()}
        print(json.dumps({"dtype": args.dtype, "R": R, "P": P, "Q": Q, "times": times, "err": err,
                          "geometry": ops.matmul_tn_geometry(R, P, Q, dtype)}), flush=True)
        del a, b


def fmt(v):
    return f"{statistics.median(v):9.4f} [{min(v):9.4f} .. {max(v):9.4f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--block-timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matmul_tn.txt"))
    ap.add_argument("--block", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--dtype", default="float32", help=argparse.SUPPRESS)
    ap.add_argument("--rows", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.block:
        return block(args)
    lines = [f"ops.matmul_tn(a [R,P], b [R,Q]) against ops.matmul(transpose_contiguous(a), b) (the weight gradients' route before it) and "
             f"torch.mm(a.t(), b): ms per call, median [min .. max] of {args.samples} samples, the three alternating in one process.",
             f"tn GB/s = R * (P + Q) elements over the whole call (both stages); copy ceiling {COPY_CEILING_GBS:.0f} GB/s measured, {SPEC_GBS:.0f} GB/s specified (bench.py).",
             "ahead = tn median < old minimum. err = max |got - float64| / max |float64|.", ""]
    for name, tname in DTYPES:
        for R in ROWS:
            cmd = [sys.executable, os.path.abspath(__file__), "--block", "--dtype", tname, "--rows", str(R), "--samples", str(args.samples),
                   "--window-ms", str(args.window_ms)]
            try:
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.block_timeout)
            except subprocess.TimeoutExpired:
                lines.append(f"{name} R={R}: the block ran past {args.block_timeout} s; nothing recorded, and nothing further is started")
                break
            if res.returncode != 0:
                lines.append(f"{name} R={R}: the block failed with status {res.returncode}; nothing further is started\n{res.stderr[-2000:]}")
                open(args.out, "w").write("\n".join(lines) + "\n")
                raise SystemExit(res.returncode)
            lines.append(f"{name}  R = {R}")
            lines.append(f"  {'P':>4} {'Q':>5} {'slabs':>5} | {'tn ms':^33} | {'old ms':^33} | {'torch.mm ms':^33} | tn GB/s  of ceiling | ahead | err tn / old")
            for row in res.stdout.strip().splitlines():
                r = json.loads(row)
                t, es = r["times"], 4 if tname == "float32" else 2
                gbs = r["R"] * (r["P"] + r["Q"]) * es / statistics.median(t["tn"]) / 1e6
                ahead = "yes" if statistics.median(t["tn"]) < min(t["old"]) else "no"
                lines.append(f"  {r['P']:>4} {r['Q']:>5} {r['geometry']['slabs']:>5} | {fmt(t['tn'])} | {fmt(t['old'])} | {fmt(t['torch'])} | "
                             f"{gbs:8.1f}  {100 * gbs / COPY_CEILING_GBS:5.1f} %   | {ahead:>5} | {r['err']['tn']:.1e} / {r['err']['old']:.1e}")
            lines.append("")
            print("\n".join(lines[-(len(WIDTHS) + 3):]), flush=True)
        else:
            continue
        break
    open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
