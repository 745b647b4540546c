"""SpMM with max / mean reduce (gnnops.spmm_reduce, csrc/spmm_reduce.hip) against the chain it replaces, at N = 1M rows,
nnz = 10M uniform, D = 128, fp32 and bf16; forward, and forward + backward (d value and d matrix).

Three legs, alternating inside one process (drift of the clock or of a shared host lands on all of them); each repeat is an
event-timed batch of `--iters` calls after one untimed call, the line shows median (min .. max) over the repeats:
  fused    gnnops.spmm_reduce(rowptr, col, value, x, reduce)                                     no [nnz, D] tensor exists
  chain    gnnops.index_select(x, 0, col) * value[:, None] -> gnnops.scatter(.., row, reduce)    this package's own ops, plans warm
  stock    x.index_select(0, col) * value[:, None] -> Tensor.scatter_reduce / index_add_         stock torch ops
Before timing, the fused forward is compared with the chain's once (max-relative distance printed). `index` is the [2, nnz]
(row, col) tensor a SparseTensor keeps: with it the backward of a mean finds the plan of `col` in the cache, as the chain's does.
usage (GPU box): python tools/time_spmm_reduce.py [--repeats 5] [--iters 3] [--rows 1000000] [--nnz 10000000] [--dim 128]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnn-ops-benchmark_amd"))
import torch

import gnnops


def ev_ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def spread(xs):
    return f"{statistics.median(xs):9.3f} ms ({min(xs):.3f} .. {max(xs):.3f})"


def legs(rowptr, row, col, index, value, x, reduce, M):
    def fused():   # index: the [2, nnz] tensor a SparseTensor keeps, so the backward of a mean finds its plan in the cache
        r = gnnops.spmm_reduce(rowptr, col, value, x, reduce, index=index)
        return r[0] if isinstance(r, tuple) else r

    def chain():
        r = gnnops.scatter(gnnops.index_select(x, 0, col) * value.unsqueeze(1), row, 0, None, M, reduce)
        return r[0] if isinstance(r, tuple) else r

    ix = row.unsqueeze(1).expand(-1, x.size(1))

    def stock():
        src = x.index_select(0, col) * value.unsqueeze(1)
        out = torch.zeros((M, x.size(1)), dtype=x.dtype, device=x.device)
        if reduce == "max":
            return out.scatter_reduce(0, ix, src, "amax", include_self=False)
        return out.scatter_reduce(0, ix, src, "mean", include_self=False)

    return {"fused": fused, "chain": chain, "stock": stock}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--nnz", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU only"
    dev = torch.device("cuda")
    M, NNZ, D = args.rows, args.nnz, args.dim
    g = torch.Generator(device=dev).manual_seed(42)
    row = torch.randint(0, M, (NNZ,), generator=g, device=dev).sort().values
    rowptr = torch.zeros(M + 1, dtype=torch.int32, device=dev)
    rowptr[1:] = torch.bincount(row, minlength=M).cumsum(0).to(torch.int32)
    col = torch.randint(0, M, (NNZ,), generator=g, device=dev)
    index = torch.stack([row, col])
    print(f"{torch.cuda.get_device_name(0)}: M = N = {M}, nnz = {NNZ} uniform, D = {D}; {args.repeats} repeats of {args.iters} calls, legs alternating",
          flush=True)
    for dtype in (torch.float32, torch.bfloat16):
        value0 = (torch.rand(NNZ, generator=g, device=dev) + 0.5).to(dtype)
        x0 = torch.randn(M, D, generator=g, device=dev).to(dtype)
        R = torch.randn(M, D, generator=g, device=dev).to(dtype)
        for reduce in ("max", "mean"):
            with torch.no_grad():
                outs = {k: f() for k, f in legs(rowptr, row, col, index, value0, x0, reduce, M).items() if k != "stock"}
            scale = float(outs["chain"].float().abs().max())
            print(f"{str(dtype)[6:]} {reduce}: forward, fused vs chain, max |diff| / max |out|: "
                  f"{float((outs['fused'].float() - outs['chain'].float()).abs().max()) / scale:.2e}", flush=True)
            del outs
            for mode in ("forward", "forward+backward"):
                train = mode != "forward"
                value, x = value0.clone().requires_grad_(train), x0.clone().requires_grad_(train)
                fns = legs(rowptr, row, col, index, value, x, reduce, M)

                def step(f):
                    if not train:
                        with torch.no_grad():
                            return f()
                    value.grad = x.grad = None
                    (f() * R).sum().backward()

                times = {k: [] for k in fns}
                for _ in range(args.repeats):
                    for k, f in list(fns.items()):
                        try:
                            times[k].append(ev_ms(lambda f=f: step(f), args.iters))
                        except (RuntimeError, NotImplementedError) as e:     # a leg torch cannot run in this dtype is reported, not hidden
                            print(f"{str(dtype)[6:]} {reduce} {mode}: leg {k} does not run: {str(e).splitlines()[0][:160]}", flush=True)
                            times[k] = [float("nan")]
                            del fns[k]
                med = {k: statistics.median(v) for k, v in times.items()}
                print(f"{str(dtype)[6:]:>8} {reduce:>4} {mode:<16}  fused {spread(times['fused'])}  chain {spread(times['chain'])}  "
                      f"stock {spread(times['stock'])}  chain/fused {med['chain'] / med['fused']:.2f}x  stock/fused {med['stock'] / med['fused']:.2f}x",
                      flush=True)
                del fns, value, x
        del value0, x0, R


if __name__ == "__main__":
    main()
