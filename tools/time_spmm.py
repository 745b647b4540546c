"""Config 3 SpMM (CSR 2M x 2M, nnz 40M, D = 256 and 128 bf16): time spmm_rows_kernel and the bandwidth of its gathers,
then the untiled route against the tiled one (gnnops.spmm_tiles + spmm_csr(..., tiles=plan)) on the three column structures
of bench.py's config-3 leg: uniform, banded_w4096, community_1000_p90.

Per structure: untiled ms, tiled ms (median, min .. max over the repeats; the two routes alternate inside one process, each
repeat is an event-timed batch of `--iters` calls), plan build ms (host clock around a build that ends synchronised),
staged_share, the number of tiled calls that amortise the build, and whether the two results are bit-identical.
`--share-sweep` adds community matrices of falling in-community share, to find the staged_share at which the routes cross.
`--pmc-workload STRUCTURE:ROUTE` runs a few calls of one route only, for a counter pass of its own
(rocprofv3 --pmc FETCH_SIZE -- python tools/time_spmm.py --pmc-workload community_1000_p90:tiled).
usage (GPU box): python tools/time_spmm.py [--repeats 7] [--iters 5] [--share-sweep]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gnn-ops-benchmark_amd"))
import torch

import gnnops

M, NNZ = 2_000_000, 40_000_000


def ev_ms(fn, iters=5):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def csr_rows(g, dev):
    row = torch.randint(0, M, (NNZ,), generator=g, device=dev).sort().values
    rowptr = torch.zeros(M + 1, dtype=torch.int32, device=dev)
    rowptr[1:] = torch.bincount(row, minlength=M).cumsum(0).to(torch.int32)
    return rowptr, row


def community(g, dev, row_of, p):
    """bench.py's community generator with in-community share p (0.9 there): 2000 blocks of 1000 nodes."""
    return torch.where(torch.rand(NNZ, generator=g, device=dev) < p,
                       (row_of // 1000) * 1000 + torch.randint(0, 1000, (NNZ,), generator=g, device=dev),
                       torch.randint(0, M, (NNZ,), generator=g, device=dev))


def columns(name, g, dev, row_of):
    if name == "uniform":
        return torch.randint(0, M, (NNZ,), generator=g, device=dev)
    if name == "banded_w4096":
        return (row_of + torch.randint(-4096, 4097, (NNZ,), generator=g, device=dev)).clamp_(0, M - 1)
    if name.startswith("community_1000_p"):
        return community(g, dev, row_of, int(name[len("community_1000_p"):]) / 100)
    raise ValueError(name)


def spread(xs):
    return f"{statistics.median(xs):.3f} ms ({min(xs):.3f} .. {max(xs):.3f})"


def compare(name, rowptr, col, val, Bm, repeats, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tiles = gnnops.spmm_tiles(rowptr, col)
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    same = torch.equal(gnnops.spmm_csr(rowptr, col, val, Bm), gnnops.spmm_csr(rowptr, col, val, Bm, tiles=tiles))
    plain, tiled = [], []
    for _ in range(repeats):   # alternate the routes: drift of the clock or of the shared host lands on both
        plain.append(ev_ms(lambda: gnnops.spmm_csr(rowptr, col, val, Bm), iters))
        tiled.append(ev_ms(lambda: gnnops.spmm_csr(rowptr, col, val, Bm, tiles=tiles), iters))
    mp, mt = statistics.median(plain), statistics.median(tiled)
    gain = mp - mt
    amortise = f"{build_ms / gain:.0f} tiled calls" if gain > 0 else "never (tiled is not faster)"
    print(f"{name}: untiled {spread(plain)}  tiled {spread(tiled)}  ratio {mp / mt:.3f}x  plan build {build_ms:.1f} ms "
          f"= {amortise}  staged_share {tiles.staged_share:.4f}  R={tiles.block_rows} S={tiles.slots}  "
          f"staged columns {tiles.tile_cols.numel()}  bit-identical {same}", flush=True)
    del tiles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--share-sweep", action="store_true")
    ap.add_argument("--pmc-workload", default=None, metavar="STRUCTURE:ROUTE")
    args = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(42)
    rowptr, row_of = csr_rows(g, dev)
    val = torch.rand(NNZ, generator=g, device=dev).to(torch.bfloat16)
    if args.pmc_workload:
        name, route = args.pmc_workload.split(":")
        col = columns(name, g, dev, row_of)
        Bm = torch.rand(M, 256, generator=g, device=dev).to(torch.bfloat16)
        tiles = gnnops.spmm_tiles(rowptr, col) if route == "tiled" else None
        for _ in range(3):
            gnnops.spmm_csr(rowptr, col, val, Bm, tiles=tiles)
        torch.cuda.synchronize()
        print("done", name, route)
        return
    col = columns("uniform", g, dev, row_of)
    for D in (256, 128):
        Bm = torch.rand(M, D, generator=g, device=dev).to(torch.bfloat16)
        ms = ev_ms(lambda: gnnops.spmm_csr(rowptr, col, val, Bm))
        print(f"D={D}: {ms:.3f} ms  gathered {NNZ * D * 2 / ms / 1e6:.0f} GB/s", flush=True)
        del Bm
    Bm = torch.rand(M, 256, generator=g, device=dev).to(torch.bfloat16)
    print(f"untiled vs tiled, D=256 bf16, {args.repeats} repeats of {args.iters} calls each, alternating:", flush=True)
    names = ["uniform", "banded_w4096", "community_1000_p90"]
    if args.share_sweep:
        names += ["community_1000_p70", "community_1000_p50", "community_1000_p30", "community_1000_p15"]
    for name in names:
        if name != "uniform":
            col = columns(name, g, dev, row_of)
        compare(name, rowptr, col, val, Bm, args.repeats, args.iters)
        del col


if __name__ == "__main__":
    main()
