"""Workload for tools/pmc_gemm_f32.sh: the fp32 GEMM at 8192^3 (the 256 x 256 ping-pong kernel) and the library's kernel,
same operands."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gnn-ops-benchmark_amd"), ROOT]
import torch
import gnnops

L = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
g = torch.Generator(device="cuda").manual_seed(1)
a32, b32, c32 = [torch.rand(L, L, generator=g, device="cuda") * 2 - 1 for _ in range(3)]
for _ in range(4):
    out = gnnops.addmm(c32, a32, b32)
for _ in range(4):
    ref = torch.addmm(c32, a32, b32)
torch.cuda.synchronize()
print("done")
