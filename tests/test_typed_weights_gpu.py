"""gnnops.segment_matmul (csrc/segment_matmul.hip), HeteroLinear and RGCNConv on the GPU.

Exact cases: integer operands from [-4, 4] and K <= 130, so every sum is an integer below 2^24 and the result must equal the int64
product of the CPU converted once, bit for bit, with a different weight per type (a row multiplied by its neighbour's weight shows).
The seams come from segment_matmul_geometry: segment lengths around the row tile, K around the K-step and over load8's four
alignment classes, N around the column tile; one dimension varies against small fixed others, plus the all-largest corner.
Same bits as the GEMM: a segment's rows equal ops.matmul of that slice where the GEMM takes its register-staged kernel.
Random cases, autograd and the layers: max |got - ref| / max |ref| against the float64 chain (tests/hetero_chain.py), bar 4 x the
same metric of the float32 computation of the CPU rounded once (floor: one unit in the last place at max |ref|)."""

import pytest
import torch

import hetero_chain as hc
from helpers import assert_bits_equal, to_np
from hetero_chain import DNAME, DTYPES

pytestmark = pytest.mark.gpu
IDS = [DNAME[d] for d in DTYPES]


@pytest.fixture(scope="module")
def G():
    import gnnops

    gnnops.load_library()
    return gnnops


def _geo(dtype):
    from gnnops import ops

    g = ops.segment_matmul_geometry(dtype)
    return g["tile_m"], g["tile_n"], g["k_step"]


# ---- exact cases ------------------------------------------------------------------------------------------------------------------
def _exact_cases(dtype):
    tm, tn, ks = _geo(dtype)
    seg_lists = [[tm], [1], [0, tm + 1, 0, 0, 1, tm - 1, 0], [0, 0, 2 * tm + 1, 0], [1, tm, tm + 1, 2 * tm + 1, tm - 1, 0, tm],
                 [0, 0, 0], [0], []]
    Ks = [1, 8, 11, ks - 1, ks, ks + 1, 2 * ks + 2]
    Ns = [1, 8, 44, tn - 1, tn, tn + 1]
    assert max(Ks) <= 130
    cases = []
    for lens in seg_lists:
        cases += [(lens, 11, 8), (lens, 8, 44)]
    for K in Ks:
        cases += [([1, tm + 1, 0, 3], K, 8), ([tm + 1, 1], K, 44)]
    for N in Ns:
        cases += [([1, tm + 1, 0, 3], 11, N), ([tm + 1, 1], 8, N)]
    cases.append((seg_lists[4], Ks[-1], Ns[-1]))
    seen, out = set(), []
    for lens, K, N in cases:
        if (tuple(lens), K, N) not in seen:
            seen.add((tuple(lens), K, N))
            out.append((lens, K, N))
    return out


_INTS = {}


def _ints(lens, K, N, seed):
    """Integer operands in [-4, 4] and the int64 result of the CPU, with and without bias: computed once, shared by the dtypes."""
    key = (tuple(lens), K, N, seed)
    if key not in _INTS:
        g = torch.Generator().manual_seed(seed)
        M, T = sum(lens), len(lens)
        x = torch.randint(-4, 5, (M, K), generator=g)
        w = torch.randint(-4, 5, (T, K, N), generator=g)
        b = torch.randint(-4, 5, (T, N), generator=g)
        ptr = hc.ptr_of(lens)
        _INTS[key] = (x, w, b, ptr, hc.segment_matmul_ref(x, ptr, w), hc.segment_matmul_ref(x, ptr, w, b))
    return _INTS[key]


def _place(t, dtype, offset):
    """The tensor on the device, `offset` elements into its allocation and ending flush with it; the head holds 3s, not zeros."""
    buf = torch.full((offset + t.numel(),), 3, dtype=dtype, device="cuda")
    buf[offset:] = t.to(dtype).reshape(-1).cuda()
    return buf[offset:].view(t.shape)


def _run_exact(G, dtype, cases, offset, seed0):
    for n, (lens, K, N) in enumerate(cases):
        x, w, b, ptr, plain, biased = _ints(lens, K, N, seed0 + n)
        with_bias = n % 2 == 1
        dx, dw = _place(x, dtype, offset), _place(w, dtype, offset)
        db = _place(b, dtype, offset) if with_bias else None
        got = G.segment_matmul(dx, ptr if n % 3 else ptr.cuda(), dw, db)
        assert got.dtype == dtype and got.shape == (sum(lens), N)
        want = (biased if with_bias else plain).to(dtype)        # converted once
        assert_bits_equal(to_np(got), to_np(want), f"{DNAME[dtype]} lens={lens} K={K} N={N} bias={with_bias} offset={offset}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_at_every_seam(G, dtype):
    _run_exact(G, dtype, _exact_cases(dtype), 0, 1000)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("offset", [1, 3])
def test_exact_off_the_start_of_the_allocation(G, dtype, offset):
    """Operands that start 1 and 3 elements into their allocation and end flush with it: a read past a row or column bound leaves the
    allocation's own data (3s) instead of zeros and changes the integer result."""
    tm, tn, ks = _geo(dtype)
    cases = [([1, tm + 1, 0, 3], 11, 44), ([tm + 1, 1], 8, 8), ([tm - 1, 0, tm + 1], ks + 1, tn + 1), ([2 * tm + 1], 2 * ks + 2, 44),
             ([0, 5, tm], ks, tn), ([3, 0], 1, 1)]
    _run_exact(G, dtype, cases, offset, 2000 + 100 * offset)


# ---- the GEMM's bits --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("K,N", [(72, 136), (11, 44), (200, 8)])
def test_rows_carry_the_bits_of_the_gemm(G, K, N, dtype):
    """Shapes at which the GEMM plans its register-staged kernel (not all-aligned, N < 512): the same tile body, the same bits."""
    from gnnops import ops

    lens = [300, 0, 129, 1, 128]
    g = torch.Generator().manual_seed(K * 131 + N)
    x = torch.randn(sum(lens), K, generator=g).to(dtype).cuda()
    w = torch.randn(len(lens), K, N, generator=g).to(dtype).cuda()
    b = torch.randn(len(lens), N, generator=g).to(dtype).cuda()
    ptr = hc.ptr_of(lens)
    plain, biased = ops.segment_matmul(x, ptr, w), ops.segment_matmul(x, ptr, w, b)
    for t in range(len(lens)):
        a, e = int(ptr[t]), int(ptr[t + 1])
        if e > a:
            assert torch.equal(plain[a:e], ops.matmul(x[a:e], w[t])), (t, "plain")
            assert torch.equal(biased[a:e], ops.addmm(b[t], x[a:e], w[t])), (t, "bias")


# ---- random operands --------------------------------------------------------------------------------------------------------------
_RANDOM = {}


def _random_case(lens, K, N, dtype):
    key = (tuple(lens), K, N, dtype)
    if key not in _RANDOM:
        g = torch.Generator().manual_seed(K * 4099 + N + len(lens))
        x = torch.randn(sum(lens), K, generator=g).to(dtype)
        w = torch.randn(len(lens), K, N, generator=g).to(dtype)
        b = torch.randn(len(lens), N, generator=g).to(dtype)
        ptr = hc.ptr_of(lens)
        ref = hc.segment_matmul_ref(x.double(), ptr, w.double(), b.double())
        single = hc.segment_matmul_ref(x.float(), ptr, w.float(), b.float()).to(dtype)
        _RANDOM[key] = (x, w, b, ptr, ref, hc.bar(single, ref, dtype))
    return _RANDOM[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("lens,K,N", [([3000, 1], 64, 64), ([257, 0, 1000, 33], 11, 44), ([500, 700], 256, 136)], ids=["3000+1", "odd", "wide"])
def test_random_against_float64(G, lens, K, N, dtype):
    x, w, b, ptr, ref, bar = _random_case(lens, K, N, dtype)
    got = G.segment_matmul(x.cuda(), ptr.cuda(), w.cuda(), b.cuda())
    err = hc.metric(got.cpu(), ref)
    print(f"{DNAME[dtype]} lens={lens} K={K} N={N}: {err:.3e} (bar {bar:.3e})")
    assert err <= bar
    assert torch.equal(G.segment_matmul(x.cuda(), ptr, w.cuda(), b.cuda()), got)      # a CPU ptr: the same bits


# ---- the clamp --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ptr_past_the_end_is_clamped(G, dtype):
    """ptr[-1] > M through the raw ABI: the output is that of the clamped ptr and the guard rows behind `out` keep their values."""
    from gnnops import _lib, ops

    tm = _geo(dtype)[0]
    M, K, N, T, guard = tm + 37, 24, 40, 3, 2 * tm
    g = torch.Generator().manual_seed(77)
    x = torch.randn(M, K, generator=g).to(dtype).cuda()
    w = torch.randn(T, K, N, generator=g).to(dtype).cuda()
    want = ops.segment_matmul(x, torch.tensor([0, 20, 20, M]), w)
    bad = torch.tensor([0, 20, 20, M + tm + 5]).cuda()
    buf = torch.full((M + guard, N), 7.0, dtype=dtype, device="cuda")
    L = _lib.load()
    ws_bytes = L.gnnops_segment_matmul_workspace_bytes(T)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    rc = L.gnnops_segment_matmul(x.data_ptr(), bad.data_ptr(), w.data_ptr(), None, buf.data_ptr(), M, K, N, T, ops._DT[dtype],
                                 ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.OK, L.gnnops_last_error()
    torch.cuda.synchronize()
    assert torch.equal(buf[:M], want)
    assert bool((buf[M:] == 7.0).all()), "rows past M were written"


# ---- autograd ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("lens,gpu_ptr", [([130, 0, 77, 1], True), ([10001, 0, 300], False)], ids=["gpu_ptr", "tall_cpu_ptr"])
def test_autograd_against_float64(G, lens, gpu_ptr, dtype):
    """d x, d W, d bias against the float64 chain; type 1 is empty: its d W is exactly zero. The tall case sends d W[0] through
    ops.matmul_tn (ops.matmul_tn_preferred holds from 10^4 rows on), the others through transpose + GEMM."""
    K, N, T = 11, 44, len(lens)
    g = torch.Generator().manual_seed(41)
    x, w, b = (torch.randn(s, generator=g).to(dtype) for s in ((sum(lens), K), (T, K, N), (T, N)))
    coef = torch.randn(sum(lens), N, generator=g).to(dtype)
    ptr = hc.ptr_of(lens)

    def chain(ftype):
        leaves = [t.to(ftype).clone().requires_grad_(True) for t in (x, w, b)]
        out = hc.segment_matmul_ref(leaves[0], ptr, leaves[1], leaves[2])
        (out * coef.to(ftype)).sum().backward()
        return [out.detach()] + [t.grad for t in leaves]

    want, single = chain(torch.float64), [t.to(dtype) for t in chain(torch.float32)]
    dx, dw, db = (t.cuda().requires_grad_(True) for t in (x, w, b))
    out = G.segment_matmul(dx, ptr.cuda() if gpu_ptr else ptr, dw, db)
    assert out.requires_grad
    (out.float() * coef.cuda().float()).sum().backward()
    assert float(dw.grad[1].abs().max()) == 0.0 and float(db.grad[1].abs().max()) == 0.0
    for name, got, ref, one in zip(("out", "d x", "d W", "d bias"), (out.detach(), dx.grad, dw.grad, db.grad), want, single):
        err, bar = hc.metric(got.cpu(), ref), hc.bar(one, ref, dtype)
        print(f"{DNAME[dtype]} {name}: {err:.3e} (bar {bar:.3e})")
        assert got.dtype == dtype and err <= bar, name


# ---- the layers -------------------------------------------------------------------------------------------------------------------
LAYER_DTYPES = [torch.float32, torch.bfloat16]
LAYER_IDS = ["f32", "bf16"]
N_NODES, N_EDGES, N_REL = 300, 2000, 5


def _compare(names, got, want, single, dtype, what):
    for name, g_, ref, one in zip(names, got, want, single):
        err, bar = hc.metric(g_.detach().cpu(), ref), hc.bar(one, ref, dtype)
        print(f"{what} {DNAME[dtype]} {name}: {err:.3e} (bar {bar:.3e})")
        assert err <= bar, (what, name)


@pytest.mark.parametrize("dtype", LAYER_DTYPES, ids=LAYER_IDS)
@pytest.mark.parametrize("cin,cout", [(11, 44), (64, 64)])
@pytest.mark.parametrize("is_sorted", [False, True], ids=["unsorted", "sorted"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "no_bias"])
def test_hetero_linear_forward_and_backward(G, bias, is_sorted, cin, cout, dtype):
    from gnnops import conv

    torch.manual_seed(5)
    layer = conv.HeteroLinear(cin, cout, N_REL, is_sorted=is_sorted, bias=bias).to(dtype)
    shapes = {"weight": (N_REL, cin, cout)}
    if bias:
        shapes["bias"] = (N_REL, cout)
        with torch.no_grad():
            layer.bias.copy_(torch.randn(N_REL, cout).to(dtype))
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == shapes
    g = torch.Generator().manual_seed(6)
    types = torch.randint(0, N_REL, (N_NODES,), generator=g)
    types[types == 1] = 3                                    # a type without a row
    if is_sorted:
        types = torch.sort(types)[0]
    x, coef = torch.randn(N_NODES, cin, generator=g).to(dtype), torch.randn(N_NODES, cout, generator=g).to(dtype)
    names = sorted(shapes)

    def chain(ftype):
        P = {k: v.detach().to(ftype).clone().requires_grad_(True) for k, v in layer.state_dict().items()}
        xl = x.to(ftype).clone().requires_grad_(True)
        out = hc.hetero_linear_ref(P, xl, types, N_REL)
        (out * coef.to(ftype)).sum().backward()
        return [out.detach(), xl.grad] + [P[k].grad for k in names]

    want, single = chain(torch.float64), [t.to(dtype) for t in chain(torch.float32)]
    dev = layer.cuda()
    dx = x.cuda().requires_grad_(True)
    out = dev(dx, types.cuda())
    (out.float() * coef.cuda().float()).sum().backward()
    got = [out, dx.grad] + [getattr(dev, k).grad for k in names]
    _compare(["out", "d x"] + ["d " + k for k in names], got, want, single, dtype, "HeteroLinear")


@pytest.mark.parametrize("dtype", LAYER_DTYPES, ids=LAYER_IDS)
@pytest.mark.parametrize("cin,cout", [(11, 44), (64, 64)])
@pytest.mark.parametrize("aggr", ["mean", "sum"])
@pytest.mark.parametrize("num_bases", [None, 2], ids=["full", "bases"])
@pytest.mark.parametrize("root_weight", [True, False], ids=["root", "no_root"])
def test_rgcn_forward_and_backward(G, root_weight, num_bases, aggr, cin, cout, dtype):
    """Unsorted edge_type, node 3 without an incoming edge, relation 1 without an edge, one edge four times."""
    from gnnops import conv

    torch.manual_seed(8)
    layer = conv.RGCNConv(cin, cout, N_REL, num_bases=num_bases, aggr=aggr, root_weight=root_weight).to(dtype)
    with torch.no_grad():
        layer.bias.copy_(torch.randn(cout).to(dtype))
    shapes = {"weight": (num_bases or N_REL, cin, cout), "bias": (cout,)}
    if num_bases:
        shapes["comp"] = (N_REL, num_bases)
    if root_weight:
        shapes["root"] = (cin, cout)
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == shapes
    ei, et = hc.graph(9, N_NODES, N_EDGES, N_REL)
    assert not bool((ei[1] == 3).any()) and not bool((et == 1).any()) and not bool((et[1:] >= et[:-1]).all())
    g = torch.Generator().manual_seed(10)
    x, coef = torch.randn(N_NODES, cin, generator=g).to(dtype), torch.randn(N_NODES, cout, generator=g).to(dtype)
    names = sorted(shapes)
    rd = hc.straight_through(dtype)

    def chain(ftype):
        P = {k: v.detach().to(ftype).clone().requires_grad_(True) for k, v in layer.state_dict().items()}
        xl = x.to(ftype).clone().requires_grad_(True)
        out = hc.rgcn_ref(P, xl, ei, et, N_REL, aggr, rd=rd)
        (out * coef.to(ftype)).sum().backward()
        return [out.detach(), xl.grad] + [P[k].grad for k in names]

    want, single = chain(torch.float64), [t.to(dtype) for t in chain(torch.float32)]
    dev = layer.cuda()
    dx = x.cuda().requires_grad_(True)
    out = dev(dx, ei.cuda(), et.cuda())
    (out.float() * coef.cuda().float()).sum().backward()
    got = [out, dx.grad] + [getattr(dev, k).grad for k in names]
    _compare(["out", "d x"] + ["d " + k for k in names], got, want, single, dtype, f"RGCNConv {aggr}")


# ---- graph capture ------------------------------------------------------------------------------------------------------------------
def test_captured_forward_replays_bit_for_bit(G):
    from gnnops import ops

    tm = _geo(torch.bfloat16)[0]
    lens = [tm + 3, 0, 2 * tm + 1, 5]
    gen = torch.Generator(device="cuda").manual_seed(12)
    x = torch.randn(sum(lens), 72, generator=gen, device="cuda").to(torch.bfloat16)
    w = torch.randn(len(lens), 72, 136, generator=gen, device="cuda").to(torch.bfloat16)
    b = torch.randn(len(lens), 136, generator=gen, device="cuda").to(torch.bfloat16)
    ptr = hc.ptr_of(lens).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                    # warm-up outside capture
        ops.segment_matmul(x, ptr, w, b)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.segment_matmul(x, ptr, w, b)
    for trial in range(3):
        x.copy_(torch.randn(x.shape, generator=gen, device="cuda").to(torch.bfloat16))
        w.copy_(torch.randn(w.shape, generator=gen, device="cuda").to(torch.bfloat16))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ops.segment_matmul(x, ptr, w, b)), trial
