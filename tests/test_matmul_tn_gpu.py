"""gnnops.matmul_tn (csrc/gemm_tn.hip): a^T @ b split along the long dimension, on the GPU.

Exact cases: integer operands from [-4, 4], so every partial and total sum is an integer below 2^24 (R <= 10^6) and every summation
order gives the same fp32 value: the result must equal the int64 product of the CPU, converted once, bit for bit — a dropped, doubled
or out-of-range row or column shows exactly. Shapes come from matmul_tn_geometry: every seam of one dimension against two fixed small
values of the others, plus the all-largest corner. Random cases: max |got - ref| / max |ref| against the float64 product, bar 4 x the
same metric of the CPU's float32 product rounded once (floor: one unit in the last place of the dtype at max |ref|). Routes: where
ops.matmul_tn_preferred holds the weight gradients of autograd.matmul and conv._EdgeLinear ARE ops.matmul_tn(x, g), elsewhere the
transpose + GEMM, bit for bit; and one GATv2Conv / GATConv train step with edge_dim = 8 against the float64 chain."""
import math

import pytest
import torch

from helpers import assert_bits_equal, to_np

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
DNAME = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
MANTISSA = {torch.float32: 23, torch.float16: 10, torch.bfloat16: 7}


def _ulp_rel(scale, dtype):
    """One unit in the last place of the dtype at |value| = scale, as a fraction of scale."""
    return 2.0 ** (math.floor(math.log2(scale)) - MANTISSA[dtype]) / scale


@pytest.fixture(scope="module")
def G():
    import gnnops

    gnnops.load_library()
    return gnnops


def _geometry(G, R, P, Q, dtype):
    from gnnops import ops

    return ops.matmul_tn_geometry(R, P, Q, dtype)


def _exact_shapes(G, dtype):
    geo = _geometry(G, 1, 8, 8, dtype)
    tp, tq, sr = geo["tile_p"], geo["tile_q"], geo["slab_rows"]
    Rs = [1, 7, sr - 1, sr, sr + 1, 3 * sr + 5, 40 * sr + 3]
    Ps = [1, 8, 11, tp - 1, tp, tp + 1]
    Qs = [1, 8, 44, tq - 1, tq, tq + 1, 2 * tq + 3]
    shapes = []
    for R in Rs:
        shapes += [(R, 8, 44), (R, 11, 8)]
    for P in Ps:
        shapes += [(7, P, 8), (sr + 1, P, 44)]
    for Q in Qs:
        shapes += [(7, 8, Q), (sr + 1, 11, Q)]
    shapes.append((Rs[-1], Ps[-1], Qs[-1]))
    return list(dict.fromkeys(shapes)), sr


_INTS = {}


def _ints(R, P, Q, dtype, seed, offset=0):
    """Integer operands in [-4, 4]; offset: they start `offset` elements into their allocation and end flush with it."""
    key = (R, P, Q, seed)
    if key not in _INTS:                  # the int64 product of the CPU: computed once, shared by the dtypes
        g = torch.Generator().manual_seed(seed)
        a = torch.randint(-4, 5, (R, P), generator=g)
        b = torch.randint(-4, 5, (R, Q), generator=g)
        _INTS[key] = (a, b, a.t() @ b)
    a, b, want = _INTS[key]
    want = want.to(dtype)                 # converted once
    dev = []
    for t in (a, b):
        buf = torch.zeros(offset + t.numel(), dtype=dtype, device="cuda")
        buf[offset:] = t.to(dtype).reshape(-1).cuda()
        dev.append(buf[offset:offset + t.numel()].view(t.shape))
    return dev[0], dev[1], want


@pytest.mark.parametrize("dtype", DTYPES, ids=[DNAME[d] for d in DTYPES])
def test_exact_at_every_seam(G, dtype):
    shapes, sr = _exact_shapes(G, dtype)
    slabs_seen = set()
    for n, (R, P, Q) in enumerate(shapes):
        geo = _geometry(G, R, P, Q, dtype)
        assert geo["slab_rows"] == sr, (R, P, Q, geo)      # the seams above are the seams of THIS shape
        slabs_seen.add(geo["slabs"])
        a, b, want = _ints(R, P, Q, dtype, seed=100 + n)
        got = G.matmul_tn(a, b)
        assert got.dtype == dtype and got.shape == (P, Q)
        assert_bits_equal(to_np(got), to_np(want), f"{DNAME[dtype]} R={R} P={P} Q={Q}")
    assert {1, 2, 4} <= slabs_seen and max(slabs_seen) >= 40


@pytest.mark.parametrize("dtype", DTYPES, ids=[DNAME[d] for d in DTYPES])
def test_exact_one_element_into_the_allocation(G, dtype):
    """buf[1:1 + R*P].view(R, P): a misaligned head, and a tail that ends flush with the allocation."""
    sr = _geometry(G, 1, 8, 8, dtype)["slab_rows"]
    for n, (R, P, Q) in enumerate([(7, 8, 44), (sr + 1, 11, 8), (sr + 1, 8, 128), (3 * sr + 5, 11, 44), (77, 129, 259), (sr + 1, 128, 256)]):
        a, b, want = _ints(R, P, Q, dtype, seed=200 + n, offset=1)
        assert a.data_ptr() % 16 != 0 and b.data_ptr() % 16 != 0
        assert_bits_equal(to_np(G.matmul_tn(a, b)), to_np(want), f"offset {DNAME[dtype]} R={R} P={P} Q={Q}")


@pytest.mark.parametrize("dtype", DTYPES, ids=[DNAME[d] for d in DTYPES])
def test_no_rows_gives_zeros_and_empty_outputs_return(G, dtype):
    out = G.matmul_tn(torch.empty(0, 11, dtype=dtype, device="cuda"), torch.empty(0, 44, dtype=dtype, device="cuda"))
    assert out.shape == (11, 44) and float(out.abs().max()) == 0.0
    assert G.matmul_tn(torch.ones(5, 0, dtype=dtype, device="cuda"), torch.ones(5, 3, dtype=dtype, device="cuda")).shape == (0, 3)
    assert G.matmul_tn(torch.ones(5, 3, dtype=dtype, device="cuda"), torch.ones(5, 0, dtype=dtype, device="cuda")).shape == (3, 0)


def test_strided_operands_and_refusals(G):
    from gnnops import ops

    g = torch.Generator().manual_seed(3)
    a = torch.randint(-4, 5, (300, 24), generator=g).float().cuda()
    b = torch.randint(-4, 5, (300, 40), generator=g).float().cuda()
    want = a.cpu().long().t() @ b.cpu().long()
    assert torch.equal(G.matmul_tn(a[:, ::2], b.t()[::3].t()).cpu().long(), want[::2, ::3])
    with pytest.raises(RuntimeError, match="same number of rows"):
        G.matmul_tn(a, b[:299])
    with pytest.raises(RuntimeError, match="same dtype"):
        G.matmul_tn(a, b.half())
    with pytest.raises(RuntimeError, match="matrices"):
        G.matmul_tn(a[0], b)
    with pytest.raises(RuntimeError, match="ROCm device tensor"):
        G.matmul_tn(a.cpu(), b)
    with pytest.raises(NotImplementedError, match="not supported"):
        G.matmul_tn(a.double(), b.double())
    with pytest.raises(NotImplementedError, match="requires grad"):
        ops.matmul_tn(a.clone().requires_grad_(True), b)


# ---- random operands ----------------------------------------------------------------------------------------------------------
def _metric(got, ref):
    return float((got.double() - ref).abs().max()) / float(ref.abs().max())


def _bar(a, b, ref, dtype):
    """4 x the error of the CPU product accumulated in float32 and rounded once, at least 4 units in the last place at max |ref|."""
    cpu = (a.float().t() @ b.float()).to(dtype)
    return 4 * max(_metric(cpu, ref), _ulp_rel(float(ref.abs().max()), dtype))


_RANDOM = {}


def _random_case(P, Q, dtype):
    key = (P, Q, dtype)
    if key not in _RANDOM:
        g = torch.Generator().manual_seed(P * 4099 + Q)
        a = torch.randn(70001, P, generator=g).to(dtype)
        b = torch.randn(70001, Q, generator=g).to(dtype)
        ref = a.double().t() @ b.double()
        _RANDOM[key] = (a, b, ref, _bar(a, b, ref, dtype))
    return _RANDOM[key]


@pytest.mark.parametrize("dtype", DTYPES, ids=[DNAME[d] for d in DTYPES])
@pytest.mark.parametrize("P,Q", [(8, 128), (11, 44), (128, 1024)])
def test_random_against_float64(G, P, Q, dtype):
    a, b, ref, bar = _random_case(P, Q, dtype)
    da, db = a.cuda(), b.cuda()
    got = G.matmul_tn(da, db)
    err = _metric(got.cpu(), ref)
    print(f"{DNAME[dtype]} R=70001 P={P} Q={Q}: {err:.3e} (bar {bar:.3e})")
    assert err <= bar
    assert torch.equal(G.matmul_tn(da, db), got)      # the same bits on a second call


@pytest.mark.parametrize("dtype", DTYPES, ids=[DNAME[d] for d in DTYPES])
def test_autograd_against_float64(G, dtype):
    g = torch.Generator().manual_seed(17)
    R, P, Q = 5003, 11, 44
    a, b, coef = torch.randn(R, P, generator=g).to(dtype), torch.randn(R, Q, generator=g).to(dtype), torch.randn(P, Q, generator=g).to(dtype)
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = a64.t() @ b64
    (ref * coef.double()).sum().backward()
    da, db = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    out = G.autograd.matmul_tn(da, db)
    assert out.requires_grad
    (out.float() * coef.cuda().float()).sum().backward()
    assert _metric(out.detach().cpu(), ref.detach()) <= _bar(a, b, ref.detach(), dtype)
    # d a = b @ coef^T, d b = a @ coef: the float32 CPU products of the same operands set the bars
    for name, got, want, cpu in (("d a", da.grad, a64.grad, (b.float() @ coef.float().t()).to(dtype)),
                                 ("d b", db.grad, b64.grad, (a.float() @ coef.float()).to(dtype))):
        err, bar = _metric(got.cpu(), want), 4 * max(_metric(cpu, want), _ulp_rel(float(want.abs().max()), dtype))
        print(f"{DNAME[dtype]} {name}: {err:.3e} (bar {bar:.3e})")
        assert err <= bar, name


# ---- routes ---------------------------------------------------------------------------------------------------------------------
def _shape_where(pref, want, P, Q, dtype):
    for R in (512, 2048, 8192, 32768, 131072, 524288):
        if pref(R, P, Q, dtype) == want:
            return R
    pytest.fail(f"matmul_tn_preferred is never {want} for P={P} Q={Q} {dtype} up to 524288 rows")


@pytest.mark.parametrize("dtype", DTYPES, ids=[DNAME[d] for d in DTYPES])
@pytest.mark.parametrize("taken", [True, False], ids=["preferred", "not_preferred"])
def test_weight_gradient_routes(G, taken, dtype):
    from gnnops import conv, ops
    from gnnops.sparse import transpose_contiguous

    P, Q = 8, 128
    R = _shape_where(ops.matmul_tn_preferred, taken, P, Q, dtype)
    g = torch.Generator().manual_seed(23)
    x, w, go = (torch.randn(s, generator=g).to(dtype).cuda() for s in ((R, P), (P, Q), (R, Q)))
    want = ops.matmul_tn(x, go) if taken else ops.matmul(transpose_contiguous(x), go)
    w1 = w.clone().requires_grad_(True)
    G.autograd.matmul(x, w1).backward(go)
    assert torch.equal(w1.grad, want), "autograd.matmul"
    w2 = w.clone().requires_grad_(True)
    conv._EdgeLinear.apply(x, w2).backward(go)
    assert torch.equal(w2.grad, want), "_EdgeLinear"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["gatv2", "gat"])
def test_edge_dim_8_train_step(G, kind, dtype):
    """lin_edge.weight.grad of one train step on a graph just large enough for lin_edge's weight gradient to take the new route,
    against the float64 chain. The chain records no self error for this case: the bar is the random-case bar, 4 x the error of the
    same chain run in float32 on the CPU and rounded once to the dtype (at least 4 units in the last place at the gradient's scale)."""
    import attention_edge_chain as ec
    from gnnops import conv, ops

    H, C, cin, edge_dim, n = 4, 8, 16, 8, 300
    width = H * C if kind == "gatv2" else None
    E = None
    for cand in (2048, 8192, 32768, 131072):
        # the rows of lin_edge's product: the edges that are no self loops plus one loop per node; its width is what the layer packs
        if ops.matmul_tn_preferred(cand, edge_dim, width or 8, dtype):
            E = cand
            break
    assert E is not None, "matmul_tn_preferred never holds for lin_edge up to 131072 edges"
    torch.manual_seed(31)
    layer = (conv.GATv2Conv if kind == "gatv2" else conv.GATConv)(cin, C, heads=H, edge_dim=edge_dim).to(dtype)
    g = torch.Generator().manual_seed(32)
    src, dst = torch.randint(0, n, (E,), generator=g), torch.randint(0, n, (E,), generator=g)
    dst = torch.where(src == dst, (dst + 1) % n, dst)          # no self loops in the input: E + n rows reach lin_edge
    ei = torch.stack([src, dst])
    x, ea, coef = ec._rand(g, n, cin), ec._rand(g, E, edge_dim), ec._rand(g, n, H * C)
    ref_fn = ec.gatv2_edge_ref if kind == "gatv2" else ec.gat_edge_ref

    def chain(ftype):
        P = {k: v.detach().to(ftype).requires_grad_(True) for k, v in layer.named_parameters()}
        rd = ec._straight_through(dtype)
        out = ref_fn(P, ei, n, H, C, True, 0.2, True, "mean", x.to(dtype).to(ftype), ea.to(dtype).to(ftype), rd=rd)
        (out * coef.to(ftype)).sum().backward()
        return P["lin_edge.weight"].grad

    want = chain(torch.float64)
    self_err = ec.rel_err(chain(torch.float32).to(dtype).double(), want)
    bar = 4 * max(self_err, _ulp_rel(float(want.abs().max()), dtype))
    calls = []
    real = ops.matmul_tn
    ops.matmul_tn = lambda a, b: (calls.append(tuple(a.shape)), real(a, b))[1]
    try:
        dev = layer.cuda()
        out = dev(x.to(dtype).cuda(), ei.cuda(), ea.to(dtype).cuda())
        (out.float() * coef.cuda()).sum().backward()
    finally:
        ops.matmul_tn = real
    assert any(s[1] == edge_dim for s in calls), f"lin_edge's weight gradient did not take matmul_tn: {calls}"
    err = ec.rel_err(dev.lin_edge.weight.grad.double().cpu(), want)
    print(f"{kind} {DNAME[dtype]} E={E} lin_edge.weight.grad: {err:.3e} (bar {bar:.3e}; float32 chain {self_err:.3e})")
    assert err <= bar
