"""The seams of the hub passes (csrc/hub.h: a row with more than 8192 contributions is finished piecewise, pieces of 4096):
hubs that end on a piece boundary or one past it, more hubs in one bucket than are set aside, more than one column chunk,
the fewest lanes and a part-filled lane group — the lines the shared piece walk concentrates.

The inputs are small integers (+-1 for products), so every sum, product, minimum and maximum is exact in fp32 in ANY
association (the sum of |values| of a row stays below 2^24; checked on the CPU from the inputs alone): the re-associated
results of the hubs are compared bit for bit with the sequential oracle, like everything else. Only the mean (a quotient)
keeps the tolerance of test_oneshot_gpu.py::test_hubs_are_reduced_piecewise and the composite ops (expf) the fp32 hub bar
of test_composite_gpu.py."""
import functools

import numpy as np
import pytest
import torch

import composite_chain as cc
from helpers import TORCH_DT, assert_bits_equal, to_np

T_HUB, PART = 8192, 4096
N = 700
DEGREES = {69: 8192, 71: 8193, 330: 12288, 600: 12289}       # 69 is NOT a hub; 71: pieces of 4096, 4096 and 1; 330: three full pieces
FIVE = (260, 300, 301, 400, 511)                             # five hubs of 8193 in the bucket of destinations 256 .. 511
GEOMETRY = [("f32", 8), ("f32", 24), ("f32", 320), ("bf16", 8)]   # fewest lanes; 6 lanes of a group of 8; 80 lanes = two column chunks
REDUCES = ["sum", "mean", "min", "max", "mul"]
MEAN_TOL = dict(rtol=3e-4, atol=3e-3)                        # test_hubs_are_reduced_piecewise
HUB_BAR = dict(rtol=2e-5, atol=2e-6)                         # test_composite_gpu.py: fp32 hubs against float64


@functools.lru_cache(maxsize=None)
def _index(kind):
    """Destinations of the contributions, shuffled: the special rows with their exact degrees, a few contributions for every
    other row (so ordinary destinations lie around each hub, in its bucket too)."""
    g = torch.Generator().manual_seed(77)
    special = dict(DEGREES) if kind == "degrees" else {d: T_HUB + 1 for d in FIVE}
    others = torch.tensor([d for d in range(N) if d not in special])
    parts = [torch.full((n,), d, dtype=torch.int64) for d, n in special.items()]
    parts += [others, others[torch.randint(0, len(others), (2300,), generator=g)]]       # every other row at least once
    idx = torch.cat(parts)
    return idx[torch.randperm(idx.numel(), generator=g)].contiguous()


@functools.lru_cache(maxsize=None)
def _values(kind, K, reduce, dname):
    g = torch.Generator().manual_seed(K + len(reduce))
    E = _index(kind).numel()
    v = torch.randint(0, 2, (E, K), generator=g) * 2 - 1 if reduce == "mul" else torch.randint(-3, 4, (E, K), generator=g)
    return v.to(TORCH_DT[dname])


@functools.lru_cache(maxsize=None)
def _expected(kind, K, reduce, dname):
    from oracle import oracle

    return oracle.scatter(to_np(_values(kind, K, reduce, dname)), _index(kind).numpy(), dim=0, dim_size=N, reduce=reduce,
                          dtype=None if dname == "f32" else dname)


@pytest.mark.parametrize("kind", ["degrees", "five"])
def test_inputs_have_the_intended_hubs_and_exact_sums(kind):
    """No GPU: the hub count of each input, the special degrees, and sum |values| < 2^24 for every destination."""
    idx = _index(kind).numpy()
    deg = np.bincount(idx, minlength=N)
    hubs = np.flatnonzero(deg > T_HUB)
    if kind == "degrees":
        assert all(deg[d] == n for d, n in DEGREES.items())
        assert list(hubs) == [71, 330, 600] and deg[69] == T_HUB
        assert [-(-deg[h] // PART) for h in hubs] == [3, 3, 4] and deg[71] % PART == 1 and deg[330] % PART == 0
    else:
        assert list(hubs) == list(FIVE) and all(deg[h] == T_HUB + 1 for h in hubs) and len({h // 256 for h in hubs}) == 1
    assert (deg[[d for d in range(N) if d not in hubs and d != 69]] > 0).all() and deg.max() * 3 < 2 ** 24
    for reduce in ("sum", "mul"):
        v = np.abs(_values(kind, 8, reduce, "f32").numpy()).max(axis=1)
        assert np.bincount(idx, weights=v, minlength=N).max() < 2 ** 24


@pytest.fixture(scope="module")
def gnnops():
    import gnnops as g

    g.load_library()
    yield g
    g.set_plan_cache(True)


def _check_reduce(gnnops, kind, K, reduce, dname, cache):
    src, idx = _values(kind, K, reduce, dname), _index(kind)
    exp = _expected(kind, K, reduce, dname)
    gnnops.set_plan_cache(cache)
    try:
        got = gnnops.scatter(src.cuda(), idx.cuda(), 0, dim_size=N, reduce=reduce)
    finally:
        gnnops.set_plan_cache(True)
    what = f"{kind} {reduce} {dname} K={K} cache={cache}"
    if reduce in ("min", "max"):
        assert_bits_equal(to_np(got[0]), exp[0], what)
        assert np.array_equal(got[1].cpu().numpy(), exp[1]), what + ": positions"
    elif reduce == "mean":
        hubs = np.bincount(idx.numpy(), minlength=N) > T_HUB
        assert_bits_equal(to_np(got)[~hubs], exp[~hubs], what)
        np.testing.assert_allclose(to_np(got)[hubs], exp[hubs], err_msg=what, **MEAN_TOL)
    else:
        assert_bits_equal(to_np(got), exp, what)


_SEAMS = [(d, k, r) for d, k in GEOMETRY for r in REDUCES if not (r == "mean" and d != "f32")]   # the mean's tolerance is an fp32 one


@pytest.mark.gpu
@pytest.mark.parametrize("cache", [True, False], ids=["plan", "oneshot"])
@pytest.mark.parametrize("dname,K,reduce", _SEAMS, ids=[f"{d}-K{k}-{r}" for d, k, r in _SEAMS])
def test_hub_degrees_at_the_piece_seams(gnnops, dname, K, reduce, cache):
    _check_reduce(gnnops, "degrees", K, reduce, dname, cache)


@pytest.mark.gpu
@pytest.mark.parametrize("cache", [True, False], ids=["plan", "oneshot"])
@pytest.mark.parametrize("reduce", ["sum", "max", "mul"])
def test_five_hubs_in_one_bucket(gnnops, reduce, cache):
    """One-shot form: MAX_PER_BUCKET = 4 are set aside, the fifth is reduced sequentially; all five rows must be right."""
    _check_reduce(gnnops, "five", 8, reduce, "f32", cache)


@pytest.mark.gpu
@pytest.mark.parametrize("dt,K", [(torch.float32, 8), (torch.float32, 320), (torch.float16, 24)], ids=["f32-K8", "f32-K320", "f16-K24"])
def test_index_select_rows_selected_a_piece_seam_number_of_times(gnnops, dt, K):
    from test_oneshot_gpu import _bucket_select

    g = torch.Generator().manual_seed(5)
    table = torch.randint(-1000, 1000, (N, K), generator=g).to(dt).cuda()
    idx = torch.cat([torch.full((T_HUB + 1,), 71), torch.full((3 * PART,), 330), torch.randint(0, N, (3000,), generator=g)])
    idx = idx[torch.randperm(idx.numel(), generator=g)].cuda()
    exp = table[idx]
    assert torch.equal(_bucket_select(gnnops, table, idx), exp), "bucketed"
    assert torch.equal(gnnops.index_select(table, 0, idx, plan=gnnops.Plan(idx, N)), exp), "planned"


@pytest.mark.gpu
@pytest.mark.parametrize("dname,D", [("f32", 8), ("f32", 320), ("bf16", 8)], ids=["f32-D8", "f32-D320", "bf16-D8"])
def test_spmm_row_of_8193_nonzeros(gnnops, dname, D):
    from oracle import oracle

    m, n = 300, 200
    g = torch.Generator().manual_seed(D)
    row = torch.cat([torch.full((T_HUB + 1,), 7), torch.randint(0, m, (2000,), generator=g)])
    row = row[torch.randperm(row.numel(), generator=g)]
    col = torch.randint(0, n, (row.numel(),), generator=g)
    val = torch.randint(-3, 4, (row.numel(),), generator=g).to(TORCH_DT[dname])
    B = torch.randint(-3, 4, (n, D), generator=g).to(TORCH_DT[dname])
    assert (np.bincount(row.numpy(), minlength=m) > T_HUB).sum() == 1 and 9 * (T_HUB + 1 + 2000) < 2 ** 24
    exp = oracle.spmm(torch.stack([row, col]).numpy(), to_np(val), m, n, to_np(B), dtype=dname)
    order = torch.sort(row, stable=True).indices
    rowptr = torch.zeros(m + 1, dtype=torch.int64)
    rowptr[1:] = torch.bincount(row, minlength=m).cumsum(0)
    assert_bits_equal(to_np(gnnops.spmm(torch.stack([row, col]).cuda(), val.cuda(), m, n, B.cuda())), exp, "spmm")
    assert_bits_equal(to_np(gnnops.spmm_csr(rowptr.cuda(), col[order].cuda(), val[order].cuda(), B.cuda())), exp, "spmm_csr")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["softmax", "logsumexp", "std"])
@pytest.mark.parametrize("K", [8, 320])
def test_composite_group_of_8193_members(gnnops, K, mode):
    import torch_scatter as ts

    g = torch.Generator().manual_seed(K)
    row = torch.cat([torch.full((T_HUB + 1,), 5), torch.randint(0, 400, (1500,), generator=g)])
    row = row[torch.randperm(row.numel(), generator=g)]
    src = torch.randn(row.numel(), K, generator=g)
    want, _ = cc.composite_grads(src, row, 0, 400, mode)
    fn = {"softmax": ts.scatter_softmax, "logsumexp": ts.scatter_logsumexp, "std": ts.scatter_std}[mode]
    got = fn(src.cuda(), row.cuda(), dim=0, dim_size=400).double().cpu()
    assert got.shape == want.shape and cc.same_specials(got, want)
    fin = torch.isfinite(want)
    np.testing.assert_allclose(got[fin].numpy(), want[fin].numpy(), err_msg=f"{mode} K={K}", **HUB_BAR)
