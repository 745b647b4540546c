"""Seams of the four on-chip counting sorts that share the ballot ranking of csrc/lds_sort.h: the one-shot bucket finish
(bucket.hip), the long 1-D sum finish (scatter1d.hip), the row sort (sort_rows.hip: tests/test_sparse_sort_gpu.py
::test_sort_rows_on_chip carries its sizes) and the radix engine (sort_engine_impl.h). Sizes sit on both sides of a row of
64 keys, a wave's share, a chunk (4096 / 1024 pairs) and a radix tile (8192 keys); the index patterns make one peer group
of all 64 lanes, 64 leaders per row, the same reversed, and three long groups. All fp32 and bit-exact: sums of values in
[-1, 1) change with the order of the adds, so equality with the sequential oracle pins stability; `min` over a handful of
distinct values pins it through the positions.

The one-shot form is defined for N > 256 only (ops.scatter and gnnops_bucket_reduce both refuse N == 256), so "one
bucket" is N = 257 with every contribution inside destinations [0, 256): the second bucket is one untouched row."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PATTERNS = ["equal", "mod256", "rev256", "three"]


def _pattern(kind, E, g, lo=0, keys=None):
    """E destinations inside [lo, lo + 256)."""
    i = torch.arange(E)
    if kind == "equal":
        return torch.full((E,), lo + 5, dtype=torch.int64)
    if kind == "mod256":
        return lo + i % 256
    if kind == "rev256":
        return lo + 255 - i % 256
    keys = torch.tensor(keys if keys is not None else [lo + 3, lo + 130, lo + 255])
    return keys[torch.randint(0, 3, (E,), generator=g)]


def _values(reduce, shape, g):
    if reduce == "min":
        return torch.randint(-2, 3, shape, generator=g).float() * 0.5      # heavy ties: arg is the smallest position
    x = torch.rand(shape, generator=g)
    return 1 + x / 128 if reduce == "mul" else x * 2 - 1


def _check(got, exp, reduce):
    if reduce == "min":
        assert np.array_equal(got[1].cpu().numpy(), exp[1]), "positions"
        got, exp = got[0], exp[0]
    got = got.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), f"{(got != exp).sum()} values differ"


@pytest.fixture()
def spied(monkeypatch):
    """gnnops with the library wrapped so that the entry points a call reaches are recorded by name."""
    import gnnops
    from gnnops import _lib

    lib = gnnops.load_library()
    calls = []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name in ("gnnops_bucket_reduce_hubs", "gnnops_scatter1d_sum", "gnnops_plan_build"):
                return lambda *a: (calls.append(name), fn(*a))[1]
            return fn

    monkeypatch.setattr(_lib, "load", lambda: Spy())
    yield gnnops, calls
    gnnops.set_plan_cache(True)


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o

    return o


# ---- bucket.hip: rows of 64, a wave's share of a chunk, chunks of 4096 ---------------------------------------------------
@pytest.mark.parametrize("kind", PATTERNS)
@pytest.mark.parametrize("reduce", ["sum", "min"])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191])
def test_oneshot_bucket_finish(spied, oracle, reduce, kind, E):
    gnnops, calls = spied
    N, K = 257, 4
    g = torch.Generator().manual_seed(E * 4 + PATTERNS.index(kind))
    src = _values(reduce, (E, K), g)
    idx = _pattern(kind, E, g)
    gnnops.set_plan_cache(False)
    got = gnnops.scatter(src.cuda(), idx.cuda(), 0, dim_size=N, reduce=reduce)
    assert "gnnops_bucket_reduce_hubs" in calls, "the one-shot bucket finish did not run"
    _check(got, oracle.scatter(src.numpy(), idx.numpy(), dim=0, dim_size=N, reduce=reduce), reduce)


@pytest.mark.parametrize("reduce", ["sum", "min"])
def test_oneshot_two_buckets_meet_at_a_chunk_seam(spied, oracle, reduce):
    gnnops, calls = spied
    N, K, E = 300, 4, 4097
    g = torch.Generator().manual_seed(11)
    src = _values(reduce, (E, K), g)
    idx = _pattern("three", E, g, keys=[255, 256, 257])
    gnnops.set_plan_cache(False)
    got = gnnops.scatter(src.cuda(), idx.cuda(), 0, dim_size=N, reduce=reduce)
    assert "gnnops_bucket_reduce_hubs" in calls, "the one-shot bucket finish did not run"
    _check(got, oracle.scatter(src.numpy(), idx.numpy(), dim=0, dim_size=N, reduce=reduce), reduce)


# ---- scatter1d.hip: chunks of 1024 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", PATTERNS)
@pytest.mark.parametrize("reduce", ["sum", "mul"])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_long_1d_sum_finish(spied, oracle, monkeypatch, reduce, kind, E):
    gnnops, calls = spied
    from gnnops import ops

    monkeypatch.setattr(ops, "_SCATTER1D_MIN_N", 32769)
    N = 32768 * 2 + 5
    g = torch.Generator().manual_seed(E * 4 + PATTERNS.index(kind) + 1)
    src = _values(reduce, (E,), g)
    idx = _pattern(kind, E, g, lo=512)
    got = gnnops.scatter(src.cuda(), idx.cuda(), 0, dim_size=N, reduce=reduce)
    assert "gnnops_scatter1d_sum" in calls, "the carried-value sum form did not run"
    _check(got, oracle.scatter(src.numpy(), idx.numpy(), dim=0, dim_size=N, reduce=reduce), reduce)


# ---- sort_rows.hip: ties whose order only the source position decides ------------------------------------------------------
@pytest.mark.parametrize("rows,E", [(3, 1), (3, 63), (3, 64), (3, 65), (2, 22527)])
@pytest.mark.parametrize("descending", [False, True])
def test_sort_rows_ties(rows, E, descending):
    import gnnops

    gnnops.load_library()
    g = torch.Generator().manual_seed(rows + E)
    x = torch.tensor([-0.0, 0.0, 1.0, float("nan")])[torch.randint(0, 4, (rows, E), generator=g)]
    ev, ei = torch.sort(x, dim=1, descending=descending, stable=True)
    v, i = gnnops.sort(x.cuda(), dim=1, descending=descending, stable=True)
    assert torch.equal(i.cpu(), ei), "indices"
    assert torch.equal(v.cpu().view(torch.int32), ev.view(torch.int32)), "values (bits)"


# ---- sort_engine_impl.h: rows of 64, a wave's 1024 keys, tiles of 8192 -----------------------------------------------------
ENGINE_SIZES = [1, 63, 64, 65, 511, 512, 513, 8191, 8192, 8193, 16385]


@pytest.mark.parametrize("n", ENGINE_SIZES)
def test_engine_sort_1d(n):
    import gnnops

    gnnops.load_library()
    g = torch.Generator().manual_seed(n)
    x = torch.tensor([-1.5, 0.25, 3.0, 1e-3])[torch.randint(0, 4, (n,), generator=g)]
    ev, ei = torch.sort(x, stable=True)
    v, i = gnnops.sort(x.cuda(), stable=True)
    assert torch.equal(i.cpu(), ei), "indices"
    assert torch.equal(v.cpu().view(torch.int32), ev.view(torch.int32)), "values (bits)"


@pytest.mark.parametrize("kind", PATTERNS)
@pytest.mark.parametrize("E", ENGINE_SIZES)
def test_engine_plan_scatter(spied, oracle, kind, E):
    """The plan build: the first pass reads the int64 index, the later ones u32 keys. The engine's own output, the plan's
    permutation, is the stable argsort exactly. So is the sum, bit for bit against the oracle — except where one destination
    takes more than 8192 contributions ("equal" at E = 8193 and 16385): such a hub is summed piecewise by csrc/hub.h, in
    another order by design, so there the sum is held to the bound of ANY order of n fp32 adds against the float64 sum,
    (n - 1) * 2^-24 * sum |x| (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4, first order)."""
    gnnops, calls = spied
    N, K = 70000, 4
    g = torch.Generator().manual_seed(E * 4 + PATTERNS.index(kind) + 2)
    src = _values("sum", (E, K), g)
    idx = _pattern(kind, E, g, lo=66000, keys=[3, 300, 69999])
    gnnops.set_plan_cache(True)
    got = gnnops.scatter(src.cuda(), idx.cuda(), 0, dim_size=N, reduce="sum")
    assert "gnnops_plan_build" in calls, "the radix engine did not build the plan"
    plan = gnnops.Plan(idx.cuda(), N)
    assert torch.equal(plan.perm[:E].cpu().long(), torch.sort(idx, stable=True)[1]), "the plan's permutation is not the stable one"
    exp = oracle.scatter(src.numpy(), idx.numpy(), dim=0, dim_size=N, reduce="sum")
    hubs = np.bincount(idx.numpy(), minlength=N) > 8192
    got = got.cpu().numpy()
    assert np.array_equal(got[~hubs].view(np.uint32), exp[~hubs].view(np.uint32)), "values differ (bits)"
    for d in np.flatnonzero(hubs):
        x = src.numpy()[idx.numpy() == d].astype(np.float64)
        bound = (len(x) - 1) * 2.0 ** -24 * np.abs(x).sum(0)
        assert (np.abs(got[d] - x.sum(0)) <= bound).all(), f"hub {d}: {np.abs(got[d] - x.sum(0))} > {bound}"
