"""gnnops.pool on the GPU: topk (every route, size seam, ratio form, order convention, dtype) and the edge compaction behind
filter_adj / remove_self_loops against the plain-torch chain of unet_chain.py. Everything here is an integer: exact."""
import pytest
import torch

import unet_chain as uc

pytestmark = pytest.mark.gpu
DTYPES = uc.DTYPES


@pytest.fixture(scope="module")
def pool():
    import gnnops.pool as pool

    return pool


def _batch(sizes):
    return torch.cat([torch.full((n,), i, dtype=torch.long) for i, n in enumerate(sizes)]) if sizes else torch.zeros(0, dtype=torch.long)


def _scores(n, dtype, seed=0, ties=False):
    g = torch.Generator().manual_seed(seed)
    s = torch.randint(-6, 7, (n,), generator=g).float() / 4 if ties else torch.randn(n, generator=g)
    return s.to(dtype)


def _check(pool, score, ratio, sizes, route="auto"):
    batch = _batch(sizes)
    want, want_ptr = uc.topk(score.double(), ratio, batch, len(sizes))
    ptr = torch.tensor([0] + list(torch.tensor(sizes).cumsum(0)), dtype=torch.int32).cuda()
    perm, out_ptr = pool._topk_ptr(score.cuda(), ratio, ptr, route=route)
    assert torch.equal(out_ptr.cpu().long(), want_ptr)
    assert torch.equal(perm.cpu(), want)
    return perm


def _seam_sizes(pool):
    L = pool.topk_max_len()
    return [1, 2, 0, 63, 64, 65, 255, 256, 257, L - 1, L, L + 1]


@pytest.mark.parametrize("dtype", DTYPES, ids=uc.DNAME.get)
@pytest.mark.parametrize("ratio", [0.5, 0.8, 1.0, 1e-5, 3])
def test_topk_size_seams(pool, dtype, ratio):
    sizes = _seam_sizes(pool)                      # the last graph sends the call down the long route
    _check(pool, _scores(sum(sizes), dtype, ties=(dtype != torch.float32)), ratio, sizes)
    _check(pool, _scores(sum(sizes[:-1]), dtype, 1, ties=True), ratio, sizes[:-1])     # all on chip


@pytest.mark.parametrize("dtype", DTYPES, ids=uc.DNAME.get)
def test_topk_routes_agree(pool, dtype):
    sizes = _seam_sizes(pool)[:-1]
    score = _scores(sum(sizes), dtype, 2, ties=True)
    a = _check(pool, score, 0.5, sizes, route="on_chip")
    b = _check(pool, score, 0.5, sizes, route="long")
    assert torch.equal(a, b)


def test_topk_batching(pool):
    score = _scores(777, torch.float32, 3)
    want, _ = uc.topk(score.double(), 0.5, torch.zeros(777, dtype=torch.long), 1)
    assert torch.equal(pool.topk(score.cuda(), 0.5).cpu(), want)                       # batch=None
    sizes = [5 + (i * 7) % 23 for i in range(300)]
    score = _scores(sum(sizes), torch.float32, 4)
    batch = _batch(sizes)
    want, _ = uc.topk(score.double(), 0.8, batch, 300)
    assert torch.equal(pool.topk(score.cuda(), 0.8, batch.cuda()).cpu(), want)          # num_graphs read from the device
    assert torch.equal(pool.topk(score.cuda(), 0.8, batch.cuda(), 300).cpu(), want)
    assert pool.topk(score.cuda().requires_grad_(True), 0.8, batch.cuda(), 300).requires_grad is False


@pytest.mark.parametrize("route", ["on_chip", "long"])
def test_topk_order_conventions(pool, route):
    sizes = [70, 40, 300]
    n = sum(sizes)
    ptr = torch.tensor([0, 70, 110, 410], dtype=torch.int32).cuda()
    perm, _ = pool._topk_ptr(torch.full((n,), 0.25).cuda(), 0.5, ptr, route=route)     # all equal: lowest ids first
    assert perm.tolist() == list(range(35)) + list(range(70, 90)) + list(range(110, 260))
    score = torch.tensor([-1.0, 0.0, -0.0, -2.0, 0.0, -0.0, -0.5] * 10)                  # -0.0 orders as +0.0: ties by id
    _check(pool, score, 1.0, [70], route=route)
    score = _scores(n, torch.float32, 5)
    score[75] = float("nan")                                                            # a NaN ranks above every number
    perm, out_ptr = pool._topk_ptr(score.cuda(), 0.5, ptr, route=route)
    assert int(perm[int(out_ptr[1])]) == 75
    score[200] = float("nan")                                                           # and one in a graph of more than 64 nodes
    perm, out_ptr = pool._topk_ptr(score.cuda(), 0.5, ptr, route=route)
    assert int(perm[int(out_ptr[1])]) == 75 and int(perm[int(out_ptr[2])]) == 200
    rest = score.clone()
    rest[75] = rest[200] = float("inf")
    want, _ = uc.topk(rest.double(), 0.5, _batch(sizes), 3)
    assert torch.equal(perm.cpu(), want)
    zeros = torch.tensor([-1.0, 0.0, -0.0, -2.0, 0.0, -0.0, -0.5] * 5)                   # 35 nodes: the one-wave kernel
    _check(pool, zeros, 1.0, [35], route=route)
    _check(pool, zeros, 0.5, [35], route=route)


def _filter_want(ei, ea, nmap, drop):
    row, col = ei[0], ei[1]
    if nmap is not None:
        row, col = nmap[row], nmap[col]
    keep = (row >= 0) & (col >= 0)
    if drop:
        keep &= row != col
    return torch.stack([row[keep], col[keep]]), (ea[keep] if ea is not None else None)


def _filter_case(pool, E, pattern, value, use_map, drop, seed=0):
    g = torch.Generator().manual_seed(seed)
    n = 500
    ei = torch.randint(0, n, (2, E), generator=g)
    e = torch.arange(E)
    nmap = None
    if use_map:
        if pattern == "all":
            kept_nodes = torch.ones(n, dtype=torch.bool)
        elif pattern == "none":
            kept_nodes = torch.zeros(n, dtype=torch.bool)
        else:
            kept_nodes = torch.arange(n) % 2 == 0
            # lanes: survivors alternate per lane; waves: whole waves of 64 edges survive or go
            alive = (e % 2 == 0) if pattern == "lanes" else ((e // 64) % 2 == 0) if pattern == "waves" else torch.rand(E, generator=g) < 0.5
            ei = torch.where(alive, ei - ei % 2, ei - ei % 2 + 1)
        perm = torch.nonzero(kept_nodes).view(-1)
        perm = perm[torch.randperm(perm.numel(), generator=g)]
        nmap = torch.full((n,), -1, dtype=torch.long)
        nmap[perm] = torch.arange(perm.numel())
    ea = None
    if value == "f32":
        ea = torch.randn(E, generator=g)
    elif value == "f16x3":
        ea = torch.randn(E, 3, generator=g).half()
    want_i, want_a = _filter_want(ei, ea, nmap, drop)
    if use_map and not drop:
        got_i, got_a = pool.filter_adj(ei.cuda(), ea.cuda() if ea is not None else None, perm.cuda(), n)
    elif not use_map:
        got_i, got_a = pool.remove_self_loops(ei.cuda(), ea.cuda() if ea is not None else None)
    else:
        got_i, got_a = pool._filter(ei.cuda(), ea.cuda() if ea is not None else None, pool.node_map(perm.cuda(), n), True, "filter")
    assert got_i.shape == want_i.shape and torch.equal(got_i.cpu(), want_i)
    if ea is not None:
        assert got_a.size(0) == want_i.size(1) and torch.equal(got_a.cpu(), want_a)
    else:
        assert got_a is None


@pytest.mark.parametrize("value", [None, "f32", "f16x3"])
def test_filter_edges_tile_seams(pool, value):
    T = pool.filter_tile()
    for E in (0, T - 1, T, T + 1, 3 * T + 1):
        _filter_case(pool, E, "random", value, True, False, seed=E)


@pytest.mark.parametrize("pattern", ["all", "none", "lanes", "waves"])
def test_filter_edges_survival_patterns(pool, pattern):
    _filter_case(pool, 2 * pool.filter_tile() + 77, pattern, "f16x3", True, False)


@pytest.mark.parametrize("value", [None, "f32", "f16x3"])
def test_filter_edges_self_loops(pool, value):
    _filter_case(pool, 3000, "random", value, False, True)       # node_map absent
    _filter_case(pool, 3000, "random", value, True, True)        # both together


def test_filter_refusals(pool):
    ei = torch.zeros((2, 4), dtype=torch.long)
    with pytest.raises(RuntimeError):
        pool.remove_self_loops(ei)
    with pytest.raises(RuntimeError):
        pool.topk(torch.zeros(4), 0.5)
    with pytest.raises(NotImplementedError):
        pool.filter_adj(ei.cuda(), torch.zeros(4, device="cuda", requires_grad=True), torch.arange(2).cuda(), 4)
