"""CPU suite: the spatial oracle (oracle/spatial_oracle.py) is pinned before the GPU tests trust it.

- the vectorised float32 forms of knn / radius / nearest / fps equal the per-pair float32 loop definitions on random clouds
  and on dyadic lattices (multiples of 1/8: every distance exact, ties everywhere);
- known answers worked out by hand for the edge rules: NaN never a neighbour, +inf last, a NaN query gets nothing, a point at
  exactly distance r is outside, ties to the smaller index, fewer candidates than k;
- fp16 / bf16 inputs answer as their exact float32 widening;
- the distance is the kernels' float32 sum in dimension order, not the float64 one.
"""
import numpy as np
import pytest
import torch

from oracle import spatial_oracle as so


def _random(seed, n, m, D, B):
    rng = np.random.default_rng(seed)
    x = rng.random((n, D), dtype=np.float32)
    y = rng.random((m, D), dtype=np.float32)
    bx = np.sort(rng.integers(0, B, n)) if B > 1 else None
    by = np.sort(rng.integers(0, B, m)) if B > 1 else None
    return x, y, bx, by


def _dyadic(seed, n, m, D, B):
    """multiples of 1/8 (half the queries offset by 1/16): every squared distance is exact, ties abound."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 5, (n, D)).astype(np.float32) / 8
    y = rng.integers(0, 5, (m, D)).astype(np.float32) / 8 + np.float32(1 / 16) * (rng.random((m, 1)) < 0.5)
    x[20:30] = x[10:20]                                          # duplicated points
    bx = np.sort(rng.integers(0, B, n)) if B > 1 else None
    by = np.sort(rng.integers(0, B, m)) if B > 1 else None
    return x, y.astype(np.float32), bx, by


def _starts(batch, n):
    if batch is None:
        return np.array([0])
    return np.searchsorted(batch, np.arange(int(batch.max()) + 1))


@pytest.mark.parametrize("cloud", [_random, _dyadic])
@pytest.mark.parametrize("D", [1, 2, 3, 5])
@pytest.mark.parametrize("B", [1, 4])
def test_fast_forms_equal_the_loop_definitions(cloud, D, B):
    x, y, bx, by = cloud(10 * D + B, 240, 70, D, B)
    for k in (1, 7, 33, 300):                                    # 300: more than any batch holds
        assert np.array_equal(so.knn(x, y, k, bx, by), so.knn_loop(x, y, k, bx, by)), k
    if cloud is _random:                                         # cosine: no exact zero-vector / tie structure on a lattice
        assert np.array_equal(so.knn(x, y, 9, bx, by, cosine=True), so.knn_loop(x, y, 9, bx, by, cosine=True))
    for r, cap in ((0.25, 5), (0.4, 32), (0.0, 4), (2.0, 500)):
        assert np.array_equal(so.radius(x, y, r, bx, by, cap), so.radius_loop(x, y, r, bx, by, cap)), (r, cap)
    assert np.array_equal(so.nearest(x, y, bx, by), so.nearest_loop(x, y, bx, by))
    st = _starts(bx, len(x))
    for ratio in (0.3, 1.0):
        assert np.array_equal(so.fps(x, bx, ratio, st), so.fps_loop(x, bx, ratio, st)), ratio
    st2 = st + (np.bincount(bx, minlength=len(st)) // 2 if bx is not None else len(x) // 2)
    assert np.array_equal(so.fps(x, bx, 0.5, st2), so.fps_loop(x, bx, 0.5, st2))


def test_blocks_of_queries_do_not_change_the_answer(monkeypatch):
    x, y, bx, by = _dyadic(3, 400, 150, 3, 3)
    whole = (so.knn(x, y, 12, bx, by), so.radius(x, y, 0.3, bx, by, 9))
    monkeypatch.setattr(so, "_CHUNK", 500)                       # one or two queries per block
    assert np.array_equal(so.knn(x, y, 12, bx, by), whole[0])
    assert np.array_equal(so.radius(x, y, 0.3, bx, by, 9), whole[1])


def test_knn_known_answers_for_the_edge_rules():
    nan, inf = np.nan, np.inf
    x = np.array([[0.0, 0.0],      # 0: distance 1 from q0
                  [nan, 0.0],      # 1: never a neighbour
                  [2.0, 0.0],      # 2: distance 1 from q0, ties with 0 -> after it
                  [inf, 0.0],      # 3: distance inf -> after every finite one
                  [1.0, 3.0]],     # 4: distance 9
                 np.float32)
    y = np.array([[1.0, 0.0], [nan, 1.0]], np.float32)
    got = so.knn(x, y, 10, None, None)
    # q0: 0, 2 (tie, smaller index first), 4, 3 (inf); 1 (NaN) never; fewer than k: four pairs. q1 (NaN): nothing.
    assert got.tolist() == [[0, 0, 0, 0], [0, 2, 4, 3]]
    assert so.knn(x, y, 2).tolist() == [[0, 0], [0, 2]]
    assert so.knn_loop(x, y, 10).tolist() == got.tolist()
    # two inf distances tie among themselves: the smaller index first
    x2 = np.array([[inf, 0.0], [0.5, 0.0], [-inf, 0.0]], np.float32)
    assert so.knn(x2, np.zeros((1, 2), np.float32), 3).tolist() == [[0, 0, 0], [1, 0, 2]]
    # a batch with fewer points than k is cut short; a batch without candidates gives nothing
    bx = np.array([0, 0, 0, 2, 2])
    by = np.array([0, 1, 2])
    xs = np.array([[0.0], [1.0], [2.0], [5.0], [6.0]], np.float32)
    ys = np.array([[0.9], [0.0], [5.9]], np.float32)
    assert so.knn(xs, ys, 4, bx, by).tolist() == [[0, 0, 0, 2, 2], [1, 0, 2, 4, 3]]
    assert so.nearest(ys, xs, by, bx).tolist() == [1, -1, 4]


def test_radius_and_nearest_known_answers():
    # spacing 1/8 on a line: the points at exactly r = 1/8 are OUTSIDE (strict <); one fp32 ulp above r they are inside
    x = (np.arange(6, dtype=np.float32) / 8).reshape(-1, 1)
    x[4] = np.nan
    y = np.array([[0.25], [np.nan]], np.float32)
    assert so.radius(x, y, 0.125, max_num_neighbors=8).tolist() == [[0], [2]]
    up = float(np.nextafter(np.float32(0.125), np.float32(1)))
    assert so.radius(x, y, up, max_num_neighbors=8).tolist() == [[0, 0, 0], [1, 2, 3]]
    assert so.radius(x, y, up, max_num_neighbors=2).tolist() == [[0, 0], [1, 2]]     # the first two by index
    assert so.radius(x, y, 10.0, max_num_neighbors=8).tolist() == [[0] * 5, [0, 1, 2, 3, 5]]   # NaN never inside
    assert so.radius(x, y, 0.0, max_num_neighbors=8).shape == (2, 0)
    # nearest: ties to the smaller index
    assert so.nearest(np.array([[0.5], [2.0]], np.float32), np.array([[0.0], [1.0], [3.0]], np.float32)).tolist() == [0, 1]


def test_fps_known_answers():
    x = np.array([[0.0], [1.0], [10.0], [4.0], [4.0], [6.0]], np.float32)
    # from 0: 10 (index 2); then 4, 4 and 6 are 4 from a chosen point -> the first maximum, index 3; then 6 (index 5), then 1;
    # every distance is 0 then (the duplicate of 3 included): the first index, 0, again
    assert so.fps(x, None, 1.0, [0]).tolist() == [0, 2, 3, 5, 1, 0]
    assert so.fps(x, None, 0.01, [4]).tolist() == [4]             # ceil(6 * 0.01) = 1
    one = np.array([[3.0, 1.0]], np.float32)
    assert so.fps(one, None, 0.3, [0]).tolist() == [0]           # ceil(0.3) = 1 on a cloud of one point
    b = np.array([0, 0, 0, 1, 1])
    xb = np.array([[0.0], [1.0], [3.0], [7.0], [9.0]], np.float32)
    assert so.fps(xb, b, 1.0, [1, 4]).tolist() == [1, 2, 0, 4, 3]


def test_distance_is_the_float32_sum_in_dimension_order():
    # (1, 2^-12, 2^-12): float32 ((1 + 2^-24) rounds to 1) + 2^-24 -> 1; float64 and a pairwise/reversed order -> 1 + 2^-23
    q = np.zeros((1, 3), np.float32)
    a = np.array([[1.0, 2.0 ** -12, 2.0 ** -12]], np.float32)
    assert so._sqdist32(a, q)[0, 0] == np.float32(1.0)
    # so a point at exactly distance 1 (index 1) ties with it and the smaller index wins; float64 would put a second
    b = np.concatenate([a, np.array([[0.0, 0.0, 1.0]], np.float32)])
    assert so.knn(b, q, 1).tolist() == [[0], [0]]
    b2 = np.concatenate([np.array([[0.0, 0.0, 1.0]], np.float32), a])
    assert so.knn(b2, q, 2).tolist() == [[0, 0], [0, 1]]
    assert so.radius(b2, q, np.sqrt(1.0 + 2.0 ** -23)).tolist() == [[0, 0], [0, 1]]   # r^2 = 1 + 2^-23: both inside
    assert so.radius(b2, q, 1.0).shape == (2, 0)
    assert so.knn_loop(b, q, 1).tolist() == [[0], [0]]
    d64 = ((b.astype(np.float64) - q) ** 2).sum(1)
    assert d64[0] > d64[1]                                       # in float64 the pair ranks the other way


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_half_inputs_answer_as_their_float32_widening(dt):
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(500, 3, generator=g) * 4).to(dt)
    y = (torch.rand(80, 3, generator=g) * 4).to(dt)
    xf, yf = x.float().numpy(), y.float().numpy()
    assert np.array_equal(so.knn(x, y, 16), so.knn(xf, yf, 16))
    assert np.array_equal(so.knn(x, y, 5, cosine=True), so.knn(xf, yf, 5, cosine=True))
    assert np.array_equal(so.radius(x, y, 0.7, max_num_neighbors=40), so.radius(xf, yf, 0.7, max_num_neighbors=40))
    assert np.array_equal(so.nearest(y, x), so.nearest(yf, xf))
    assert np.array_equal(so.fps(x, None, 0.4, [3]), so.fps(xf, None, 0.4, [3]))
    if dt == torch.float16:                                      # numpy float16 arrays widen the same way
        assert np.array_equal(so.knn(x.numpy(), y.numpy(), 16), so.knn(xf, yf, 16))
