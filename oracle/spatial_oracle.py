"""CPU oracle for the spline-convolution and clustering ops of the reference's list (ops.txt:17-19, 29-41; SURVEY.md §8f
rank 4). TEST INFRASTRUCTURE ONLY: only ``tests/`` may import this module; the product package never does.

PARITY UNPINNED: torch-spline-conv 1.2.1 and torch-cluster 1.5.9 (requirements.txt:214, :210) are neither in the reference
tree nor installed, and the reference holds no script, output or fixture for these ops. The functions restate the packages'
published definitions:
  spline_basis / spline_weighting / spline_conv   SplineCNN (Fey et al., CVPR 2018) closed B-splines of degree 1-3 over
      pseudo-coordinates in [0, 1]; open splines use kernel_size - degree intervals; the product basis over dimensions;
      spline_conv sums at edge_index[0] the weighted x[edge_index[1]], mean-normalised by degree, + root + bias.
      float64 numpy loops (small cases only).
  grid_cluster   voxel index = sum_d trunc((pos_d - start_d) / size_d) * prod_{d' < d} (trunc((end - start) / size) + 1)
  fps            iterative farthest point (squared Euclidean), first maximum on ties
  knn            k smallest (distance, index) per query inside its batch; radius: ascending index, distance^2 < r^2, capped
  nearest        argmin over the batch's candidates

knn / radius / nearest / fps are vectorised numpy in FLOAT32 with the kernels' rounding (csrc/cluster.hip dist2 / cos_dist,
built with -ffp-contract=off), so that integer outputs can be required to be EXACTLY equal, ties included:
  distance   inputs widened to float32 (fp16 / bf16 exactly; torch tensors are accepted for bf16, which numpy lacks), then
             t_d = x_d - y_d, s = t_0 * t_0, s = s + t_1 * t_1, ... in dimension order, every step rounded to float32 — never
             ``.sum(axis)``, whose order numpy does not promise. Cosine: ab, aa, bb accumulated the same way from 0,
             1 - ab / (sqrt(aa) * sqrt(bb)) in float32.
  knn        the k smallest distances of the batch's candidates, ties to the smaller index (stable over index order); a NaN
             distance is never chosen, +inf is a distance like any other and ranks after every finite one; fewer than k
             candidates: fewer pairs. A NaN query therefore gets none.
  radius     d < float32(r * r), r * r computed in double and rounded once (gnnops_radius); the first max_num_neighbors
             by ascending index. NaN is never inside.
  fps        running distance = fmin(previous, d) (the kernel's fminf: a NaN distance leaves it as it was), first maximum.
  nearest    knn with k = 1 and the roles swapped; -1 where a batch has no candidate.
The *_loop functions are the readable definitions, one (query, candidate) pair at a time in float32 scalars; the fast forms
must equal them (tests/test_spatial_oracle_cpu.py).
"""
import itertools

import numpy as np


def _bspline(v, k, m):
    if m == 1:
        return 1 - v if k == 0 else v
    if m == 2:
        return (0.5 * v * v - v + 0.5, -v * v + v + 0.5, 0.5 * v * v)[k]
    return ((1 - v) ** 3 / 6, (3 * v ** 3 - 6 * v * v + 4) / 6, (-3 * v ** 3 + 3 * v * v + 3 * v + 1) / 6, v ** 3 / 6)[k]


def spline_basis(pseudo, kernel_size, is_open_spline, degree):
    pseudo = np.asarray(pseudo, np.float64)
    E, D = pseudo.shape
    S = (degree + 1) ** D
    basis = np.ones((E, S))
    wi = np.zeros((E, S), np.int64)
    for e in range(E):
        for s, ks in enumerate(itertools.product(range(degree + 1), repeat=D)):
            ks = ks[::-1]                                  # dimension 0 is the fastest digit of s
            off = 1
            for d in range(D):
                v = pseudo[e, d] * (int(kernel_size[d]) - degree * int(is_open_spline[d]))
                fl = np.floor(v)
                wi[e, s] += ((int(fl) + ks[d]) % int(kernel_size[d])) * off
                off *= int(kernel_size[d])
                basis[e, s] *= _bspline(v - fl, ks[d], degree)
    return basis, wi


def spline_weighting(x, weight, basis, weight_index):
    x, weight, basis = (np.asarray(t, np.float64) for t in (x, weight, basis))
    out = np.zeros((x.shape[0], weight.shape[2]))
    for e in range(x.shape[0]):
        for s in range(basis.shape[1]):
            out[e] += basis[e, s] * (x[e] @ weight[weight_index[e, s]])
    return out


def spline_conv(x, edge_index, pseudo, weight, kernel_size, is_open_spline, degree=1, norm=True, root_weight=None, bias=None):
    x = np.asarray(x, np.float64)
    row, col = edge_index
    basis, wi = spline_basis(pseudo, kernel_size, is_open_spline, degree)
    msg = spline_weighting(x[col], weight, basis, wi)
    out = np.zeros((x.shape[0], msg.shape[1]))
    np.add.at(out, row, msg)
    if norm:
        deg = np.maximum(np.bincount(row, minlength=x.shape[0]), 1).reshape(-1, 1)
        out = out / deg
    if root_weight is not None:
        out = out + x @ np.asarray(root_weight, np.float64)
    if bias is not None:
        out = out + np.asarray(bias, np.float64)
    return out


def grid_cluster(pos, size, start, end, dtype=np.float32):
    pos = np.asarray(pos, dtype)
    size, start, end = (np.asarray(t, dtype) for t in (size, start, end))
    c = ((pos - start) / size).astype(np.int64)
    nvox = ((end - start) / size).astype(np.int64) + 1
    mult = np.concatenate([[1], np.cumprod(nvox)[:-1]])
    return (c * mult).sum(1)


def _segments(batch, n):
    if batch is None:
        return [np.arange(n)]
    return [np.nonzero(np.asarray(batch) == b)[0] for b in range(int(np.max(batch)) + 1)]


def fps_loop(x, batch, ratio, start):
    """start: first index of every batch (absolute)."""
    x = np.asarray(x, np.float32)
    out = []
    for b, seg in enumerate(_segments(batch, len(x))):
        if len(seg) == 0:
            continue
        k = int(np.ceil(len(seg) * ratio))
        cur = int(start[b])
        dist = np.full(len(seg), np.inf, np.float32)
        chosen = [cur]
        for _ in range(k - 1):
            d = np.array([_dist(x[i], x[cur], False) for i in seg], np.float32)
            dist = np.fmin(dist, d)
            cur = int(seg[np.argmax(dist)])
            chosen.append(cur)
        out += chosen
    return np.array(out, np.int64)


def _dist(a, b, cosine):
    """one (candidate a, query b) distance, float32 scalars step by step: dist2 / cos_dist of csrc/cluster.hip."""
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    f = np.float32
    if cosine:
        ab = aa = bb = f(0)
        for u, v in zip(a, b):
            ab, aa, bb = f(ab + f(u * v)), f(aa + f(u * u)), f(bb + f(v * v))
        return f(f(1) - f(ab / f(f(np.sqrt(aa)) * f(np.sqrt(bb)))))
    s = f(0)
    for u, v in zip(a, b):
        t = f(u - v)
        s = f(s + f(t * t))
    return s


def knn_loop(x, y, k, batch_x=None, batch_y=None, cosine=False):
    rows, cols = [], []
    for j in range(len(y)):
        cand = np.arange(len(x)) if batch_x is None else np.nonzero(np.asarray(batch_x) == batch_y[j])[0]
        d = np.array([_dist(x[i], y[j], cosine) for i in cand])
        order = [o for o in np.lexsort((cand, d)) if not np.isnan(d[o])][:k]
        rows += [j] * len(order)
        cols += list(cand[order])
    return np.array([rows, cols], np.int64)


def radius_loop(x, y, r, batch_x=None, batch_y=None, max_num_neighbors=32):
    rows, cols = [], []
    for j in range(len(y)):
        cand = np.arange(len(x)) if batch_x is None else np.nonzero(np.asarray(batch_x) == batch_y[j])[0]
        hit = [i for i in cand if _dist(x[i], y[j], False) < np.float32(r * r)]
        hit = hit[:max_num_neighbors]
        rows += [j] * len(hit)
        cols += hit
    return np.array([rows, cols], np.int64)


def nearest_loop(x, y, batch_x=None, batch_y=None):
    out = np.zeros(len(x), np.int64)
    for i in range(len(x)):
        cand = np.arange(len(y)) if batch_x is None else np.nonzero(np.asarray(batch_y) == batch_x[i])[0]
        d = np.array([_dist(y[c], x[i], False) for c in cand])
        order = [o for o in np.lexsort((cand, d)) if not np.isnan(d[o])]
        out[i] = cand[order[0]] if order else -1
    return out


# ---- fast forms: vectorised float32 with the kernels' rounding (the rules are in the module header) ----------------------
_CHUNK = 1 << 21        # distance-matrix entries per block of queries: memory stays bounded


def _points32(a):
    """[N, D] float32. fp16 and bf16 widen exactly (a torch tensor is read through .float(), numpy has no bf16)."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().float().numpy()
    a = np.asarray(a)
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    return np.ascontiguousarray(a, dtype=np.float32)


def _sqdist32(xs, ys):
    """[len(ys), len(xs)] squared distances in float32, summed over the dimensions in order (dist2 of csrc/cluster.hip)."""
    s = None
    with np.errstate(invalid="ignore", over="ignore"):        # inf - inf: NaN, never chosen
        for d in range(xs.shape[1]):
            t = xs[None, :, d] - ys[:, None, d]
            t = t * t
            s = t if s is None else s + t
    return s


def _cosdist32(xs, ys):
    """[len(ys), len(xs)] 1 - cos in float32 (cos_dist of csrc/cluster.hip)."""
    ab = np.zeros((len(ys), len(xs)), np.float32)
    aa = np.zeros(len(xs), np.float32)
    bb = np.zeros(len(ys), np.float32)
    for d in range(xs.shape[1]):
        u, v = xs[:, d], ys[:, d]
        ab = ab + u[None, :] * v[:, None]
        aa = aa + u * u
        bb = bb + v * v
    with np.errstate(invalid="ignore", divide="ignore"):        # a NaN or all-zero point: NaN, never chosen
        return np.float32(1) - ab / (np.sqrt(aa)[None, :] * np.sqrt(bb)[:, None])


def _batch_pairs(nx, ny, batch_x, batch_y):
    """(query indices, candidate indices) of every batch, both ascending."""
    if batch_x is None and batch_y is None:
        yield np.arange(ny), np.arange(nx)
        return
    bx, by = np.asarray(batch_x).reshape(-1), np.asarray(batch_y).reshape(-1)
    B = int(max(bx.max() if bx.size else -1, by.max() if by.size else -1)) + 1
    for b in range(B):
        yield np.nonzero(by == b)[0], np.nonzero(bx == b)[0]


def _blocks(qs, n):
    step = max(1, _CHUNK // max(n, 1))
    for q0 in range(0, len(qs), step):
        yield qs[q0:q0 + step]


def _pairs_out(rows, cols):
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    cols = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    o = np.argsort(rows, kind="stable")            # batches in query order; inside a query the blocks' own order
    return np.stack([rows[o], cols[o]]).astype(np.int64)


def _k_smallest(d, k):
    """(row, position) of the k smallest entries of every row of d, ascending, ties to the smaller position, NaN never."""
    kk = min(k, d.shape[1])
    kth = np.partition(d, kk - 1, axis=1)[:, kk - 1]            # NaN sorts last: a NaN here means fewer than kk non-NaN
    lt = d < kth[:, None]
    eq = d == kth[:, None]
    need = kk - lt.sum(1)                                        # ties at the k-th value: the smallest positions
    take = lt | (eq & (np.cumsum(eq, axis=1) <= need[:, None]))
    short = np.isnan(kth)
    if short.any():
        take[short] = ~np.isnan(d[short])
    r, c = np.nonzero(take)
    o = np.lexsort((c, d[r, c], r))
    return r[o], c[o]


def knn(x, y, k, batch_x=None, batch_y=None, cosine=False):
    """[2, M] (query, candidate): for every y its k nearest x of its batch, nearest first, ties to the smaller index."""
    x, y = _points32(x), _points32(y)
    rows, cols = [], []
    for qs, cand in _batch_pairs(len(x), len(y), batch_x, batch_y):
        if len(qs) == 0 or len(cand) == 0:
            continue
        xs = x[cand]
        for q in _blocks(qs, len(cand)):
            d = _cosdist32(xs, y[q]) if cosine else _sqdist32(xs, y[q])
            r, c = _k_smallest(d, int(k))
            rows.append(q[r])
            cols.append(cand[c])
    return _pairs_out(rows, cols)


def radius(x, y, r, batch_x=None, batch_y=None, max_num_neighbors=32):
    """[2, M] (query, candidate): for every y the first max_num_neighbors x of its batch, by index, with d < float32(r * r)."""
    x, y = _points32(x), _points32(y)
    r2 = np.float32(float(r) * float(r))
    rows, cols = [], []
    for qs, cand in _batch_pairs(len(x), len(y), batch_x, batch_y):
        if len(qs) == 0 or len(cand) == 0:
            continue
        xs = x[cand]
        for q in _blocks(qs, len(cand)):
            hit = _sqdist32(xs, y[q]) < r2
            hit &= np.cumsum(hit, axis=1) <= max_num_neighbors
            rr, cc = np.nonzero(hit)                          # row-major: ascending index inside a query
            rows.append(q[rr])
            cols.append(cand[cc])
    return _pairs_out(rows, cols)


def nearest(x, y, batch_x=None, batch_y=None):
    """For every x the index of its nearest y of the same batch (ties: the smaller index; -1 when there is none)."""
    pairs = knn(y, x, 1, batch_y, batch_x)
    out = np.full(len(_points32(x)), -1, np.int64)
    out[pairs[0]] = pairs[1]
    return out


def fps(x, batch, ratio, start):
    """Farthest point sampling; start: first index of every batch (absolute). ceil(n_b * ratio) points per batch."""
    x = _points32(x)
    out = []
    for b, seg in enumerate(_segments(batch, len(x))):
        if len(seg) == 0:
            continue
        k = int(np.ceil(len(seg) * ratio))
        xs = x[seg]
        axes = [np.ascontiguousarray(xs[:, d]) for d in range(xs.shape[1])]
        cur = int(np.nonzero(seg == int(start[b]))[0][0])
        dist = np.full(len(seg), np.inf, np.float32)
        chosen = [cur]
        for _ in range(k - 1):
            s = None
            for d, a in enumerate(axes):
                t = a - xs[cur, d]
                t = t * t
                s = t if s is None else s + t
            np.fmin(dist, s, out=dist)
            cur = int(np.argmax(dist))
            chosen.append(cur)
        out.append(seg[chosen])
    return np.concatenate(out).astype(np.int64) if out else np.zeros(0, np.int64)
