"""Tiled SpMM: `gnnops.spmm_tiles` (the plan) and `gnnops.spmm_csr(..., tiles=plan)` (csrc/spmm.hip spmm_tiled_kernel).

The plan is compared element for element with a numpy restatement of its definition (include/gnnops.h, "Tiled SpMM
plan"); the product is required bit-identical to the oracle's sequential fp32 sum AND to the untiled `spmm_csr`: the tiled
kernel forms the same products in the same order and only fetches the operand rows from LDS instead of global memory.

Standard input: M = 2300, n = 3000, 12 nonzeros per row on average, 90 % of a row's columns inside its own block of 500
(five communities), the rest uniform. At the default plan (256 rows, 1024 slots) most nonzeros are staged and some are
not; slots=64 makes every row block overflow, so both operand sources and the cut by reference count are exercised."""
import functools

import numpy as np
import pytest
import torch

from helpers import TORCH_DT, assert_bits_equal, to_np

pytestmark = pytest.mark.gpu

NONE = 0xFFFF


@pytest.fixture(scope="module")
def gnnops():
    import gnnops as g

    g.load_library()
    return g


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o

    return o


def _rowptr_of(row, M):
    rowptr = torch.zeros(M + 1, dtype=torch.int64)
    rowptr[1:] = torch.bincount(row, minlength=M).cumsum(0)
    return rowptr


@functools.lru_cache(maxsize=None)
def _standard():
    """(row, col, rowptr, M, n) on the CPU; row sorted, so (row, col) is the CSR order."""
    g = torch.Generator().manual_seed(42)
    M, n = 2300, 3000
    nnz = 12 * M
    row = torch.sort(torch.randint(0, M, (nnz,), generator=g)).values
    local = (row // 500) * 500 + torch.randint(0, 500, (nnz,), generator=g)
    col = torch.where(torch.rand(nnz, generator=g) < 0.9, local, torch.randint(0, n, (nnz,), generator=g))
    return row, col, _rowptr_of(row, M), M, n


@functools.lru_cache(maxsize=None)
def _standard_gpu():
    row, col, rowptr, M, n = _standard()
    return rowptr.cuda(), col.cuda()


@functools.lru_cache(maxsize=None)
def _standard_plan(slots):
    import gnnops

    rowptr, col = _standard_gpu()
    return gnnops.spmm_tiles(rowptr, col, slots=slots)


@functools.lru_cache(maxsize=None)
def _operands(dname, D, n, nnz, seed=7):
    g = torch.Generator().manual_seed(seed + D)
    val = torch.rand(nnz, generator=g).to(TORCH_DT[dname])
    B = torch.rand(n, D, generator=g).to(TORCH_DT[dname])
    return val, B


def _plan_np(rowptr, col, R, S):
    """The plan's definition, block by block: candidates are the columns referenced at least twice in the block, the S
    most-referenced are staged (ties to the smaller id), stored ascending; every nonzero gets its column's position or
    0xFFFF. Also returns the number of candidates per block."""
    M = len(rowptr) - 1
    nblocks = (M + R - 1) // R
    tile_ptr, tile_cols, ncand = [0], [], []
    slot = np.full(len(col), NONE, dtype=np.uint16)
    for b in range(nblocks):
        lo, hi = int(rowptr[b * R]), int(rowptr[min((b + 1) * R, M)])
        c = col[lo:hi]
        u, cnt = np.unique(c, return_counts=True)
        cu, cc = u[cnt >= 2], cnt[cnt >= 2]
        ncand.append(len(cu))
        order = np.lexsort((cu, -cc))          # by references descending, then column ascending
        staged = np.sort(cu[order[:S]])
        tile_cols.extend(staged.tolist())
        tile_ptr.append(len(tile_cols))
        if len(staged):
            pos = np.minimum(np.searchsorted(staged, c), len(staged) - 1)
            hit = staged[pos] == c
            slot[lo:hi][hit] = pos[hit].astype(np.uint16)
    return np.array(tile_ptr, dtype=np.int32), np.array(tile_cols, dtype=np.int64), slot, np.array(ncand)


def _plan_arrays(t):
    return (t.tile_ptr.cpu().numpy(), t.tile_cols.cpu().numpy(), t.slot.cpu().numpy().view(np.uint16))


def _check_plan(t, rowptr, col):
    """Plan == restatement, and the two properties the kernel relies on. Returns (slot, candidates per block)."""
    rowptr, col = np.asarray(rowptr), np.asarray(col)
    R, S = t.block_rows, t.slots
    tp, tc, sl = _plan_arrays(t)
    etp, etc, esl, ncand = _plan_np(rowptr, col, R, S)
    assert tp.dtype == np.int32 and tc.dtype == np.int64 and sl.dtype == np.uint16
    assert np.array_equal(tp, etp), "tile_ptr"
    assert np.array_equal(tc, etc), "tile_cols"
    assert np.array_equal(sl, esl), "slot"
    M = len(rowptr) - 1
    assert t.M == M and t.nnz == len(col)
    assert (np.diff(tp) <= S).all()
    blk = np.repeat(np.arange(M) // R, np.diff(rowptr))
    staged = sl != NONE
    assert np.array_equal(tc[tp[blk[staged]] + sl[staged]], col[staged]), "a slot names another column"
    for b in range(len(tp) - 1):
        cols_b = col[blk == b]
        for c in tc[tp[b]:tp[b + 1]]:
            assert (cols_b == c).sum() >= 2, f"block {b} stages column {c}, referenced fewer than 2 times"
        assert (np.diff(tc[tp[b]:tp[b + 1]]) > 0).all(), f"block {b}: staged columns not ascending"
    share = staged.mean() if len(col) else 0.0
    assert t.staged_share == pytest.approx(share, abs=1e-12)
    return sl, ncand


def _same_bits(a, b):
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


def _check_product(gnnops, oracle, t, row, col, rowptr_gpu, col_gpu, val, B, M, n, dname, what):
    """tiled == oracle (bits) and tiled == untiled (bits); val may be None."""
    exp = oracle.spmm(torch.stack([row, col]).numpy(), None if val is None else to_np(val), M, n, to_np(B), dtype=dname)
    vg, Bg = (None if val is None else val.cuda()), B.cuda()
    got = gnnops.spmm_csr(rowptr_gpu, col_gpu, vg, Bg, tiles=t)
    assert_bits_equal(to_np(got), exp, what + " vs oracle")
    assert _same_bits(got, gnnops.spmm_csr(rowptr_gpu, col_gpu, vg, Bg, tiles=None)), what + " vs untiled"
    return got


# ------------------------------------------------------------------------------------------------
# 1. the plan
# ------------------------------------------------------------------------------------------------
def test_default_plan_equals_restatement(gnnops):
    row, col, rowptr, M, n = _standard()
    t = _standard_plan(None)
    assert isinstance(t, gnnops.SpmmTiles) and isinstance(t.staged_share, float)
    assert t.block_rows & (t.block_rows - 1) == 0 and t.slots >= 1
    sl, ncand = _check_plan(t, rowptr.numpy(), col.numpy())
    assert t.staged_share > 0.5, t.staged_share
    assert (sl == NONE).any(), "the standard input must leave some nonzeros unstaged"


def test_overflowing_plan_equals_restatement(gnnops):
    row, col, rowptr, M, n = _standard()
    t = _standard_plan(64)
    assert t.slots == 64
    sl, ncand = _check_plan(t, rowptr.numpy(), col.numpy())
    assert (ncand > 64).all(), f"every block must have more candidates than slots: {ncand}"
    assert (np.diff(t.tile_ptr.cpu().numpy()) == 64).all()
    assert 0 < t.staged_share < _standard_plan(None).staged_share


def test_block_rows_is_honoured(gnnops):
    row, col, rowptr, M, n = _standard()
    rp, cg = _standard_gpu()
    t = gnnops.spmm_tiles(rp, cg, block_rows=64, slots=200)
    assert (t.block_rows, t.slots) == (64, 200) and t.tile_ptr.numel() == (M + 63) // 64 + 1
    _check_plan(t, rowptr.numpy(), col.numpy())
    with pytest.raises(ValueError):
        gnnops.spmm_tiles(rp, cg, block_rows=100)
    with pytest.raises(ValueError):
        gnnops.spmm_tiles(rp, cg, slots=0)
    with pytest.raises(ValueError):
        gnnops.spmm_tiles(rp, cg, slots=1 << 16)   # beyond the LDS of one workgroup (and the 16-bit slot)


# ------------------------------------------------------------------------------------------------
# 2. bit-exact product
# ------------------------------------------------------------------------------------------------
# 16-bit: D = 8 one lane of one chunk, 64 exactly one 128-byte chunk, 72 a second chunk of one lane, 256 four chunks,
# 520 a ragged fifth chunk; f32 (4 elements per lane): 4, 36 (chunk of 32 + one lane), 256 (eight chunks).
CASES = [(d, D) for d in ("bf16", "f16") for D in (8, 64, 72, 256, 520)] + [("f32", D) for D in (4, 36, 256)]


@pytest.mark.parametrize("slots", [None, 64])
@pytest.mark.parametrize("dname,D", CASES)
def test_tiled_bit_exact(gnnops, oracle, dname, D, slots):
    row, col, rowptr, M, n = _standard()
    rp, cg = _standard_gpu()
    t = _standard_plan(slots)
    val, B = _operands(dname, D, n, col.numel())
    _check_product(gnnops, oracle, t, row, col, rp, cg, val, B, M, n, dname, f"{dname} D={D} slots={slots}")


@pytest.mark.parametrize("slots", [None, 64])
@pytest.mark.parametrize("dname,D", [("bf16", 256), ("f32", 36)])
def test_tiled_value_none_bit_exact(gnnops, oracle, dname, D, slots):
    row, col, rowptr, M, n = _standard()
    rp, cg = _standard_gpu()
    _, B = _operands(dname, D, n, col.numel())
    _check_product(gnnops, oracle, _standard_plan(slots), row, col, rp, cg, None, B, M, n, dname, f"value=None {dname} D={D}")


@pytest.mark.parametrize("slots", [None, 64])
@pytest.mark.parametrize("rp_dtype", [torch.int32, torch.int64])
def test_tiled_rowptr_dtypes(gnnops, oracle, rp_dtype, slots):
    """The plan is tied to the rowptr OBJECT it was built from, of either dtype."""
    row, col, rowptr, M, n = _standard()
    rp, cg = rowptr.to(rp_dtype).cuda(), _standard_gpu()[1]
    t = gnnops.spmm_tiles(rp, cg, slots=slots)
    assert all(np.array_equal(a, b) for a, b in zip(_plan_arrays(t), _plan_arrays(_standard_plan(slots))))
    val, B = _operands("bf16", 72, n, col.numel())
    _check_product(gnnops, oracle, t, row, col, rp, cg, val, B, M, n, "bf16", f"rowptr {rp_dtype}")


@pytest.mark.parametrize("slots", [None, 64])
def test_rows_off_the_vector_path_fall_through(gnnops, oracle, slots):
    """bf16 D = 7: rows of 14 bytes cannot take 16-byte accesses; the call runs the untiled kernels, same bits."""
    row, col, rowptr, M, n = _standard()
    rp, cg = _standard_gpu()
    val, B = _operands("bf16", 7, n, col.numel())
    _check_product(gnnops, oracle, _standard_plan(slots), row, col, rp, cg, val, B, M, n, "bf16", "bf16 D=7")


# ------------------------------------------------------------------------------------------------
# 3. edges
# ------------------------------------------------------------------------------------------------
def _edge(name):
    """-> (row, col, M, n, block_rows, slots); row sorted."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    rnd = lambda hi, k: torch.randint(0, hi, (k,), generator=g)
    if name == "one_row":
        return torch.zeros(5, dtype=torch.int64), torch.tensor([3, 3, 1, 4, 1]), 1, 6, None, None
    if name == "fewer_rows_than_a_block":
        return torch.sort(rnd(100, 700)).values, rnd(40, 700), 100, 40, None, None
    if name == "last_block_of_one_row":
        row = torch.sort(torch.cat([rnd(129, 800), torch.full((6,), 128)])).values
        col = rnd(50, 806)
        col[-6:] = torch.tensor([4, 4, 9, 9, 1, 2])   # row 128's own nonzeros: two columns referenced twice
        return row, col, 129, 50, 64, None
    if name == "no_nonzeros":
        return torch.empty(0, dtype=torch.int64), torch.empty(0, dtype=torch.int64), 300, 10, None, None
    if name == "empty_block_between_full_ones":
        row = torch.sort(torch.cat([rnd(64, 500), 128 + rnd(64, 500)])).values
        return row, rnd(90, 1000), 192, 90, 64, 16
    if name == "empty_rows":
        return torch.sort(rnd(150, 900) * 2).values, rnd(70, 900), 300, 70, 64, None
    if name == "column_in_every_row_of_a_block":
        row = torch.sort(torch.cat([torch.arange(128), rnd(128, 600)])).values
        col = rnd(400, 728)
        first = torch.ones(728, dtype=torch.bool)
        first[1:] = row[1:] != row[:-1]
        col[first] = 7            # the first nonzero of every row references column 7
        return row, col, 128, 400, 64, 8
    if name == "same_column_twice_in_a_row":
        return torch.tensor([0, 1, 1, 2]), torch.tensor([1, 5, 5, 2]), 3, 9, None, None
    if name == "last_column_staged":
        row = torch.sort(rnd(200, 1500)).values
        col = rnd(300, 1500)
        col[::5] = 299
        return row, col, 200, 300, 64, 4
    raise KeyError(name)


EDGES = ["one_row", "fewer_rows_than_a_block", "last_block_of_one_row", "no_nonzeros", "empty_block_between_full_ones",
         "empty_rows", "column_in_every_row_of_a_block", "same_column_twice_in_a_row", "last_column_staged"]


@pytest.mark.parametrize("name", EDGES)
def test_edges_bit_exact(gnnops, oracle, name):
    row, col, M, n, R, S = _edge(name)
    rowptr = _rowptr_of(row, M)
    rp, cg = rowptr.to(torch.int32).cuda(), col.cuda()
    t = gnnops.spmm_tiles(rp, cg, block_rows=R, slots=S)
    sl, ncand = _check_plan(t, rowptr.numpy(), col.numpy())
    tp, tc, _ = _plan_arrays(t)
    if name == "last_block_of_one_row":
        assert M % t.block_rows == 1 and tp[-1] > tp[-2], "the one-row block must stage something"
    if name == "empty_block_between_full_ones":
        assert tp[2] == tp[1] and tp[1] > 0 and tp[3] > tp[2] and (ncand[[0, 2]] > t.slots).all()
    if name == "column_in_every_row_of_a_block":
        assert 7 in tc[tp[0]:tp[1]] and 7 in tc[tp[1]:tp[2]]
    if name == "same_column_twice_in_a_row":
        assert tc.tolist() == [5] and sl.tolist() == [NONE, 0, 0, NONE]
    if name == "last_column_staged":
        assert all(n - 1 in tc[tp[b]:tp[b + 1]] for b in range(len(tp) - 1)) and (sl == NONE).any()
    if name == "no_nonzeros":
        assert t.staged_share == 0.0 and tp.tolist() == [0, 0, 0]
    for dname, D in (("bf16", 72), ("f32", 4)):
        val, B = _operands(dname, D, n, col.numel(), seed=11)
        got = _check_product(gnnops, oracle, t, row, col, rp, cg, val, B, M, n, dname, f"{name} {dname}")
        assert got.shape == (M, D)


@pytest.mark.parametrize("dname", ["bf16", "f16", "f32"])
def test_non_finite_operand_rows(gnnops, oracle, dname):
    """+-inf and NaN in a staged row of B and in an unstaged one: they travel through LDS and registers alike."""
    M, n, D = 64, 12, 16
    row = torch.sort(torch.arange(64).repeat(3)).values            # 3 nonzeros per row
    col = torch.tensor([2, 5, 3]).repeat(64)                        # columns 2, 5, 3 in every row: staged
    col[3 * 10 + 1] = 9                                             # one reference to column 9: not staged
    col[3 * 40 + 2] = 10                                            # and one to column 10
    rowptr = _rowptr_of(row, M)
    rp, cg = rowptr.cuda(), col.cuda()
    t = gnnops.spmm_tiles(rp, cg)
    sl, _ = _check_plan(t, rowptr.numpy(), col.numpy())
    assert t.tile_cols.tolist() == [2, 3, 5] and sl[31] == NONE and sl[122] == NONE and (sl != NONE).sum() == 190
    val, B = _operands(dname, D, n, col.numel(), seed=3)
    B = B.clone()
    for r in (2, 9):                                                # a staged row and an unstaged row
        B[r, 0], B[r, 1], B[r, 2], B[r, 9] = float("inf"), float("-inf"), float("nan"), float("inf")
    B[3, 0] = float("-inf")                                         # inf + -inf inside rows that take columns 2 and 3
    got = _check_product(gnnops, oracle, t, row, col, rp, cg, val, B, M, n, dname, f"non-finite {dname}")
    nan0 = torch.isnan(got[:, 0])                                   # inf + -inf, except in row 40, which lost column 3
    assert nan0[:40].all() and nan0[41:].all() and got[40, 0] == float("inf")
    assert torch.isinf(got[10, 9]) and torch.isfinite(got[:, 3:9]).all()


# ------------------------------------------------------------------------------------------------
# 4. rows of B that nothing references are never read
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [None, 64])
@pytest.mark.parametrize("dname,D", [("bf16", 72), ("f32", 36)])
def test_unreferenced_rows_are_never_read(gnnops, oracle, dname, D, slots):
    row, col, rowptr, M, n = _standard()
    rp, cg = _standard_gpu()
    val, B = _operands(dname, D, n, col.numel())
    B = B.clone()
    unreferenced = torch.ones(n, dtype=torch.bool)
    unreferenced[col] = False
    assert unreferenced.sum() >= 100          # columns 2500 .. 2999 are reached by the uniform tenth only
    B[unreferenced] = float("nan")
    got = _check_product(gnnops, oracle, _standard_plan(slots), row, col, rp, cg, val, B, M, n, dname, "NaN rows")
    assert torch.isfinite(got).all()


# ------------------------------------------------------------------------------------------------
# 5. refusals
# ------------------------------------------------------------------------------------------------
def test_refusals(gnnops):
    row, col, rowptr, M, n = _standard()
    rp, cg = _standard_gpu()
    t = _standard_plan(None)
    val, B = (x.cuda() for x in _operands("bf16", 64, n, col.numel()))
    with pytest.raises(RuntimeError):
        gnnops.spmm_tiles(rowptr, col)                               # CPU tensors: no CPU path
    with pytest.raises(RuntimeError):
        gnnops.spmm_tiles(rp, col)
    with pytest.raises(RuntimeError):
        gnnops.spmm_csr(rp, cg, val, B.cpu(), tiles=t)
    with pytest.raises(NotImplementedError):
        gnnops.spmm_csr(rp, cg, val.clone().requires_grad_(), B, tiles=t)
    with pytest.raises(NotImplementedError):
        gnnops.spmm_csr(rp, cg, val, B.clone().requires_grad_(), tiles=t)
    with pytest.raises(RuntimeError):
        gnnops.spmm_csr(rp, cg.clone(), val, B, tiles=t)             # equal contents, another tensor
    with pytest.raises(RuntimeError):
        gnnops.spmm_csr(rp.clone(), cg, val, B, tiles=t)
    c2 = cg.clone()
    t2 = gnnops.spmm_tiles(rp, c2)
    gnnops.spmm_csr(rp, c2, val, B, tiles=t2)
    c2[0] = c2[1]                                                    # modified in place: the slots may be stale
    with pytest.raises(RuntimeError):
        gnnops.spmm_csr(rp, c2, val, B, tiles=t2)
    with pytest.raises(RuntimeError):                                # a plan for another matrix shape
        gnnops.spmm_csr(rp[:-1], cg, val, B, tiles=t)


def test_hub_row_is_refused_at_build(gnnops):
    rowptr = torch.tensor([0, 8193, 8193], dtype=torch.int32).cuda()
    col = (torch.arange(8193) % 10).cuda()
    with pytest.raises(ValueError):
        gnnops.spmm_tiles(rowptr, col)
    rowptr = torch.tensor([0, 8192, 8193], dtype=torch.int32).cuda()  # 8192 is still an ordinary row
    assert gnnops.spmm_tiles(rowptr, col).staged_share == 1.0


# ------------------------------------------------------------------------------------------------
# 6. graph capture
# ------------------------------------------------------------------------------------------------
def test_tiled_spmm_in_a_graph(gnnops):
    row, col, rowptr, M, n = _standard()
    rp, cg = rowptr.to(torch.int32).cuda(), _standard_gpu()[1]
    t = gnnops.spmm_tiles(rp, cg)
    gen = torch.Generator(device="cuda").manual_seed(5)
    val = torch.rand(col.numel(), generator=gen, device="cuda").to(torch.bfloat16)
    B = torch.rand(n, 256, generator=gen, device="cuda").to(torch.bfloat16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                    # warm-up outside capture (one-time attribute)
        gnnops.spmm_csr(rp, cg, val, B, tiles=t)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = gnnops.spmm_csr(rp, cg, val, B, tiles=t)
    for trial in range(3):
        B.copy_(torch.rand(n, 256, generator=gen, device="cuda").to(torch.bfloat16))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, gnnops.spmm_csr(rp, cg, val, B, tiles=t)), trial
        assert torch.equal(out, gnnops.spmm_csr(rp, cg, val, B)), trial
