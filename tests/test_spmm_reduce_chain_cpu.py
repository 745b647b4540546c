"""Pins tests/spmm_reduce_chain.py — the yardstick of test_spmm_reduce_gpu.py — against independent statements of the same op on the
CPU: a dense masked torch.amax / amin / mean, torch.autograd.gradcheck, a hand-written tied row, and the recorded self-error table."""
import pytest
import torch

import spmm_reduce_chain as sc


def _dense(rowptr, col, value, mat, reduce):
    """Row by row over a dense [len, D] block of products: no scatter, no positions table."""
    M, D = rowptr.numel() - 1, mat.size(1)
    out = torch.zeros((M, D), dtype=mat.dtype)
    arg = torch.full((M, D), col.numel(), dtype=torch.int64)
    for i in range(M):
        b, e = int(rowptr[i]), int(rowptr[i + 1])
        if b == e:
            continue
        prod = mat[col[b:e]] * (value[b:e].unsqueeze(1) if value is not None else 1.0)
        if reduce == "sum":
            out[i] = prod.sum(0)
        elif reduce == "mean":
            out[i] = prod.mean(0)
        else:
            out[i] = prod.amax(0) if reduce == "max" else prod.amin(0)
            for k in range(D):
                arg[i, k] = b + int((prod[:, k] == out[i, k]).nonzero()[0])
    return out, (arg if reduce in ("min", "max") else None)


SMALL = [c for c in sc.SEAMS if c.D in (1, 3, 8)] + [sc.TIES, sc.EMPTY, sc.NO_ROWS]


@pytest.mark.parametrize("reduce", sc.REDUCES)
@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_chain_equals_dense_masked_reduction(case, reduce):
    ops, rowptr, col, _ = sc.inputs(case, torch.float32)
    out, arg = sc.spmm_reduce(rowptr, col, ops.get("value"), ops["mat"], reduce)
    want, want_arg = _dense(rowptr, col, ops.get("value"), ops["mat"], reduce)
    assert out.shape == (case.M, case.D)
    if reduce in ("min", "max"):
        assert torch.equal(out, want) and torch.equal(arg, want_arg)
    else:
        assert arg is None
        assert sc.rel_err(out, want) <= 1e-14


def test_mean_divides_by_the_number_of_nonzeros_not_the_weights():
    rowptr, col = torch.tensor([0, 2, 2]), torch.tensor([0, 1])
    value, mat = torch.tensor([3.0, 5.0], dtype=torch.float64), torch.tensor([[1.0], [2.0]], dtype=torch.float64)
    out, _ = sc.spmm_reduce(rowptr, col, value, mat, "mean")
    assert out.tolist() == [[(3.0 + 10.0) / 2], [0.0]]


@pytest.mark.parametrize("reduce", sc.REDUCES)
def test_gradcheck_without_ties(reduce):
    g = torch.Generator().manual_seed(3)
    lengths = torch.tensor([3, 0, 5, 1, 4])
    rowptr = torch.zeros(6, dtype=torch.int64)
    rowptr[1:] = lengths.cumsum(0)
    nnz = int(rowptr[-1])
    col = torch.cat([torch.randperm(6, generator=g)[:int(n)] for n in lengths])      # no column twice in a row
    value = (torch.rand(nnz, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    mat = torch.randn(6, 3, generator=g, dtype=torch.float64).requires_grad_(True)
    prod = mat.detach()[col] * value.detach().unsqueeze(1)
    for i in range(5):      # no ties: the products of a row are pairwise apart by far more than gradcheck's step
        p = prod[rowptr[i]:rowptr[i + 1]]
        if p.size(0) > 1:
            assert float((p.unsqueeze(0) - p.unsqueeze(1)).abs().add(torch.eye(p.size(0)).unsqueeze(-1)).min()) > 1e-3
    assert torch.autograd.gradcheck(lambda v, m: sc.spmm_reduce(rowptr, col, v, m, reduce)[0], (value, mat), eps=1e-6, atol=1e-7)


@pytest.mark.parametrize("reduce", ["min", "max"])
def test_tie_goes_to_the_smallest_position_by_hand(reduce):
    # row 0: positions 0..4 hold (col 1, w 2), (col 0, w 1), (col 1, w 2), (col 2, w 4), (col 2, w 4); row 1 is empty; row 2: one entry
    rowptr, col = torch.tensor([0, 5, 5, 6]), torch.tensor([1, 0, 1, 2, 2, 0])
    value = torch.tensor([2.0, 1.0, 2.0, 4.0, 4.0, -1.0], dtype=torch.float64)
    mat = torch.tensor([[8.0, -8.0], [4.0, -4.0], [2.0, -2.0]], dtype=torch.float64)       # products of row 0: all 8 / all -8
    out, arg = sc.spmm_reduce(rowptr, col, value, mat, reduce)
    assert out.tolist() == [[8.0, -8.0], [0.0, 0.0], [-8.0, 8.0]]
    assert arg.tolist() == [[0, 0], [6, 6], [5, 5]]
    # the gradient of a tied element goes to the first position only, and nowhere for the empty row
    v, m = value.clone().requires_grad_(True), mat.clone().requires_grad_(True)
    sc.spmm_reduce(rowptr, col, v, m, reduce)[0].sum().backward()
    assert v.grad.tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]          # 4 - 4 at position 0, 8 - 8 at position 5
    assert m.grad.tolist() == [[-1.0, -1.0], [2.0, 2.0], [0.0, 0.0]]


@pytest.mark.parametrize("reduce", ["min", "max"])
@pytest.mark.parametrize("dtype", sc.DTYPES, ids=lambda d: sc.DNAME[d])
def test_ties_case_is_unambiguous(dtype, reduce):
    """Equal products in the ties matrix come only from identical (column, weight) pairs, and its single-pair rows exist."""
    assert sc.ties_come_from_identical_pairs(sc.TIES, dtype, reduce)
    ops, rowptr, col, _ = sc.inputs(sc.TIES, dtype)
    _, arg = sc.spmm_reduce(rowptr, col, ops["value"], ops["mat"], reduce)
    for r in sc.TIE_SINGLE_ROWS:
        assert int(rowptr[r + 1] - rowptr[r]) >= 2
        assert bool((arg[r] == rowptr[r]).all())
    for r in sc.TIE_MIXED_ROWS:      # a winner that is not the row's first entry occurs too
        assert bool((arg[r] >= rowptr[r]).all()) and bool((arg[r] < rowptr[r + 1]).all())
    assert any(bool((arg[r] != rowptr[r]).any()) for r in sc.TIE_MIXED_ROWS)


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=lambda d: sc.DNAME[d])
def test_rounded_chain_picks_the_float64_chains_winners(dtype):
    """On grid inputs the products are exact in float32: the two chains agree on every arg, and on out up to the store rounding."""
    for case in (sc.SEAMS[4], sc.SEAMS[11], sc.TIES):
        for reduce in ("min", "max"):
            out, arg, _ = sc.case_grads(case, dtype, reduce)
            out_r, arg_r, _ = sc.case_grads(case, dtype, reduce, rnd=dtype)
            assert torch.equal(arg, arg_r)
            assert torch.equal(out.to(dtype), out_r.to(dtype))


def test_coo_sorted_matches_structure_up_to_column_order():
    case = sc.SEAMS[7]
    row, col, value, perm = sc.permuted(case, torch.float32)
    ops, rowptr, col0, _ = sc.inputs(case, torch.float32)
    assert torch.equal(col[perm], col0) and torch.equal(value[perm], ops["value"])
    srow, scol, sval = sc.coo_sorted(row, col, value, case.N)
    assert torch.equal(sc.rowptr_of(srow, case.M), rowptr)
    assert bool((srow[1:] * case.N + scol[1:] >= srow[:-1] * case.N + scol[:-1]).all())
    a, _ = sc.spmm_reduce(rowptr, col0, ops["value"], ops["mat"], "max")
    b, _ = sc.spmm_reduce(rowptr, scol, sval, ops["mat"], "max")
    assert torch.equal(a, b)


def test_recorded_self_error_table_is_current():
    table = sc.load_self_error()
    keys = {c.key(d, r, t) for c, d, r in sc.self_error_cases() for t in (("out", "mat", "value") if c.values != "none" else ("out", "mat"))}
    assert set(table) == keys
    for c, d, r in [(sc.SEAMS[1], sc.BF16, "max"), (sc.SEAMS[10], sc.BF16, "mean"), (sc.TIES, sc.BF16, "min")]:
        for t, v in sc.self_error(c, d, r).items():
            assert table[c.key(d, r, t)] == pytest.approx(v, rel=1e-9, abs=1e-12)
    assert max(table.values()) < 2e-2     # bf16: a few roundings of 2^-9


def test_shim_surface_imports_and_refuses_cpu_tensors():
    """No GPU needed: the names exist, the library exports the entry points, and a CPU tensor raises instead of being emulated."""
    import inspect

    import gnnops
    import torch_sparse
    from torch_sparse import SparseTensor, matmul, spmm_add, spmm_max, spmm_mean, spmm_min, spmm_sum  # noqa: F401

    lib = gnnops.load_library()
    assert hasattr(lib, "gnnops_spmm_reduce") and hasattr(lib, "gnnops_spmm_reduce_grad_terms")
    assert list(inspect.signature(SparseTensor.__init__).parameters)[1:] == ["row", "rowptr", "col", "value", "sparse_sizes", "is_sorted"]
    assert list(inspect.signature(SparseTensor.from_edge_index).parameters) == ["edge_index", "edge_attr", "sparse_sizes", "is_sorted"]
    assert list(inspect.signature(matmul).parameters) == ["src", "other", "reduce"] and inspect.signature(matmul).parameters["reduce"].default == "sum"
    assert list(inspect.signature(gnnops.spmm_reduce).parameters)[:5] == ["rowptr", "col", "value", "matrix", "reduce"]
    assert {"SparseTensor", "matmul", "spmm_sum", "spmm_add", "spmm_mean", "spmm_min", "spmm_max"} <= set(torch_sparse.__all__)
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(RuntimeError, match="no CPU path"):
        SparseTensor.from_edge_index(ei)
    with pytest.raises(RuntimeError, match="no CPU path"):
        gnnops.spmm_reduce(torch.tensor([0, 1, 2]), ei[1], None, torch.rand(2, 4), "max")
    with pytest.raises(ValueError):
        gnnops.spmm_reduce(torch.tensor([0, 1, 2]), ei[1], None, torch.rand(2, 4), "mul")
