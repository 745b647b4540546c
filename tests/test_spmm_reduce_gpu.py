"""gnnops.spmm_reduce (csrc/spmm_reduce.hip: CSR x dense with mean / min / max, arg positions, trainable) and the torch_sparse
SparseTensor / matmul shim on it, against tests/spmm_reduce_chain.py (pinned on the CPU by test_spmm_reduce_chain_cpu.py).

min / max forward: out and arg equal the ``rnd=dtype`` chain exactly in all three dtypes — the fp32 product is one rounding on both sides,
a product of 16-bit numbers is exact in fp32, rounding the winner is monotone. mean / sum forward and every gradient: conv_chain.rel_err
against the float64 chain at PROJECT_BAR (fp32 3e-5, fp16 1e-2), bf16 at 4 x the chain's recorded self error."""
import functools

import pytest
import torch

import chain_harness as ch
import spmm_reduce_chain as sc

pytestmark = pytest.mark.gpu

DT_IDS = lambda d: sc.DNAME[d]   # noqa: E731
CASE_IDS = lambda c: c.name      # noqa: E731


@functools.lru_cache(maxsize=None)
def chain(case, dtype, reduce, rounded):
    """(out, arg, grads) of the chain, computed once per (case, dtype, reduce) and shared; nobody writes to it."""
    return sc.case_grads(case, dtype, reduce, rnd=dtype if rounded else None)


@functools.lru_cache(maxsize=None)
def table():
    return sc.load_self_error()


def device_operands(case, dtype, grad=True):
    ops, rowptr, col, R = sc.inputs(case, dtype)
    mat = ops["mat"].to(dtype).cuda().requires_grad_(grad)
    value = ops["value"].to(dtype).cuda().requires_grad_(grad) if "value" in ops else None
    return rowptr.cuda(), col.cuda(), value, mat, R.float().cuda()


def run(case, dtype, reduce, backward=True):
    """(out, arg or None, {"mat", "value"?} gradients of sum(out * R)) on the device."""
    import gnnops

    rowptr, col, value, mat, R = device_operands(case, dtype, grad=backward)
    res = gnnops.spmm_reduce(rowptr, col, value, mat, reduce)
    out, arg = res if isinstance(res, tuple) else (res, None)
    assert (arg is not None) == (reduce in ("min", "max"))
    grads = {}
    if backward:
        (out.float() * R).sum().backward()
        grads = {"mat": mat.grad, **({"value": value.grad} if value is not None else {})}
    return out.detach(), arg, grads


def check(case, dtype, reduce, name, got, want):
    """PROJECT_BAR for fp32 / fp16; bf16: 4 x the chain's recorded self error (attention_chain.py's rule)."""
    ch.judge(f"{case.name}-{sc.DNAME[dtype]}-{reduce}", name, got, want, sc.PROJECT_BAR.get(dtype), self_bar=dtype == sc.BF16,
             key=case.key(dtype, reduce, name), recorded=table())


def exact_forward(case, dtype, reduce, out, arg):
    want, want_arg, _ = chain(case, dtype, reduce, True)
    assert out.dtype == dtype and arg.dtype == torch.int64 and out.shape == arg.shape == (case.M, case.D)
    assert torch.equal(arg.cpu(), want_arg), f"arg differs at {int((arg.cpu() != want_arg).sum())} of {arg.numel()} places"
    assert torch.equal(out.cpu(), want.to(dtype)), f"out differs at {int((out.cpu() != want.to(dtype)).sum())} of {out.numel()} places"


# ---- the seams matrix: M = 40, row lengths 0 1 2 7 8 9 15 16 17 63 64 65 129, D = 1 3 4 8 260 520, value none / mixed / negative --------
@pytest.mark.parametrize("reduce", sc.REDUCES)
@pytest.mark.parametrize("dtype", sc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", sc.SEAMS + [sc.TIES], ids=CASE_IDS)
def test_forward_and_gradients_against_the_float64_chain(case, dtype, reduce):
    """One device run per case: min / max forward and arg exactly the rounded chain's (empty rows: out 0, arg nnz), then the forward
    and every gradient against the float64 chain."""
    out, arg, grads = run(case, dtype, reduce)
    if reduce in ("min", "max"):
        exact_forward(case, dtype, reduce, out, arg)
        empty = torch.tensor(case.lengths) == 0
        assert bool(empty.any()) and bool((arg.cpu()[empty] == sum(case.lengths)).all()) and bool((out.cpu()[empty] == 0).all())
    want, _, want_grads = chain(case, dtype, reduce, False)
    check(case, dtype, reduce, "out", out, want)
    assert set(grads) == set(want_grads)
    for k in want_grads:
        check(case, dtype, reduce, k, grads[k], want_grads[k])


# ---- with perm: the kernel's operand, and COO in random order through SparseTensor ------------------------------------------------------
@pytest.mark.parametrize("reduce", sc.REDUCES)
@pytest.mark.parametrize("dtype", sc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", [c for c in sc.SEAMS if c.values == "mixed" and c.D in (3, 8, 260)], ids=CASE_IDS)
def test_perm_operand_gives_the_bits_of_the_row_order(case, dtype, reduce):
    import gnnops

    out0, arg0, grads0 = run(case, dtype, reduce)
    rowptr, _, _, mat, R = device_operands(case, dtype)
    _, col_s, value_s, perm = sc.permuted(case, dtype)
    value = value_s.to(dtype).cuda().requires_grad_(True)
    res = gnnops.spmm_reduce(rowptr, col_s.cuda(), value, mat, reduce, perm=perm.to(torch.int32).cuda())
    out, arg = res if isinstance(res, tuple) else (res, None)
    (out.float() * R).sum().backward()
    assert torch.equal(out, out0) and (arg is None or torch.equal(arg, arg0))       # arg counts in the row order, never perm[j]
    assert torch.equal(mat.grad, grads0["mat"])
    assert torch.equal(value.grad[perm.cuda()], grads0["value"])


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", [c for c in sc.SEAMS if c.D in (3, 8, 520) and c.values != "negative"], ids=CASE_IDS)
def test_sparse_tensor_from_shuffled_coo_equals_is_sorted(case, dtype):
    from torch_sparse import SparseTensor, matmul, spmm_max, spmm_min

    ops, _, _, _ = sc.inputs(case, dtype)
    row, col, value, _ = sc.permuted(case, dtype)
    srow, scol, sval = sc.coo_sorted(row, col, value, case.N)        # the storage a SparseTensor must arrive at
    srowptr = sc.rowptr_of(srow, case.M)
    dev = lambda t: None if t is None else (t.to(dtype) if t.is_floating_point() else t).cuda()   # noqa: E731
    shuffled = SparseTensor(row=dev(row), col=dev(col), value=dev(value), sparse_sizes=(case.M, case.N))
    ordered = SparseTensor(row=dev(srow), col=dev(scol), value=dev(sval), sparse_sizes=(case.M, case.N), is_sorted=True)
    by_rowptr = SparseTensor(rowptr=dev(srowptr), col=dev(scol), value=dev(sval), sparse_sizes=(case.M, case.N))
    for a, b in zip(shuffled.coo() + shuffled.csr(), ordered.coo() + ordered.csr()):
        assert (a is None and b is None) or torch.equal(a, b)
    assert torch.equal(shuffled.csr()[0].cpu(), srowptr) and torch.equal(shuffled.coo()[1].cpu(), scol)
    assert shuffled.nnz() == col.numel() and shuffled.sparse_sizes() == (case.M, case.N) and shuffled.size(1) == case.N
    x = dev(ops["mat"])
    for reduce in sc.REDUCES:
        got = matmul(shuffled, x, reduce=reduce)
        assert torch.equal(got, matmul(ordered, x, reduce=reduce)) and torch.equal(got, by_rowptr.matmul(x, reduce))
        if reduce in ("min", "max"):
            want, want_arg = sc.spmm_reduce(srowptr, scol, None if sval is None else sval.float(), ops["mat"].float(), reduce)
            out, arg = (spmm_max if reduce == "max" else spmm_min)(shuffled, x)
            assert torch.equal(out, got) and torch.equal(arg.cpu(), want_arg) and torch.equal(out.cpu(), want.to(dtype))


# ---- ties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", ["min", "max"])
@pytest.mark.parametrize("dtype", sc.DTYPES, ids=DT_IDS)
def test_ties_go_to_the_smallest_position(dtype, reduce):
    """Rows of one repeated (column, weight) pair: every product of the row is the same number, every arg the row's first position;
    rows that cycle through two or three pairs: the chain's arg (equal products there come from identical pairs only — pinned on the
    CPU)."""
    out, arg, _ = run(sc.TIES, dtype, reduce, backward=False)
    exact_forward(sc.TIES, dtype, reduce, out, arg)
    _, rowptr, _, _ = sc.inputs(sc.TIES, dtype)
    for r in sc.TIE_SINGLE_ROWS:
        assert bool((arg[r].cpu() == rowptr[r]).all()), (r, arg[r].tolist(), int(rowptr[r]))


# ---- one long row, nothing at all ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", ["max", "mean"])
@pytest.mark.parametrize("dtype", sc.DTYPES, ids=DT_IDS)
def test_one_row_longer_than_the_hub_threshold(dtype, reduce):
    assert sc.LONG.lengths[0] > sc.T_HUB
    out, arg, grads = run(sc.LONG, dtype, reduce)
    if reduce == "max":
        exact_forward(sc.LONG, dtype, reduce, out, arg)
    want, _, want_grads = chain(sc.LONG, dtype, reduce, False)
    check(sc.LONG, dtype, reduce, "out", out, want)
    for k in want_grads:
        check(sc.LONG, dtype, reduce, k, grads[k], want_grads[k])


@pytest.mark.parametrize("reduce", sc.REDUCES)
@pytest.mark.parametrize("case", [sc.EMPTY, sc.NO_ROWS], ids=CASE_IDS)
def test_empty_matrix_and_no_rows(case, reduce):
    out, arg, grads = run(case, torch.float32, reduce)
    assert out.shape == (case.M, case.D) and bool((out == 0).all())
    if arg is not None:
        assert arg.shape == (case.M, case.D) and bool((arg == 0).all())        # nnz = 0: the slot of a row without nonzeros
    assert grads["mat"].shape == (case.N, case.D) and bool((grads["mat"] == 0).all())
    assert grads["value"].shape == (0,)


# ---- determinism --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", sc.REDUCES)
def test_two_runs_give_the_same_bits(reduce):
    import gnnops

    g = torch.Generator().manual_seed(17)
    M, N, nnz, D = 3000, 2500, 60000, 64
    row = torch.randint(0, M, (nnz,), generator=g).sort().values
    rowptr = sc.rowptr_of(row, M).cuda()
    col = torch.randint(0, N, (nnz,), generator=g).cuda()
    res = []
    for _ in range(2):
        gg = torch.Generator().manual_seed(18)
        value = torch.randn(nnz, generator=gg).to(torch.bfloat16).cuda().requires_grad_(True)
        mat = torch.randn(N, D, generator=gg).to(torch.bfloat16).cuda().requires_grad_(True)
        R = torch.randn(M, D, generator=gg).cuda()
        r = gnnops.spmm_reduce(rowptr, col, value, mat, reduce)
        out = r[0] if isinstance(r, tuple) else r
        (out.float() * R).sum().backward()
        res.append((out.detach(),) + ((r[1],) if isinstance(r, tuple) else ()) + (value.grad, mat.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ---- the shim ---------------------------------------------------------------------------------------------------------------------------
def _graph(sort, grid=None, seed=23, n_src=70, n_dst=50, e=900, D=24):
    g = torch.Generator().manual_seed(seed)
    ei = torch.stack([torch.randint(0, n_src, (e,), generator=g), torch.randint(0, n_dst, (e,), generator=g)])
    ei[:, 100:130] = ei[:, 200:230]                                    # repeated edges: kept, not merged
    if sort:
        ei = ei[:, torch.sort(ei[0] * n_dst + ei[1], stable=True).indices].contiguous()
    draw = (lambda *s: torch.randn(*s, generator=g)) if grid is None else (lambda *s: torch.randint(-grid, grid + 1, s, generator=g).float() / grid)
    return ei, draw(e), draw(n_src, D), n_src, n_dst


def test_import_surface():
    import torch_sparse
    from torch_sparse import SparseTensor, matmul, spmm_add, spmm_max, spmm_mean, spmm_min, spmm_sum  # noqa: F401

    for name in ("coalesce", "spmm", "spspmm", "transpose", "SparseTensor", "matmul", "spmm_max"):
        assert name in torch_sparse.__all__
    import gnnops

    assert gnnops.SparseTensor is SparseTensor and callable(gnnops.spmm_reduce)


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=DT_IDS)
def test_matmul_equals_spmm_reduce_on_the_same_storage(dtype):
    import gnnops
    from torch_sparse import SparseTensor, matmul

    ei, w, x, n_src, n_dst = _graph(sort=False)
    adj = SparseTensor.from_edge_index(ei.cuda(), w.to(dtype).cuda(), sparse_sizes=(n_src, n_dst))
    rowptr, col, value = adj.csr()
    assert rowptr.dtype == torch.int64 and rowptr.numel() == n_src + 1 and value.dtype == dtype
    xd = torch.randn(n_dst, 24, generator=torch.Generator().manual_seed(5)).to(dtype).cuda()
    for reduce in ("sum", "add", "mean", "min", "max"):
        want = gnnops.spmm_reduce(rowptr, col, value, xd, reduce)
        got = matmul(adj, xd, reduce=reduce)
        assert torch.is_tensor(got), "matmul returns the values alone for min / max, as upstream does"
        assert torch.equal(got, want[0] if isinstance(want, tuple) else want)
    assert torch.equal(adj @ xd, matmul(adj, xd)) and torch.equal(adj.spmm(xd, "mean"), matmul(adj, xd, "mean"))
    assert torch.equal(matmul(adj, xd[:, 0].contiguous(), "max"), matmul(adj, xd[:, :1].contiguous(), "max").squeeze(1))
    plain = adj.set_value(None)
    assert plain.coo()[2] is None and torch.equal(matmul(plain, xd, "max"), gnnops.spmm_reduce(rowptr, col, None, xd, "max")[0])


@pytest.mark.parametrize("sort,grid", [(True, None), (False, 64)], ids=["edges_sorted-random_floats", "edges_shuffled-grid_64"])
def test_transposed_adjacency_sum_equals_spmm_t_bit_for_bit(sort, grid):
    """adj.t() holds the entries by (destination, source); gnnops.spmm_t sums a destination's edges in edge_index order. For an
    edge_index ordered by (source, destination) — what PyG's datasets hold — the two orders are the same and so are the bits, for any
    values. For a shuffled edge_index the orders differ, and the bits agree where the sums are exact: values and features on a grid of
    1 / 64 (products multiples of 2^-12, row sums below 2^6)."""
    import gnnops
    from torch_sparse import SparseTensor, matmul

    ei, w, x, n_src, n_dst = _graph(sort=sort, grid=grid)
    ei, w, x = ei.cuda(), w.cuda(), x.cuda()
    adj_t = SparseTensor.from_edge_index(ei, w, sparse_sizes=(n_src, n_dst)).t()
    assert adj_t.sparse_sizes() == (n_dst, n_src)
    assert torch.equal(matmul(adj_t, x, reduce="sum"), gnnops.spmm_t(ei, w, n_src, n_dst, x))
    adj_1 = SparseTensor.from_edge_index(ei, sparse_sizes=(n_src, n_dst)).t()
    assert torch.equal(matmul(adj_1, x, reduce="sum"), gnnops.spmm_t(ei, None, n_src, n_dst, x))


@pytest.mark.parametrize("reduce", sc.REDUCES)
def test_backward_through_matmul_reaches_x_and_the_edge_weights(reduce):
    from torch_sparse import SparseTensor, matmul

    ei, w, x, n_src, n_dst = _graph(sort=False, grid=1024)
    w = w.cuda().requires_grad_(True)
    x = x.cuda().requires_grad_(True)
    adj_t = SparseTensor.from_edge_index(ei.cuda(), w, sparse_sizes=(n_src, n_dst)).t()
    out = matmul(adj_t, x, reduce=reduce)
    R = torch.randn(n_dst, x.size(1), generator=torch.Generator().manual_seed(2)).cuda()
    (out * R).sum().backward()
    assert x.grad is not None and w.grad is not None and x.grad.shape == x.shape and w.grad.shape == w.shape
    # the same through the chain, on the storage adj_t holds: entries by (destination, source), weights in the caller's order
    order = torch.sort(ei[1] * n_src + ei[0], stable=True).indices
    wl, xl = w.detach().cpu().double().requires_grad_(True), x.detach().cpu().double().requires_grad_(True)
    ref, _ = sc.spmm_reduce(sc.rowptr_of(ei[1][order], n_dst), ei[0][order], wl[order], xl, reduce)
    (ref * R.cpu().double()).sum().backward()
    ch.judge(reduce, "out", out, ref.detach(), sc.PROJECT_BAR[sc.F32])
    ch.judge(reduce, "d x", x.grad, xl.grad, sc.PROJECT_BAR[sc.F32])
    ch.judge(reduce, "d value", w.grad, wl.grad, sc.PROJECT_BAR[sc.F32])


def test_sparse_times_sparse_and_cpu_tensors_raise():
    from torch_sparse import SparseTensor, matmul

    ei, w, x, n_src, n_dst = _graph(sort=False)
    adj = SparseTensor.from_edge_index(ei.cuda(), w.cuda(), sparse_sizes=(n_src, n_dst))
    with pytest.raises(NotImplementedError, match="spspmm"):
        adj @ adj.t()
    with pytest.raises(NotImplementedError, match="spspmm"):
        matmul(adj, adj.t())
    with pytest.raises(RuntimeError, match="no CPU path"):
        SparseTensor.from_edge_index(ei, w)
    with pytest.raises(RuntimeError, match="no CPU path"):
        matmul(adj, torch.rand(n_dst, 4))
