"""The yardstick of the spmm_reduce tests: gnnops.spmm_reduce / torch_sparse.matmul(SparseTensor, dense, reduce) (csrc/spmm_reduce.hip)
restated per nonzero in torch on the CPU, on the row-ordered (CSR) storage:

    prod[e, :] = value[e] * mat[col[e], :]                                    gather, multiply
    sum / mean   index_add_ by row; a mean divides by max(number of nonzeros, 1) — torch_sparse's rule, not the sum of the weights
    min / max    scatter_reduce_ amin / amax by row gives the winner's value; arg[i, k] is the FIRST position of row i whose product
                 equals it (an explicit search: amin over the matching positions), nnz for a row without nonzeros; out is the product
                 gathered at arg (0 for such a row), so that autograd sends the gradient of out[i, k] to position arg[i, k] only

In float64 torch's own autograd differentiates it. ``rnd`` (a torch dtype) runs it the way the library has to for that storage type, as
attention_edge_chain.py does: float32 products (one rounding for fp32 inputs, exact for 16-bit ones), float32 sums in row order
(torch's sequential CPU index_add_), the division in float32, the output rounded once; on the way back the steps of
gnnops.autograd._SpMMReduce with every tensor it materialises rounded: min / max — the per-element terms value[arg] * g and
mat[col[arg], k] * g rounded, summed in float32 by destination, rounded; sum / mean — g / count rounded, then A^T g and the sampled
products <g[row], mat[col]> in float32, rounded. ``self_error`` is the distance between the two chains (tests/golden/
spmm_reduce_self_error.json, ``write_self_error_table`` regenerates it); the bf16 bar of the GPU tests is 4 x that, the rule of
attention_chain.py.

Inputs lie on a grid of 1 / 1024 in [-1, 1] before they are rounded to the storage type: a product of two such numbers is exact in
float32 and in float64, so both chains and the kernel compare the SAME numbers and pick the same winner; with continuous fp32 inputs two
products within an ulp would now and then order differently in float64 and move a whole gradient term."""
import os
from dataclasses import dataclass

import torch

import chain_harness as ch
from chain_harness import BF16, DNAME, DTYPES, F16, F32, PROJECT_BAR, rel_err  # noqa: F401
from conv_chain import _q

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spmm_reduce_self_error.json")
REDUCES = ("sum", "mean", "min", "max")
T_HUB = 8192
SEAM_LENGTHS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 129)    # every seam of the fetch loop (U = 8) and of the 64-id hand-out
SEAM_D = (1, 3, 4, 8, 260, 520)     # single column; element path; 16-B row fp32; 16-B row 16-bit; two chunks fp32; two chunks 16-bit
VALUES = ("none", "mixed", "negative")


def rows_of(rowptr):
    return torch.repeat_interleave(torch.arange(rowptr.numel() - 1), rowptr[1:] - rowptr[:-1])


def spmm_reduce(rowptr, col, value, mat, reduce):
    """(out [M, D], arg int64 [M, D] or None). rowptr / col int64 on the CPU, row-ordered; the dtype of mat is the arithmetic."""
    M, nnz, D = rowptr.numel() - 1, col.numel(), mat.size(1)
    row = rows_of(rowptr)
    prod = mat[col] if value is None else mat[col] * value.unsqueeze(1)
    if reduce in ("sum", "add", "mean"):
        out = torch.zeros((M, D), dtype=mat.dtype).index_add_(0, row, prod)
        if reduce == "mean":
            out = out / (rowptr[1:] - rowptr[:-1]).clamp(min=1).to(mat.dtype).unsqueeze(1)
        return out, None
    ix = row.unsqueeze(1).expand(nnz, D)
    p = prod.detach()
    worst = float("-inf") if reduce == "max" else float("inf")
    win = torch.full((M, D), worst, dtype=mat.dtype).scatter_reduce_(0, ix, p, "amax" if reduce == "max" else "amin", include_self=True)
    pos = torch.where(p == win[row], torch.arange(nnz).unsqueeze(1).expand(nnz, D), torch.full((nnz, D), nnz))
    arg = torch.full((M, D), nnz, dtype=torch.int64).scatter_reduce_(0, ix, pos, "amin", include_self=True)
    out = torch.cat([prod, torch.zeros((1, D), dtype=mat.dtype)]).gather(0, arg)
    return out, arg


def library_backward(rowptr, col, value, mat, reduce, arg, g, rnd):
    """The steps of gnnops.autograd._SpMMReduce.backward on float32 operands, every tensor it materialises rounded to ``rnd``."""
    r = lambda t: _q(t, rnd)   # noqa: E731
    M, nnz, (n, D) = rowptr.numel() - 1, col.numel(), mat.shape
    row = rows_of(rowptr)
    grads = {}
    if nnz == 0:
        return {"mat": torch.zeros_like(mat), **({"value": torch.zeros_like(value)} if value is not None else {})}
    if reduce in ("min", "max"):
        col_x = torch.cat([col, torch.tensor([0])])[arg]
        live = (arg < nnz).to(mat.dtype)
        v = torch.ones((M, D)) if value is None else torch.cat([value, torch.zeros(1)])[arg]
        to_mat = r(v * g) * live
        grads["mat"] = r(torch.zeros((n, D), dtype=torch.float32).scatter_add_(0, col_x, to_mat))
        if value is not None:
            to_val = r(mat.gather(0, col_x) * g) * live
            grads["value"] = r(torch.zeros(nnz + 1, dtype=torch.float32).scatter_add_(0, arg.reshape(-1), to_val.reshape(-1)))[:nnz]
        return grads
    if reduce == "mean":
        g = r(g / (rowptr[1:] - rowptr[:-1]).clamp(min=1).float().unsqueeze(1))
    ge = g[row]
    grads["mat"] = r(torch.zeros((n, D), dtype=torch.float32).index_add_(0, col, ge if value is None else ge * value.unsqueeze(1)))
    if value is not None:
        grads["value"] = r((ge * mat[col]).sum(1))
    return grads


def grads(ops, rowptr, col, reduce, R, rnd=None):
    """ops: {"mat", "value" (or absent)} float64 tensors of storage-rounded values. (out, arg, {name: d sum(out * R)}) as float64."""
    if rnd is None:
        leaf = {k: v.detach().clone().requires_grad_(True) for k, v in ops.items()}
        out, arg = spmm_reduce(rowptr, col, leaf.get("value"), leaf["mat"], reduce)
        if out.requires_grad:
            (out * R).sum().backward()
        return out.detach(), arg, {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}
    f = {k: v.float() for k, v in ops.items()}
    out, arg = spmm_reduce(rowptr, col, f.get("value"), f["mat"], reduce)
    out = _q(out, rnd)
    gr = library_backward(rowptr, col, f.get("value"), f["mat"], reduce, arg, R.float(), rnd)
    return out.double(), arg, {k: v.double() for k, v in gr.items()}


# ---- cases --------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    lengths: tuple          # nonzeros per row
    N: int                  # columns of the sparse operand = rows of the dense one
    D: int
    values: str = "mixed"   # none | mixed | negative | ties
    seed: int = 0

    @property
    def M(self):
        return len(self.lengths)

    def key(self, dtype, reduce, tensor):
        return f"{self.name}/{DNAME[dtype]}/{reduce}/{tensor}"


def _seam_lengths():
    g = torch.Generator().manual_seed(7)
    fill = torch.randint(0, 6, (40 - len(SEAM_LENGTHS),), generator=g).tolist()
    return tuple(SEAM_LENGTHS) + tuple(fill)      # M = 40


SEAMS = [Case(f"seams-D{D}-{v}", _seam_lengths(), 50, D, v, seed=D) for D in SEAM_D for v in VALUES]
LONG = Case("long_row-D8", (9000,), 300, 8, "mixed", seed=3)           # one row above T_HUB
EMPTY = Case("nnz0-D8", (0,) * 5, 6, 8, "mixed")
NO_ROWS = Case("M0-D8", (), 6, 8, "mixed")
# rows whose products are equal by construction: one (column, weight) pair repeated 2 .. 65 times, and rows that interleave two or three
# repeated pairs; the random rows around them keep the row pointer off round numbers
TIES = Case("ties-D12", (3, 2, 8, 9, 17, 65, 0, 6, 9, 40, 5), 20, 12, "ties", seed=5)
TIE_SINGLE_ROWS = (1, 2, 3, 4, 5)         # rows of TIES made of one repeated pair: every arg is the row's first position
TIE_MIXED_ROWS = (7, 8, 9)                # rows that cycle through 2, 3 and 3 pairs
ALL_CASES = SEAMS + [LONG, EMPTY, NO_ROWS, TIES]


def _grid(g, *shape, sign=None):
    t = torch.randint(-1024, 1025, shape, generator=g).float() / 1024
    if sign == "negative":
        t = -(t.abs() + 1 / 1024).clamp(max=1.0)
    return t


def structure(case):
    """(rowptr int64 [M + 1], col int64 [nnz]) in row order; columns repeat within a row (duplicates are kept)."""
    g = torch.Generator().manual_seed(1000 + case.seed)
    lengths = torch.tensor(case.lengths, dtype=torch.int64)
    rowptr = torch.zeros(case.M + 1, dtype=torch.int64)
    rowptr[1:] = lengths.cumsum(0)
    nnz = int(rowptr[-1])
    col = torch.randint(0, case.N, (nnz,), generator=g)
    col[col == 2] = 1                                   # row 2 of the dense operand is never gathered: its gradient is 0
    if case.values == "ties":
        for r in TIE_SINGLE_ROWS:
            col[rowptr[r]:rowptr[r + 1]] = 3 + r
        for r, k in zip(TIE_MIXED_ROWS, (2, 3, 3)):
            n = int(lengths[r])
            col[rowptr[r]:rowptr[r + 1]] = 10 + (torch.arange(n) % k) + r % 2
    return rowptr, col


def inputs(case, dtype):
    """({"mat", "value"?}: float64 tensors of storage-rounded values, rowptr, col, R float64 storage-rounded)."""
    rowptr, col = structure(case)
    g = torch.Generator().manual_seed(2000 + case.seed)
    rd = lambda t: t.to(dtype).double()   # noqa: E731
    ops = {"mat": rd(_grid(g, case.N, case.D))}
    if case.values in ("mixed", "negative"):
        ops["value"] = rd(_grid(g, col.numel(), sign=case.values if case.values == "negative" else None))
    elif case.values == "ties":
        w = _grid(g, case.N)                            # one weight per column: equal columns carry equal weights
        w[w == 0] = 0.5
        ops["value"] = rd(w[col])
    return ops, rowptr, col, rd(_grid(g, case.M, case.D))


def permuted(case, dtype, seed=11):
    """The same matrix as COO in random order: (row, col, value or None) of the shuffled entries, and ``perm`` int64 with
    shuffled[perm[j]] == entry j of the row order of ``structure`` (what the kernel's ``perm`` operand holds). A stable (row, col) sort
    of the shuffled entries is another row order (``structure`` does not sort columns): ``coo_sorted`` gives the one a SparseTensor holds."""
    ops, rowptr, col, _ = inputs(case, dtype)
    row = rows_of(rowptr)
    p = torch.randperm(col.numel(), generator=torch.Generator().manual_seed(seed))
    return row[p], col[p], (ops["value"][p] if "value" in ops else None), torch.argsort(p)


def coo_sorted(row, col, value, N):
    """Entries ordered by (row, col), stable — the storage order of SparseTensor(row, col, value): (row, col, value)."""
    order = torch.sort(row * max(N, 1) + col, stable=True).indices
    return row[order], col[order], (value[order] if value is not None else None)


def rowptr_of(row_sorted, M):
    rowptr = torch.zeros(M + 1, dtype=torch.int64)
    rowptr[1:] = torch.bincount(row_sorted, minlength=M).cumsum(0)
    return rowptr


def ties_come_from_identical_pairs(case, dtype, reduce):
    """True when, for every row and column k, all products equal to the winner belong to entries with the same (column, weight):
    then 'the smallest position among the winners' does not depend on how a product is rounded."""
    ops, rowptr, col, _ = inputs(case, dtype)
    row = rows_of(rowptr)
    value = ops.get("value", torch.ones(col.numel(), dtype=torch.float64))
    out, arg = spmm_reduce(rowptr, col, ops.get("value"), ops["mat"], reduce)
    prod = ops["mat"][col] * value.unsqueeze(1)
    is_win = prod == out[row]
    wc, wv = col[arg.clamp(max=col.numel() - 1)][row], value[arg.clamp(max=col.numel() - 1)][row]     # the winner's pair, per entry
    same = (col.unsqueeze(1) == wc) & (value.unsqueeze(1) == wv)
    return bool((~is_win | same).all())


# ---- self error ---------------------------------------------------------------------------------------------------------------------
def case_grads(case, dtype, reduce, rnd=None):
    ops, rowptr, col, R = inputs(case, dtype)
    return grads(ops, rowptr, col, reduce, R, rnd=rnd)


def self_error(case, dtype, reduce):
    out, _, gr = case_grads(case, dtype, reduce)
    out_r, _, gr_r = case_grads(case, dtype, reduce, rnd=dtype)
    err = {"out": rel_err(out_r, out)}
    for k in gr:
        err[k] = rel_err(gr_r[k], gr[k])
    return err


def self_error_cases():
    return [(c, BF16, r) for c in SEAMS + [LONG, TIES] for r in REDUCES]


def self_error_table():
    return ch.build_table(self_error_cases(), self_error, lambda case, dtype, reduce, tensor: case.key(dtype, reduce, tensor))


def write_self_error_table(path=GOLDEN_FILE):
    """Regenerates tests/golden/spmm_reduce_self_error.json
    (python -c "import spmm_reduce_chain as sc; sc.write_self_error_table()")."""
    return ch.write_table(self_error_table(), path)


def load_self_error():
    return ch.load_table(GOLDEN_FILE)
