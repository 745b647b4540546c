"""torch_sparse.SparseTensor, as far as the layers of PyG 2.0.2 use it when they are handed ``adj_t`` instead of ``edge_index``:
construction from COO / CSR, ``t()``, and ``matmul(adj_t, x, reduce)`` on the gfx950 kernels (gnnops.spmm_reduce). What upstream
has and this class does not is listed in INTEGRATION.md. No CPU path.

An object is (structure, value). The structure — entries ordered by (row, col), duplicates kept, the int32 row pointer, the
[2, nnz] index the backward's plans are cached under, and the structure of the transpose — is computed once and shared by
every object derived from it (``set_value``, repeated ``t()``), so a warm ``matmul`` reads nothing back to the host. ``value`` is
kept in the row order like upstream; an unsorted constructor orders it with gnnops.index_select, so gradients reach the caller's
tensor."""
import torch

from . import ops, segment, sparse


def _order(major, minor, n_major, n_minor):
    """Stable order by (major, minor): int64 positions. The key is major * n_minor + minor (upstream's), sorted by our radix sort."""
    if n_major * n_minor >= 1 << 63:
        raise NotImplementedError("gnnops.SparseTensor: sparse sizes whose product reaches 2^63 are not supported")
    return sparse.sort(major * max(n_minor, 1) + minor, stable=True)[1]


class _Structure:
    """Row-ordered entries of an [M, N] matrix: row / col int64 [nnz], rowptr int32 [M + 1]; the rest is made on first use."""

    __slots__ = ("M", "N", "col", "rowptr", "_row", "_rowptr64", "_index", "_t")

    def __init__(self, M, N, row, rowptr, col):
        self.M, self.N, self.col, self._row, self.rowptr = M, N, col, row, rowptr
        self._rowptr64 = self._index = self._t = None
        if self.rowptr is None:
            self.rowptr = segment.rowptr_from_sorted(row, M)

    @property
    def row(self):
        if self._row is None:
            self._row = segment.expand_rowptr(self.rowptr, self.col.numel())
        return self._row

    @property
    def rowptr64(self):
        if self._rowptr64 is None:
            self._rowptr64 = self.rowptr.to(torch.int64)
        return self._rowptr64

    @property
    def index(self):
        if self._index is None:
            self._index = torch.stack([self.row, self.col])
        return self._index

    def transposed(self):
        """(perm int64 [nnz]: entry j of the transpose is entry perm[j] of this structure, the transpose's structure)."""
        if self._t is None:
            perm = _order(self.col, self.row, self.N, self.M)
            t = _Structure(self.N, self.M, ops.index_select(self.col, 0, perm), None, ops.index_select(self.row, 0, perm))
            self._t = (perm, t)
        return self._t


class SparseTensor:
    """torch_sparse.SparseTensor(row=None, rowptr=None, col=None, value=None, sparse_sizes=None, is_sorted=False).

    Give ``row`` (COO) or ``rowptr`` (CSR; its entries are then in row order already) and ``col``; int64 device tensors.
    Unless ``is_sorted``, the entries are ordered by (row, col) with the package's stable sort; duplicates are kept, as
    upstream keeps them. ``value``: [nnz] float32 / float16 / bfloat16 or None. ``sparse_sizes`` None reads the largest row /
    column id back from the device once, as upstream does."""

    def __init__(self, row=None, rowptr=None, col=None, value=None, sparse_sizes=None, is_sorted=False):
        if col is None or (row is None and rowptr is None):
            raise ValueError("SparseTensor: col and one of row / rowptr are required")
        ops._require_gpu(row, rowptr, col, value)
        ops._check_index(col, "SparseTensor")
        if col.dim() != 1 or (row is not None and (row.dim() != 1 or row.numel() != col.numel())):
            raise ValueError("SparseTensor: row and col must be 1-D and of equal length")
        if value is not None and value.size(0) != col.numel():
            raise ValueError("SparseTensor: value.size(0) must equal the number of entries")
        col = col.contiguous()
        if sparse_sizes is None or sparse_sizes[0] is None:
            M = rowptr.numel() - 1 if rowptr is not None else ops.index_max(row) + 1
        else:
            M = int(sparse_sizes[0])
        if sparse_sizes is None or sparse_sizes[1] is None:
            N = ops.index_max(col) + 1
        else:
            N = int(sparse_sizes[1])
        if rowptr is not None:
            if rowptr.dim() != 1 or rowptr.numel() != M + 1:
                raise ValueError("SparseTensor: rowptr must have sparse_sizes[0] + 1 entries")
            rowptr = sparse._rowptr32(rowptr, "SparseTensor")
        elif row is not None:
            ops._check_index(row, "SparseTensor")
            row = row.contiguous()
            if not is_sorted and col.numel():
                perm = _order(row, col, M, N)
                row, col = ops.index_select(row, 0, perm), ops.index_select(col, 0, perm)
                if value is not None:
                    from . import autograd

                    value = autograd.index_select(value, 0, perm)
        self._s = _Structure(M, N, row, rowptr, col)
        self._value = value

    @classmethod
    def _of(cls, structure, value):
        self = object.__new__(cls)
        self._s, self._value = structure, value
        return self

    @classmethod
    def from_edge_index(cls, edge_index, edge_attr=None, sparse_sizes=None, is_sorted=False):
        if edge_index.dim() != 2 or edge_index.size(0) != 2:
            raise ValueError("SparseTensor.from_edge_index: edge_index must have shape [2, nnz]")
        return cls(row=edge_index[0], col=edge_index[1], value=edge_attr, sparse_sizes=sparse_sizes, is_sorted=is_sorted)

    # ---- views of the storage ---------------------------------------------------------------------------------------------
    def coo(self):
        return self._s.row, self._s.col, self._value

    def csr(self):
        return self._s.rowptr64, self._s.col, self._value

    def sparse_sizes(self):
        return self._s.M, self._s.N

    def size(self, dim):
        return self.sparse_sizes()[dim]

    def nnz(self):
        return self._s.col.numel()

    def set_value(self, value, layout=None):
        """A tensor of the same structure with ``value`` [nnz] in the row order (``layout`` None / "coo" / "csr": the same order
        here) or without values (None)."""
        if layout not in (None, "coo", "csr"):
            raise NotImplementedError(f"gnnops.SparseTensor.set_value: layout={layout!r} is not supported (the value is kept in row order)")
        if value is not None:
            ops._require_gpu(value)
            if value.size(0) != self.nnz():
                raise ValueError("SparseTensor.set_value: value.size(0) must equal nnz()")
        return SparseTensor._of(self._s, value)

    def t(self):
        perm, structure = self._s.transposed()
        value = self._value
        if value is not None:
            from . import autograd

            value = autograd.index_select(value, 0, perm)
        return SparseTensor._of(structure, value)

    # ---- products ---------------------------------------------------------------------------------------------------------
    def spmm(self, other, reduce="sum"):
        """self @ other for a dense ``other`` [N, D] or [N], reduced over each row's entries by sum / add / mean / min / max."""
        if isinstance(other, SparseTensor):
            raise NotImplementedError("gnnops.SparseTensor: sparse @ sparse is not built on this class; use torch_sparse.spspmm "
                                      "(gnnops.spspmm) on the COO index and value")
        ops._require_gpu(other)
        if other.dim() not in (1, 2) or other.size(0) != self._s.N:
            raise RuntimeError(f"SparseTensor.matmul: other must be [{self._s.N}, D] or [{self._s.N}], got {tuple(other.shape)}")
        s = self._s
        index = s.index if s.col.numel() else None
        res = sparse.spmm_reduce(s.rowptr, s.col, self._value, other, reduce, index=index)
        return res[0] if isinstance(res, tuple) else res

    def matmul(self, other, reduce="sum"):
        return self.spmm(other, reduce)

    def __matmul__(self, other):
        return self.spmm(other, "sum")

    def __repr__(self):
        return f"SparseTensor(sparse_sizes=({self._s.M}, {self._s.N}), nnz={self.nnz()}, value={'None' if self._value is None else self._value.dtype})"


def matmul(src, other, reduce="sum"):
    """torch_sparse.matmul(src, other, reduce): min / max return the values alone, as upstream does."""
    if not isinstance(src, SparseTensor):
        raise ValueError("torch_sparse.matmul: src must be a SparseTensor")
    return src.spmm(other, reduce)


def _with_arg(src, other, reduce):
    if isinstance(other, SparseTensor):
        return src.spmm(other, reduce)    # raises, naming spspmm
    ops._require_gpu(other)
    s = src._s
    return sparse.spmm_reduce(s.rowptr, s.col, src._value, other, reduce, index=s.index if s.col.numel() else None)


def spmm_sum(src, other):
    return src.spmm(other, "sum")


def spmm_add(src, other):
    return src.spmm(other, "sum")


def spmm_mean(src, other):
    return src.spmm(other, "mean")


def spmm_min(src, other):
    """(out, arg): arg counts positions in src's row-ordered storage; nnz for a row without entries."""
    return _with_arg(src, other, "min")


def spmm_max(src, other):
    return _with_arg(src, other, "max")
