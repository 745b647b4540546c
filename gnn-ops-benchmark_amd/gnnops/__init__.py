"""gnnops — MI355X (gfx950) kernels behind the gnn-ops-benchmark op API.

``import gnnops`` exposes the reference's op signatures on ROCm device tensors (see ops.py).
``gnnops.install()`` additionally routes the ATen ops the reference scripts call by name
(torch.index_select, Tensor.index_add_, torch.gather, Tensor.scatter_add_) to these kernels, and the
sibling packages ``torch_scatter`` / ``torch_sparse`` in this directory provide the import seam
(``from torch_scatter import scatter_add``) — so an unchanged ``op_bm_scripts/benchmark_*.py`` runs on them.
"""
from ._lib import GnnopsError, LIB_PATH, load as load_library
from .ops import (
    Plan,
    index_add_select_sum,
    clear_plan_cache,
    get_plan,
    index_add,
    index_add_,
    index_max,
    index_select_sum,
    scatter_add_,
    scatter_reduce_mul_,
    set_plan_cache,
)
# the differentiable front ends (they ARE the raw ops when nothing requires grad; gnnops.ops.* are the raw forms)
from .autograd import (addmm, gather, index_select, matmul, matmul_tn, segment_matmul, scatter, scatter_add, scatter_max, scatter_mean, scatter_min,
                       scatter_mul, scatter_sum)
from .sparse import (SpmmTiles, coalesce, coalesce_sparse_tensor, sddmm, sort, sparse_mm, spgemm_hash_max_row, spgemm_max_span, spmm, spmm_csr, spmm_reduce, spmm_t, spmm_tiles,
                     spspmm, transpose, transpose_contiguous)
from .segment import (expand_rowptr, gather_coo, gather_csr, rowptr_from_sorted, scatter_log_softmax, scatter_logsumexp, scatter_softmax,
                      scatter_std, segment_coo, segment_csr)
from . import autograd, layers
from .conv import (AttentiveFP, GATConv, GATEConv, GATv2, GATv2Conv, GCNConv, GraphUNet, HeteroLinear, RGCNConv, TopKPooling, edge_attention, edge_attention_v1, gcn_propagate,
                   head_act_norm)
from .pool import filter_adj, global_add_pool, global_max_pool, global_mean_pool, remove_self_loops, topk
from . import pool
from .sparse_tensor import SparseTensor
from .aten import install, uninstall, installed

__all__ = [
    "GnnopsError", "LIB_PATH", "load_library", "Plan", "clear_plan_cache", "gather", "get_plan", "index_add",
    "index_add_", "index_max", "index_select", "index_select_sum", "scatter", "scatter_add", "scatter_add_",
    "scatter_max", "scatter_mean", "scatter_min", "scatter_mul", "scatter_reduce_mul_", "scatter_sum",
    "set_plan_cache", "install", "uninstall", "installed", "coalesce", "coalesce_sparse_tensor", "sort", "sparse_mm",
    "spmm", "spmm_csr", "spmm_tiles", "SpmmTiles", "spmm_t", "sddmm", "expand_rowptr", "spspmm", "spgemm_max_span", "spgemm_hash_max_row", "transpose", "transpose_contiguous", "addmm", "matmul", "matmul_tn", "index_add_select_sum", "segment_csr", "segment_coo", "gather_csr", "gather_coo",
    "rowptr_from_sorted", "scatter_softmax", "scatter_log_softmax", "scatter_logsumexp", "scatter_std", "autograd", "layers", "GATv2Conv", "edge_attention", "GATConv", "GATEConv", "AttentiveFP", "edge_attention_v1",
    "GCNConv", "TopKPooling", "GraphUNet", "gcn_propagate", "pool", "topk", "filter_adj", "remove_self_loops",
    "GATv2", "head_act_norm", "global_add_pool", "global_mean_pool", "global_max_pool", "spmm_reduce", "SparseTensor",
    "segment_matmul", "HeteroLinear", "RGCNConv",
]
