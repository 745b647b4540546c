"""Pooling front end: the selection steps of torch_geometric's TopKPooling / GraphUNet (2.0.2: nn/pool/topk_pool.py `topk`,
`filter_adj`; utils `remove_self_loops`) on csrc/pool.hip. torch_geometric is not available to compare against: parity unpinned.

`topk` is PyG's per-graph top-k without the dense [G, max_n] pad and sort: one wave per small graph, one workgroup per graph of
up to `topk_max_len()` nodes, the radix sort engine beyond. `filter_adj` / `remove_self_loops` are one stable compaction kernel.
Each makes one host read (the size of its result), as the upstream ops do. The selections are not differentiable: a selection has no
gradient (`topk` detaches its score by design), and `filter_adj` refuses an `edge_attr` that requires grad rather than drop it.

`global_add_pool` / `global_mean_pool` / `global_max_pool` are the graph-level read-outs (one row per graph of `batch`) on the
package's differentiable segment / scatter reductions: no kernel of their own.
"""
import torch

from . import _lib
from ._lib import check
from .ops import _check_index, _dtype_code, _on, _require_gpu, _stream
from .segment import rowptr_from_sorted
from .sparse import _coo_rows_cols

ROUTES = {"auto": 0, "on_chip": 1, "long": 2}


def topk_max_len():
    """The longest graph the on-chip route of `topk` orders in LDS."""
    return int(_lib.load().gnnops_segment_topk_max_len())


def filter_tile():
    """Edges per tile of the compaction kernel behind `filter_adj` / `remove_self_loops`."""
    return int(_lib.load().gnnops_filter_edges_tile())


def _topk_ptr(score, ratio, graph_ptr, route="auto"):
    """(perm, out_ptr int32 [G+1]) for an int32 graph pointer; `route` is for tests ("on_chip" / "long" force one)."""
    _require_gpu(score, graph_ptr)
    if score.dim() != 1:
        raise RuntimeError("topk: score must be 1-D (one value per node)")
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)):
        raise TypeError("topk: ratio must be a float in (0, 1] or an integer k >= 1")
    if isinstance(ratio, int):
        k, r = int(ratio), 0.0
        if k < 1:
            raise ValueError("topk: an integer ratio is a node count k >= 1")
    else:
        k, r = 0, float(ratio)
        if not 0.0 < r <= 1.0:
            raise ValueError("topk: a float ratio lies in (0, 1]")
    score = score.detach().contiguous()          # a selection has no gradient
    dt = _dtype_code(score, "topk")
    N, G = score.numel(), graph_ptr.numel() - 1
    dev = score.device
    L = _lib.load()
    out_ptr = torch.empty(G + 1, dtype=torch.int32, device=dev)
    info = torch.empty(2, dtype=torch.int64, device=dev)
    with _on(dev):
        check(L.gnnops_segment_topk_counts(graph_ptr.data_ptr(), G, r, k, out_ptr.data_ptr(), info.data_ptr(), _stream()),
              "topk")
        total, longest = info.tolist()           # the one host read: sizes perm and picks the route
        perm = torch.empty(total, dtype=torch.int64, device=dev)
        code = ROUTES[route]
        ws_bytes = L.gnnops_segment_topk_workspace_bytes(N, longest, code)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
        if total:
            check(L.gnnops_segment_topk(score.data_ptr(), graph_ptr.data_ptr(), out_ptr.data_ptr(), perm.data_ptr(), G, N, longest,
                                        dt, code, ws.data_ptr() if ws is not None else None, ws_bytes, _stream()), "topk")
    return perm, out_ptr


def topk(score, ratio, batch=None, num_graphs=None):
    """torch_geometric.nn.pool.topk_pool.topk(x, ratio, batch) without ``min_score``: the ids of the ceil(ratio * n_g) best-scoring
    nodes of every graph (a float ratio in (0, 1]; the product and the ceil in float32, as upstream) or of its min(k, n_g) best
    (an integer ratio), graph after graph, in descending score; ties go to the lower id. ``batch`` int64 [N], sorted (``None``:
    one graph); ``num_graphs`` saves the host read of ``batch.max()``."""
    _require_gpu(score, batch)
    N = score.numel()
    if batch is None:
        graph_ptr = torch.tensor([0, N], dtype=torch.int32, device=score.device)
    else:
        _check_index(batch, "topk")
        if batch.numel() != N:
            raise RuntimeError("topk: batch has one entry per node")
        if num_graphs is None:
            num_graphs = int(batch.max().item()) + 1 if N else 0
        graph_ptr = rowptr_from_sorted(batch, num_graphs)
    return _topk_ptr(score, ratio, graph_ptr)[0]


def node_map(perm, num_nodes):
    """int32 [num_nodes]: position of a node in ``perm``, -1 for a node that is not in it."""
    _require_gpu(perm)
    _check_index(perm, "node_map")
    perm = perm.contiguous()
    out = torch.empty(num_nodes, dtype=torch.int32, device=perm.device)
    with _on(perm.device):
        check(_lib.load().gnnops_node_map(perm.data_ptr(), perm.numel(), num_nodes, out.data_ptr(), _stream()), "node_map")
    return out


def _filter(edge_index, edge_attr, nmap, drop_self_loops, what):
    _require_gpu(edge_index, edge_attr, nmap)
    if edge_attr is not None and torch.is_grad_enabled() and edge_attr.requires_grad:
        raise NotImplementedError(f"gnnops.{what}: edge_attr requires grad, but the compaction has no backward; detach it")
    edge_index, row, col = _coo_rows_cols(edge_index, what)
    E = edge_index.size(1)
    dev = edge_index.device
    value, row_bytes = None, 0
    if edge_attr is not None:
        if edge_attr.size(0) != E:
            raise RuntimeError(f"{what}: edge_attr has one row per edge")
        _dtype_code(edge_attr, what)
        value = edge_attr.contiguous()
        row_bytes = value.element_size() * (value.numel() // E if E else 1)
    out_index = torch.empty((2, E), dtype=torch.int64, device=dev)
    out_value = torch.empty_like(value) if value is not None else None
    count = torch.empty(1, dtype=torch.int64, device=dev)
    L = _lib.load()
    ws_bytes = L.gnnops_filter_edges_workspace_bytes(E)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    has_rows = value is not None and value.numel() > 0
    with _on(dev):
        check(L.gnnops_filter_edges(row.data_ptr() if E else None, col.data_ptr() if E else None,
                                    value.data_ptr() if has_rows else None, row_bytes,
                                    nmap.data_ptr() if nmap is not None else None, E, int(drop_self_loops),
                                    out_index[0].data_ptr() if E else None, out_index[1].data_ptr() if E else None,
                                    out_value.data_ptr() if has_rows else None, count.data_ptr(), ws.data_ptr(), ws_bytes, _stream()),
              what)
    n = int(count.item())
    return out_index[:, :n], (out_value[:n] if out_value is not None else None)


def filter_adj(edge_index, edge_attr, perm, num_nodes=None):
    """torch_geometric.nn.pool.topk_pool.filter_adj: the edges between kept nodes, relabelled to positions in ``perm``, in their
    original order, with their attributes. Returns views of the surviving length, as `coalesce` does."""
    _require_gpu(perm)
    if num_nodes is None:
        num_nodes = int(edge_index.max().item()) + 1 if edge_index.numel() else 0
    return _filter(edge_index, edge_attr, node_map(perm, num_nodes), False, "filter_adj")


def remove_self_loops(edge_index, edge_attr=None):
    """torch_geometric.utils.remove_self_loops: the edges whose endpoints differ, in their original order."""
    return _filter(edge_index, edge_attr, None, True, "remove_self_loops")


# ---- graph-level pooling: one row per graph of `batch` ------------------------------------------------------------------------
def _global_pool(x, batch, size, reduce):
    from . import autograd

    _require_gpu(x, batch)
    if batch.dim() != 1 or batch.numel() != x.size(0):
        raise RuntimeError(f"global_{reduce}_pool: batch holds one graph id per row of x")
    n = batch.numel()
    is_sorted = True
    if n:       # one host read: the order of batch and, without size, its largest id
        info = torch.stack([(batch[1:] < batch[:-1]).any().to(batch.dtype), batch.max()]).tolist()
        is_sorted = not info[0]
        size = info[1] + 1 if size is None else size
    size = int(size or 0)
    if is_sorted:
        out = autograd.segment_csr(x, rowptr_from_sorted(batch, size), reduce)
    else:
        out = autograd.scatter(x, batch, 0, None, size, reduce)
    return out[0] if isinstance(out, tuple) else out


def global_add_pool(x, batch, size=None):
    """out[g] = sum of the rows of x whose batch id is g (torch_geometric.nn.global_add_pool). A sorted batch goes through
    `rowptr_from_sorted` + `segment_csr`, an unsorted one through `scatter`; a graph without nodes gets a zero row.
    Differentiable in x."""
    return _global_pool(x, batch, size, "sum")


def global_mean_pool(x, batch, size=None):
    """As `global_add_pool`, the mean (a graph without nodes gets a zero row)."""
    return _global_pool(x, batch, size, "mean")


def global_max_pool(x, batch, size=None):
    """As `global_add_pool`, the maximum (a graph without nodes gets a zero row)."""
    return _global_pool(x, batch, size, "max")
