"""unet_chain.py (the float64 restatement the GraphUNet GPU tests compare against) tied to independent formulations: a dense
D^-1/2 (A + L) D^-1/2 X W, torch.autograd.gradcheck, per-graph Python loops, a 5-node pooling level worked by hand, the float32
k formula in numpy — and the promise that lets the GPU tests demand exact selections: scores inside a graph stay apart."""
import json
import math

import numpy as np
import pytest
import torch

import unet_chain as uc
from unet_chain import BF16, DTYPES, F16, F32


def _dense_gcn(x, W, b, ei, w, n, fill):
    A = torch.zeros((n, n), dtype=torch.float64)
    L = torch.full((n,), float(fill), dtype=torch.float64)
    for e in range(ei.size(1)):
        j, i = int(ei[0, e]), int(ei[1, e])
        we = 1.0 if w is None else float(w[e])
        if i == j:
            L[i] = we
        else:
            A[i, j] += we
    A = A + torch.diag(L)
    deg = A.sum(1)
    dis = torch.where(deg > 0, deg.clamp(min=1e-300).pow(-0.5), torch.zeros_like(deg))
    return dis.view(-1, 1) * A * dis.view(1, -1) @ (x @ W.t()) + b


@pytest.mark.parametrize("improved", [False, True])
@pytest.mark.parametrize("weights", ["none", "random"])
def test_gcn_chain_is_the_dense_normalised_product(improved, weights):
    case = uc.GcnCase("t", "t", graph="loops", weights=weights, improved=improved)
    _, ei, w, n, fill, _ = uc.gcn_inputs(case, F32)
    g = torch.Generator().manual_seed(1)
    x, W, b = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((n, 7), (5, 7), (5,)))
    got = uc.gcn_conv({"lin.weight": W, "bias": b}, "", x, ei, w, improved)
    want = _dense_gcn(x, W, b, ei, w, n, fill)
    assert uc.rel_err(got, want) < 1e-13
    if weights == "random":      # node 3's only edge is a self loop of weight 0: the row is the bias
        assert torch.equal(got[uc.LOOP_NODES["dead"]], b)


def test_gcn_chain_gradcheck():
    case = uc.GcnCase("t", "t", graph="loops", K=3)
    ops, ei, w, n, fill, _ = uc.gcn_inputs(case, F32)
    h = ops["h"].clone().requires_grad_(True)
    b = ops["bias"].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda h_, b_: uc.gcn_propagate(h_, ei, w, n, fill, b_), (h, b))


def test_topk_chain_against_a_python_loop():
    g = torch.Generator().manual_seed(3)
    sizes = [0, 1, 2, 9, 0, 17, 64]
    batch = torch.cat([torch.full((n,), i, dtype=torch.long) for i, n in enumerate(sizes)])
    score = torch.randint(-4, 5, (batch.numel(),), generator=g).double() / 4     # many ties
    for ratio in (0.5, 0.8, 1.0, 1e-5, 3):
        perm, out_ptr = uc.topk(score, ratio, batch, len(sizes))
        want, start = [], 0
        for n in sizes:
            k = min(ratio, n) if isinstance(ratio, int) else int(math.ceil(np.float32(ratio) * np.float32(n)))
            order = sorted(range(n), key=lambda i: (-float(score[start + i]), i))
            want += [start + i for i in order[:k]]
            start += n
        assert perm.tolist() == want
        assert int(out_ptr[-1]) == len(want)


def test_filter_adj_chain_against_a_python_loop():
    g = torch.Generator().manual_seed(4)
    n = 30
    ei = torch.randint(0, n, (2, 200), generator=g)
    ea = torch.randn(200, 2, generator=g)
    perm = torch.randperm(n, generator=g)[:11]
    pos = {int(p): i for i, p in enumerate(perm)}
    want = [(pos[int(a)], pos[int(b)], e) for e, (a, b) in enumerate(ei.t().tolist()) if int(a) in pos and int(b) in pos]
    got_i, got_a = uc.filter_adj(ei, ea, perm, n)
    assert got_i.t().tolist() == [[a, b] for a, b, _ in want]
    assert torch.equal(got_a, ea[[e for _, _, e in want]])


def test_one_pool_level_by_hand():
    """5 nodes on a path 0-1-2-3-4, one channel, weight 2 (so score = tanh(x)), ratio 0.5 -> k = 3."""
    x = torch.tensor([[0.1], [-0.3], [0.7], [0.2], [-0.9]], dtype=torch.float64)
    ei = torch.tensor([[0, 1, 1, 2, 2, 3, 3, 4], [1, 0, 2, 1, 3, 2, 4, 3]])
    ea = torch.arange(8, dtype=torch.float64)
    out, ei2, ea2, batch, perm, kept, _ = uc.topk_pooling(x, torch.tensor([[2.0]], dtype=torch.float64), ei, ea,
                                                          torch.zeros(5, dtype=torch.long), 1, 0.5)
    assert perm.tolist() == [2, 3, 0]
    assert torch.allclose(kept, torch.tanh(torch.tensor([0.7, 0.2, 0.1], dtype=torch.float64)))
    assert torch.allclose(out.view(-1), torch.tensor([0.7 * math.tanh(0.7), 0.2 * math.tanh(0.2), 0.1 * math.tanh(0.1)], dtype=torch.float64))
    assert ei2.tolist() == [[0, 1], [1, 0]] and ea2.tolist() == [4.0, 5.0]      # only 2-3 and 3-2 survive, relabelled
    assert batch.tolist() == [0, 0, 0]
    # augment_adj of the path: two-hop neighbours appear, loops go
    a_i, a_w = uc.augment_adj(ei, torch.ones(8, dtype=torch.float64), 5)
    assert [0, 2] in a_i.t().tolist() and [0, 3] not in a_i.t().tolist() and all(a != b for a, b in a_i.t().tolist())
    assert float(a_w[a_i.t().tolist().index([0, 1])]) == 2.0 and float(a_w[a_i.t().tolist().index([0, 2])]) == 1.0


@pytest.mark.parametrize("ratio", uc.TOPK_RATIOS)
def test_float32_k_formula(ratio):
    n = torch.arange(0, 70001)
    want = np.ceil(np.float32(ratio) * n.numpy().astype(np.float32)).astype(np.int64)
    assert np.array_equal(uc.k_of(n, ratio).numpy(), want)
    assert uc.k_of_numpy(12345, ratio) == int(want[12345])
    assert (want <= n.numpy()).all()


@pytest.mark.parametrize("C,dtype", uc.POOL_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_layer_cases_keep_scores_apart(C, dtype):
    x, weight, _, _, batch = uc.pool_inputs(uc.POOL_SIZES, C, dtype)
    score = uc.pool_score(x, weight, uc.POOL_NONLINEARITY[dtype])
    assert uc.min_gap(score, batch, len(uc.POOL_SIZES)) >= uc.GAP[dtype]


@pytest.mark.parametrize("graph,depth,sum_res", uc.MODEL_CASES)
def test_model_cases_keep_scores_apart(graph, depth, sum_res):
    """At every level, inside every graph; and the graphs have the sizes the issue names."""
    sizes = uc.MODEL_GRAPHS[graph]
    assert (len(sizes) == 4 and all(20 <= n <= 40 for n in sizes)) or sizes == (300,)
    assert uc.model_gap(graph, depth, sum_res) >= uc.GAP[F32]


def test_self_error_file_is_current():
    """tests/golden/unet_self_error.json is what write_self_error_table() writes (another host's libm aside: a quarter of itself)."""
    table = uc.self_error_table()
    with open(uc.GOLDEN_FILE) as f:
        golden = json.load(f)
    assert set(golden) == set(table)
    for k, v in table.items():
        assert abs(golden[k] - v) <= 0.25 * max(abs(v), abs(golden[k])) + 1e-12, k
