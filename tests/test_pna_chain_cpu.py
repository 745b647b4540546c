"""tests/pna_chain.py (the float64 yardstick of gnnops.conv.edge_aggregate and of PNAConv's training tests) pinned on the CPU:
torch.autograd.gradcheck on a small graph, and one hand-worked destination whose min and max are both attained twice."""
import math

import torch

import pna_chain as pc

F64 = torch.float64
AVG = {"log": 1.3, "lin": 2.5}


def _small_graph():
    # 6 destinations, 15 edges: destination 3 has no edge, destination 4 exactly one
    src = torch.tensor([0, 1, 2, 3, 4, 5, 0, 2, 4, 1, 3, 5, 0, 1, 2])
    dst = torch.tensor([0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 5, 5, 4, 5])
    return torch.stack([src, dst])


def test_gradcheck_add_and_copy():
    ei = _small_graph()
    g = torch.Generator().manual_seed(3)
    q = torch.rand(6, 2, generator=g, dtype=F64).requires_grad_(True)
    p = torch.rand(6, 2, generator=g, dtype=F64).requires_grad_(True)
    w = torch.rand(15, 2, generator=g, dtype=F64).requires_grad_(True)
    add = lambda q, p, w: pc.edge_aggregate("add", q, ei, 6, p=p, w=w, aggr=pc.AGGREGATORS, scalers=pc.SCALERS, avg_deg=AVG)   # noqa: E731
    assert torch.autograd.gradcheck(add, (q, p, w), eps=1e-6, atol=1e-6)
    copy = lambda q: pc.edge_aggregate("copy", q, ei, 6, aggr=("std", "max"))   # noqa: E731
    assert torch.autograd.gradcheck(copy, (q,), eps=1e-6, atol=1e-6)


def test_forward_blocks_and_rows_without_edges():
    ei = _small_graph()
    g = torch.Generator().manual_seed(4)
    q = torch.rand(6, 3, generator=g, dtype=F64)
    out = pc.edge_aggregate("copy", q, ei, 6, aggr=("mean", "min", "max", "std"), scalers=("identity", "linear"), avg_deg=AVG)
    assert out.shape == (6, 2 * 4 * 3)
    m0 = q[ei[0][ei[1] == 0]]                       # destination 0: four edges, scaler block 1 = linear = 4 / 2.5
    want = torch.cat([m0.mean(0), m0.amin(0), m0.amax(0), torch.sqrt(torch.relu((m0 * m0).mean(0) - m0.mean(0) ** 2) + 1e-5)])
    torch.testing.assert_close(out[0], torch.cat([want, want * (4 / 2.5)]), rtol=1e-12, atol=1e-14)
    # no edge: sum / mean / min / max are 0 and std is sqrt(1e-5), times the scalers of deg = 1
    want3 = torch.tensor([0.0, 0, 0, 0, 0, 0, 0, 0, 0] + [math.sqrt(1e-5)] * 3, dtype=F64)
    torch.testing.assert_close(out[3], torch.cat([want3, want3 / 2.5]), rtol=1e-12, atol=1e-14)


def test_a_hand_worked_destination_with_ties():
    """One destination, messages 1, 1, 3, 3 on edges 0 .. 3 (copy): mean 2, var 1. Output blocks sum, mean, min, max, std under
    the scalers identity and amplification (log 5 / 1.3). The min's gradient goes to edge 0 alone, the max's to edge 2 alone."""
    ei = torch.tensor([[0, 1, 2, 3], [0, 0, 0, 0]])
    q = torch.tensor([[1.0], [1.0], [3.0], [3.0]], dtype=F64)
    G = torch.tensor([[0.5, -2.0, 3.0, 5.0, 7.0, 0.25, 1.0, -1.0, 2.0, -3.0]], dtype=F64)
    out, gr = pc.aggregate_grads("copy", {"q": q, "p": None, "w": None}, ei, 1, pc.AGGREGATORS, ("identity", "amplification"), AVG, G)
    f = math.log(5.0) / 1.3
    std = math.sqrt(1.0 + 1e-5)
    torch.testing.assert_close(out, torch.tensor([[8.0, 2.0, 1.0, 3.0, std, 8 * f, 2 * f, f, 3 * f, std * f]], dtype=F64), rtol=1e-13, atol=0)
    ga = [G[0, a] + f * G[0, 5 + a] for a in range(5)]          # sum, mean, min, max, std
    base = ga[0] + ga[1] / 4
    lo, hi = base + ga[4] * (1 - 2) / (4 * std), base + ga[4] * (3 - 2) / (4 * std)
    want = torch.tensor([[lo + ga[2]], [lo], [hi + ga[3]], [hi]], dtype=F64)
    torch.testing.assert_close(gr["q"], want, rtol=1e-13, atol=0)


def test_first_arg_is_the_smallest_edge_id():
    m = torch.tensor([[2.0, 5.0], [1.0, 5.0], [1.0, 4.0], [7.0, 4.0], [7.0, 0.0]], dtype=F64)
    dst = torch.tensor([1, 1, 1, 1, 0])
    assert pc.first_arg(m, dst, 3, False).tolist() == [[4, 4], [1, 2], [5, 5]]
    assert pc.first_arg(m, dst, 3, True).tolist() == [[4, 4], [3, 0], [5, 5]]


def test_equal_messages_and_single_edges_pass_nothing_through_std():
    ei = torch.tensor([[0, 0, 0, 1], [0, 0, 0, 1]])
    q = torch.tensor([[0.5], [2.0]], dtype=F64)
    _, gr = pc.aggregate_grads("copy", {"q": q, "p": None, "w": None}, ei, 2, ("std",), (), None, torch.ones(2, 1, dtype=F64))
    assert gr["q"].tolist() == [[0.0], [0.0]]
