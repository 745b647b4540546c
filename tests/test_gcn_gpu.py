"""gnnops.conv.gcn_propagate / GCNConv / TopKPooling on the GPU against the float64 chain of unet_chain.py: the output and the
gradients of sum(out * R). Bars: conv_chain.PROJECT_BAR for fp32 / fp16; 4 x the chain's own distance from itself
(tests/golden/unet_self_error.json) for bf16 and the heavy table. Selections (perm, batch, the filtered edges) are exact."""
import pytest
import torch

import chain_harness as ch
import unet_chain as uc
from unet_chain import BF16, DNAME, DTYPES, F32, PROJECT_BAR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return uc.load_self_error()


def _place(t, layout, dtype):
    """t as a dense tensor, or as a column block that starts 16-byte aligned / misaligned inside a wider buffer."""
    t = t.to(dtype).cuda()
    if layout == "dense":
        return t.contiguous()
    vec = 16 // t.element_size()
    off = vec if layout == "aligned" else 1
    buf = torch.zeros((t.size(0), t.size(1) + 2 * vec + (0 if layout == "aligned" else 1)), dtype=dtype, device="cuda")
    buf[:, off:off + t.size(1)] = t
    return buf[:, off:off + t.size(1)]


def _run_case(case, dtype, golden):
    import gnnops
    from gnnops.conv import gcn_propagate

    ops, ei, w, n, fill, R = uc.gcn_inputs(case, dtype)
    want, want_g = uc.gcn_case_grads(case, dtype)
    h = _place(ops["h"], case.layout, dtype).detach().requires_grad_(True)
    bias = ops["bias"].to(dtype).cuda().requires_grad_(True) if case.bias else None
    eic = ei.cuda()
    out = gcn_propagate(h, eic, w.cuda() if w is not None else None, n, fill, bias)
    (out.sum() if case.ones else (out * R.to(dtype).cuda()).sum()).backward()
    got = {"out": out.detach(), "h": h.grad, "bias": bias.grad if case.bias else None}
    want_g = dict(want_g, out=want)
    for k, v in got.items():
        if v is not None:           # None: a case without a bias
            ch.judge_case(case, dtype, k, v, want_g[k], golden)
    return out.detach()


CASES = [(c, d) for t in ("shape", "seams", "loops", "weights", "heavy", "plan") for c in uc.TABLES[t] for d in c.dtypes]


@pytest.mark.parametrize("case,dtype", CASES, ids=[c.id(d) for c, d in CASES])
def test_gcn_propagate(case, dtype, golden):
    out = _run_case(case, dtype, golden)
    if case.graph == "loops" and case.weights == "random":      # deg = 0: the row is the bias
        ops = uc.gcn_inputs(case, dtype)[0]
        assert torch.equal(out[uc.LOOP_NODES["dead"]].cpu(), ops["bias"].to(dtype))


def test_plan_cache_off_and_cold_backward(golden):
    import gnnops

    case = uc.SEAMS[0]
    _run_case(case, F32, golden)
    gnnops.set_plan_cache(False)
    try:
        _run_case(case, F32, golden)
    finally:
        gnnops.set_plan_cache(True)
    # a backward whose source plan is built cold: the cache is emptied between forward and backward
    from gnnops.conv import gcn_propagate

    ops, ei, w, n, fill, R = uc.gcn_inputs(case, F32)
    _, want_g = uc.gcn_case_grads(case, F32)
    h = ops["h"].float().cuda().requires_grad_(True)
    out = gcn_propagate(h, ei.cuda(), w.cuda(), n, fill, ops["bias"].float().cuda())
    gnnops.clear_plan_cache()
    (out * R.float().cuda()).sum().backward()
    assert uc.rel_err(h.grad.double().cpu(), want_g["h"]) <= PROJECT_BAR[F32]


def test_edge_weight_requiring_grad_raises():
    from gnnops.conv import gcn_propagate

    ei = torch.tensor([[0, 1], [1, 0]]).cuda()
    with pytest.raises(NotImplementedError, match="edge_weight requires grad"):
        gcn_propagate(torch.zeros(2, 4).cuda(), ei, torch.ones(2, device="cuda", requires_grad=True), 2)


@pytest.mark.parametrize("improved", [False, True])
@pytest.mark.parametrize("dtype", DTYPES, ids=DNAME.get)
def test_gcn_conv_layer(dtype, improved, golden):
    from gnnops.conv import GCNConv

    ops, ei, w, R = uc.conv_inputs(dtype, improved)
    want, want_g = uc.conv_grads(ops, ei, w, improved, R)
    layer = GCNConv(24, 40, improved=improved).cuda().to(dtype)
    assert sorted(layer.state_dict()) == ["bias", "lin.weight"]
    layer.load_state_dict({"lin.weight": ops["lin.weight"].to(dtype), "bias": ops["bias"].to(dtype)})
    x = ops["x"].to(dtype).cuda().requires_grad_(True)
    out = layer(x, ei.cuda(), w.cuda())
    (out * R.to(dtype).cuda()).sum().backward()
    got = {"out": out.detach(), "x": x.grad, "lin.weight": layer.lin.weight.grad, "bias": layer.bias.grad}
    want_g = dict(want_g, out=want)
    for k, v in got.items():
        ch.judge(f"improved{int(improved)}-{DNAME[dtype]}", k, v, want_g[k], PROJECT_BAR.get(dtype), self_bar=dtype == BF16,
                 key=f"conv/improved{int(improved)}/bf16/{k}", recorded=golden)
    with torch.no_grad():
        assert torch.equal(layer.eval()(x.detach(), ei.cuda(), w.cuda()), out.detach())


@pytest.mark.parametrize("C,dtype", uc.POOL_CASES, ids=[f"C{C}-{DNAME[d]}" for C, d in uc.POOL_CASES])
def test_topk_pooling(C, dtype, golden):
    from gnnops.conv import TopKPooling

    x, weight, ei, ea, batch = uc.pool_inputs(uc.POOL_SIZES, C, dtype)
    want, want_g, (w_ei, w_ea, w_batch, w_perm, w_kept, _) = uc.pool_case_grads(C, dtype)
    layer = TopKPooling(C, 0.5, nonlinearity=uc.POOL_NONLINEARITY[dtype]).cuda().to(dtype)
    layer.load_state_dict({"weight": weight.to(dtype)})
    xg = x.to(dtype).cuda().requires_grad_(True)
    out, g_ei, g_ea, g_batch, g_perm, g_kept = layer(xg, ei.cuda(), ea.to(dtype).cuda(), batch.cuda(), len(uc.POOL_SIZES))
    assert torch.equal(g_perm.cpu(), w_perm) and torch.equal(g_batch.cpu(), w_batch)
    assert torch.equal(g_ei.cpu(), w_ei) and torch.equal(g_ea.cpu(), w_ea.to(dtype))
    R = torch.randn(out.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64).to(dtype)
    (out * R.cuda()).sum().backward()
    got = {"out": out.detach(), "x": xg.grad, "weight": layer.weight.grad}
    want_g = dict(want_g, out=want)
    for k, v in got.items():
        ch.judge(f"C{C}-{DNAME[dtype]}", k, v, want_g[k], PROJECT_BAR.get(dtype), self_bar=dtype == BF16, key=f"pool/C{C}/bf16/{k}", recorded=golden)


def test_refusals():
    from gnnops.conv import GCNConv, TopKPooling

    for kw in ({"cached": True}, {"normalize": False}, {"add_self_loops": False}):
        with pytest.raises(NotImplementedError):
            GCNConv(4, 4, **kw)
    with pytest.raises(NotImplementedError):
        TopKPooling(4, min_score=0.1)
    with pytest.raises(RuntimeError):
        GCNConv(4, 4)(torch.zeros(3, 4), torch.zeros((2, 0), dtype=torch.long))
    with pytest.raises(RuntimeError):
        TopKPooling(4)(torch.zeros(3, 4), torch.zeros((2, 0), dtype=torch.long))
