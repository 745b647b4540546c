"""gnnops.conv.GraphUNet on the GPU against the float64 chain of unet_chain.py (fp32, hidden 16, depth 1 and 3, a batch of four
graphs of 24-40 nodes and one 300-node graph, sum_res both ways): the selections of every level are exact, the output and every
parameter's gradient within conv_chain.PROJECT_BAR. unet_chain.model_case builds inputs whose scores stay 1e-3 apart at every level
(test_unet_chain_cpu.py checks it), which is what lets perms be demanded exactly. TopKPooling's own cases: test_gcn_gpu.py."""
import pytest
import torch

import chain_harness as ch
import unet_chain as uc
from unet_chain import F32, PROJECT_BAR

pytestmark = pytest.mark.gpu
S = uc.UNET_SHAPES


@pytest.fixture(scope="module")
def reference():
    return {c: uc.model_grads(*c) for c in uc.MODEL_CASES}


def _model(P, depth, sum_res):
    from gnnops.conv import GraphUNet

    model = GraphUNet(S["in"], S["hidden"], S["out"], depth, sum_res=sum_res).cuda()
    assert sorted(model.state_dict()) == sorted(P)
    model.load_state_dict({k: v.float() for k, v in P.items()})
    return model


@pytest.mark.parametrize("graph,depth,sum_res", uc.MODEL_CASES)
def test_graph_unet(graph, depth, sum_res, reference):
    P, x, ei, batch, G = uc.model_case(graph, depth, sum_res)
    want, want_perms, want_g, R = reference[(graph, depth, sum_res)]
    model = _model(P, depth, sum_res)
    xg = x.float().cuda().requires_grad_(True)
    eic, bc = ei.cuda(), (batch.cuda() if graph == "molecules" else None)      # the single graph goes in as batch=None
    out, perms = model(xg, eic, bc, G if bc is not None else None, return_perms=True)
    assert len(perms) == depth
    for got_p, want_p in zip(perms, want_perms):
        assert torch.equal(got_p.cpu(), want_p)
    (out * R.float().cuda()).sum().backward()
    got = {k: p.grad for k, p in model.named_parameters()}
    got.update(x=xg.grad, out=out.detach())
    want_g = dict(want_g, out=want)
    assert set(got) == set(want_g)
    for k, v in got.items():
        ch.judge(f"{graph}-depth{depth}-sum_res{int(sum_res)}", k, v, want_g[k], PROJECT_BAR[F32])
    # a state_dict round trip between two instances, and eval / no_grad against training: bit for bit
    from gnnops.conv import GraphUNet

    other = GraphUNet(S["in"], S["hidden"], S["out"], depth, sum_res=sum_res).cuda()
    other.load_state_dict(model.state_dict())
    with torch.no_grad():
        assert torch.equal(other(xg.detach(), eic, bc), out.detach())
        assert torch.equal(model.eval()(xg.detach(), eic, bc), out.detach())


def test_refusals():
    from gnnops.conv import GCNConv, GraphUNet, TopKPooling

    with pytest.raises(RuntimeError):
        GraphUNet(4, 8, 2, 1)(torch.zeros(3, 4), torch.zeros((2, 0), dtype=torch.long))
    with pytest.raises(NotImplementedError):
        TopKPooling(4, min_score=0.5)
    for kw in ({"cached": True}, {"normalize": False}, {"add_self_loops": False}):
        with pytest.raises(NotImplementedError):
            GCNConv(4, 4, **kw)
