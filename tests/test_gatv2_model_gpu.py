"""gnnops.conv.GATv2 (the reference's GATv2REG on this package's kernels), the refactored GATv2Conv.forward and
gnnops.pool.global_{add, mean, max}_pool. The model runs on the fixture of tests/norm_chain.py (5 graphs of 20 to 40 nodes, input
7, hidden 16, heads 3, 2 layers) against the float64 model there: the eval forward and the train-mode forward + backward with
dropout 0.3, the masks being those of the fixture handed to the model through its one mask function. Bars: fp32 3e-5 and fp16 1e-2
(conv_chain.PROJECT_BAR); bf16 4 x the chain's self error (tests/golden/head_act_norm_self_error.json)."""
import pytest
import torch

import chain_harness as ch
import norm_chain as nc

pytestmark = pytest.mark.gpu

SELF_ERROR = nc.load_self_error()
_REFERENCE = {}


@pytest.fixture(scope="module")
def conv():
    return ch.load_conv()


def _reference(dtype, train):
    key = (dtype, train)
    if key not in _REFERENCE:
        _REFERENCE[key] = nc.model_grads(dtype, train)[:2]
    return _REFERENCE[key]


def _model(conv, dtype):
    P, x, ei, batch, masks = nc.model_fixture()
    model = conv.GATv2(**nc.MODEL)
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == nc.model_state_shapes(7, 16, 2, 3)
    model.load_state_dict(P, strict=True)
    return model.to(dtype).cuda(), x.to(dtype).cuda(), ei.cuda(), batch.cuda(), [m.to(dtype).cuda() for m in masks]


def _judge(dtype, mode, tensor, got, want):
    """bf16: 4 x the recorded self error of the model chain; fp32 / fp16: the project's bar."""
    ch.judge(f"{mode} {nc.DNAME[dtype]}", tensor, got, want, nc.PROJECT_BAR.get(dtype), self_bar=dtype == nc.BF16,
             key=nc.model_key(mode, dtype, tensor), recorded=SELF_ERROR)


@pytest.mark.parametrize("dtype", nc.DTYPES, ids=[nc.DNAME[d] for d in nc.DTYPES])
def test_eval_forward(conv, dtype, monkeypatch):
    model, x, ei, batch, _ = _model(conv, dtype)
    model.eval()
    monkeypatch.setattr(conv, "_feature_scale", lambda *a: pytest.fail("a mask drawn in eval mode"))
    with torch.no_grad():
        out = model(x, ei, batch)
    assert out.shape == (5, 1) and out.dtype == dtype
    _judge(dtype, "eval", "forward", out, _reference(dtype, False)[0])

    class Data:
        pass

    data = Data()
    data.x, data.edge_index, data.batch = x, ei, batch
    with torch.no_grad():
        assert torch.equal(model(data), out)


@pytest.mark.parametrize("dtype", nc.DTYPES, ids=[nc.DNAME[d] for d in nc.DTYPES])
def test_train_step_gradients(conv, dtype, monkeypatch):
    model, x, ei, batch, masks = _model(conv, dtype)
    model.train()
    calls = []

    def recorded(n, channels, p, dt, device):
        calls.append((n, channels, p, dt))
        return masks[len(calls) - 1]

    monkeypatch.setattr(conv, "_feature_scale", recorded)
    out = model(x, ei, batch)
    assert calls == [(x.size(0), 16, nc.P_DROP, dtype)] * 2
    coef = nc._rand(torch.Generator().manual_seed(99), 5, 1)
    (out.float() * coef.cuda()).sum().backward()
    want_out, want = _reference(dtype, True)
    _judge(dtype, "train", "forward", out, want_out)
    named = dict(model.named_parameters())
    for k in nc.used_parameters():
        assert named[k].grad is not None, k
        _judge(dtype, "train", f"d {k}", named[k].grad, want[k])
    for k, prm in named.items():            # the last conv and the last norm: parameters the forward never uses
        if k not in want:
            assert (k.startswith("convs.2.") or k.startswith("lns.1.")) and prm.grad is None, k


def test_the_mask_function(conv):
    torch.manual_seed(3)
    m = conv._feature_scale(1000, 16, 0.3, torch.float16, torch.device("cuda"))
    assert m.shape == (1000, 16) and m.dtype == torch.float16 and not m.requires_grad
    keep = torch.tensor(1.0 / 0.7).to(torch.float16).cuda()
    assert bool(((m == 0) | (m == keep)).all()) and 0.6 < float((m != 0).float().mean()) < 0.8


def test_state_dict_of_the_reference_model_loads(conv):
    shapes = nc.model_state_shapes(9, 32, 3, 4)
    assert len([k for k in shapes if k.startswith("convs.")]) == 4 * 6 and len([k for k in shapes if k.startswith("lns.")]) == 3 * 2
    model = conv.GATv2(9, 32, 0.1, 3, 4)
    res = model.load_state_dict({k: torch.full(s, 0.25) for k, s in shapes.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert float(model.post_mp[0].weight.min()) == 0.25 and float(model.convs[3].att.max()) == 0.25


@pytest.mark.parametrize("dtype", nc.DTYPES, ids=[nc.DNAME[d] for d in nc.DTYPES])
@pytest.mark.parametrize("concat", [False, True], ids=["mean_heads", "concat"])
def test_layer_forward_is_bit_identical_to_its_composition(conv, concat, dtype):
    """GATv2Conv.forward after the refactor = edge_attention + mean + bias composed by hand, as the forward was written before."""
    torch.manual_seed(5)
    H, C, n = 3, 16, 120
    layer = conv.GATv2Conv(7, C, heads=H, concat=concat).to(dtype).cuda()
    with torch.no_grad():
        layer.bias.copy_(torch.rand_like(layer.bias) - 0.5)
    x = (torch.rand(n, 7) - 0.5).to(dtype).cuda()
    ei = torch.randint(0, n, (2, 700)).cuda()
    with torch.no_grad():
        got = layer(x, ei)
        q = torch.nn.functional.linear(x, layer.lin_l.weight, layer.lin_l.bias)
        qp = conv._dense(x.contiguous(), layer._pk_both.get([layer.lin_l.weight, layer.lin_r.weight, layer.lin_l.bias, layer.lin_r.bias],
                                                            [(layer.lin_l.weight, layer.lin_l.bias), (layer.lin_r.weight, layer.lin_r.bias)]))
        assert nc.rel_err(qp[:, :H * C].double(), q.double()) < 2e-2
        keep = ei[0] != ei[1]
        loops = torch.arange(n, device="cuda")
        looped = torch.cat([ei[:, keep], torch.stack([loops, loops])], dim=1).contiguous()
        want = conv.edge_attention(qp[:, :H * C], qp[:, H * C:], layer.att, looped, n, H, 0.2)
        assert torch.equal(layer._attend(x, ei), want)
        if not concat:
            want = want.view(n, H, C).mean(dim=1)
        want = want + layer.bias
    assert torch.equal(got, want)


def _pool_reference(x, batch, G, reduce):
    x = x.double()
    if reduce == "max":
        return torch.zeros((G, x.size(1)), dtype=x.dtype).scatter_reduce_(0, batch.unsqueeze(1).expand(-1, x.size(1)), x, "amax", include_self=False)
    out = torch.zeros((G, x.size(1)), dtype=x.dtype).index_add_(0, batch, x)
    if reduce == "mean":
        out = out / torch.bincount(batch, minlength=G).clamp(min=1).to(x.dtype).unsqueeze(1)
    return out


@pytest.mark.parametrize("order", ["sorted", "unsorted"])
@pytest.mark.parametrize("reduce", ["add", "mean", "max"])
def test_global_pools(reduce, order):
    """Against index_add_ / scatter_reduce in float64: graph 2 of 6 has no node, and size = 8 leaves two more rows empty."""
    import gnnops
    from gnnops import pool

    g = torch.Generator().manual_seed(8)
    batch = torch.cat([torch.full((n,), i, dtype=torch.int64) for i, n in ((0, 30), (1, 1), (3, 77), (4, 20), (5, 9))])
    x = nc._rand(g, batch.numel(), 24)
    if order == "unsorted":
        perm = torch.randperm(batch.numel(), generator=g)
        batch, x = batch[perm], x[perm]
        assert bool((batch[1:] < batch[:-1]).any())
    fn = getattr(pool, f"global_{reduce}_pool")
    assert fn is getattr(gnnops, f"global_{reduce}_pool")
    R = nc._rand(g, 8, 24)
    for size, G in ((None, 6), (8, 8)):
        leaf = x.cuda().requires_grad_(True)
        out = fn(leaf, batch.cuda(), size)
        assert out.shape == (G, 24)
        ref_leaf = x.double().requires_grad_(True)
        want = _pool_reference(ref_leaf, batch, G, reduce)
        assert nc.rel_err(out.detach().double().cpu(), want.detach()) <= nc.PROJECT_BAR[torch.float32]
        assert float(out[2].detach().abs().max()) == 0.0
        (out * R[:G].cuda()).sum().backward()
        (want * R[:G].double()).sum().backward()
        assert nc.rel_err(leaf.grad.double().cpu(), ref_leaf.grad) <= nc.PROJECT_BAR[torch.float32]
    with pytest.raises(RuntimeError, match="no CPU path"):
        fn(x, batch)
