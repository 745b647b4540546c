"""Training through torch_spline_conv.{spline_basis, spline_weighting, spline_conv} and gnnops.conv.SplineConv on the GPU.
Every gradient is that of a random linear functional sum(out * R) of the output, compared with torch autograd over the
float64 CPU restatement of the chain (tests/spline_chain.py, tied to oracle/spatial_oracle.py by test_spline_train_cpu.py) on the
same storage-rounded inputs, as max |got - want| / max |want|.

Bars. fp32 3e-5 and fp16 1e-2 are the project's own (tests/test_conv_train_gpu.py). The two that have no precedent are 4 x the
restatement's distance from itself when it is run as a kernel has to run (fp32 arithmetic, intermediates rounded to the storage
type: spline_chain.self_error; the factor 4 is headroom for another summation order and the once-rounded basis * x operand
of the matrix-core contraction). Measured with spline_chain on the CPU, never on the kernels:
    shapes of the grid below (N 500, E 6000, 16 -> 24), worst over the four configurations, norm on/off and the five operands:
        fp32 2.1e-6 (d weight)    fp16 4.8e-4 (d pseudo)    bf16 3.29e-3 (d weight; d pseudo 2.98e-3, d x 2.31e-3)
        -> bf16 bar 1.3e-2
    hub case (E 200 000 edges on one pseudo-coordinate, 8 -> 8, norm off), worst over d x, d pseudo, d weight:
        fp32 1.32e-5 (d weight)   fp16 4.37e-4 (d pseudo)
        -> hub bars fp32 5.3e-5, fp16 1.75e-3
Pseudo-coordinates keep 1e-2 of a cell away from every knot (a degree-1 spline's derivative is one-sided there)."""
import pytest
import torch

import spline_chain as sc

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 3e-5, torch.float16: 1e-2, torch.bfloat16: 1.3e-2}
HUB_TOL = {torch.float32: 5.3e-5, torch.float16: 1.75e-3}
NAMES = ("x", "pseudo", "weight", "root_weight", "bias")
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
_ids = {"ids": lambda v: str(v).replace("torch.", "") if isinstance(v, torch.dtype) else None}


@pytest.fixture(scope="module")
def tsc():
    import torch_spline_conv

    return torch_spline_conv


def _check(got, want, tol, what):
    assert got is not None, f"{what}: no gradient"
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = sc.rel_err(got, want)
    print(f"{what}: {err:.3e} (bar {tol:.1e})")
    assert err <= tol, f"{what}: error {err:.3e} of scale exceeds {tol:.1e}"


def _device(inputs, dtype, requires=NAMES):
    return {k: (v.to(dtype).cuda().requires_grad_(k in requires) if v is not None else None) for k, v in inputs.items()}


def _meta(ks, op):
    return torch.tensor(ks).cuda(), torch.tensor(op, dtype=torch.uint8).cuda()


def _conv_dev(tsc, dev, ei, R, cfg, norm, dtype):
    degree, D, ks, op = cfg
    out = tsc.spline_conv(dev["x"], ei.cuda(), dev["pseudo"], dev["weight"], *_meta(ks, op), degree, norm, dev["root_weight"], dev["bias"])
    (out.float() * R.to(dtype).cuda().float()).sum().backward()
    return out


def _conv_case(tsc, seed, n, e, cfg, m_in, m_out, root, norm, dtype, tol):
    inputs, R, ei = sc.make_inputs(seed, n, e, cfg, m_in, m_out, root, dtype)
    dev = _device(inputs, dtype)
    out = _conv_dev(tsc, dev, ei, R, cfg, norm, dtype)
    want_out, want = sc.conv_grads(inputs, ei, R, cfg[2], cfg[3], cfg[0], norm)
    _check(out, want_out, tol, "out")
    for k, w in want.items():
        _check(dev[k].grad, w, tol, f"d {k}")


@pytest.mark.parametrize("root", [True, False], ids=["root_bias", "bare"])
@pytest.mark.parametrize("norm", [True, False], ids=["norm", "sum"])
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("ci", range(4), ids=[f"deg{c[0]}_D{c[1]}" for c in sc.CONFIGS])
def test_spline_conv_gradients(tsc, ci, dtype, norm, root):
    _conv_case(tsc, 100 + ci, 500, 6000, sc.CONFIGS[ci], 16, 24, root, norm, dtype, TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_spline_conv_gradients_odd_widths(tsc, dtype):
    _conv_case(tsc, 200, 500, 6000, sc.CONFIGS[0], 11, 65, True, True, dtype, TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("ci", range(4), ids=[f"deg{c[0]}_D{c[1]}" for c in sc.CONFIGS])
def test_basis_and_weighting_alone(tsc, ci, dtype):
    degree, D, ks, op = sc.CONFIGS[ci]
    inputs, _, _ = sc.make_inputs(300 + ci, 10, 3000, sc.CONFIGS[ci], 16, 24, False, dtype)
    g = torch.Generator().manual_seed(9)
    E, S = 3000, (degree + 1) ** D
    tol = TOL[dtype]
    # spline_basis: d pseudo
    Rb = (torch.rand(E, S, generator=g) * 2 - 1).to(dtype).double()
    p64 = inputs["pseudo"].clone().requires_grad_(True)
    b64, wi64 = sc.spline_basis(p64, ks, op, degree)
    (b64 * Rb).sum().backward()
    pd = inputs["pseudo"].to(dtype).cuda().requires_grad_(True)
    bd, wid = tsc.spline_basis(pd, *_meta(ks, op), degree)
    assert not wid.requires_grad and torch.equal(wid.cpu(), wi64)
    (bd.float() * Rb.cuda().float()).sum().backward()
    _check(bd, b64.detach(), tol, "basis")
    _check(pd.grad, p64.grad, tol, "d pseudo")
    # spline_weighting: d x, d weight, d basis (x has one row per edge here)
    xe = (torch.rand(E, 16, generator=g) * 2 - 1).to(dtype).double()
    Rw = (torch.rand(E, 24, generator=g) * 2 - 1).to(dtype).double()
    basis_in = b64.detach().to(dtype).double()
    l64 = [t.clone().requires_grad_(True) for t in (xe, inputs["weight"], basis_in)]
    o64 = sc.spline_weighting(l64[0], l64[1], l64[2], wi64)
    (o64 * Rw).sum().backward()
    ld = [t.to(dtype).cuda().requires_grad_(True) for t in (xe, inputs["weight"], basis_in)]
    od = tsc.spline_weighting(ld[0], ld[1], ld[2], wid)
    (od.float() * Rw.cuda().float()).sum().backward()
    _check(od, o64.detach(), tol, "weighting out")
    for name, a, b in zip(("x", "weight", "basis"), ld, l64):
        _check(a.grad, b.grad, tol, f"weighting d {name}")


@pytest.mark.parametrize("only", ["weight", "x", "pseudo"])
def test_partial_graphs(tsc, only):
    cfg = sc.CONFIGS[0]
    inputs, R, ei = sc.make_inputs(400, 200, 2000, cfg, 16, 24, True, torch.float32)
    dev = _device(inputs, torch.float32, requires=(only,))
    _conv_dev(tsc, dev, ei, R, cfg, True, torch.float32)
    _, want = sc.conv_grads(inputs, ei, R, cfg[2], cfg[3], cfg[0], True)
    for k in NAMES:
        if k == only:
            _check(dev[k].grad, want[k], TOL[torch.float32], f"d {k}")
        else:
            assert dev[k].grad is None, k


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], **_ids)
def test_hub_kernel(tsc, dtype):
    """Every edge on the same pseudo-coordinate: both kernels touched collect all 200 000 pairs (25 pieces of 8192)."""
    cfg = (1, 1, [5], [1])
    inputs, R, ei = sc.hub_inputs(dtype)
    dev = _device(inputs, dtype)
    out = _conv_dev(tsc, dev, ei, R, cfg, False, dtype)
    want_out, want = sc.conv_grads(inputs, ei, R, cfg[2], cfg[3], cfg[0], False)
    # the forward here is the existing fused kernel (one fp32 accumulator over ~3000 edges x 2 x 8 terms per output): it is
    # not what this test is about and has no bar of its own at this row length, so its distance is only reported
    print(f"out: {sc.rel_err(out.detach().double().cpu(), want_out):.3e} (reported, not asserted)")
    for k, w in want.items():
        _check(dev[k].grad, w, HUB_TOL[dtype], f"d {k}")
    untouched = want["weight"].abs().amax((1, 2)) == 0
    assert int(untouched.sum()) == 3 and bool((dev["weight"].grad.cpu()[untouched] == 0).all())


def test_mostly_empty_kernel_table(tsc):
    """K = 25^3 kernels, 6000 edges (48 000 pairs): the kernels no pair lands on (about a thousand) get rows of exactly 0.0."""
    cfg = (1, 3, [25, 25, 25], [1, 1, 0])
    inputs, R, ei = sc.make_inputs(500, 300, 6000, cfg, 4, 6, False, torch.float32)
    dev = _device(inputs, torch.float32)
    _conv_dev(tsc, dev, ei, R, cfg, True, torch.float32)
    _, want = sc.conv_grads(inputs, ei, R, cfg[2], cfg[3], cfg[0], True)
    for k, w in want.items():
        _check(dev[k].grad, w, TOL[torch.float32], f"d {k}")
    _, wi = sc.spline_basis(inputs["pseudo"], cfg[2], cfg[3], cfg[0])
    used = torch.zeros(25 ** 3, dtype=torch.bool)
    used[wi.view(-1)] = True
    assert int((~used).sum()) > 100
    got = dev["weight"].grad.cpu()
    assert bool((got[~used] == 0).all()) and not bool(torch.signbit(got[~used]).any())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], **_ids)
def test_backward_is_deterministic(tsc, dtype):
    cfg = sc.CONFIGS[1]
    inputs, R, ei = sc.make_inputs(600, 500, 6000, cfg, 16, 24, True, dtype)
    runs = []
    for _ in range(2):
        dev = _device(inputs, dtype)
        _conv_dev(tsc, dev, ei, R, cfg, True, dtype)
        runs.append({k: dev[k].grad.clone() for k in NAMES})
    for k in NAMES:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_no_grad_results_are_the_raw_bodies(tsc):
    from gnnops import spatial

    cfg = sc.CONFIGS[0]
    degree, D, ks, op = cfg
    inputs, R, ei = sc.make_inputs(700, 200, 2000, cfg, 16, 24, True, torch.float32)
    (ksd, opd), eid = _meta(ks, op), ei.cuda()
    plain = _device(inputs, torch.float32, requires=())
    raw_conv = spatial._spline_conv_raw(plain["x"], eid, plain["pseudo"], plain["weight"], ksd, opd, degree, True, plain["root_weight"], plain["bias"])
    raw_basis, raw_wi = spatial._spline_basis_raw(plain["pseudo"], ksd, opd, degree)
    xe = plain["x"][eid[1]]
    raw_w = spatial._spline_weighting_raw(xe, plain["weight"], raw_basis, raw_wi)
    for params_require_grad in (False, True):
        t = _device(inputs, torch.float32, requires=NAMES if params_require_grad else ())
        with torch.set_grad_enabled(not params_require_grad):   # grad-requiring operands under no_grad; plain operands with grad mode on
            out = tsc.spline_conv(t["x"], eid, t["pseudo"], t["weight"], ksd, opd, degree, True, t["root_weight"], t["bias"])
            b, wi = tsc.spline_basis(t["pseudo"], ksd, opd, degree)
            w = tsc.spline_weighting(xe, t["weight"], raw_basis, raw_wi)
        assert not out.requires_grad and not b.requires_grad and not w.requires_grad
        assert torch.equal(out, raw_conv) and torch.equal(b, raw_basis) and torch.equal(wi, raw_wi) and torch.equal(w, raw_w)
    # and with a graph attached the forward values are still the same kernel's
    t = _device(inputs, torch.float32)
    out = tsc.spline_conv(t["x"], eid, t["pseudo"], t["weight"], ksd, opd, degree, True, t["root_weight"], t["bias"])
    assert out.requires_grad and torch.equal(out.detach(), raw_conv)


def test_empty_and_one_dimensional_forms(tsc):
    ks, op = _meta([5], [1])
    g = torch.Generator().manual_seed(1)
    # E = 0: the spline part contributes nothing, gradients are zeros of the operands' shapes
    x = torch.rand(7, 3, generator=g).cuda().requires_grad_(True)
    w = torch.rand(5, 3, 4, generator=g).cuda().requires_grad_(True)
    p = torch.zeros(0, 1).cuda().requires_grad_(True)
    out = tsc.spline_conv(x, torch.zeros(2, 0, dtype=torch.int64).cuda(), p, w, ks, op, 1, True)
    assert tuple(out.shape) == (7, 4) and not bool(out.any())
    out.sum().backward()
    assert tuple(x.grad.shape) == (7, 3) and not bool(x.grad.any())
    assert tuple(w.grad.shape) == (5, 3, 4) and not bool(w.grad.any())
    assert tuple(p.grad.shape) == (0, 1)
    # x 1-D (one channel) and pseudo 1-D (one coordinate)
    n, e = 30, 200
    ei = sc.graph(2, n, e)
    x1 = torch.rand(n, generator=g) * 2 - 1
    p1 = sc.pseudo_coords(g, e, 1, [5], [1])[:, 0]
    w1 = torch.rand(5, 1, 4, generator=g) - 0.5
    R = torch.rand(n, 4, generator=g).double()
    xd, pd, wd = (t.cuda().requires_grad_(True) for t in (x1, p1, w1))
    out = tsc.spline_conv(xd, ei.cuda(), pd, wd, ks, op, 1, True)
    (out.float() * R.cuda().float()).sum().backward()
    inputs = {"x": x1.double().unsqueeze(1), "pseudo": p1.double().unsqueeze(1), "weight": w1.double(), "root_weight": None, "bias": None}
    want_out, want = sc.conv_grads(inputs, ei, R.float().double(), [5], [1], 1, True)
    _check(out, want_out, 3e-5, "out")
    _check(xd.grad, want["x"][:, 0], 3e-5, "d x (1-D)")
    _check(pd.grad, want["pseudo"][:, 0], 3e-5, "d pseudo (1-D)")
    _check(wd.grad, want["weight"], 3e-5, "d weight")


@pytest.mark.parametrize("aggr", ["mean", "add"])
def test_spline_conv_layer_gradients(aggr):
    from gnnops.conv import SplineConv

    torch.manual_seed(3)
    cfg = (2, 2, [4, 4], [1, 1])
    inputs, R, ei = sc.make_inputs(800, 300, 3000, cfg, 8, 12, True, torch.float32)
    layer = SplineConv(8, 12, dim=2, kernel_size=4, is_open_spline=True, degree=2, aggr=aggr).cuda()
    with torch.no_grad():
        layer.bias.uniform_(-1, 1)
    x = inputs["x"].float().cuda().requires_grad_(True)
    ea = inputs["pseudo"].float().cuda().requires_grad_(True)
    out = layer(x, ei.flip(0).cuda(), ea)          # PyG flow: edge_index = (source, target); spline_chain sums at row 0
    (out * R.float().cuda()).sum().backward()
    ref_in = {"x": inputs["x"], "pseudo": inputs["pseudo"], "weight": layer.weight.detach().double().cpu(),
              "root_weight": layer.root.detach().double().cpu(), "bias": layer.bias.detach().double().cpu()}
    want_out, want = sc.conv_grads(ref_in, ei, R, cfg[2], cfg[3], cfg[0], aggr == "mean")
    _check(out, want_out, 3e-5, "out")
    for name, got in (("x", x.grad), ("pseudo", ea.grad), ("weight", layer.weight.grad), ("root_weight", layer.root.grad),
                      ("bias", layer.bias.grad)):
        _check(got, want[name], 3e-5, f"d {name}")


def test_a_spline_cnn_trains():
    """Two SplineConv layers, Adam, twenty steps on a fixed random graph: the loss falls, every parameter moves, nothing is NaN."""
    from gnnops.conv import SplineConv

    torch.manual_seed(5)
    n, e, d = 400, 3000, 16
    ei = sc.graph(6, n, e).cuda()
    g = torch.Generator().manual_seed(10)
    x = (torch.rand(n, d, generator=g) * 2 - 1).cuda()
    ea = torch.rand(e, 2, generator=g).cuda()
    y = (torch.rand(n, 4, generator=g) * 2 - 1).cuda()
    l1, l2 = SplineConv(d, 16, dim=2, kernel_size=5).cuda(), SplineConv(16, 4, dim=2, kernel_size=5, degree=2, aggr="add").cuda()
    params = list(l1.parameters()) + list(l2.parameters())
    start = [p.detach().clone() for p in params]
    opt = torch.optim.Adam(params, lr=1e-2)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(l2(torch.relu(l1(x, ei, ea)), ei, ea), y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(l == l for l in losses) and losses[-1] < 0.7 * losses[0], losses
    assert all(not torch.equal(a, b.detach()) for a, b in zip(start, params))


# ---- norm=True with a row whose degree the storage type cannot hold --------------------------------------------------------
def _hub_row_inputs(dtype, hub, n=64, e=2000, m=8):
    """make_inputs on (1, 1, [5], [1]) with row 5 brought to exactly ``hub`` edges: the extra ones come from columns 0 .. 9,
    which feed no other row."""
    cfg = (1, 1, [5], [1])
    inputs, R, ei = sc.make_inputs(900, n, e, cfg, m, m, True, dtype)
    g = torch.Generator().manual_seed(901)
    ei[1] = 10 + ei[1] % (n - 10)
    more = hub - int((ei[0] == 5).sum())
    ei = torch.cat([ei, torch.stack([torch.full((more,), 5), torch.randint(0, 10, (more,), generator=g)])], 1)
    inputs["pseudo"] = torch.cat([inputs["pseudo"], sc.pseudo_coords(g, more, 1, [5], [1]).to(dtype).double()])
    return cfg, inputs, R, ei


def _degree_scaled(grads, ei, n):
    """d pseudo[e] times the degree of the row e belongs to, d x[j] times the smallest degree among the rows j feeds: a member
    of the 70 000-edge row has 1 / 70 000 of the gradient of the rest and would vanish under a max-relative measure."""
    import conv_chain as cc

    s = cc.mean_scales(torch.stack([ei[1], ei[0]]), n, n)
    return {k: (v * s["w"] if k == "pseudo" else v * s["q"] if k == "x" else v) for k, v in grads.items()}


@pytest.mark.parametrize("via", ["op", "layer"])
@pytest.mark.parametrize("dtype,hub", [(torch.float16, 70000), (torch.bfloat16, 257)], ids=["float16-70000", "bfloat16-257"])
def test_norm_with_a_degree_the_storage_type_cannot_hold(tsc, dtype, hub, via):
    """spline_conv(norm=True) / SplineConv(aggr="mean"): the backward divides G by the degree, counted and divided in float32.
    fp16: 70 000 is inf, so a degree in the storage type zeroes the row's gradient and that of every column feeding it (an error
    of 1.0 of scale on the degree-scaled d x): this is what the case pins. bf16: 257 is 256, the largest relative error a bf16
    degree can have (0.39 %); that is BELOW what bf16 storage of the gradients costs by itself (self error of d pseudo 2e-3, bar
    8e-3), so no bf16 bar derived from the chain can tell a rounded degree from an exact one — the case covers the branch and
    says so, it does not pin the bf16 degree.
    Bars: the three tensors the degree reaches (d x, d pseudo, d weight, degree-scaled) take 4 x the distance of the chain run in
    the storage type (spline_chain with ``rnd``, each gradient stored once in that type) from the float64 chain, TOL where that is tighter, measured here on the CPU from the chain alone; out, d
    root_weight and d bias, whose storage roundings that chain does not model, keep this file's TOL."""
    cfg, inputs, R, ei = _hub_row_inputs(dtype, hub)
    n = inputs["x"].size(0)
    deg = torch.bincount(ei[0], minlength=n)
    assert int(deg[5]) == hub and not bool((ei[1][ei[0] != 5] < 10).any())
    assert float(deg[5].to(dtype)) != hub            # the storage type cannot hold this degree
    want_out, want = sc.conv_grads(inputs, ei, R, cfg[2], cfg[3], cfg[0], True)
    _, self_grads = sc.conv_grads(inputs, ei, R, cfg[2], cfg[3], cfg[0], True, rnd=dtype)
    self_grads = {k: v.to(dtype).double() for k, v in self_grads.items()}       # each gradient is stored in the storage type
    want_s, self_s = _degree_scaled(want, ei, n), _degree_scaled(self_grads, ei, n)
    bars = {k: TOL[dtype] for k in list(want) + ["out"]}
    for k in ("x", "pseudo", "weight"):
        bars[k] = min(4 * sc.rel_err(self_s[k], want_s[k]), TOL[dtype])         # never looser than this file's own bar
        assert bars[k] > 0, k
    if dtype == torch.float16:                       # the bug, in the chain's terms: the hub's feeders get 0, an error of 1.0
        lost = {k: v.clone() for k, v in want.items()}
        lost["x"][:10] = 0
        assert sc.rel_err(_degree_scaled(lost, ei, n)["x"], want_s["x"]) > 100 * bars["x"]
    dev = _device(inputs, dtype)
    if via == "op":
        out = _conv_dev(tsc, dev, ei, R, cfg, True, dtype)
        got = {k: dev[k].grad for k in want}
    else:
        from gnnops.conv import SplineConv

        layer = SplineConv(8, 8, dim=1, kernel_size=5, is_open_spline=True, degree=1, aggr="mean").to(dtype).cuda()
        with torch.no_grad():
            layer.weight.copy_(dev["weight"]), layer.root.copy_(dev["root_weight"]), layer.bias.copy_(dev["bias"])
        out = layer(dev["x"], ei.flip(0).cuda(), dev["pseudo"])
        (out.float() * R.to(dtype).cuda().float()).sum().backward()
        got = {"x": dev["x"].grad, "pseudo": dev["pseudo"].grad, "weight": layer.weight.grad, "root_weight": layer.root.grad,
               "bias": layer.bias.grad}
    _check(out, want_out, bars["out"], "out")
    got_s = _degree_scaled({k: v.detach().double().cpu() for k, v in got.items()}, ei, n)
    for k in want:
        _check(got_s[k], want_s[k], bars[k], f"d {k} (degree-scaled)")
