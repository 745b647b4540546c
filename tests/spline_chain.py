"""The yardstick of the spline training tests: torch_spline_conv's chain restated in torch float64 on the CPU, so that torch's
own autograd differentiates it. basis by the published formulas with floor().detach() (no gradient through the knot
index), messages by einsum('es,ei,esio->eo') in edge chunks, index_add_ at edge_index[0], degree division, root, bias.
test_spline_train_cpu.py ties its forward to oracle/spatial_oracle.py and its gradients to torch.autograd.gradcheck.

``rnd`` (a torch dtype) runs the same chain the way a kernel for that storage type has to: float32 arithmetic (torch's CPU
float32 sums stand for the fp32 accumulators) with the intermediates — basis and, on the way back, d basis; the per-edge
rows basis * x[col] and the message rows and, on the way back, their gradients; the degree-scaled output — rounded to the
storage type. The distance between that chain and the float64 one is the reference's own estimate of what a storage type
costs, long fp32 sums included; the bars of the GPU tests that have no precedent in the project (bf16, the 200 000-term sums
of the hub case) are 4 x that distance, see ``self_error``."""
import itertools

import torch


class _RoundBothWays(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, dtype):
        ctx.dtype = dtype
        return t.to(dtype).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dtype).to(g.dtype), None


def _r(t, rnd):
    return t if rnd is None else _RoundBothWays.apply(t, rnd)


def _bspline(v, k, m):
    if m == 1:
        return 1 - v if k == 0 else v
    if m == 2:
        return (0.5 * v * v - v + 0.5, -v * v + v + 0.5, 0.5 * v * v)[k]
    return ((1 - v) ** 3 / 6, (3 * v ** 3 - 6 * v ** 2 + 4) / 6, (-3 * v ** 3 + 3 * v ** 2 + 3 * v + 1) / 6, v ** 3 / 6)[k]


def spline_basis(pseudo, kernel_size, is_open_spline, degree):
    """pseudo float64 [E, D] -> basis float64 [E, S] (differentiable), weight_index int64 [E, S]."""
    E, D = pseudo.shape
    ks = [int(k) for k in kernel_size]
    op = [int(o) for o in is_open_spline]
    v = pseudo * torch.tensor([ks[d] - degree * op[d] for d in range(D)], dtype=pseudo.dtype)
    fl = v.floor().detach()
    fr = v - fl
    cols_b, cols_w = [], []
    for digits in itertools.product(range(degree + 1), repeat=D):
        digits = digits[::-1]                                  # dimension 0 is the fastest digit of s
        b = torch.ones(E, dtype=pseudo.dtype)
        wi = torch.zeros(E, dtype=torch.int64)
        off = 1
        for d in range(D):
            b = b * _bspline(fr[:, d], digits[d], degree)
            wi = wi + ((fl[:, d].long() + digits[d]) % ks[d]) * off
            off *= ks[d]
        cols_b.append(b)
        cols_w.append(wi)
    return torch.stack(cols_b, 1), torch.stack(cols_w, 1)


def spline_weighting(x, weight, basis, weight_index, chunk=None, rnd=None):
    """out[e] = sum_s basis[e, s] * x[e] @ weight[weight_index[e, s]], in edge chunks that keep [chunk, S, Min, Mout] near 64 MB."""
    E, S = basis.shape
    if chunk is None:
        chunk = max(1, (8 << 20) // max(S * weight.size(1) * weight.size(2), 1))
    if rnd is None:
        outs = [torch.einsum("es,ei,esio->eo", basis[a:a + chunk], x[a:a + chunk], weight[weight_index[a:a + chunk]])
                for a in range(0, E, chunk)]
    else:
        outs = [torch.einsum("esi,esio->eo", _r(basis[a:a + chunk].unsqueeze(2) * x[a:a + chunk].unsqueeze(1), rnd),
                             weight[weight_index[a:a + chunk]]) for a in range(0, E, chunk)]
    return torch.cat(outs) if outs else x.new_zeros((0, weight.size(2)))


def spline_conv(x, edge_index, pseudo, weight, kernel_size, is_open_spline, degree=1, norm=True, root_weight=None, bias=None,
                rnd=None):
    row, col = edge_index
    basis, wi = spline_basis(pseudo, kernel_size, is_open_spline, degree)
    msg = _r(spline_weighting(x[col], weight, _r(basis, rnd), wi, rnd=rnd), rnd)
    out = torch.zeros((x.size(0), weight.size(2)), dtype=x.dtype).index_add_(0, row, msg)
    if norm:
        out = out / torch.bincount(row, minlength=x.size(0)).clamp(min=1).to(x.dtype).unsqueeze(1)
    out = _r(out, rnd)
    if root_weight is not None:
        out = out + x @ root_weight
    if bias is not None:
        out = out + bias
    return out


def conv_grads(inputs, edge_index, R, kernel_size, is_open_spline, degree, norm, rnd=None):
    """inputs: {name: float64 tensor or None} for x, pseudo, weight, root_weight, bias. Returns (out, {name: gradient of
    sum(out * R)})."""
    cdt = torch.float64 if rnd is None else torch.float32
    leaves = {k: (v.detach().to(cdt).clone().requires_grad_(True) if v is not None else None) for k, v in inputs.items()}
    out = spline_conv(leaves["x"], edge_index, leaves["pseudo"], leaves["weight"], kernel_size, is_open_spline, degree, norm,
                      leaves["root_weight"], leaves["bias"], rnd=rnd)
    (out * R.to(cdt)).sum().backward()
    return out.detach().double(), {k: v.grad.double() for k, v in leaves.items() if v is not None}


def rel_err(got, want):
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-6)


def self_error(inputs, edge_index, R, kernel_size, is_open_spline, degree, norm, rnd):
    """{"out" or operand name: error of the chain with intermediates rounded to ``rnd`` against the unrounded chain, relative to
    the reference tensor's max}: the reference against itself, never the kernels."""
    out, exact = conv_grads(inputs, edge_index, R, kernel_size, is_open_spline, degree, norm)
    out_r, rounded = conv_grads(inputs, edge_index, R, kernel_size, is_open_spline, degree, norm, rnd=rnd)
    return {"out": rel_err(out_r, out), **{k: rel_err(rounded[k], exact[k]) for k in exact}}


# ---- the inputs the CPU and GPU tests share -----------------------------------------------------------------------------
CONFIGS = [  # (degree, D, kernel_size, is_open_spline): the grid of the issue
    (1, 2, [5, 5], [1, 0]),
    (2, 3, [4, 4, 5], [1, 1, 0]),
    (3, 1, [6], [1]),
    (1, 3, [5, 5, 5], [0, 0, 0]),
]


def graph(seed, n, e):
    """edge_index [2, E]: messages are summed at row 0. Node 3 receives nothing, node 5 is a small hub
    (as test_conv_train_gpu._graph)."""
    g = torch.Generator().manual_seed(seed)
    row = torch.randint(0, n, (e,), generator=g)
    col = torch.randint(0, n, (e,), generator=g)
    if n > 8 and e > 50:
        row[row == 3] = 4
        row[:40] = 5
    return torch.stack([row, col])


def pseudo_coords(g, e, degree, kernel_size, is_open_spline, margin=0.01):
    """[E, D] in [0, 1) whose scaled coordinates keep ``margin`` away from every knot (the derivative of a degree-1 spline is
    one-sided there)."""
    cols = []
    for k, o in zip(kernel_size, is_open_spline):
        cells = k - degree * o
        c = torch.randint(0, cells, (e,), generator=g).float()
        f = margin + (1 - 2 * margin) * torch.rand(e, generator=g)
        cols.append((c + f) / cells)
    return torch.stack(cols, 1)


def make_inputs(seed, n, e, cfg, m_in, m_out, root=True, dtype=torch.float32):
    """Storage-rounded CPU inputs as float64 (what both the device and the restatement get), the functional R, edge_index."""
    degree, D, ks, op = cfg
    g = torch.Generator().manual_seed(seed)
    K = 1
    for k in ks:
        K *= k
    rnd = lambda t: t.to(dtype).double()   # noqa: E731
    inputs = {
        "x": rnd(torch.rand(n, m_in, generator=g) * 2 - 1),
        "pseudo": rnd(pseudo_coords(g, e, degree, ks, op)),
        "weight": rnd((torch.rand(K, m_in, m_out, generator=g) * 2 - 1) * 0.5),
        "root_weight": rnd((torch.rand(m_in, m_out, generator=g) * 2 - 1) * 0.5) if root else None,
        "bias": rnd(torch.rand(m_out, generator=g) * 2 - 1) if root else None,
    }
    R = rnd(torch.rand(n, m_out, generator=g) * 2 - 1)
    return inputs, R, graph(seed + 1, n, e)


def hub_inputs(dtype, e=200_000, n=64, m=8):
    """Test 7's hub: every edge has the same pseudo-coordinate (D = 1, degree 1, kernel_size 5, open), so both kernels touched
    collect all E pairs."""
    g = torch.Generator().manual_seed(77)
    rnd = lambda t: t.to(dtype).double()   # noqa: E731
    inputs = {
        "x": rnd(torch.rand(n, m, generator=g) * 2 - 1),
        "pseudo": rnd(torch.full((e, 1), 0.3)),
        "weight": rnd((torch.rand(5, m, m, generator=g) * 2 - 1) * 0.5),
        "root_weight": None,
        "bias": None,
    }
    R = rnd(torch.rand(n, m, generator=g) * 2 - 1)
    ei = torch.stack([torch.randint(0, n, (e,), generator=g), torch.randint(0, n, (e,), generator=g)])
    return inputs, R, ei
