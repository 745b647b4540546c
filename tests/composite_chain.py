"""The yardstick of the composite and scatter-backward tests: torch_scatter's scatter_softmax / scatter_log_softmax /
scatter_logsumexp / scatter_std restated in torch float64 on the CPU along any ``dim`` with a row index, so that torch's own
autograd differentiates them. The formulas are those in the header of csrc/composite.hip: std is two-pass with cnt' + 1e-6 under
the root, an empty group has max 0 and sum 0, log(s + eps), and a NaN from x - max (that is (-inf) - (-inf)) counts as -inf. The
scatter / segment reductions sum, mean, min, max and the selections (index_select, gather) are restated for the backward
tests; the gradient of min / max goes to ONE position per output, the ``arg`` of oracle.scatter (torch's amax splits the
gradient between ties). test_composite_cpu.py ties all of it to oracle/oracle.py, to torch's per-group functions and to
torch.autograd.gradcheck.

``rnd`` (a torch dtype) runs the same formulas the way the library has to for that storage type: float32 arithmetic (torch's
sequential CPU index_add_ stands for the fp32 accumulators), the output rounded once to the storage type, and on the way back
the Python backward of gnnops/autograd.py step by step, every tensor it materialises (g * y, the group sums, exp(y), scale,
the group mean, ...) rounded to the storage type. ``self_error`` is the distance between that chain and the float64 one: the
reference against itself, never the kernels. The bars of the GPU tests that have no precedent in the project are 4 x that
distance (the factor of tests/spline_chain.py: device expf / logf a few ulp from torch's, another summation order).

The input tables of the CPU and GPU tests live here, drawn with CPU generators so that both see the same bits."""
from dataclasses import dataclass

import torch

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
DNAME = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
VEC = {torch.float32: 4, torch.float16: 8, torch.bfloat16: 8}          # Elem<T>::VEC: elements of a 16-byte lane access
T_HUB = 8192                                                           # csrc/hub.h
MODES = ("softmax", "log_softmax", "logsumexp", "std", "std_biased")   # std both ways: unbiased, then biased
NO_STD = MODES[:3]
NEG_INF = float("-inf")


def _q(t, rnd):
    return t if rnd is None else t.to(rnd).to(t.dtype)


def _cdt(rnd):
    return torch.float64 if rnd is None else torch.float32


def split_mode(mode):
    return ("std", mode == "std") if mode.startswith("std") else (mode, True)


# ---- forward restatements (differentiable; the dtype of ``src`` is the arithmetic) ----------------------------------------
def _group_sum(x, row, N):
    return torch.zeros((N,) + tuple(x.shape[1:]), dtype=x.dtype).index_add(0, row, x)


def _col(t, x):
    return t.view((-1,) + (1,) * (x.dim() - 1))


def composite(src, row, dim, N, mode, eps=1e-12, unbiased=True):
    x = src.movedim(dim, 0)
    cnt = torch.bincount(row, minlength=N)
    if mode == "std":
        mean = _group_sum(x, row, N) / _col(cnt.clamp(min=1).to(x.dtype), x)
        d = x - mean[row]
        var = _group_sum(d * d, row, N)
        c = _col((cnt - 1 if unbiased else cnt).clamp(min=1).to(x.dtype), x) + 1e-6
        pos = var > 0                                       # out == 0 has gradient 0 (autograd.py), not the root's 0 * inf
        return torch.where(pos, (torch.where(pos, var, torch.ones_like(var)) / c).sqrt(), torch.zeros_like(var)).movedim(0, dim)
    m = torch.full((N,) + tuple(x.shape[1:]), NEG_INF, dtype=x.dtype).index_reduce(0, row, x.detach(), "amax")
    m = torch.where(_col(cnt, x) == 0, torch.zeros_like(m), m)
    d = x - m[row]
    d = torch.where(torch.isnan(d), torch.full_like(d, NEG_INF), d)
    e = d.exp()
    s = _group_sum(e, row, N)
    if mode == "softmax":
        out = e / s[row]
    elif mode == "log_softmax":
        out = d - (s + eps).log()[row]
    elif mode == "logsumexp":
        out = m + (s + eps).log()
    else:
        raise ValueError(mode)
    return out.movedim(0, dim)


def reduce_rows(src, row, dim, N, reduce, arg=None):
    """scatter / segment_csr / segment_coo with a row index. ``arg`` (int64, the output's shape, E where nothing arrived):
    the position min / max took, from oracle.scatter."""
    x = src.movedim(dim, 0)
    if reduce in ("min", "max"):
        ext = torch.cat([x, torch.zeros((1,) + tuple(x.shape[1:]), dtype=x.dtype)])
        return ext.gather(0, arg.movedim(dim, 0)).movedim(0, dim)
    out = _group_sum(x, row, N)
    if reduce == "mean":
        out = out / _col(torch.bincount(row, minlength=N).clamp(min=1).to(x.dtype), x)
    return out.movedim(0, dim)


def select(src, dim, index):
    """index_select, gather_coo, gather_csr (index = the segment of each position) for a 1-D index; torch.gather otherwise."""
    return src.index_select(dim, index) if index.dim() == 1 else src.gather(dim, index)


# ---- gradients of sum(out * R): float64 autograd, or the library's steps in fp32 with storage rounding ------------------
def _leaf(src, rnd):
    return src.detach().to(_cdt(rnd)).clone().requires_grad_(rnd is None)


def composite_grads(src, row, dim, N, mode, R=None, rnd=None, eps=1e-12):
    """(out, d src or None) as float64. src: storage-rounded values as float64; R: the functional, shaped like out."""
    mode, unbiased = split_mode(mode)
    x = _leaf(src, rnd)
    out = composite(x, row, dim, N, mode, eps, unbiased)
    if R is None:
        return _q(out.detach(), rnd).double(), None
    if rnd is None:
        out.backward(R)                  # d sum(out * R); a masked member's log_softmax is -inf and its gradient still R
        return out.detach(), x.grad
    # gnnops/autograd.py::_Composite.backward, each materialised tensor rounded to the storage type
    q = lambda t: _q(t, rnd)   # noqa: E731
    y = q(out).movedim(dim, 0)
    g = R.to(_cdt(rnd)).movedim(dim, 0)
    xs = x.movedim(dim, 0)
    if mode == "softmax":
        s = q(_group_sum(q(g * y), row, N))
        dx = q(y * q(g - s[row]))
    elif mode == "log_softmax":
        s = q(_group_sum(g, row, N))
        dx = q(g - q(q(y.exp()) * s[row]))
    elif mode == "logsumexp":
        dx = q(g[row] * q(q(xs - y[row]).exp()))
    else:
        cnt = torch.bincount(row, minlength=N)
        mean = q(_group_sum(xs, row, N) / _col(cnt.clamp(min=1).float(), xs))
        denom = (_col((cnt - 1 if unbiased else cnt).clamp(min=1).float(), xs) + 1e-6) * y
        scale = q(torch.where(y != 0, g / denom, torch.zeros_like(denom)))
        dx = q(scale[row] * q(xs - mean[row]))
    return y.movedim(0, dim).double(), dx.movedim(0, dim).double()


def reduce_grads(src, row, dim, N, reduce, R, arg=None, rnd=None):
    x = _leaf(src, rnd)
    out = reduce_rows(x, row, dim, N, reduce, arg)
    if rnd is None:
        out.backward(R)
        return out.detach(), x.grad
    g = R.to(_cdt(rnd)).movedim(dim, 0)
    if reduce == "mean":                                     # _ScatterMean / _SegmentCSR: g / count, then the gather back
        dx = _q(g / _col(torch.bincount(row, minlength=N).clamp(min=1).float(), g), rnd)[row]
    elif reduce == "sum":
        dx = g[row]
    else:                                                    # one position per output; slot E swallows the empty groups
        a = arg.movedim(dim, 0)
        dx = torch.zeros((x.size(dim) + 1,) + tuple(g.shape[1:]), dtype=g.dtype).scatter_add(0, a, g)[:-1]
    return _q(out.detach(), rnd).double(), dx.movedim(0, dim).double()


def select_grads(src, dim, index, R, rnd=None):
    x = _leaf(src, rnd)
    out = select(x, dim, index)
    if rnd is None:
        out.backward(R)
        return out.detach(), x.grad
    g = R.to(_cdt(rnd))
    z = torch.zeros(x.shape, dtype=g.dtype)
    dx = z.index_add(dim, index, g) if index.dim() == 1 else z.scatter_add(dim, index, g)
    return out.detach().double(), _q(dx, rnd).double()      # the fp32 accumulator of the scatter-add back, rounded once


def rel_err(got, want):
    """max |got - want| / max |want| over the positions where the reference is finite (the others are compared exactly)."""
    fin = torch.isfinite(want)
    if not bool(fin.any()):
        return 0.0
    return float((got[fin] - want[fin]).abs().max()) / max(float(want[fin].abs().max()), 1e-6)


def same_specials(got, want):
    """NaN where the reference has NaN, the same infinity where it has one, finite elsewhere."""
    fin = torch.isfinite(want)
    return bool((torch.isfinite(got) == fin).all() and (torch.isnan(got) == torch.isnan(want)).all()
                and (got[torch.isinf(want)] == want[torch.isinf(want)]).all())


def self_error(exact, rounded):
    """exact, rounded: (out, grad) pairs of one *_grads call without and with ``rnd``."""
    err = {"out": rel_err(rounded[0], exact[0])}
    if exact[1] is not None:
        err["grad"] = rel_err(rounded[1], exact[1])
    return err


# ---- input tables ---------------------------------------------------------------------------------------------------------
def row_index(g, E, N, big=0, seam_all=False):
    """int64 [E] in random order: group 0 empty, group 1 one member, group 2 eight, group 3 nine (the two sides of the U seam),
    group 5 ``big`` members if given, the rest spread at random over the other groups; group N - 1 is never empty.
    ``seam_all``: every group has 0, 1, 8, 9, 7, 16 or 17 members in turn (E is then whatever that adds up to)."""
    sizes = torch.zeros(N, dtype=torch.int64)
    if seam_all:
        sizes = torch.tensor([0, 1, 8, 9, 7, 16, 17])[torch.arange(N) % 7]
        sizes[N - 1] = 9
    else:
        sizes[1], sizes[2], sizes[3] = 1, 8, 9
        if big:
            sizes[5] = big
        free = torch.tensor([n for n in range(4, N) if not (big and n == 5)])
        rest = E - int(sizes.sum()) - 1
        assert rest >= 0 and len(free) > 0
        sizes += torch.bincount(free[torch.randint(0, len(free), (rest,), generator=g)], minlength=N)
        sizes[N - 1] += 1
    row = torch.repeat_interleave(torch.arange(N), sizes)
    return row[torch.randperm(row.numel(), generator=g)]


@dataclass(frozen=True)
class Fwd:
    name: str                      # carries the branch of dispatch<T>() the case is built for
    branch: object                 # str, or {dtype: str} where the branch depends on the element size
    E: int
    N: int
    vecs: int = 0                  # K = vecs * VEC[dtype] ...
    K: object = None               # ... or K itself; None with vecs == 0: the group dimension is the last one
    lead: tuple = ()               # dimensions in front of the group dimension (B = their product)
    big: int = 0                   # members of group 5
    seam_all: bool = False
    values: str = "randn3"         # randn3 | offsets | masked | all_neg_inf | mean1e4
    offset1: bool = False          # the tensor starts one element into its allocation
    plan: bool = False             # a Plan is passed as the index
    implicit: bool = False         # dim_size=None
    default_dim: bool = False      # dim is left at the op's default (-1)
    modes: tuple = MODES
    dtypes: tuple = tuple(DTYPES)
    bar: str = "small"             # small | hub: the project's fp32 bars; self: 4 x self_error also in fp32

    def k(self, dtype):
        k = self.K[dtype] if isinstance(self.K, dict) else self.K
        return k if k is not None else (self.vecs * VEC[dtype] if self.vecs else None)

    def dim(self):
        return len(self.lead)

    def branch_of(self, dtype):
        return self.branch[dtype] if isinstance(self.branch, dict) else self.branch


F32, F16, BF16 = DTYPES
FORWARD = [
    Fwd("rows_1lane", "rows_g1_kc1", 300, 40, vecs=1),
    Fwd("rows_2lanes_implicit_dim_size", "rows_g2_kc1", 300, 40, vecs=2, implicit=True),
    Fwd("rows_64lanes", "rows_g64_kc1", 200, 24, vecs=64),
    Fwd("rows_64lanes_2chunks", "rows_g64_kc2", 200, 24, vecs=80),
    Fwd("elem_K7", "elem", 300, 40, K=7),
    Fwd("elem_K13_plan_index", "elem", 300, 40, K=13, plan=True),
    Fwd("elem_aligned_K_offset_pointer", "elem", 300, 40, vecs=4, offset1=True),
    Fwd("rows_B3_dim1_plan_index", "rows_g2_kc1", 300, 40, vecs=2, lead=(3,), plan=True),
    Fwd("rows_B2_2chunks_dim1", "rows_g64_kc2", 120, 16, vecs=80, lead=(2,)),
    Fwd("elem_B3_dim1_K7", "elem", 300, 40, K=7, lead=(3,)),
    Fwd("elem_B4_default_dim", "elem", 300, 40, lead=(4,), default_dim=True),
    Fwd("rows_seam_0_1_8_9", "rows_g2_kc1", 0, 42, vecs=2, seam_all=True),
    Fwd("rows_B2_stream_20000", "rows_g1_kc1_stream", 20600, 40, vecs=1, lead=(2,), big=20000, bar="self"),
    Fwd("hub", {F32: "rows_g64_kc2_hub", F16: "rows_g2_kc1_hub", BF16: "rows_g2_kc1_hub"}, 12000, 40,
        K={F32: 320, F16: 16, BF16: 16}, big=8500, bar="hub"),
    Fwd("hub_elem_K7", "elem", 12000, 40, K=7, big=8500, bar="hub"),
    # values
    Fwd("large_offsets_rows", "rows_g2_kc1", 300, 40, vecs=2, values="offsets", bar="self"),
    Fwd("large_offsets_elem_B2", "elem", 300, 40, K=7, lead=(2,), values="offsets", bar="self"),
    Fwd("masked_rows", "rows_g2_kc1", 300, 40, vecs=2, values="masked", modes=NO_STD),
    Fwd("masked_elem", "elem", 300, 40, K=7, values="masked", modes=NO_STD),
    Fwd("all_neg_inf_group_rows", "rows_g2_kc1", 300, 40, vecs=2, values="all_neg_inf", modes=NO_STD),
    Fwd("all_neg_inf_group_elem", "elem", 300, 40, K=7, values="all_neg_inf", modes=NO_STD),
    Fwd("std_mean_1e4_rows", "rows_g2_kc1", 300, 40, vecs=2, values="mean1e4", modes=MODES[3:], dtypes=(F32,), bar="self"),
    Fwd("std_mean_1e4_elem", "elem", 300, 40, K=7, values="mean1e4", modes=MODES[3:], dtypes=(F32,), bar="self"),
]
FORWARD_BY_NAME = {c.name: c for c in FORWARD}
# fp16: |x| <= 3.0e4, so that x - max >= -6e4 stays finite. bf16 has 8 bits: at 1e4 its spacing is 64 and a spread of 30
# would collapse every group to one value, so its offsets are 1e3 (spacing 4).
OFFSET = {torch.float32: 1e4, torch.bfloat16: 1e3, torch.float16: 2.995e4}


def fwd_shape(case, dtype, E):
    k = case.k(dtype)
    return case.lead + (E,) + (() if k is None else (k,))


def _values(g, case, dtype, shape, row, dim):
    if case.values == "mean1e4":
        return 1e4 + torch.randn(shape, generator=g)
    x = torch.randn(shape, generator=g) * 3
    if case.values == "offsets":        # spread about 30 around a per-group offset of +-OFFSET
        x = (torch.randn(shape, generator=g) * 5).clamp(-15, 15)
        sign = (torch.arange(case.N) % 2 * 2 - 1).to(x.dtype)
        x = (x.movedim(dim, 0) + _col((sign * OFFSET[dtype])[row], x.movedim(dim, 0))).movedim(0, dim)
    if case.values == "masked":         # a fifth of the members masked; the first member of every group stays finite
        mask = torch.rand(shape, generator=g) < 0.2
        first = torch.zeros(row.numel(), dtype=torch.bool)
        seen = set()
        for i, r in enumerate(row.tolist()):
            if r not in seen:
                seen.add(r)
                first[i] = True
        mask = (mask.movedim(dim, 0) & ~_col(first, x.movedim(dim, 0))).movedim(0, dim)
        x = x.masked_fill(mask, NEG_INF)
    if case.values == "all_neg_inf":    # groups 3 (nine members) and 6 wholly -inf, beside ordinary ones
        dead = (row == 3) | (row == 6)
        x = x.movedim(dim, 0).masked_fill(_col(dead, x.movedim(dim, 0)), NEG_INF).movedim(0, dim)
    return x


def fwd_inputs(case, dtype, seed=1234):
    """(src as float64 holding storage-rounded values, row int64 [E], N)."""
    g = torch.Generator().manual_seed(seed + len(case.name))
    row = row_index(g, case.E, case.N, case.big, case.seam_all)
    shape = fwd_shape(case, dtype, row.numel())
    src = _values(g, case, dtype, shape, row, case.dim()).to(dtype).double()
    return src, row, case.N


def dispatch_branch(B, E, K, max_group, dtype, aligned=True):
    """dispatch<T>() of csrc/composite.hip restated: which kernel family and geometry a call takes."""
    vec = VEC[dtype]
    if K % vec != 0 or not aligned:
        return "elem"
    vecs = K // vec
    gshift = 0
    while (1 << gshift) < vecs and gshift < 6:
        gshift += 1
    G = 1 << gshift
    name = f"rows_g{G}_kc{-(-vecs // G)}"
    if max_group > T_HUB:
        name += "_hub" if (B == 1 and E > T_HUB) else "_stream"
    return name


def place(t, offset1, device):
    """t on ``device``; with ``offset1`` as a contiguous tensor that starts one element into its allocation."""
    if not offset1:
        return t.to(device)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
    buf[1:].copy_(t.reshape(-1))
    return buf[1:].view(t.shape)


def functional(g, shape, dtype):
    return (torch.rand(shape, generator=g) * 2 - 1).to(dtype).double()


# backward of the composite ops
@dataclass(frozen=True)
class Bwd:
    name: str
    E: int
    N: int
    K: object = None
    lead: tuple = ()
    big: int = 0
    masked: bool = False
    modes: tuple = MODES
    hub: bool = False


BACKWARD = [
    Bwd("dim0_K8", 400, 30, K=8),
    Bwd("dim0_K7", 400, 30, K=7),
    Bwd("dim1_of_3d_K8", 300, 30, K=8, lead=(2,)),
    Bwd("dim1_of_3d_K5", 300, 30, K=5, lead=(2,)),
    Bwd("last_dim_B3", 300, 30, lead=(3,)),
    Bwd("hub_group_K8", 9500, 30, K=8, big=8400, hub=True),
    Bwd("masked_finite_max_K8", 400, 30, K=8, masked=True, modes=NO_STD),
    Bwd("masked_finite_max_last_dim", 300, 30, lead=(3,), masked=True, modes=NO_STD),
]


def bwd_inputs(case, dtype, mode, seed=4321):
    """(src float64 of storage-rounded values, row, N, dim, R shaped like the op's output)."""
    g = torch.Generator().manual_seed(seed + len(case.name))
    row = row_index(g, case.E, case.N, case.big)
    fc = Fwd(case.name, "", case.E, case.N, K=case.K, lead=case.lead, values="masked" if case.masked else "randn3")
    shape = fwd_shape(fc, dtype, case.E)
    dim = len(case.lead)
    src = _values(g, fc, dtype, shape, row, dim).to(dtype).double()
    oshape = list(shape)
    if mode in ("logsumexp", "std", "std_biased"):
        oshape[dim] = case.N
    return src, row, case.N, dim, functional(g, oshape, dtype)


# backward of scatter / segment / gather: the index tables
@dataclass(frozen=True)
class Route:
    name: str
    E: int
    N: int                          # groups the index reaches (the largest index is N - 1)
    K: object = None
    lead: tuple = ()
    big: int = 0
    extra: int = 0                  # dim_size = N + extra
    implicit: bool = False
    ties: bool = False


ROUTES = [
    Route("dim0_K8", 500, 40, K=8),
    Route("dim0_K5_dim_size_beyond", 500, 40, K=5, extra=7),
    Route("dim0_K8_implicit_dim_size", 500, 40, K=8, implicit=True),
    Route("dim1_of_3d_K5", 400, 40, K=5, lead=(2,)),
    Route("last_dim_B3", 400, 40, lead=(3,)),
    Route("ties_K8", 500, 40, K=8, ties=True),
    Route("ties_last_dim_B3", 400, 40, lead=(3,), ties=True),
    Route("big_70000_and_300_K8", 71000, 40, K=8, big=70000),
]


def route_inputs(case, dtype, seed=999, sorted_index=False):
    """(src float64 of storage-rounded values, row, dim_size, dim, R). Group 4 gets 300 members in the ``big`` table (a bf16
    count above 256 is not exact), group 5 gets 70 000 (more than T_HUB contributions; above fp16's 65 504 as well)."""
    g = torch.Generator().manual_seed(seed + len(case.name))
    row = row_index(g, case.E, case.N, case.big)
    if case.big:
        row[torch.nonzero((row >= 6) & (row < case.N - 1)).flatten()[:300]] = 4
    if sorted_index:
        row = row.sort().values
    dim = len(case.lead)
    shape = case.lead + (case.E,) + (() if case.K is None else (case.K,))
    x = torch.rand(shape, generator=g) * 4 - 2
    if case.ties:                       # min / max must pick ONE position among equals: values on a grid of 0.5 (both zeros
        xs = x.movedim(dim, 0)          # among them: -0.2 rounds to -0.0), and every other row a copy of the one before it
        xs.copy_((xs * 2).round() / 2)
        xs[1::2] = xs[0::2][: xs[1::2].size(0)]
        x = xs.movedim(0, dim).contiguous()
    src = x.to(dtype).double()
    Nout = case.N + case.extra
    oshape = list(shape)
    oshape[dim] = Nout
    return src, row, Nout, dim, functional(g, oshape, dtype)


def select_inputs(case, dtype, kind, seed=555):
    """(table float64 of storage-rounded values [.., N + extra, ..], index, dim, R shaped like the selection).
    kind: index_select (the case's row index), sorted (gather_coo / gather_csr), gather (a full random index)."""
    g = torch.Generator().manual_seed(seed + len(case.name))
    _, row, Nout, dim, _ = route_inputs(case, dtype, sorted_index=(kind == "sorted"))
    tshape = case.lead + (Nout,) + (() if case.K is None else (case.K,))
    oshape = case.lead + (case.E,) + (() if case.K is None else (case.K,))
    table = (torch.rand(tshape, generator=g) * 4 - 2).to(dtype).double()
    index = torch.randint(0, Nout, oshape, generator=g) if kind == "gather" else row
    return table, index, dim, functional(g, oshape, dtype)


def oracle_arg(src, row, dim, Nout, reduce, dtype):
    """The position oracle.scatter's min / max takes for every output (E where nothing arrived), on the storage-typed values."""
    from helpers import to_np
    from oracle import oracle

    _, arg = oracle.scatter(to_np(src.to(dtype)), row.numpy(), dim=dim, dim_size=Nout, reduce=reduce, dtype=DNAME[dtype])
    return torch.from_numpy(arg)


def forward_self_error(case, mode, dtype):
    src, row, N = fwd_inputs(case, dtype)
    exact = composite_grads(src, row, case.dim(), N, mode)
    return self_error(exact, composite_grads(src, row, case.dim(), N, mode, rnd=dtype))["out"]


def backward_self_error(case, mode, dtype):
    src, row, N, dim, R = bwd_inputs(case, dtype, mode)
    return self_error(composite_grads(src, row, dim, N, mode, R), composite_grads(src, row, dim, N, mode, R, rnd=dtype))


def times_count(dx, row, dim, N):
    """A mean's gradient times the size of the group it belongs to, which puts every group on the scale of R. Measured against
    the largest gradient of the whole tensor, a 70 000-member group (gradients of 1e-5 beside 1 in a one-member group) could be
    lost altogether without a trace."""
    x = dx.movedim(dim, 0)
    return (x * _col(torch.bincount(row, minlength=N).clamp(min=1).to(x.dtype)[row], x)).movedim(0, dim)


def mean_self_error(case, dtype, sorted_index):
    src, row, Nout, dim, R = route_inputs(case, dtype, sorted_index=sorted_index)
    out, dx = reduce_grads(src, row, dim, Nout, "mean", R)
    out_r, dx_r = reduce_grads(src, row, dim, Nout, "mean", R, rnd=dtype)
    return self_error((out, times_count(dx, row, dim, Nout)), (out_r, times_count(dx_r, row, dim, Nout)))


def select_self_error(case, dtype, kind):
    table, index, dim, R = select_inputs(case, dtype, kind)
    return self_error(select_grads(table, dim, index, R), select_grads(table, dim, index, R, rnd=dtype))["grad"]


def self_error_table():
    """{key: self error}: every number a bar of test_composite_gpu.py can be taken from (tests/golden/composite_self_error.json
    is a recording of this table)."""
    t = {}
    for c in FORWARD:
        for d in c.dtypes:
            for m in c.modes:
                t[f"fwd/{c.name}/{m}/{DNAME[d]}"] = forward_self_error(c, m, d)
    for c in BACKWARD:
        for d in DTYPES:
            for m in c.modes:
                e = backward_self_error(c, m, d)
                t[f"bwd/{c.name}/{m}/{DNAME[d]}/out"], t[f"bwd/{c.name}/{m}/{DNAME[d]}/grad"] = e["out"], e["grad"]
    for c in ROUTES:
        for d in DTYPES:
            for srt in (False, True):
                if srt and c.lead:
                    continue
                e = mean_self_error(c, d, srt)
                tag = "sorted" if srt else "unsorted"
                t[f"mean/{c.name}/{tag}/{DNAME[d]}/out"], t[f"mean/{c.name}/{tag}/{DNAME[d]}/grad"] = e["out"], e["grad"]
            for kind in ("index_select", "sorted", "gather"):
                if kind == "sorted" and c.lead:
                    continue
                t[f"select/{c.name}/{kind}/{DNAME[d]}"] = select_self_error(c, d, kind)
    return t
