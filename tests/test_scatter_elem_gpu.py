"""csrc/scatter_elem.hip at every route, cell width and chunk seam, from the table of scatter_elem_cases.py.

Every case calls gnnops_scatter_elementwise_ixa directly (narrowed ids made by gnnops_narrow_index). Before the call the
route query is asked with the addresses the call will see and must report the route and geometry the case names, and ids
outside [0, N) are only ever handed to the LDS routes, which drop them (the atomic kernels do not check ids). Values, arg rows
(int32 or int64 as asked) and the `out` elements nothing reaches are compared bit for bit with the sequential oracle: the
inputs are built so that every sum, mean and product is exact in any arrival order (test_scatter_elem_routes_cpu.py).
`out` and `arg` sit between guard words that must survive. About twenty calls go through gnnops.scatter as well."""
import numpy as np
import pytest
import torch

import scatter_elem_cases as sc
from scatter_elem_cases import ATOMICS, CHUNKS, LDS

pytestmark = pytest.mark.gpu

CASES = sc.all_cases()
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
IVIEW = {"f32": torch.int32, "f16": torch.int16, "bf16": torch.int16}
IDT = {8: torch.int64, 4: torch.int32, 2: torch.int16}
GUARD = 64


@pytest.fixture(scope="module")
def L():
    import gnnops

    return gnnops.load_library()


def _stream():
    from gnnops.ops import _stream as s

    return s()


def _bits(a):
    """numpy storage array -> CPU tensor of its integer view."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(f"i{a.dtype.itemsize}").copy())


def _place(bits, off_elems):
    """Integer-view CPU tensor -> device copy `off_elems` elements off a 16-byte boundary."""
    es = bits.element_size()
    buf = torch.empty(bits.numel() * es + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    x = buf[off_elems * es:off_elems * es + bits.numel() * es].view(bits.dtype).view(bits.shape)
    x.copy_(bits)
    assert x.data_ptr() % 16 == (off_elems * es) % 16
    return x


def _guarded(shape, dtype, fill):
    """(whole buffer, view of `shape` in its middle): GUARD elements of `fill` on either side."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


def _index_for(L, c, index64):
    """The index the call reads: int64 as built, or the 4- / 2-byte copy gnnops_narrow_index makes of it."""
    N = c.N
    if c.ib == 8:
        return _place(torch.from_numpy(index64), c.idx_off)
    if c.ib == 2 and N > 65535:                               # the narrowing pass cannot mark an id "outside" here: 0xFFFF is one
        assert index64.min() >= 0 and index64.max() < N
        return _place(torch.from_numpy(index64.astype(np.uint16).view(np.int16)), c.idx_off)
    wide = torch.from_numpy(index64).cuda()
    es = c.ib
    buf = torch.empty(index64.size * es + 64, dtype=torch.uint8, device="cuda")
    out = buf[c.idx_off * es:c.idx_off * es + index64.size * es].view(IDT[es]).view(index64.shape)
    assert L.gnnops_narrow_index(wide.data_ptr(), out.data_ptr(), index64.size, es, N, _stream()) == 0
    want = np.where((index64 >= 0) & (index64 < N), index64, -1).astype(np.int32 if es == 4 else np.int16)
    assert torch.equal(out.cpu(), torch.from_numpy(want)), "narrow_index"
    return out


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_direct_call(L, c):
    inp = sc.inputs(c.name)
    want_out, want_arg = sc.expected(c.name)
    src = _place(_bits(inp.src), c.src_off)
    index = _index_for(L, c, inp.index)
    d = sc.check_route(c, src.data_ptr(), index.data_ptr())    # with the addresses of this call
    valid = bool(((inp.index >= 0) & (inp.index < c.N)).all())
    assert valid or c.route in (LDS, CHUNKS), "ids outside [0, N) may only reach the LDS routes"
    shape = (c.B, c.N, c.K)
    fill = 0x5a5a if sc.EB[c.dt] == 2 else 0x5a5a5a5a
    obuf, out = _guarded(shape, IVIEW[c.dt], fill)
    if c.init:
        out.copy_(_bits(inp.out_init))
    is_arg = c.red in ("min", "max")
    abuf, arg = _guarded(shape, torch.int32 if c.ab == 4 else torch.int64, -7) if is_arg else (None, None)
    ws_bytes = L.gnnops_scatter_elementwise_workspace_bytes(c.B, c.N, c.K, sc.DT[c.dt], sc.RED[c.red])
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda")
    rc = L.gnnops_scatter_elementwise_ixa(src.data_ptr(), index.data_ptr(), c.ib, out.data_ptr(), arg.data_ptr() if is_arg else None,
                                          c.ab, c.B, c.E, c.K, c.N, sc.DT[c.dt], sc.RED[c.red], c.init, ws.data_ptr(), ws_bytes, _stream())
    assert rc == 0, L.gnnops_last_error()
    got = out.cpu()
    exp = _bits(want_out)
    if not torch.equal(got, exp):
        bad = (got != exp).nonzero()
        b, n, k = bad[0].tolist()
        raise AssertionError(f"{c.name}: {len(bad)} of {got.numel()} values differ; first at {(b, n, k)} (chunks {sc.chunks_of(c)[:3]}, "
                             f"detail {d}): got {got[b, n, k].item():#x} expected {exp[b, n, k].item():#x}")
    if is_arg:
        ga = arg.cpu().to(torch.int64)
        ea = torch.from_numpy(want_arg)
        if not torch.equal(ga, ea):
            bad = (ga != ea).nonzero()
            b, n, k = bad[0].tolist()
            raise AssertionError(f"{c.name}: {len(bad)} arg rows differ; first at {(b, n, k)}: got {ga[b, n, k].item()} expected {ea[b, n, k].item()}")
        assert _guards_intact(abuf, -7), "arg guard"
    assert _guards_intact(obuf, fill), "out guard"
    assert torch.equal(src.cpu(), _bits(inp.src)), "src was written"


@pytest.mark.parametrize("c,status", sc.refusal_cases(), ids=[c.name for c, _ in sc.refusal_cases()])
def test_refusals(L, c, status):
    """Host-side refusals: the status the header names, and nothing written."""
    src = torch.ones(c.B * c.E * c.K, dtype=torch.float32, device="cuda")
    index = torch.zeros(c.B * c.E * c.K, dtype=torch.int64, device="cuda")      # valid as any index width
    obuf, out = _guarded((c.B, c.N, c.K), torch.int32, 0x5a5a5a5a)
    abuf, arg = _guarded((c.B, c.N, c.K), torch.int64, -7)
    rc = L.gnnops_scatter_elementwise_ixa(src.data_ptr(), index.data_ptr(), c.ib, out.data_ptr(), arg.data_ptr(), c.ab, c.B, c.E, c.K, c.N,
                                          sc.DT[c.dt], sc.RED[c.red], 0, None, 0, _stream())
    assert rc == status, (rc, L.gnnops_last_error())
    torch.cuda.synchronize()
    assert bool((obuf == 0x5a5a5a5a).all()) and bool((abuf == -7).all())


@pytest.mark.parametrize("out_bytes", [4, 2])
@pytest.mark.parametrize("in_off,out_off", [(0, 0), (1, 0), (0, 1)], ids=["aligned", "input-off-16", "output-off-pair"])
def test_narrow_index(L, out_bytes, in_off, out_off):
    """gnnops_narrow_index at 0, 1, 2 ids, around one workgroup's share and around one full eight-load sweep of its grid;
    ids -1, bound and bound + 65536 + 5 become all ones, bound - 1 is kept."""
    bound = 65535 if out_bytes == 2 else 70001
    g = torch.Generator().manual_seed(out_bytes * 10 + in_off * 2 + out_off)
    for n in sc.narrow_lengths():
        ids = torch.randint(0, bound, (n,), generator=g)
        special = torch.tensor([-1, bound, bound + 65536 + 5, bound - 1, 0])
        for j in range(min(n, 5)):
            ids[(j * 977) % n] = special[j]
        if n >= 8:
            ids[-1], ids[-2], ids[0], ids[1] = -1, bound - 1, bound, bound - 1
        ibuf = torch.zeros(n + 4, dtype=torch.int64, device="cuda")
        src = ibuf[in_off:in_off + n]
        src.copy_(ids)
        assert n == 0 or src.data_ptr() % 16 == 8 * in_off
        obuf = torch.full((n + 2 * GUARD,), 0x1234, dtype=IDT[out_bytes], device="cuda")
        out = obuf[GUARD + out_off:GUARD + out_off + n]
        assert n == 0 or out.data_ptr() % (2 * out_bytes) == out_bytes * out_off
        assert L.gnnops_narrow_index(src.data_ptr(), out.data_ptr(), n, out_bytes, bound, _stream()) == 0, L.gnnops_last_error()
        want = torch.where((ids >= 0) & (ids < bound), ids, torch.tensor(-1)).to(IDT[out_bytes])
        assert torch.equal(out.cpu(), want), n
        rest = torch.cat([obuf[:GUARD + out_off], obuf[GUARD + out_off + n:]])
        assert bool((rest == 0x1234).all()), n
    assert L.gnnops_narrow_index(ibuf.data_ptr(), obuf.data_ptr(), 4, 2, 65536, _stream()) == sc.EINVAL      # 0xFFFF must stay free
    assert L.gnnops_narrow_index(ibuf.data_ptr(), obuf.data_ptr(), 4, 4, 2 ** 31, _stream()) == sc.EINVAL


# ---------------------------------------------------------------------------------------------- through gnnops.scatter
def _through(c, dim_kind):
    """A case's operands reshaped for gnnops.scatter: [B, E, K] along its middle dim, or 2-D along dim 0 / dim 1."""
    if dim_kind == "dim0":
        assert c.B == 1
        return (c.E, c.K), (c.N, c.K), 0
    if dim_kind == "dim1":
        assert c.K == 1
        return (c.B, c.E), (c.B, c.N), 1
    return (c.B, c.E, c.K), (c.B, c.N, c.K), 1


# (case, how its [B, E, K] operands are handed over, the route of the launch that must have produced the result)
WRAPPER = [("one-k2-at-sum-f32", "dim0", LDS), ("one-k2-over-sum-f32", "dim0", CHUNKS), ("one-k2-at-max-f32", "dim0", LDS),
           ("one-k2-over-min-f16", "dim0", CHUNKS), ("atomics-sum-f32-dim0", "dim0", ATOMICS), ("atomics-min-f16-dim0", "dim0", ATOMICS),
           ("atomics-max-f32-init-k2", "dim0", ATOMICS), ("strip-tc1-sum-f16", "dim1", LDS), ("edges-sum-f32", "dim1", CHUNKS),
           ("edges-max-bf16", "dim1", CHUNKS), ("width-chunks-sum-i4-a8", "dim1", CHUNKS), ("atomics-sum-f32-k1", "dim1", ATOMICS),
           ("atomics-min-f16-k1", "dim1", ATOMICS), ("atomics-sum-f16-init", "dim1", ATOMICS), ("atomics-min-f32-init", "dim1", ATOMICS),
           ("strip-tc3-max-f32", "mid", LDS), ("edges-min-f32", "mid", CHUNKS), ("edges-mean-f16", "mid", CHUNKS),
           ("width-chunks-max-i4-a8", "mid", CHUNKS), ("atomics-mul-bf16-k2", "mid", ATOMICS), ("atomics-mean-f32-k2", "mid", ATOMICS),
           ("atomics-max-f32-k2", "mid", ATOMICS)]


def _record_launches(monkeypatch, L):
    """Every call gnnops.scatter makes to the two element-wise entry points it uses: [(route the query reports for the
    call's own arguments and addresses, status)]."""
    import ctypes

    seen = []

    def spy(name, has_ab):
        real = getattr(L, name)

        def call(*a):
            src, index, ib = a[0], a[1], a[2]
            ab, rest = (a[5], a[6:]) if has_ab else (8, a[5:])
            B, E, K, N, dt, red = rest[:6]
            d = (ctypes.c_int64 * 8)()
            r = L.gnnops_scatter_elementwise_route(B, E, K, N, dt, red, ib, ab, src or 0, index or 0, d)
            rc = real(*a)
            seen.append((r, rc))
            return rc

        monkeypatch.setattr(L, name, call)

    spy("gnnops_scatter_elementwise_ix", False)
    spy("gnnops_scatter_elementwise_ixa", True)
    return seen


@pytest.mark.parametrize("name,dim_kind,route", WRAPPER, ids=[f"{n}-{k}" for n, k, _ in WRAPPER])
def test_through_scatter(L, monkeypatch, name, dim_kind, route):
    """The same operands through gnnops.scatter: each route along dim 0, dim 1 and a 3-D middle dim, `out=` on the LDS, the
    chunked and the atomic route. The launches the wrapper makes are recorded: the one that succeeds is on the route named.
    Along dim 0 without `out=`, an N of the atomic form first goes to the transposed route, whose narrowed operands the
    library refuses (GNNOPS_EUNSUPPORTED, nothing launched), and then to the atomics with the int64 index along dim 1."""
    import gnnops

    c = sc.by_name(name)
    inp = sc.inputs(name)
    idx = np.where((inp.index >= 0) & (inp.index < c.N), inp.index, 0) if c.dropped else inp.index   # the wrapper's contract: ids in [0, N)
    sshape, oshape, dim = _through(c, dim_kind)
    src = _bits(inp.src).cuda().view(TDT[c.dt]).view(sshape)
    index = torch.from_numpy(idx).cuda().view(sshape)
    from oracle import oracle

    kw = {"out": inp.out_init} if c.init else {"dim_size": c.N}
    exp = oracle.scatter(inp.src, idx, dim=1, reduce=c.red, dtype=c.dt, **kw)
    out = _bits(inp.out_init).cuda().view(TDT[c.dt]).view(oshape) if c.init else None
    seen = _record_launches(monkeypatch, L)
    gnnops.set_plan_cache(False)
    try:
        got = gnnops.scatter(src, index, dim, out=out, dim_size=None if c.init else c.N, reduce=c.red)
    finally:
        gnnops.set_plan_cache(True)
    assert seen and seen[-1] == (route, 0), seen
    assert all(rc == sc.EUNSUPPORTED and r == sc.NONE for r, rc in seen[:-1]), seen
    if dim_kind == "dim0" and route == ATOMICS and not c.init:
        assert len(seen) == 2, seen                              # the transposed route was tried and refused
    else:
        assert len(seen) == 1, seen
    gv, ga = got if isinstance(got, tuple) else (got, None)
    ev, ea = exp if isinstance(exp, tuple) else (exp, None)
    assert gv.shape == oshape and (out is None or gv.data_ptr() == out.data_ptr())
    assert torch.equal(gv.contiguous().view(IVIEW[c.dt]).cpu().view(c.B, c.N, c.K), _bits(ev)), name
    if ea is not None:
        assert torch.equal(ga.cpu().view(c.B, c.N, c.K), torch.from_numpy(ea)), name + " arg"


@pytest.mark.parametrize("red,dt", [("sum", "f32"), ("max", "f32"), ("min", "f16"), ("mean", "bf16")])
def test_transposed_route_starts_where_a_column_stops_fitting(red, dt, monkeypatch):
    """dim 0 of a matrix: N * cell == budget stays on the strip kernel (chunked), one destination more goes through the
    transposes; both give the oracle's bits."""
    import gnnops
    from gnnops import ops
    from oracle import oracle

    E, K = 400, 6
    n_fit = sc.budget() // sc.cell(dt, red, E)
    took = []
    real = ops._scatter_transposed
    monkeypatch.setattr(ops, "_scatter_transposed", lambda *a: (lambda r: (took.append(r is not None), r)[1])(real(*a)))
    for N, transposed in ((n_fit, False), (n_fit + 1, True)):
        c = sc.Case(f"wrap-{red}-{dt}-{N}", 1, E, K, N, dt, red, 8, 8, 0, CHUNKS, {}, (), 0, 0, False, False)
        assert sc.query(c)[0] == CHUNKS and (sc.route(1, E, 1, N, dt, red)[0] == LDS) == (not transposed)
        rng = np.random.default_rng(N)
        idx = rng.permutation(np.arange(E * K) % (N - 3)).reshape(E, K) + 3
        idx[0, :], idx[E - 1, :] = N - 1, 0
        src = sc._store(sc._values(rng, (E, K), c), dt)
        del took[:]
        got = gnnops.scatter(_bits(src).cuda().view(TDT[dt]), torch.from_numpy(idx).cuda(), 0, dim_size=N, reduce=red)
        assert took == ([True] if transposed else []), (N, took)
        exp = oracle.scatter(src, idx, dim=0, dim_size=N, reduce=red, dtype=dt)
        gv, ga = got if isinstance(got, tuple) else (got, None)
        ev, ea = exp if isinstance(exp, tuple) else (exp, None)
        assert torch.equal(gv.view(IVIEW[dt]).cpu(), _bits(ev)), (red, dt, N)
        if ea is not None:
            assert torch.equal(ga.cpu(), torch.from_numpy(ea)), (red, dt, N)
