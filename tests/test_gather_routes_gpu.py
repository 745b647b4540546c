"""csrc/gather.hip at every route and seam: index_select (pull: ROWS / K1 / LDS / LONGROWS / ELEMS; planned push),
gather (LDS / ELEMS) and index_select_sum (ROWS / LDS / LONGROWS / ELEMS), from the tables of gather_cases.py.

Every case first asks the library's route query (with the addresses the call will see) and fails unless it reports the
route and geometry the case aims at. Copies are compared bit for bit on the integer view against torch's own indexing
on the CPU copy: tables hold random bit patterns (NaN payloads, -0.0 and subnormals occur), indices repeat rows and
leave rows unselected. index_select_sum tables hold integers |v| <= 3 with 3*B*E*K < 2^24, so the fp32 sum is exact in
any order and must equal the int64 sum. The two grid-wrap cases (0.27 and 0.14 GB of output) are compared on the device."""
import zlib

import pytest
import torch

import gather_cases as gc

pytestmark = pytest.mark.gpu

TDT = {"u8": torch.uint8, "f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "i64": torch.int64}
IDT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
IRANGE = {1: (0, 256), 2: (-2 ** 15, 2 ** 15), 4: (-2 ** 31, 2 ** 31), 8: (-2 ** 63, 2 ** 63 - 1)}


@pytest.fixture(scope="module")
def gnnops():
    import gnnops as g

    g.load_library()
    return g


def _gen(c):
    return torch.Generator().manual_seed(zlib.crc32(f"{c.op}/{c.name}".encode()))


def _shape(c, n):
    """Shape and indexed dimension of a [B, n, K] tensor in the case's layout."""
    return {"3d": ((c.B, n, c.K), 1), "1d": ((n,), 0), "2d0": ((n, c.K), 0), "2d1": ((c.B, n), 1)}[c.layout]


def _place(values, c, dtype):
    """`values` (CPU) copied to the device `c.off` bytes into a 16-byte aligned flat buffer, viewed as `dtype`."""
    nbytes = values.numel() * values.element_size()
    buf = torch.empty(nbytes + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    x = buf[c.off:c.off + nbytes].view(values.dtype).view(values.shape)
    x.copy_(values)
    assert x.data_ptr() % 16 == c.off % 16 and x.is_contiguous()
    return x.view(dtype)


def _table(c, g):
    """Random bit patterns: (CPU integer view, device tensor of the case's dtype at the case's offset)."""
    eb = gc.EB[c.dt]
    shape, _ = _shape(c, c.N)
    xi = torch.randint(*IRANGE[eb], shape, generator=g, dtype=IDT[eb])
    return xi, _place(xi, c, TDT[c.dt])


def _rows(N, shape, g):
    """Row numbers of the given shape over [0, N): rows n % 5 == 2 stay unselected, the rest repeat; the first and the last
    four rows (a staged tile's vector tail) are always among them when there is room."""
    allowed = torch.tensor([n for n in range(N) if n % 5 != 2 or N < 3])
    idx = allowed[torch.randint(0, len(allowed), shape, generator=g)]
    flat = idx.view(-1)
    if flat.numel() >= 8:
        forced = torch.tensor([N - 1, 0, N - 1, max(N - 2, 0), max(N - 3, 0), max(N - 4, 0), 0])
        flat[:7] = forced
        flat[-1] = N - 1
    return idx


def _index(c, idx_cpu):
    ibuf = torch.empty(idx_cpu.numel() + 2, dtype=torch.int64, device="cuda")
    assert ibuf.data_ptr() % 16 == 0
    idx = ibuf[c.idx_off:c.idx_off + idx_cpu.numel()].view(idx_cpu.shape)
    idx.copy_(idx_cpu)
    assert idx.data_ptr() % 16 == 8 * c.idx_off
    return idx


def _setmap(monkeypatch, c):
    if c.pmap is None:
        monkeypatch.delenv("GNNOPS_PULL_MAP", raising=False)
    else:
        monkeypatch.setenv("GNNOPS_PULL_MAP", c.pmap)


def _ids(cases):
    return [c.name for c in cases]


# ------------------------------------------------------------------------------------------------ index_select
@pytest.mark.parametrize("c", gc.select_cases(), ids=_ids(gc.select_cases()))
def test_index_select(gnnops, monkeypatch, c):
    g = _gen(c)
    xi, x = _table(c, g)
    _, dim = _shape(c, c.N)
    idx_cpu = _rows(c.N, (c.E,), g)
    idx = _index(c, idx_cpu)
    gc.check_route(gnnops.load_library(), c, x.data_ptr())
    _setmap(monkeypatch, c)
    got = gnnops.index_select(x, dim, idx)
    assert got.data_ptr() % 16 == 0 and got.dtype == x.dtype      # the route was asked for an aligned output
    ref = xi[idx_cpu] if dim == 0 else xi[:, idx_cpu]
    assert torch.equal(got.view(xi.dtype).cpu(), ref)
    assert torch.equal(x.view(xi.dtype).cpu(), xi)                 # the table is untouched


@pytest.mark.parametrize("c", gc.select_wrap_cases(), ids=_ids(gc.select_wrap_cases()))
def test_index_select_grid_wrap(gnnops, monkeypatch, c):
    """The grid is capped at 16384 workgroups: the loop of select_rows_kernel takes a second trip, under both maps."""
    g = _gen(c)
    xi, x = _table(c, g)
    idx_cpu = _rows(c.N, (c.E,), g)
    idx = _index(c, idx_cpu)
    d = gc.check_route(gnnops.load_library(), c, x.data_ptr())
    items = c.B * d[1] * c.E
    assert d[3] == gc.ROWS_GRID_CAP and d[3] * gc.step_items(d[0]) < items       # a second trip, not a full one
    ref = x.view(xi.dtype)[:, idx]                                               # torch's own indexing, on the device
    outs = []                                                                    # both results stay alive: the second map
    for pmap in (None, "g"):                                                     # cannot inherit the first one's block
        _setmap(monkeypatch, c._replace(pmap=pmap))
        outs.append(gnnops.index_select(x, 1, idx))
    assert outs[0].data_ptr() != outs[1].data_ptr()
    for pmap, got in zip(("default", "g"), outs):
        assert torch.equal(got.view(xi.dtype), ref), pmap
    del outs
    probe = torch.arange(0, c.E, 4099)                                           # and a sample against the CPU copy
    assert torch.equal(ref[:, probe].cpu(), xi[:, idx_cpu[probe]])


def _plan_index(c, g):
    N = c.N
    if c.plan == "small":
        counts = torch.randint(0, 4, (N,), generator=g)
        counts[[0, 1, 2, 20, 21, N - 3, N - 2, N - 1]] = 0       # empty segments at the front, in the middle, at the end
        counts[5], counts[6], counts[7] = gc.PUSH_PU - 1, gc.PUSH_PU, gc.PUSH_PU + 1
    else:
        counts = torch.randint(0, 9, (N,), generator=g)
        counts[[0, N - 1]] = 0
        counts[11] = c.plan[1]
    idx = torch.repeat_interleave(torch.arange(N), counts)
    return idx[torch.randperm(idx.numel(), generator=g)]


@pytest.mark.parametrize("c", gc.push_cases(), ids=_ids(gc.push_cases()))
def test_index_select_planned_push(gnnops, monkeypatch, c):
    """Push form over a plan equals the pull form equals torch: empty segments, segments of PU - 1, PU and PU + 1
    positions, and a row on each side of the hub threshold (more than hub::T_HUB positions: written by the hub pass)."""
    g = _gen(c)
    xi, x = _table(c, g)
    idx_cpu = _plan_index(c, g)
    c = c._replace(E=idx_cpu.numel())
    idx = _index(c, idx_cpu)
    if isinstance(c.plan, tuple):
        assert c.B == 1 and c.E > gc.T_HUB and int((idx_cpu == 11).sum()) == c.plan[1]
    gc.check_route(gnnops.load_library(), c, x.data_ptr())        # the pull form of the same call: ROWS
    _setmap(monkeypatch, c)
    plan = gnnops.Plan(idx, c.N)
    push = gnnops.index_select(x, 1, idx, plan=plan)
    pull = gnnops.index_select(x, 1, idx)
    ref = xi[:, idx_cpu]
    assert torch.equal(push.view(xi.dtype).cpu(), ref)
    assert torch.equal(pull.view(xi.dtype).cpu(), ref)


# ------------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("c", gc.gather_cases(), ids=_ids(gc.gather_cases()))
def test_gather(gnnops, c):
    g = _gen(c)
    xi, x = _table(c, g)
    ishape, dim = _shape(c, c.E)
    idx_cpu = _rows(c.N, ishape, g)
    idx = _index(c, idx_cpu)
    gc.check_route(gnnops.load_library(), c)
    got = gnnops.gather(x, dim, idx)
    assert got.shape == idx.shape and got.dtype == x.dtype
    assert torch.equal(got.view(xi.dtype).cpu(), torch.gather(xi, dim, idx_cpu))


# ------------------------------------------------------------------------------------------- index_select_sum
@pytest.mark.parametrize("c", gc.sum_cases(), ids=_ids(gc.sum_cases()))
def test_index_select_sum(gnnops, c):
    g = _gen(c)
    shape, dim = _shape(c, c.N)
    xi = torch.randint(-3, 4, shape, generator=g)                  # exact in fp16, bf16 and fp32
    assert 3 * c.B * c.E * c.K < 2 ** 24
    x = _place(xi.to(TDT[c.dt]), c, TDT[c.dt])
    idx_cpu = _rows(c.N, (c.E,), g)
    idx = _index(c, idx_cpu)
    gc.check_route(gnnops.load_library(), c, x.data_ptr())
    got = gnnops.index_select_sum(x, dim, idx)
    assert got.dtype == torch.float32 and got.dim() == 0
    ref = int((xi[idx_cpu] if dim == 0 else xi[:, idx_cpu]).sum())
    assert got.item() == float(ref), (got.item(), ref)
