"""GPU suite: the row-wise SpGEMM behind gnnops.spspmm(..., method="rowwise" | "auto") (csrc/spgemm.hip).

One wave owns an output row: it marks an LDS bitmap over the row's column window [lo, lo + span), accumulates in fp32 in LDS while
it walks A's row one nonzero at a time in stored order, and writes the row in ascending column order, 64 columns per step. Index,
values and count are compared BIT FOR BIT with oracle.spspmm and with method="esc" (expand - sort - compress, the default), on
the smallest shapes at which each mechanism can go wrong: rows of B around the 64-lane seam, stored order different from sorted
order, columns at the 32- and 64-bit seams of the bitmap walk, windows of exactly W and W + 1 columns (W is read from
gnnops.spgemm_max_span()), summation order, signed and cancelled zeros, repeats in a row of B (not eligible: "rowwise" raises,
"auto" falls back), more rows than one sweep of the grid (4 rows per workgroup, 2048 workgroups) and than one scan tile (8192).
"""
import numpy as np
import pytest
import torch

from helpers import TORCH_DT, assert_bits_equal, to_np

pytestmark = pytest.mark.gpu

DNAMES = ["f32", "f16", "bf16"]
ROWS_PER_WG, SWEEP = 4, 4 * 2048   # csrc/spgemm.hip: waves per workgroup; rows one sweep of the capped grid covers (= scan tile)


@pytest.fixture(scope="module")
def gnnops():
    import gnnops as g

    g.load_library()
    return g


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o

    return o


@pytest.fixture(scope="module")
def W(gnnops):
    w = gnnops.spgemm_max_span()
    assert w >= 4096
    return w


def _rand(g, shape, dname):
    return (torch.rand(shape, generator=g) * 2 - 1).to(TORCH_DT[dname])


def _raw(t):
    """Bit image of a value tensor: tells -0.0 from +0.0, which helpers.assert_bits_equal does not."""
    return t.cpu().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _run(gnnops, method, iA, vA, iB, vB, m, k, n):
    return gnnops.spspmm(iA.cuda(), vA.cuda(), iB.cuda(), vB.cuda(), m, k, n, method=method)


def check(gnnops, oracle, iA, vA, iB, vB, m, k, n, dname, what, use_oracle=True):
    """rowwise == auto == esc (raw bits) and == oracle.spspmm; returns nnz(C)."""
    ei, ev = _run(gnnops, "esc", iA, vA, iB, vB, m, k, n)
    for method in ("rowwise", "auto"):
        gi, gv = _run(gnnops, method, iA, vA, iB, vB, m, k, n)
        assert gi.dtype == torch.int64 and gv.dtype == vA.dtype
        assert tuple(gi.shape) == tuple(ei.shape) and tuple(gv.shape) == tuple(ev.shape), f"{what} {method}: {tuple(gi.shape)} vs {tuple(ei.shape)}"
        assert torch.equal(gi.cpu(), ei.cpu()), f"{what} {method}: index differs from esc"
        assert torch.equal(_raw(gv), _raw(ev)), f"{what} {method}: value bits differ from esc"
        if use_oracle:
            oi, ov = oracle.spspmm(iA.numpy(), to_np(vA), iB.numpy(), to_np(vB), m, k, n, dtype=dname)
            assert tuple(gi.shape) == oi.shape, f"{what} {method}: count {gi.shape[1]} vs oracle {oi.shape[1]}"
            assert_bits_equal(to_np(gi), oi, f"{what} {method}: index")
            assert_bits_equal(to_np(gv), ov, f"{what} {method}: values")
    return ei.shape[1]


def check_falls_back(gnnops, iA, vA, iB, vB, m, k, n, why, what):
    with pytest.raises(NotImplementedError, match=why):
        _run(gnnops, "rowwise", iA, vA, iB, vB, m, k, n)
    ei, ev = _run(gnnops, "esc", iA, vA, iB, vB, m, k, n)
    gi, gv = _run(gnnops, "auto", iA, vA, iB, vB, m, k, n)
    assert torch.equal(gi.cpu(), ei.cpu()) and torch.equal(_raw(gv), _raw(ev)), f"{what}: auto differs from esc"


def rows_of_lengths(g, lengths, n, lo=0):
    """COO of a matrix whose row r holds lengths[r] DISTINCT columns of [lo, n), in shuffled stored order (rows interleaved)."""
    rows = torch.cat([torch.full((ln,), r, dtype=torch.int64) for r, ln in enumerate(lengths)])
    cols = torch.cat([torch.randperm(n - lo, generator=g)[:ln] + lo for ln in lengths])
    p = torch.randperm(rows.numel(), generator=g)
    return torch.stack([rows[p], cols[p]])


def assert_unsorted(idx, width):
    key = (idx[0] * width + idx[1]).numpy()
    assert (np.diff(key) < 0).any(), "stored order must differ from sorted order"


# ---- lane-group seams and stored order ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
def test_lane_group_seams_and_stored_order(gnnops, oracle, dname):
    """Rows of B of length 0, 1, 63, 64, 65, 129 (one lane step less one, exact, plus one, two steps plus one); every row of B and
    every row of A shuffled, A with repeated (i, kk) entries, rows of A from 0 to 70 nonzeros (more than one 64-nonzero batch)."""
    g = torch.Generator().manual_seed(11)
    lengths = [0, 1, 63, 64, 65, 129, 0, 64]
    k, n, m = len(lengths), 300, 9
    iB = rows_of_lengths(g, lengths, n)
    a_rows = torch.cat([torch.full((c,), r, dtype=torch.int64) for r, c in enumerate([0, 1, 3, 8, 70, 6, 0, 2, 5])])
    iA = torch.stack([a_rows, torch.randint(0, k, (a_rows.numel(),), generator=g)])
    iA = iA[:, torch.randperm(iA.size(1), generator=g)]
    assert np.unique((iA[0] * k + iA[1]).numpy()).size < iA.size(1), "A repeats (i, kk)"
    assert_unsorted(iA, k)
    assert_unsorted(iB, n)
    assert sorted(set(np.bincount(iB[0].numpy(), minlength=k))) == [0, 1, 63, 64, 65, 129]
    check(gnnops, oracle, iA, _rand(g, (iA.size(1),), dname), iB, _rand(g, (iB.size(1),), dname), m, k, n, dname, "lane seams")


# ---- bitmap word seams ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
def test_bitmap_word_seams(gnnops, oracle, dname, W):
    """Output rows whose columns sit at window offsets 31/32/33 and 63/64/65, at the first and the last bit of a full window, all
    of them at once, and one row that fills its window; the windows start at column 7."""
    g = torch.Generator().manual_seed(12)
    lo = 7
    offs = [31, 32, 33, 63, 64, 65, W - 1]
    rows, cols = [], []
    for r, off in enumerate(offs):              # row r of B: {lo, lo + off}
        rows += [r, r]
        cols += [lo + off, lo]
    dense_row = len(offs)
    rows += [dense_row] * W
    cols += (torch.randperm(W, generator=g) + lo).tolist()
    k, n = dense_row + 1, lo + W + 3
    iB = torch.tensor([rows, cols], dtype=torch.int64)
    # A: row r -> row r of B; row k: the six seam rows together; row k + 1: all offsets and the last bit; row k + 2: the dense row twice
    a = [(r, r) for r in range(k)] + [(k, r) for r in (5, 2, 0, 4, 1, 3)] + [(k + 1, r) for r in (6, 3, 0, 5, 1, 4, 2)]
    a += [(k + 2, dense_row), (k + 2, 0), (k + 2, dense_row)]
    iA = torch.tensor(a, dtype=torch.int64).t().contiguous()
    m = k + 3
    nnz = check(gnnops, oracle, iA, _rand(g, (iA.size(1),), dname), iB, _rand(g, (iB.size(1),), dname), m, k, n, dname, "word seams")
    assert nnz == 2 * len(offs) + W + 7 + 8 + W


# ---- window edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
def test_window_of_exactly_W_and_W_plus_1(gnnops, oracle, dname, W):
    """Two narrow rows of B whose union spans exactly W columns run row-wise; one column further and "rowwise" raises, "auto" equals
    "esc". A row of B that is wide on its own: not eligible when A references it, ignored (repeat and all) when A does not."""
    g = torch.Generator().manual_seed(13)
    k, m = 4, 3

    def operands(last_col, reference_wide):
        # rows of B: 0 = {10, 12}, 1 = {11, last_col}, 2 = empty, 3 = wide on its own, holding column 5 twice
        iB = torch.tensor([[1, 0, 3, 0, 1, 3, 3], [last_col, 12, 5, 10, 11, W + 40, 5]], dtype=torch.int64)
        iA = torch.tensor([[0, 2, 0, 2, 1], [1, 0, 0, 2, 3 if reference_wide else 2]], dtype=torch.int64)
        return iA, _rand(g, (iA.size(1),), dname), iB, _rand(g, (iB.size(1),), dname)

    n = W + 50
    check(gnnops, oracle, *operands(10 + W - 1, False), m, k, n, dname, "span W")
    check_falls_back(gnnops, *operands(10 + W, False), m, k, n, "wide", "span W + 1")
    check_falls_back(gnnops, *operands(10 + W - 1, True), m, k, n, "wide", "wide row of B")


@pytest.mark.parametrize("dname", DNAMES)
def test_block_diagonal_unequal_blocks(gnnops, oracle, dname):
    """Four diagonal blocks of 3, 70, 200 and 33 nodes: every window but the first block's starts at a non-zero column."""
    g = torch.Generator().manual_seed(14)
    sizes, dens = [3, 70, 200, 33], [2, 9, 12, 33]
    parts, start = [], 0
    for s, d in zip(sizes, dens):
        parts.append(rows_of_lengths(g, [d] * s, s) + start)
        start += s
    idx = torch.cat(parts, dim=1)
    idx = idx[:, torch.randperm(idx.size(1), generator=g)]
    n = start
    v = _rand(g, (idx.size(1),), dname)
    nnz = check(gnnops, oracle, idx, v, idx, v, n, n, n, dname, "block diagonal")
    assert nnz <= sum(s * s for s in sizes)


# ---- order of summation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
def test_order_of_summation(gnnops, oracle, dname):
    """C[0, 3] is fed by 40 nonzeros of A's row 0 (10 rows of B, each referenced 4 times: repeated (i, kk) entries) with magnitudes
    over 2^-12 .. 2^12; in fp32 the sum depends on the order, so only A's stored order reproduces the bits."""
    g = torch.Generator().manual_seed(15)
    k, n, m = 10, 8, 2
    kk = torch.arange(k).repeat(4)[torch.randperm(40, generator=g)]
    iA = torch.stack([torch.zeros(40, dtype=torch.int64), kk])
    iA = torch.cat([iA, torch.tensor([[1], [4]])], dim=1)
    expo = torch.randint(-12, 13, (41,), generator=g).float()
    vA = ((torch.rand(41, generator=g) + 1) * torch.exp2(expo) * (torch.randint(0, 2, (41,), generator=g) * 2 - 1)).to(TORCH_DT[dname])
    iB = torch.cat([torch.stack([torch.arange(k), torch.full((k,), 3)]), rows_of_lengths(g, [2] * k, 3)], dim=1)
    iB = iB[:, torch.randperm(iB.size(1), generator=g)]
    vB = (torch.rand(iB.size(1), generator=g) + 0.5).to(TORCH_DT[dname])
    if dname == "f32":   # the case is sharp: summing the same products in sorted order gives other bits
        bcol3 = {int(r): float(vB[j]) for j, (r, c) in enumerate(iB.t().tolist()) if c == 3}
        prods = np.array([np.float32(vA[t]) * np.float32(bcol3[int(kk[t])]) for t in range(40)], dtype=np.float32)
        stored = np.float32(0)
        for p in prods:
            stored = np.float32(stored + p)
        other = np.float32(0)
        for p in np.sort(prods):
            other = np.float32(other + p)
        assert stored != other
    check(gnnops, oracle, iA, vA, iB, vB, m, k, n, dname, "summation order")


# ---- zeros ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
def test_zeros(gnnops, oracle, dname):
    """A lone -0.0 product comes out as +0.0 (the accumulator starts at +0.0); a sum that cancels exactly stays as a stored zero."""
    dt = TORCH_DT[dname]
    iA = torch.tensor([[0, 1, 1, 2], [0, 1, 2, 1]], dtype=torch.int64)
    vA = torch.tensor([-1.0, 3.0, -1.5, 2.0], dtype=dt)
    iB = torch.tensor([[0, 1, 2, 1], [4, 2, 2, 6]], dtype=torch.int64)
    vB = torch.tensor([0.0, 0.5, 1.0, 0.25], dtype=dt)
    assert check(gnnops, oracle, iA, vA, iB, vB, 3, 3, 8, dname, "zeros") == 5
    gi, gv = _run(gnnops, "rowwise", iA, vA, iB, vB, 3, 3, 8)
    assert gi.cpu().tolist() == [[0, 1, 1, 2, 2], [4, 2, 6, 2, 6]]
    vals = dict(zip(map(tuple, gi.cpu().t().tolist()), _raw(gv).tolist()))
    assert vals[(0, 4)] == 0, "-1 * 0 = -0.0 must come out as +0.0"
    assert vals[(1, 2)] == 0, "3 * 0.5 - 1.5 * 1 cancels to a stored +0.0"


@pytest.mark.parametrize("dname", DNAMES)
def test_no_output(gnnops, oracle, dname):
    """All-empty A; A whose every column meets an empty row of B; empty B: nnz(C) = 0 without a numeric launch."""
    g = torch.Generator().manual_seed(17)
    m, k, n = 6, 8, 9
    iB = rows_of_lengths(g, [3, 0, 2, 0, 4, 0, 1, 0], n)
    vB = _rand(g, (iB.size(1),), dname)
    empty_i, empty_v = torch.zeros((2, 0), dtype=torch.int64), torch.zeros(0, dtype=TORCH_DT[dname])
    assert check(gnnops, oracle, empty_i, empty_v, iB, vB, m, k, n, dname, "empty A") == 0
    iA = torch.stack([torch.randint(0, m, (20,), generator=g), torch.randint(0, 4, (20,), generator=g) * 2 + 1])
    assert check(gnnops, oracle, iA, _rand(g, (20,), dname), iB, vB, m, k, n, dname, "empty rows of B only") == 0
    assert check(gnnops, oracle, iA, _rand(g, (20,), dname), empty_i, empty_v, m, k, n, dname, "empty B") == 0


# ---- repeats in a row of B ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
def test_repeat_in_a_row_of_B(gnnops, oracle, dname):
    """One (row, column) of B stored twice, 70 entries apart in its row (two lane steps): not eligible. Without it: row-wise."""
    g = torch.Generator().manual_seed(18)
    k, n, m = 5, 150, 6
    iB = rows_of_lengths(g, [4, 100, 0, 64, 9], n)
    vB = _rand(g, (iB.size(1),), dname)
    iA = torch.stack([torch.randint(0, m, (30,), generator=g), torch.randint(0, k, (30,), generator=g)])
    vA = _rand(g, (30,), dname)
    check(gnnops, oracle, iA, vA, iB, vB, m, k, n, dname, "repeat-free")
    in_row1 = torch.nonzero(iB[0] == 1).view(-1)
    first, late = int(in_row1[3]), int(in_row1[73])
    iB2 = iB.clone()
    iB2[1, late] = iB2[1, first]
    check_falls_back(gnnops, iA, vA, iB2, vB, m, k, n, "repeat", "repeat in row 1 of B")


# ---- workgroup, sweep and scan-tile seams ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
def test_more_rows_than_one_sweep(gnnops, oracle, dname):
    """m = 8192 + 9 output rows: the grid's second sweep and the row scan's second tile; empty output rows on both sides of the
    workgroup seam (rows 3, 4), of the sweep / tile seam (8191, 8192) and at the very end."""
    g = torch.Generator().manual_seed(19)
    m, k, n = SWEEP + 9, 40, 64
    rows = torch.arange(m)
    empty = torch.zeros(m, dtype=torch.bool)
    empty[[ROWS_PER_WG - 1, ROWS_PER_WG, SWEEP - 1, SWEEP, m - 1]] = True
    empty |= torch.rand(m, generator=g) < 0.2
    rows = rows[~empty]
    rows = torch.cat([rows, rows[torch.randint(0, rows.numel(), (3000,), generator=g)]])       # some rows with several nonzeros
    iA = torch.stack([rows, torch.randint(0, k, (rows.numel(),), generator=g)])
    iA = iA[:, torch.randperm(iA.size(1), generator=g)]
    iB = rows_of_lengths(g, [int(x) for x in torch.randint(0, 7, (k,), generator=g)], n)
    iB[0, 0], iB[0, 1] = 0, 1                                                                   # not every row of B is empty
    assert iA.size(1) <= 20000
    nnz = check(gnnops, oracle, iA, _rand(g, (iA.size(1),), dname), iB, _rand(g, (iB.size(1),), dname), m, k, n, dname, "two sweeps")
    assert nnz > SWEEP


# ---- the use case -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
def test_squared_adjacency_of_small_graphs(gnnops, oracle, dname):
    """(A + I)^2 of 8 random graphs of 250 nodes at in-degree 60 (GraphUNet's third level): against "esc", and nnz(C) against the
    dense boolean product (weights are positive: no product cancels)."""
    g = torch.Generator().manual_seed(20)
    G, per, deg = 8, 250, 60
    n = G * per
    parts = []
    for b in range(G):
        blk = rows_of_lengths(g, [deg] * per, per)
        parts.append(blk[:, blk[0] != blk[1]] + b * per)
    loops = torch.arange(n)
    idx = torch.cat(parts + [torch.stack([loops, loops])], dim=1)
    idx = idx[:, torch.randperm(idx.size(1), generator=g)]
    v = (torch.rand(idx.size(1), generator=g) + 0.5).to(TORCH_DT[dname])
    nnz = check(gnnops, oracle, idx, v, idx, v, n, n, n, dname, "(A+I)^2", use_oracle=False)
    dense = torch.zeros(n, n, device="cuda")
    dense[idx[0].cuda(), idx[1].cuda()] = 1.0
    assert nnz == int(((dense @ dense) != 0).sum())


@pytest.mark.parametrize("dname", DNAMES)
def test_graph_unet_same_bits(gnnops, dname, monkeypatch):
    """GraphUNet(8, 16, 1, depth=2) on 4 graphs of 40 nodes (distinct edges: level 0 is repeat-free): with augment_adj's product forced
    to "esc" and to "rowwise", the outputs and every parameter gradient are equal bit for bit."""
    import gnnops.sparse as sparse
    from gnnops import conv

    g = torch.Generator().manual_seed(21)
    G, per = 4, 40
    n = G * per
    blocks = [rows_of_lengths(g, [5] * per, per) + b * per for b in range(G)]
    ei = torch.cat(blocks, dim=1).cuda()
    batch = torch.arange(G).repeat_interleave(per).cuda()
    torch.manual_seed(0)
    model = conv.GraphUNet(8, 16, 1, 2).to(TORCH_DT[dname]).cuda()
    x = _rand(g, (n, 8), dname).cuda()
    coef = _rand(g, (n, 1), dname).cuda()
    real, calls = sparse.spspmm, []

    def forced(method):
        def f(*args, **kwargs):
            kwargs["method"] = method
            calls.append(method)
            return real(*args, **kwargs)
        return f

    results = {}
    for method in ("esc", "rowwise"):
        monkeypatch.setattr(sparse, "spspmm", forced(method))
        for p in model.parameters():
            p.grad = None
        out = model(x, ei, batch, G)
        (out * coef).sum().backward()
        results[method] = (out.detach().clone(), [p.grad.clone() for p in model.parameters()])
    monkeypatch.setattr(sparse, "spspmm", real)
    assert calls == ["esc", "esc", "rowwise", "rowwise"]
    assert torch.equal(_raw(results["esc"][0].float()), _raw(results["rowwise"][0].float()))
    for a, b in zip(results["esc"][1], results["rowwise"][1]):
        assert torch.equal(_raw(a.float()), _raw(b.float()))


# ---- arguments ----------------------------------------------------------------------------------------------------------------------
def test_arguments(gnnops, W):
    import torch_sparse

    assert torch_sparse.spspmm is gnnops.spspmm and W == gnnops.spgemm_max_span()
    i = torch.tensor([[0, 1], [1, 0]], dtype=torch.int64).cuda()
    v = torch.ones(2).cuda()
    with pytest.raises(ValueError, match="method"):
        gnnops.spspmm(i, v, i, v, 2, 2, 2, method="hash")
    for method in ("esc", "rowwise", "auto"):
        with pytest.raises(RuntimeError, match="same dtype"):
            gnnops.spspmm(i, v, i, v.half(), 2, 2, 2, method=method)
    gi, gv = torch_sparse.spspmm(i, v, i, v, 2, 2, 2, method="rowwise")
    assert gi.cpu().tolist() == [[0, 1], [0, 1]] and gv.cpu().tolist() == [1.0, 1.0]
