"""GPU suite: the hashed row-wise SpGEMM behind gnnops.spspmm(..., method="rowhash") (csrc/spgemm.hip).

One wave owns an output row and keeps its accumulators in an open-addressing hash table in LDS, keyed by the column's 32-bit
offset from the row's smallest column (all ones = empty); the occupied slots are compacted, sorted in the wave and written once.
The order of summation is the window route's, so index, values and count are compared BIT FOR BIT (raw value bits) with
method="esc" and with oracle.spspmm, for f32, f16 and bf16, on the smallest shapes at which each mechanism can go wrong: rows the
window route refuses, lane seams and stored order, summation order and signed zeros across a span of more than 4096 columns, key
patterns that cluster under modulo and multiplicative hashes, the row limit R (read from gnnops.spgemm_hash_max_row()) from both
sides, repeats in a wide row of B, the largest 32-bit key, stale slots across rows and sweeps, the seams of the table classes,
calls without output, and the use cases at small size.

Two of the issue's cases are restated, because rows of B that repeat a column are out of this route's scope: the existing "wide
row of B" operands reference a row of B that stores column 5 twice, so "rowhash" must refuse them ("repeat"); the same operands
with that repeat removed run. The "span W + 1" operands hold the same row unreferenced and run as they are.
"""
import numpy as np
import pytest
import torch

from helpers import TORCH_DT, assert_bits_equal, to_np

pytestmark = pytest.mark.gpu

DNAMES = ["f32", "f16", "bf16"]
ROWS_PER_WG, SWEEP = 4, 4 * 2048        # csrc/spgemm.hip: waves per workgroup; rows one sweep of the capped grid covers (= scan tile)
SMALL_ROW, MEDIUM_ROW = 256, 1024       # csrc/spgemm.hip: HASH_SLOTS_S / 2, HASH_SLOTS_M / 2: largest row of the small / medium table class


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
def R(gnnops):
    r = gnnops.spgemm_hash_max_row()
    assert r >= 2048
    return r


def _rand(g, shape, dname):
    return (torch.rand(shape, generator=g) * 2 - 1).to(TORCH_DT[dname])


def _raw(t):
    """Bit image of a value tensor: tells -0.0 from +0.0."""
    return t.cpu().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _run(gnnops, method, iA, vA, iB, vB, m, k, n):
    return gnnops.spspmm(iA.cuda(), vA.cuda(), iB.cuda(), vB.cuda(), m, k, n, method=method)


def check(gnnops, oracle, iA, vA, iB, vB, m, k, n, dname, what, use_oracle=True, methods=("rowhash", "auto")):
    """rowhash (and auto) == esc on raw bits, and == oracle.spspmm; returns (index, values) of the rowhash run."""
    ei, ev = _run(gnnops, "esc", iA, vA, iB, vB, m, k, n)
    first = None
    for method in methods:
        gi, gv = _run(gnnops, method, iA, vA, iB, vB, m, k, n)
        first = first or (gi, gv)
        assert gi.dtype == torch.int64 and gv.dtype == vA.dtype
        assert tuple(gi.shape) == tuple(ei.shape) and tuple(gv.shape) == tuple(ev.shape), f"{what} {method}: {tuple(gi.shape)} vs {tuple(ei.shape)}"
        assert torch.equal(gi.cpu(), ei.cpu()), f"{what} {method}: index differs from esc"
        assert torch.equal(_raw(gv), _raw(ev)), f"{what} {method}: value bits differ from esc"
    if use_oracle:
        gi, gv = first
        oi, ov = oracle.spspmm(iA.numpy(), to_np(vA), iB.numpy(), to_np(vB), m, k, n, dtype=dname)
        assert tuple(gi.shape) == oi.shape, f"{what}: count {gi.shape[1]} vs oracle {oi.shape[1]}"
        assert_bits_equal(to_np(gi), oi, f"{what}: index")
        assert_bits_equal(to_np(gv), ov, f"{what}: values")
    return first


def check_refused(gnnops, iA, vA, iB, vB, m, k, n, why, what):
    """rowhash raises NotImplementedError naming `why`; auto equals esc."""
    with pytest.raises(NotImplementedError, match=why):
        _run(gnnops, "rowhash", iA, vA, iB, vB, m, k, n)
    ei, ev = _run(gnnops, "esc", iA, vA, iB, vB, m, k, n)
    gi, gv = _run(gnnops, "auto", iA, vA, iB, vB, m, k, n)
    assert torch.equal(gi.cpu(), ei.cpu()) and torch.equal(_raw(gv), _raw(ev)), f"{what}: auto differs from esc"


def rows_of_lengths(g, lengths, n, lo=0):
    """COO of a matrix whose row r holds lengths[r] DISTINCT columns of [lo, n), in shuffled stored order (rows interleaved)."""
    rows = torch.cat([torch.full((ln,), r, dtype=torch.int64) for r, ln in enumerate(lengths)])
    cols = torch.cat([torch.randperm(n - lo, generator=g)[:ln] + lo for ln in lengths])
    p = torch.randperm(rows.numel(), generator=g)
    return torch.stack([rows[p], cols[p]])


def coo_of_rows(g, rows_cols):
    """COO from a list of per-row column tensors, stored order shuffled."""
    rows = torch.cat([torch.full((c.numel(),), r, dtype=torch.int64) for r, c in enumerate(rows_cols)])
    cols = torch.cat([c.to(torch.int64) for c in rows_cols])
    p = torch.randperm(rows.numel(), generator=g)
    return torch.stack([rows[p], cols[p]])


def assert_unsorted(idx, width):
    key = (idx[0] * width + idx[1]).numpy()
    assert (np.diff(key) < 0).any(), "stored order must differ from sorted order"


# ---- 1. what the window route refuses ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
def test_wide_and_tiny(gnnops, oracle, dname):
    """The "span W + 1" operands of test_spgemm_gpu.py run hashed ("rowwise" still raises); its "wide row of B" operands reference
    a row of B that stores column 5 twice: refused for the repeat; with column 6 in place of the second 5 they run."""
    g = torch.Generator().manual_seed(13)
    W = gnnops.spgemm_max_span()
    k, m, n = 4, 3, W + 50

    def operands(last_col, reference_wide, second5=5):
        # rows of B: 0 = {10, 12}, 1 = {11, last_col}, 2 = empty, 3 = wide on its own, holding column 5 twice
        iB = torch.tensor([[1, 0, 3, 0, 1, 3, 3], [last_col, 12, 5, 10, 11, W + 40, second5]], dtype=torch.int64)
        iA = torch.tensor([[0, 2, 0, 2, 1], [1, 0, 0, 2, 3 if reference_wide else 2]], dtype=torch.int64)
        return iA, _rand(g, (iA.size(1),), dname), iB, _rand(g, (iB.size(1),), dname)

    ops = operands(10 + W, False)
    with pytest.raises(NotImplementedError, match="wide"):
        _run(gnnops, "rowwise", *ops, m, k, n)
    check(gnnops, oracle, *ops, m, k, n, dname, "span W + 1")
    ops = operands(10 + W - 1, True)
    with pytest.raises(NotImplementedError, match="wide"):
        _run(gnnops, "rowwise", *ops, m, k, n)
    check_refused(gnnops, *ops, m, k, n, "repeat", "wide row of B, column 5 twice")
    ops = operands(10 + W - 1, True, second5=6)
    with pytest.raises(NotImplementedError, match="wide"):
        _run(gnnops, "rowwise", *ops, m, k, n)
    check(gnnops, oracle, *ops, m, k, n, dname, "wide row of B")


# ---- 2. lane seams and stored order -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
def test_lane_seams_and_stored_order(gnnops, oracle, dname):
    """Rows of B of length 0, 1, 63, 64, 65, 129 with columns from [0, 10^6); rows of A of 0 to 70 nonzeros with repeated (i, kk)
    entries; everything shuffled."""
    g = torch.Generator().manual_seed(31)
    lengths = [0, 1, 63, 64, 65, 129, 0, 64]
    k, n, m = len(lengths), 10 ** 6, 9
    iB = rows_of_lengths(g, lengths, n)
    a_rows = torch.cat([torch.full((c,), r, dtype=torch.int64) for r, c in enumerate([0, 1, 3, 8, 70, 6, 0, 2, 5])])
    iA = torch.stack([a_rows, torch.randint(0, k, (a_rows.numel(),), generator=g)])
    iA = iA[:, torch.randperm(iA.size(1), generator=g)]
    assert np.unique((iA[0] * k + iA[1]).numpy()).size < iA.size(1), "A repeats (i, kk)"
    assert_unsorted(iA, k)
    assert_unsorted(iB, n)
    assert sorted(set(np.bincount(iB[0].numpy(), minlength=k))) == [0, 1, 63, 64, 65, 129]
    check(gnnops, oracle, iA, _rand(g, (iA.size(1),), dname), iB, _rand(g, (iB.size(1),), dname), m, k, n, dname, "lane seams")


# ---- 3. order of summation, zeros -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
def test_order_of_summation(gnnops, oracle, dname):
    """test_spgemm_gpu.py's construction with the fed column moved to 5003: C[0, 5003] is fed by 40 nonzeros of A's row 0 with
    magnitudes over 2^-12 .. 2^12, in a row that spans more than 4096 columns; only A's stored order reproduces the bits."""
    g = torch.Generator().manual_seed(15)
    k, n, m, fed = 10, 6000, 2, 5003
    kk = torch.arange(k).repeat(4)[torch.randperm(40, generator=g)]
    iA = torch.stack([torch.zeros(40, dtype=torch.int64), kk])
    iA = torch.cat([iA, torch.tensor([[1], [4]])], dim=1)
    expo = torch.randint(-12, 13, (41,), generator=g).float()
    vA = ((torch.rand(41, generator=g) + 1) * torch.exp2(expo) * (torch.randint(0, 2, (41,), generator=g) * 2 - 1)).to(TORCH_DT[dname])
    iB = torch.cat([torch.stack([torch.arange(k), torch.full((k,), fed)]), rows_of_lengths(g, [2] * k, 3)], dim=1)
    iB = iB[:, torch.randperm(iB.size(1), generator=g)]
    vB = (torch.rand(iB.size(1), generator=g) + 0.5).to(TORCH_DT[dname])
    if dname == "f32":   # the case is sharp: summing the same products in sorted order gives other bits
        bfed = {int(r): float(vB[j]) for j, (r, c) in enumerate(iB.t().tolist()) if c == fed}
        prods = np.array([np.float32(vA[t]) * np.float32(bfed[int(kk[t])]) for t in range(40)], dtype=np.float32)
        stored = np.float32(0)
        for p in prods:
            stored = np.float32(stored + p)
        other = np.float32(0)
        for p in np.sort(prods):
            other = np.float32(other + p)
        assert stored != other
    with pytest.raises(NotImplementedError, match="wide"):
        _run(gnnops, "rowwise", iA, vA, iB, vB, m, k, n)
    check(gnnops, oracle, iA, vA, iB, vB, m, k, n, dname, "summation order")


@pytest.mark.parametrize("dname", DNAMES)
def test_zeros(gnnops, oracle, dname):
    """A lone -0.0 product comes out as +0.0 (the accumulator starts at +0.0); a sum that cancels exactly stays as a stored zero;
    the rows span more than 4096 columns."""
    dt = TORCH_DT[dname]
    far, n = 5002, 6000
    iA = torch.tensor([[0, 1, 1, 2, 0], [0, 1, 2, 1, 1]], dtype=torch.int64)
    vA = torch.tensor([-1.0, 3.0, -1.5, 2.0, 1.0], dtype=dt)
    iB = torch.tensor([[0, 1, 2, 1], [4, far, far, 6]], dtype=torch.int64)
    vB = torch.tensor([0.0, 0.5, 1.0, 0.25], dtype=dt)
    gi, gv = check(gnnops, oracle, iA, vA, iB, vB, 3, 3, n, dname, "zeros")
    assert gi.cpu().tolist() == [[0, 0, 0, 1, 1, 2, 2], [4, 6, far, 6, far, 6, far]]
    vals = dict(zip(map(tuple, gi.cpu().t().tolist()), _raw(gv).tolist()))
    assert vals[(0, 4)] == 0, "-1 * 0 = -0.0 must come out as +0.0"
    assert vals[(1, far)] == 0, "3 * 0.5 - 1.5 * 1 cancels to a stored +0.0"


# ---- 4. adversarial key patterns ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
def test_adversarial_key_patterns(gnnops, oracle, dname):
    """One output row each of 1500 consecutive columns and of 1500 columns at stride 4096, 2^16 and 2^20 (n = 2^31): dense or
    clustered under modulo and under multiplicative hashing; and one row that mixes 375 of each through four rows of B."""
    g = torch.Generator().manual_seed(34)
    strides = [1, 4096, 1 << 16, 1 << 20]
    n = 1 << 31
    rows = [torch.arange(1500) * s + 3 for s in strides] + [torch.arange(375) * s + 3 for s in strides]
    assert int(rows[3].max()) < n
    iB = coo_of_rows(g, rows)
    a = [(r, r) for r in range(4)] + [(4, r) for r in (6, 4, 7, 5)]
    iA = torch.tensor(a, dtype=torch.int64).t().contiguous()
    gi, _ = check(gnnops, oracle, iA, _rand(g, (iA.size(1),), dname), iB, _rand(g, (iB.size(1),), dname), 5, 8, n, dname, "key patterns")
    assert gi.size(1) == 4 * 1500 + len(set(torch.cat(rows[4:]).tolist()))


# ---- 5. the row limit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
def test_row_limit(gnnops, oracle, dname, R):
    """Exactly R distinct columns in an output row run, from one row of B and from three overlapping rows; R + 1 is refused either
    way; a row of B of R + 5 entries is ignored while A does not reference it and refuses the call when it does."""
    g = torch.Generator().manual_seed(35)
    n = 10 ** 6
    cols = torch.randperm(n, generator=g)[:R + 5]
    third = R // 3
    rows = [cols[:R],                                                      # 0: R entries
            cols[:2 * third], cols[third:R - 5], cols[2 * third - 7:R],    # 1..3: overlapping, union = cols[:R]
            cols[R:R + 1],                                                 # 4: the column that makes R + 1
            cols[:R + 1],                                                  # 5: R + 1 entries
            cols[:R + 5]]                                                  # 6: R + 5 entries
    iB = coo_of_rows(g, rows)
    vB = _rand(g, (iB.size(1),), dname)
    k, m = len(rows), 4

    def A(*pairs):
        iA = torch.tensor(pairs, dtype=torch.int64).t().contiguous()
        return iA, _rand(g, (iA.size(1),), dname)

    # row 0: one row of B; row 1: three overlapping rows; row 3 : something small. Rows 5 and 6 of B are not referenced.
    gi, _ = check(gnnops, oracle, *A((0, 0), (1, 2), (1, 1), (3, 4), (1, 3), (1, 2)), iB, vB, m, k, n, dname, "R distinct columns")
    assert np.bincount(gi[0].cpu().numpy(), minlength=m).tolist() == [R, R, 0, 1]
    check_refused(gnnops, *A((0, 0), (0, 4)), iB, vB, m, k, n, "distinct columns", "R + 1 from two rows")
    check_refused(gnnops, *A((1, 1), (1, 3), (1, 4), (1, 2)), iB, vB, m, k, n, "distinct columns", "R + 1 from four rows")
    check_refused(gnnops, *A((2, 5)), iB, vB, m, k, n, "distinct columns", "a row of B of R + 1 entries")
    check_refused(gnnops, *A((0, 0), (2, 6)), iB, vB, m, k, n, "distinct columns", "a row of B of R + 5 entries, referenced once")


# ---- 6. a repeat in a wide row of B ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
def test_repeat_in_a_wide_row_of_B(gnnops, oracle, dname):
    """One column stored twice, 70 entries apart, in a row of B that spans 10^5 columns: refused. Without the repeat it runs."""
    g = torch.Generator().manual_seed(36)
    k, n, m = 5, 10 ** 5, 6
    iB = rows_of_lengths(g, [4, 100, 0, 64, 9], n)
    vB = _rand(g, (iB.size(1),), dname)
    iA = torch.stack([torch.randint(0, m, (30,), generator=g), torch.randint(0, k, (30,), generator=g)])
    iA[1, 0] = 1
    vA = _rand(g, (30,), dname)
    in_row1 = torch.nonzero(iB[0] == 1).view(-1)
    assert int(iB[1, in_row1].max() - iB[1, in_row1].min()) > 50000
    check(gnnops, oracle, iA, vA, iB, vB, m, k, n, dname, "repeat-free")
    first, late = int(in_row1[3]), int(in_row1[73])
    iB2 = iB.clone()
    iB2[1, late] = iB2[1, first]
    check_refused(gnnops, iA, vA, iB2, vB, m, k, n, "repeat", "repeat in row 1 of B")


# ---- 7. key range ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
def test_key_range(gnnops, oracle, dname):
    """An output row holding columns 5 and 5 + 2^32 - 2 (offset 2^32 - 2: the largest key when all ones is "empty") must run and
    must not be taken for an empty slot, alone and among 70 columns (the counting sort's four passes); a row holding 5 and
    5 + 2^32 + 7 either runs and equals esc and the oracle, or is refused as too wide with "auto" equal to esc."""
    g = torch.Generator().manual_seed(37)
    n, m, k = 1 << 33, 3, 3
    top = 5 + (1 << 32) - 2
    between = torch.randint(6, top, (70,), generator=g).unique()
    iB = coo_of_rows(g, [torch.tensor([5, top]), torch.cat([torch.tensor([top, 5]), between]), torch.tensor([5 + (1 << 32) + 7, 5])])
    vB = _rand(g, (iB.size(1),), dname)
    iA = torch.tensor([[0, 2, 2, 2], [0, 1, 0, 1]], dtype=torch.int64)
    gi, _ = check(gnnops, oracle, iA, _rand(g, (4,), dname), iB, vB, m, k, n, dname, "largest key")
    assert gi[1, 1] == top and gi[1, -1] == top and gi.size(1) == 2 + 2 + between.numel()
    iA = torch.tensor([[0, 1], [0, 2]], dtype=torch.int64)
    vA = _rand(g, (2,), dname)
    try:
        _run(gnnops, "rowhash", iA, vA, iB, vB, m, k, n)
    except NotImplementedError:
        check_refused(gnnops, iA, vA, iB, vB, m, k, n, "wide", "offset 2^32 + 7")
    else:
        check(gnnops, oracle, iA, vA, iB, vB, m, k, n, dname, "offset 2^32 + 7")


# ---- 8. table reuse across rows and sweeps -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
def test_more_rows_than_one_sweep(gnnops, oracle, dname):
    """m = 8192 + 9 output rows; empty rows at the workgroup seam (3, 4), the sweep seam (8191, 8192) and the end; a row of about
    1000 distinct columns (row 5) directly before rows of 2 on the same wave: the next row (6, next wave, same workgroup) and
    row 5 + 8192, which the same wave takes next and which a stale slot would spoil."""
    g = torch.Generator().manual_seed(38)
    m, k, n = SWEEP + 9, 42, 10 ** 6
    lengths = [int(x) for x in torch.randint(0, 7, (40,), generator=g)] + [1000, 2]
    lengths[0], lengths[1] = 3, 1
    iB = rows_of_lengths(g, lengths, n)
    rows = torch.arange(m)
    empty = torch.zeros(m, dtype=torch.bool)
    empty[[ROWS_PER_WG - 1, ROWS_PER_WG, SWEEP - 1, SWEEP, m - 1]] = True
    empty |= torch.rand(m, generator=g) < 0.2
    special = [5, 6, 5 + SWEEP]
    empty[special] = True            # filled below
    rows = rows[~empty]
    rows = torch.cat([rows, rows[torch.randint(0, rows.numel(), (3000,), generator=g)]])
    iA = torch.stack([rows, torch.randint(0, 40, (rows.numel(),), generator=g)])
    iA = torch.cat([iA, torch.tensor([[5, 5, 6, 5 + SWEEP], [40, 7, 41, 41]])], dim=1)
    iA = iA[:, torch.randperm(iA.size(1), generator=g)]
    assert iA.size(1) <= 20000
    gi, _ = check(gnnops, oracle, iA, _rand(g, (iA.size(1),), dname), iB, _rand(g, (iB.size(1),), dname), m, k, n, dname, "two sweeps")
    per_row = np.bincount(gi[0].cpu().numpy(), minlength=m)
    assert gi.size(1) > SWEEP and per_row[5] >= 1000 and per_row[6] == 2 and per_row[5 + SWEEP] == 2
    assert not per_row[[ROWS_PER_WG - 1, ROWS_PER_WG, SWEEP - 1, SWEEP, m - 1]].any()


# ---- 9. the table classes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
@pytest.mark.parametrize("largest", [SMALL_ROW, SMALL_ROW + 1, MEDIUM_ROW, MEDIUM_ROW + 1])
def test_table_classes(gnnops, oracle, dname, largest):
    """The call's largest output row holds exactly `largest` distinct columns: the last row count of a class, and the first of the
    next. The other rows are small."""
    g = torch.Generator().manual_seed(39)
    n = 10 ** 6
    cols = torch.randperm(n, generator=g)[:largest]
    half = largest // 2
    iB = coo_of_rows(g, [cols[:half + 9], cols[half - 20:], torch.tensor([17, 900000, 4]), cols[5:70]])
    iA = torch.tensor([[0, 1, 1, 3, 1, 3, 2], [2, 1, 0, 3, 1, 2, 0]], dtype=torch.int64)
    gi, _ = check(gnnops, oracle, iA, _rand(g, (7,), dname), iB, _rand(g, (iB.size(1),), dname), 4, 4, n, dname, f"largest row {largest}")
    assert np.bincount(gi[0].cpu().numpy(), minlength=4).max() == largest


@pytest.mark.parametrize("dname", DNAMES)
def test_no_output(gnnops, oracle, dname):
    """All-empty A; A whose every column meets an empty row of B; empty B: nnz(C) = 0 without a numeric launch."""
    g = torch.Generator().manual_seed(40)
    m, k, n = 6, 8, 10 ** 6
    iB = rows_of_lengths(g, [3, 0, 2, 0, 4, 0, 1, 0], n)
    vB = _rand(g, (iB.size(1),), dname)
    empty_i, empty_v = torch.zeros((2, 0), dtype=torch.int64), torch.zeros(0, dtype=TORCH_DT[dname])
    assert check(gnnops, oracle, empty_i, empty_v, iB, vB, m, k, n, dname, "empty A")[0].size(1) == 0
    iA = torch.stack([torch.randint(0, m, (20,), generator=g), torch.randint(0, 4, (20,), generator=g) * 2 + 1])
    assert check(gnnops, oracle, iA, _rand(g, (20,), dname), iB, vB, m, k, n, dname, "empty rows of B only")[0].size(1) == 0
    assert check(gnnops, oracle, iA, _rand(g, (20,), dname), empty_i, empty_v, m, k, n, dname, "empty B")[0].size(1) == 0


# ---- 10. the use cases, small --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dname", DNAMES)
def test_random_product_and_scattered_columns(gnnops, oracle, dname):
    """A random 600 x 600 product at density 0.02, and the same values with B's columns scattered over n = 10^6 by a random
    injective map: the same values, indices related by the map."""
    g = torch.Generator().manual_seed(41)
    L, n = 600, 10 ** 6
    ops = []
    for _ in range(2):
        idx = (torch.rand(L, L, generator=g) < 0.02).nonzero().t().contiguous()
        idx = idx[:, torch.randperm(idx.size(1), generator=g)]
        ops += [idx, _rand(g, (idx.size(1),), dname)]
    iA, vA, iB, vB = ops
    cmap = torch.randperm(n, generator=g)[:L]
    iB2 = torch.stack([iB[0], cmap[iB[1]]])
    gi, gv = check(gnnops, oracle, iA, vA, iB, vB, L, L, L, dname, "600 x 600", use_oracle=False)
    si, sv = check(gnnops, oracle, iA, vA, iB2, vB, L, L, n, dname, "600 x 10^6", use_oracle=False)
    gi, si = gi.cpu(), si.cpu()
    assert gi.shape == si.shape
    back = torch.full((n,), -1, dtype=torch.int64)
    back[cmap] = torch.arange(L)
    order = torch.argsort(si[0] * L + back[si[1]])          # row-major order of the narrow call
    assert torch.equal(torch.stack([si[0], back[si[1]]])[:, order], gi)
    assert torch.equal(_raw(sv)[order], _raw(gv))


@pytest.mark.parametrize("dname", DNAMES)
def test_squared_adjacency_of_one_graph(gnnops, oracle, dname):
    """(A + I)^2 of one random graph of 6000 nodes at in-degree 5: against "esc", and nnz(C) against the dense boolean product
    (weights are positive: no product cancels)."""
    g = torch.Generator().manual_seed(42)
    n, deg = 6000, 5
    key = torch.unique(torch.arange(n).repeat_interleave(deg) * n + torch.randint(0, n, (n * deg,), generator=g))   # distinct edges
    idx = torch.stack([key // n, key % n])
    idx = idx[:, idx[0] != idx[1]]
    loops = torch.arange(n)
    idx = torch.cat([idx, torch.stack([loops, loops])], dim=1)
    idx = idx[:, torch.randperm(idx.size(1), generator=g)]
    v = (torch.rand(idx.size(1), generator=g) + 0.5).to(TORCH_DT[dname])
    with pytest.raises(NotImplementedError, match="wide"):
        _run(gnnops, "rowwise", idx, v, idx, v, n, n, n)
    gi, _ = check(gnnops, oracle, idx, v, idx, v, n, n, n, dname, "(A+I)^2", use_oracle=False)
    dense = torch.zeros(n, n, device="cuda")
    dense[idx[0].cuda(), idx[1].cuda()] = 1.0
    assert gi.size(1) == int(((dense @ dense) != 0).sum())


@pytest.mark.parametrize("dname", DNAMES)
def test_graph_unet_same_bits(gnnops, dname, monkeypatch):
    """GraphUNet(8, 16, 1, depth=2) on one graph of 5000 nodes (distinct edges): with augment_adj's product forced to "esc" and to
    "rowhash", the outputs and every parameter gradient are equal bit for bit."""
    import gnnops.sparse as sparse
    from gnnops import conv

    g = torch.Generator().manual_seed(43)
    n, deg = 5000, 5
    key = torch.unique(torch.arange(n).repeat_interleave(deg) * n + torch.randint(0, n, (n * deg,), generator=g))
    ei = torch.stack([key % n, key // n])
    ei = ei[:, torch.randperm(ei.size(1), generator=g)].cuda()
    batch = torch.zeros(n, dtype=torch.int64).cuda()
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
    for method in ("esc", "rowhash"):
        monkeypatch.setattr(sparse, "spspmm", forced(method))
        for p in model.parameters():
            p.grad = None
        out = model(x, ei, batch, 1)
        (out * coef).sum().backward()
        results[method] = (out.detach().clone(), [p.grad.clone() for p in model.parameters()])
    monkeypatch.setattr(sparse, "spspmm", real)
    assert calls == ["esc", "esc", "rowhash", "rowhash"]
    assert torch.equal(_raw(results["esc"][0].float()), _raw(results["rowhash"][0].float()))
    for a, b in zip(results["esc"][1], results["rowhash"][1]):
        assert torch.equal(_raw(a.float()), _raw(b.float()))


# ---- 11. arguments ---------------------------------------------------------------------------------------------------------------------------
def test_arguments(gnnops, R):
    import torch_sparse

    assert torch_sparse.spspmm is gnnops.spspmm and R == gnnops.spgemm_hash_max_row() and R >= 2048
    i = torch.tensor([[0, 1], [1, 0]], dtype=torch.int64).cuda()
    v = torch.ones(2).cuda()
    with pytest.raises(RuntimeError, match="same dtype"):
        gnnops.spspmm(i, v, i, v.half(), 2, 2, 2, method="rowhash")
    gi, gv = torch_sparse.spspmm(i, v, i, v, 2, 2, 2, method="rowhash")
    assert gi.cpu().tolist() == [[0, 1], [0, 1]] and gv.cpu().tolist() == [1.0, 1.0]
