"""GPU suite: coalesce, spspmm, sddmm and rowptr_expand at the seams of their blocks, rounds, waves and lane groups.

coalesce (csrc/sparse.hip) walks the sorted keys in blocks of 2048 positions, 8 rounds of 256, 4 waves of 64 lanes; the
per-block head counts are scanned 256 at a time with a carry (more than 256 * 2048 = 524288 entries). The sorted key
sequence is therefore CONSTRUCTED here (where every run starts is chosen), then shuffled. spspmm (csrc/spspmm.hip) hands a
block 256 nonzeros of A and scans its block sums the same way (more than 65536 nonzeros of A). Index, values (bit for bit)
and count are compared with oracle.coalesce / oracle.spspmm.

sddmm (csrc/backward.hip) is compared twice: bit for bit with a numpy float32 restatement of its summation order, and
with float64 inside  eps_out * |ref| + 4 * D * 2^-24 * sum|a||b|  (the form test_gemm_fused_gpu.py uses for an fp32
accumulation of that length). rowptr_expand is compared with numpy.searchsorted.
"""
import numpy as np
import pytest
import torch

from helpers import TORCH_DT, assert_bits_equal, f32_of, to_np

pytestmark = pytest.mark.gpu

SCAN_TILE, SCAN_ROUND, WAVE = 2048, 256, 64   # csrc/sparse.hip: positions per block / per round / per wave
SPSPMM_T = 256                                # csrc/spspmm.hip: nonzeros of A per block, block sums per scan round
KEY32 = (65536, 65536)                        # row bits + column bits = 32: the last shape with 32-bit keys
KEY64 = (65537, 65536)                        # 33 bits: 64-bit keys
DNAMES = ["f32", "f16", "bf16"]


def _dev(t):
    return t.cuda()


@pytest.fixture(scope="module")
def gnnops():
    import gnnops as g

    g.load_library()
    return g


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o

    return o


def _rand(g, shape, dname):
    return (torch.rand(shape, generator=g) * 2 - 1).to(TORCH_DT[dname])


# ---- coalesce ---------------------------------------------------------------------------------------------------------
RUNS_ENDING_AT_SEAMS = ((60, 64), (250, 256), (2040, 2048), (4096 + 60, 4096 + 64))
RUNS_OVER_SEAMS = ((62, 66), (254, 258), (2046, 2050), (2300, 2900), (4094, 4100), (4096 + 62, 4096 + 66))
HEADS_AT_SEAMS = (0, 63, 64, 255, 256, 2047, 2048, 4096 + 63, 4096 + 64)
PATTERNS = ["runs_end_at_seams", "runs_over_seams", "heads_only_at_seams", "one_run", "all_distinct"]


def seam_heads(pattern, nnz):
    """bool [nnz]: True where a new key starts in the SORTED sequence (position 0 always).
    runs_end_at_seams: all distinct but for duplicate runs [s, e) whose successor is the first lane of a wave (64), of a
    round (256), of a block (2048); runs_over_seams: runs that hold the last position before and the first after such a
    seam (one of them, [2300, 2900), over two round seams of the second block); heads_only_at_seams: long runs with heads
    at 63/64, 255/256, 2047/2048 and nowhere else."""
    if pattern in ("runs_end_at_seams", "runs_over_seams", "all_distinct"):
        h = np.ones(nnz, dtype=bool)
        runs = {"runs_end_at_seams": RUNS_ENDING_AT_SEAMS, "runs_over_seams": RUNS_OVER_SEAMS, "all_distinct": ()}[pattern]
        for s, e in runs:
            h[s + 1:e] = False
    else:
        h = np.zeros(nnz, dtype=bool)
        if pattern == "heads_only_at_seams":
            h[[p for p in HEADS_AT_SEAMS if p < nnz]] = True
    h[0] = True
    return h


def coo_from_heads(h, m, n, rng):
    """Shuffled int64 [2, nnz] whose sorted key sequence starts a new key exactly where h is set: ascending distinct keys
    spread over [0, m * n), the last one the largest key there is (top row and top column: every key bit in use)."""
    k, total = int(h.sum()), m * n
    ukey = np.cumsum(rng.integers(1, total // k + 1, size=k, dtype=np.int64)) - 1
    ukey[-1] = total - 1
    assert k == 1 or ukey[-2] < ukey[-1]
    key = ukey[np.cumsum(h) - 1]
    idx = np.stack([key // n, key % n])[:, rng.permutation(h.size)]
    return np.ascontiguousarray(idx), k


def check_coalesce(gnnops, oracle, idx, val, dname, m, n, k, what):
    ci, cv = gnnops.coalesce(_dev(torch.from_numpy(idx)), None if val is None else _dev(val), m, n)
    ei, ev = oracle.coalesce(idx, None if val is None else to_np(val), m, n, dtype=None if val is None else dname)
    assert ei.shape == (2, k), f"{what}: the oracle finds {ei.shape[1]} distinct keys, {k} were constructed"
    assert tuple(ci.shape) == (2, k), f"{what}: count {ci.shape[1]} != {k}"
    assert_bits_equal(to_np(ci), ei, f"{what}: index")
    if val is None:
        assert cv is None
        return
    assert tuple(cv.shape) == (k,) + tuple(val.shape[1:]) and cv.dtype == val.dtype, f"{what}: values {tuple(cv.shape)} {cv.dtype}"
    assert_bits_equal(to_np(cv), ev, f"{what}: values")


def whole_units(g, nnz):
    """fp32 whole numbers 1..8 (sums stay below 2^24: exact): a position summed twice or not at all is off by a unit."""
    return torch.randint(1, 9, (nnz,), generator=g).float()


@pytest.mark.parametrize("m,n", [KEY32, KEY64], ids=["key32", "key64"])
@pytest.mark.parametrize("nnz", [2047, 2048, 2049, 4096 + 65])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_coalesce_heads_at_the_seams(gnnops, oracle, pattern, nnz, m, n):
    """Head ranks of emit_heads_kernel = block offset + earlier rounds + earlier waves + lower lanes, with heads and runs
    placed at every one of those seams. Values: none, fp32 whole numbers [nnz] (carried through the sort as its payload)
    and bf16 [nnz, 3] (gathered through the permutation)."""
    rng = np.random.default_rng(nnz)
    g = torch.Generator().manual_seed(nnz)
    h = seam_heads(pattern, nnz)
    idx, k = coo_from_heads(h, m, n, rng)
    assert k == {"one_run": 1, "all_distinct": nnz}.get(pattern, k)
    check_coalesce(gnnops, oracle, idx, None, None, m, n, k, "no values")
    check_coalesce(gnnops, oracle, idx, whole_units(g, nnz), "f32", m, n, k, "fp32 whole numbers [nnz]")
    check_coalesce(gnnops, oracle, idx, _rand(g, (nnz, 3), "bf16"), "bf16", m, n, k, "bf16 [nnz, 3]")


@pytest.mark.parametrize("tail", [(), (1,), (3,), (8,), (2, 3)], ids=["nnz", "nnz_1", "nnz_3", "nnz_8", "nnz_2_3"])
@pytest.mark.parametrize("dname", DNAMES)
def test_coalesce_value_forms(gnnops, oracle, dname, tail):
    """Every value layout in every type, both key widths: scalar fp32 rides through the sort, everything else (fp32 with
    C > 1 included) is reduced through the permutation; the result keeps the trailing dimensions of the input."""
    nnz = 4096 + 65
    for m, n in (KEY32, KEY64):
        rng = np.random.default_rng(7)
        g = torch.Generator().manual_seed(7)
        idx, k = coo_from_heads(seam_heads("runs_over_seams", nnz), m, n, rng)
        check_coalesce(gnnops, oracle, idx, _rand(g, (nnz,) + tail, dname), dname, m, n, k, f"{dname} {(nnz,) + tail} {m}x{n}")
        idx, k = coo_from_heads(seam_heads("heads_only_at_seams", nnz), m, n, rng)      # runs of up to 2048 entries
        check_coalesce(gnnops, oracle, idx, _rand(g, (nnz,) + tail, dname), dname, m, n, k, f"{dname} long runs {m}x{n}")


@pytest.mark.parametrize("m,n,nnz,pattern", [(1, 1, 1, "one_run"), (1, 1, 2049, "one_run"), (3_000_000, 1, 1, "one_run"),
                                             (3_000_000, 1, 2048, "all_distinct"), (3_000_000, 1, 4096 + 65, "runs_over_seams"),
                                             (3_000_000, 1, 4096 + 65, "runs_end_at_seams")])
def test_coalesce_single_column(gnnops, oracle, m, n, nnz, pattern):
    """n == 1: the column field of the key carries no information (the key is the row), down to the 1 x 1 matrix."""
    rng = np.random.default_rng(nnz + m)
    g = torch.Generator().manual_seed(nnz)
    idx, k = coo_from_heads(seam_heads(pattern, nnz), m, n, rng)
    assert (idx[1] == 0).all()
    check_coalesce(gnnops, oracle, idx, None, None, m, n, k, "no values")
    check_coalesce(gnnops, oracle, idx, whole_units(g, nnz), "f32", m, n, k, "fp32 whole numbers [nnz]")
    check_coalesce(gnnops, oracle, idx, _rand(g, (nnz, 3), "f16"), "f16", m, n, k, "f16 [nnz, 3]")


def second_round_heads(nnz):
    """More than 256 blocks. Blocks below 256: 200000 distinct keys (large block offsets), then runs of 4099. One run lies
    over position 524288 (the first block of the second scan round), then 30000 distinct keys and runs of 3001 to the end."""
    first = SCAN_ROUND * SCAN_TILE
    h = np.zeros(nnz, dtype=bool)
    h[:200_000] = True
    h[200_000:520_000:4099] = True
    h[520_000:first - 3] = True
    h[first + 5:530_000:977] = True
    h[530_000:560_000] = True
    h[560_000::3001] = True
    return h


@pytest.mark.parametrize("m,n", [KEY32, KEY64], ids=["key32", "key64"])
def test_coalesce_second_scan_round(gnnops, oracle, m, n):
    """nnz > 256 * 2048: scan_sums_kernel takes a second round of 256 block sums, offset by the carry of the first."""
    nnz = 600_001
    h = second_round_heads(nnz)
    first = SCAN_ROUND * SCAN_TILE
    assert -(-nnz // SCAN_TILE) == 293 and not h[first - 3 + 1:first + 5].any()
    assert int(h[first:].sum()) > 30_000 and int(h[:first].sum()) > 200_000       # heads on both sides of the carry
    rng = np.random.default_rng(11)
    g = torch.Generator().manual_seed(11)
    idx, k = coo_from_heads(h, m, n, rng)
    check_coalesce(gnnops, oracle, idx, whole_units(g, nnz), "f32", m, n, k, "fp32 whole numbers [nnz]")
    check_coalesce(gnnops, oracle, idx, _rand(g, (nnz, 3), "f16"), "f16", m, n, k, "f16 [nnz, 3]")


# ---- spspmm -----------------------------------------------------------------------------------------------------------
def products_per_nonzero(iA, iB, k):
    """Products each nonzero of A expands to = length of the row of B its column names."""
    return np.bincount(iB[0].numpy(), minlength=k)[iA[1].numpy()]


def check_spspmm(gnnops, oracle, iA, vA, iB, vB, m, k, n, dname, what):
    gi, gv = gnnops.spspmm(_dev(iA), _dev(vA), _dev(iB), _dev(vB), m, k, n)
    ei, ev = oracle.spspmm(iA.numpy(), to_np(vA), iB.numpy(), to_np(vB), m, k, n, dtype=dname)
    assert tuple(gi.shape) == ei.shape and tuple(gv.shape) == ev.shape and gv.dtype == vA.dtype, f"{what}: {tuple(gi.shape)} vs {ei.shape}"
    assert_bits_equal(to_np(gi), ei, f"{what}: index")
    assert_bits_equal(to_np(gv), ev, f"{what}: values")
    return ei.shape[1]


def rows_of_B(g, rows, nnzB, n):
    """Unsorted COO entries of B whose rows are drawn (with repetition) from `rows`."""
    rows = torch.as_tensor(rows, dtype=torch.int64)
    return torch.stack([rows[torch.randint(0, rows.numel(), (nnzB,), generator=g)], torch.randint(0, n, (nnzB,), generator=g)])


@pytest.mark.parametrize("nnzA", [255, 256, 257])
@pytest.mark.parametrize("dname", DNAMES)
def test_spspmm_block_edge(gnnops, oracle, dname, nnzA):
    """One block less one, one full block, one block and one more nonzero; A and B unsorted with duplicate entries, a third
    of B's rows empty, about 940 products for 256 threads (threads take several)."""
    m, k, n = 25, 40, 30
    g = torch.Generator().manual_seed(nnzA)
    iA = torch.stack([torch.randint(0, m, (nnzA,), generator=g), torch.randint(0, k, (nnzA,), generator=g)])
    iB = rows_of_B(g, [r for r in range(k) if r % 3], 150, n)
    for idx, width in ((iA, k), (iB, n)):
        key = (idx[0] * width + idx[1]).numpy()
        assert np.unique(key).size < key.size and (np.diff(key) < 0).any(), "duplicates, unsorted"
    per = products_per_nonzero(iA, iB, k)
    assert per.sum() > 2 * SPSPMM_T and (per == 0).any()
    check_spspmm(gnnops, oracle, iA, _rand(g, (nnzA,), dname), iB, _rand(g, (150,), dname), m, k, n, dname, f"nnzA={nnzA}")


@pytest.mark.parametrize("dname", DNAMES)
def test_spspmm_empty_rows_of_B(gnnops, oracle, dname):
    """Nonzeros of A that expand to nothing share their start offset with the next one ("the last one owns q"): alternating
    with productive ones, as the last nonzero of a block, as a whole block, and in front of a block's only productive one."""
    m, k, n = 30, 64, 50
    g = torch.Generator().manual_seed(5)
    nnzA = 3 * SPSPMM_T + 17
    even = torch.randint(0, k // 2, (nnzA,), generator=g) * 2            # rows of B with entries
    odd = even + 1                                                         # empty rows of B
    a = torch.arange(nnzA)
    productive = (a < 256) & (a % 2 == 0)                                  # block 0: alternating, a = 255 expands to nothing
    productive |= a == 767                                                 # block 1: nothing; block 2: only its last nonzero
    productive |= (a >= 772) & (a < nnzA - 1)                              # tail block: 4 empty, 12 productive, 1 empty
    iA = torch.stack([torch.randint(0, m, (nnzA,), generator=g), torch.where(productive, even, odd)])
    iB = rows_of_B(g, range(0, k, 2), 200, n)
    iB[0, :k // 2] = torch.arange(0, k, 2)                                 # every even row has at least one entry
    per = products_per_nonzero(iA, iB, k)
    assert ((per > 0) == productive.numpy()).all()
    blocks = [per[b:b + SPSPMM_T] for b in range(0, nnzA, SPSPMM_T)]
    assert per[255] == 0 and blocks[1].sum() == 0 and blocks[2][:255].sum() == 0 and blocks[2][255] > 0 and blocks[3][-1] == 0
    check_spspmm(gnnops, oracle, iA, _rand(g, (nnzA,), dname), iB, _rand(g, (200,), dname), m, k, n, dname, "empty rows")


@pytest.mark.parametrize("dname", DNAMES)
def test_spspmm_long_row_of_B(gnnops, oracle, dname):
    """One row of B with 5000 entries, named by four nonzeros of A, two of them the last of block 0 and the first of block 1:
    every thread of those blocks takes some twenty products of one nonzero; the short rows around it share the search."""
    m, k, n = 40, 20, 300
    g = torch.Generator().manual_seed(9)
    nnzA = 300
    iA = torch.stack([torch.randint(0, m, (nnzA,), generator=g), torch.randint(0, k, (nnzA,), generator=g)])
    iA[1, iA[1] == 7] = 8
    iA[1, [10, 11, 255, 256]] = 7
    iB = torch.cat([rows_of_B(g, [7], 5000, n), rows_of_B(g, [r for r in range(k) if r not in (3, 7, 12)], 40, n)], dim=1)
    iB = iB[:, torch.randperm(iB.shape[1], generator=g)]
    per = products_per_nonzero(iA, iB, k)
    assert (per == 5000).sum() == 4 and per[255] == 5000 and per[256] == 5000 and (per == 0).any()
    check_spspmm(gnnops, oracle, iA, _rand(g, (nnzA,), dname), iB, _rand(g, (iB.shape[1],), dname), m, k, n, dname, "long row")


@pytest.mark.parametrize("dname", DNAMES)
def test_spspmm_no_products(gnnops, oracle, dname):
    """P == 0 with nnzA > 0: every column of A names an empty row of B; the result is the empty matrix."""
    m, k, n = 30, 64, 50
    g = torch.Generator().manual_seed(3)
    nnzA = 300
    iA = torch.stack([torch.randint(0, m, (nnzA,), generator=g), torch.randint(0, k // 2, (nnzA,), generator=g) * 2 + 1])
    iB = rows_of_B(g, range(0, k, 2), 200, n)
    assert products_per_nonzero(iA, iB, k).sum() == 0
    assert check_spspmm(gnnops, oracle, iA, _rand(g, (nnzA,), dname), iB, _rand(g, (200,), dname), m, k, n, dname, "P == 0") == 0


@pytest.mark.parametrize("dname", DNAMES)
def test_spspmm_second_scan_round(gnnops, oracle, dname):
    """nnzA > 256 * 256: the block sums are scanned in two rounds; the product offsets of blocks 256.. carry the first
    round's total. B's rows hold two entries on average (an eighth of them none)."""
    m, k, n = 2000, 40000, 2000
    nnzA, nnzB = 67_000, 80_000
    g = torch.Generator().manual_seed(13)
    iA = torch.stack([torch.randint(0, m, (nnzA,), generator=g), torch.randint(0, k, (nnzA,), generator=g)])
    iB = torch.stack([torch.randint(0, k, (nnzB,), generator=g), torch.randint(0, n, (nnzB,), generator=g)])
    per = products_per_nonzero(iA, iB, k)
    assert -(-nnzA // SPSPMM_T) == 262 and per[SPSPMM_T * SPSPMM_T:].sum() > 1000 and (per == 0).sum() > 1000
    check_spspmm(gnnops, oracle, iA, _rand(g, (nnzA,), dname), iB, _rand(g, (nnzB,), dname), m, k, n, dname, "two scan rounds")


# ---- sddmm ------------------------------------------------------------------------------------------------------------
VEC = {"f32": 4, "f16": 8, "bf16": 8}                      # elements per 16-byte piece
EPS_OUT = {"f32": 2.0 ** -24, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}
SDDMM_GRID_CAP = 8192                                      # blocks of 256 threads


def group_shift(D, dname):
    """Lanes per nonzero = 2^shift: the smallest power of two that gives every 16-byte piece of a row a lane, at most 64."""
    pieces, s = -(-D // VEC[dname]), 0
    while (1 << s) < pieces and s < 6:
        s += 1
    return s


def narrow(x32, dname):
    """float32 -> storage type, round to nearest even, as numpy array in the form to_np() gives."""
    if dname == "f32":
        return x32
    if dname == "f16":
        return x32.astype(np.float16)
    u = x32.view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def sddmm_restated(a32, b32, ra, rb, dname, aligned):
    """The kernel's order in numpy float32: lane l of the G lanes of a nonzero takes the pieces l, l + G, ... of the row (16
    bytes each; single elements when D is no multiple of a piece or an operand is not 16-byte aligned) and adds their
    products one by one from 0; then log2(G) levels v[l] = v[l] + v[l ^ o], o = G/2 .. 1; lane 0 rounds once. Columns past D
    are padded with +0 products, which change no sum. Returns (values, pieces per lane)."""
    D = a32.shape[1]
    vec = VEC[dname] if D % VEC[dname] == 0 and aligned else 1
    G = 1 << group_shift(D, dname)
    per_lane = -(-D // (G * vec))
    prod = np.zeros((ra.size, per_lane * G * vec), dtype=np.float32)
    prod[:, :D] = a32[ra] * b32[rb]
    steps = prod.reshape(ra.size, per_lane, G, vec).transpose(1, 3, 0, 2).reshape(per_lane * vec, ra.size, G)
    acc = np.zeros((ra.size, G), dtype=np.float32)
    for p in steps:
        acc = acc + p
    lane, o = np.arange(G), G >> 1
    while o:
        acc = acc + acc[:, lane ^ o]
        o >>= 1
    assert acc.dtype == np.float32
    return narrow(np.ascontiguousarray(acc[:, 0]), dname), per_lane


def check_sddmm(gnnops, a, b, ra, rb, dname, what, d_a=None, d_b=None):
    """(a) bit for bit against the restated order, (b) against float64 inside the stated bound. d_a / d_b: device operands
    prepared by the caller (views at an odd offset), else plain copies, which must be 16-byte aligned."""
    D = a.shape[1]
    d_a = _dev(a) if d_a is None else d_a
    d_b = _dev(b) if d_b is None else d_b
    aligned = d_a.data_ptr() % 16 == 0 and d_b.data_ptr() % 16 == 0
    got = gnnops.sddmm(_dev(ra), _dev(rb), d_a, d_b)
    assert tuple(got.shape) == (ra.numel(),) and got.dtype == a.dtype
    got = to_np(got)
    a32, b32 = f32_of(to_np(a), dname), f32_of(to_np(b), dname)
    exp, per_lane = sddmm_restated(a32, b32, ra.numpy(), rb.numpy(), dname, aligned)
    err_over_bound = 0.0
    for s in range(0, ra.numel(), 8192):                                   # float64 in slices: 40000 x 512 at the largest
        pa, pb = a32[ra.numpy()[s:s + 8192]].astype(np.float64), b32[rb.numpy()[s:s + 8192]].astype(np.float64)
        ref = (pa * pb).sum(1)
        bound = EPS_OUT[dname] * np.abs(ref) + 4 * D * 2.0 ** -24 * (np.abs(pa) * np.abs(pb)).sum(1)
        err = np.abs(f32_of(got[s:s + 8192], dname).astype(np.float64) - ref)
        assert (err <= bound).all(), f"{what}: |err| exceeds the bound by up to {(err - bound).max():.3e}"
        err_over_bound = max(err_over_bound, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"sddmm {what}: G={1 << group_shift(D, dname)} pieces/lane={per_lane} vector={aligned and D % VEC[dname] == 0} "
          f"max err/bound={err_over_bound:.3f}")
    assert_bits_equal(got, exp, f"{what}: restated order")
    return aligned, per_lane


def sddmm_rows(g, nnz, Ra, Rb):
    """Row ids with the first and last row, a row named many times and one (row, row) pair twice."""
    ra, rb = torch.randint(0, Ra, (nnz,), generator=g), torch.randint(0, Rb, (nnz,), generator=g)
    ra[:8] = torch.tensor([0, Ra - 1, Ra - 1, Ra - 1, 0, 0, 5, 5])
    rb[:8] = torch.tensor([0, Rb - 1, 0, Rb - 1, Rb - 1, 0, 6, 6])
    return ra, rb


def sddmm_lengths(dname):
    """Row lengths that take every lane-group width 1 .. 64 with whole pieces, a second piece per lane (64 pieces + 1), lengths
    that are no multiple of a piece (element route, one and several elements per lane) and the empty row."""
    V = VEC[dname]
    return [0, V, 2 * V, 3 * V, 8 * V, 9 * V, 17 * V, 33 * V, 64 * V + V, 7, 3 * V + 2, 64 * V + V + 3]


@pytest.mark.parametrize("dname", DNAMES)
def test_sddmm_every_group_width(gnnops, dname):
    g = torch.Generator().manual_seed(4)
    seen = set()
    for D in sddmm_lengths(dname):
        a, b = _rand(g, (90, D), dname), _rand(g, (70, D), dname)
        ra, rb = sddmm_rows(g, 700, 90, 70)
        aligned, per_lane = check_sddmm(gnnops, a, b, ra, rb, dname, f"{dname} D={D}")
        assert aligned
        seen.add((group_shift(D, dname), per_lane, D % VEC[dname] == 0))
    assert {(s, 1, True) for s in range(7)} <= seen and (6, 2, True) in seen     # whole pieces: every width; two pieces per lane
    assert any(not whole and s < 6 and n > 1 for s, n, whole in seen)              # elements, several per lane, narrow group
    assert any(not whole and s == 6 and n > 1 for s, n, whole in seen)             # elements, several per lane, all 64 lanes


@pytest.mark.parametrize("which", ["a", "b", "both"])
@pytest.mark.parametrize("dname", DNAMES)
def test_sddmm_operand_off_16_bytes(gnnops, dname, which):
    """Rows of whole pieces in an operand that starts one element into its buffer: the element route, not 16-byte loads."""
    g = torch.Generator().manual_seed(8)
    for D in (64, 33 * VEC[dname]):
        flat_a, flat_b = _rand(g, (1 + 90 * D,), dname), _rand(g, (1 + 70 * D,), dname)
        a, b = flat_a[1:].view(90, D), flat_b[1:].view(70, D)
        d_a = _dev(flat_a)[1:].view(90, D) if which in ("a", "both") else _dev(a.contiguous())
        d_b = _dev(flat_b)[1:].view(70, D) if which in ("b", "both") else _dev(b.contiguous())
        assert d_a.is_contiguous() and d_b.is_contiguous()
        ra, rb = sddmm_rows(g, 700, 90, 70)
        aligned, _ = check_sddmm(gnnops, a, b, ra, rb, dname, f"{dname} D={D} offset {which}", d_a, d_b)
        assert not aligned and D % VEC[dname] == 0


def test_sddmm_more_nonzeros_than_groups(gnnops):
    """40000 nonzeros at D = 512 fp32: 64 lanes per nonzero, 4 groups per block, 8192 blocks at the most, so 32768 groups,
    and the first 7232 of them take a second nonzero."""
    nnz, D = 40000, 512
    assert group_shift(D, "f32") == 6 and nnz > SDDMM_GRID_CAP * (256 >> 6)
    g = torch.Generator().manual_seed(12)
    a, b = _rand(g, (50, D), "f32"), _rand(g, (60, D), "f32")
    ra, rb = sddmm_rows(g, nnz, 50, 60)
    check_sddmm(gnnops, a, b, ra, rb, "f32", "grid stride")


# ---- rowptr_expand ----------------------------------------------------------------------------------------------------
def big_rowptr():
    """5000 segments over more positions than one sweep of the grid (4096 blocks of 256), a fifth of them empty, the first
    segment starting at 17 and the last ending 300 before E."""
    E = 4096 * 256 + 1000
    rng = np.random.default_rng(2)
    cuts = np.sort(rng.integers(17, E - 300, size=4997))
    cuts[1::5] = cuts[0::5][:cuts[1::5].size]                              # empty segments in the middle
    return np.concatenate([[17, 17], cuts, [E - 300, E - 300]]), E


ROWPTRS = {
    "empty_front_middle_end": ([3, 3, 7, 7, 7, 12, 12], 20),              # first > 0, last < E
    "one_segment": ([2, 5], 9),
    "one_empty_segment": ([4, 4], 6),
    "well_formed": ([0, 1, 1, 300], 300),
    "above_one_sweep": big_rowptr(),
}


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("case", list(ROWPTRS))
def test_rowptr_expand(gnnops, case, dtype):
    """index[e] = the segment that holds e: the last n with rowptr[n] <= e, so empty segments own nothing; N where
    e < rowptr[0] or e >= rowptr[N]."""
    rowptr, E = ROWPTRS[case]
    rowptr = np.asarray(rowptr, dtype=np.int64)
    N = rowptr.size - 1
    e = np.arange(E)
    exp = np.searchsorted(rowptr, e, side="right") - 1
    exp[(e < rowptr[0]) | (e >= rowptr[N])] = N
    assert (np.diff(rowptr) >= 0).all()
    if case == "above_one_sweep":
        assert E > 4096 * 256 and (np.diff(rowptr) == 0).sum() > 900 and rowptr[0] > 0 and rowptr[N] < E
    got = gnnops.expand_rowptr(_dev(torch.from_numpy(rowptr).to(dtype)), E)
    assert got.dtype == torch.int64
    assert_bits_equal(to_np(got), exp, case)
