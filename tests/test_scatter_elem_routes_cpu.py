"""The case table of scatter_elem_cases.py against gnnops_scatter_elementwise_route, without a device: every case lands on
the route and geometry it names, every threshold of csrc/scatter_elem.hip has a named case on each side (the side is
re-derived here from the case's numbers), the seams sit at the numbers the code implies, a dozen queries are worked by
hand, the workspace size follows the header, gnnops/ops.py agrees with the library on where a column stops fitting an LDS
strip, and the inputs of every sum / mean / product case give the same bits in any order."""
import ctypes

import pytest

import scatter_elem_cases as sc
from scatter_elem_cases import ATOMICS, CHUNKS, LDS, NONE, SLOT

CASES = sc.all_cases()
BG = 163328                  # 160 KiB - 512: stated once; test_budget compares it with the library's and with ops.py's


@pytest.fixture(scope="module")
def lib():
    return sc.library()


def _q(lib, *args):
    d = (ctypes.c_int64 * 8)()
    return lib.gnnops_scatter_elementwise_route(*args, d), list(d)


def test_budget():
    from gnnops import ops

    assert sc.budget() == BG == ops._LDS_STRIP_BYTES


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_case_takes_its_route(c):
    d = sc.check_route(c)
    off = 1 << 40                                         # only the low four bits of an address matter
    assert sc.query(c, c.src_off * sc.EB[c.dt] + off, c.idx_off * c.ib + off) == sc.query(c)
    if c.route in (LDS, CHUNKS):
        tc, rows, nchunks, threads, cell, tshift, grid, flags = d
        assert 1 <= tc <= min(c.K, 64) and rows * tc * cell <= BG and (1 << tshift) >= tc and (tshift == 0 or (1 << (tshift - 1)) < tc)
        assert nchunks == -(-c.N // rows) and (nchunks == 1) == (c.route == LDS) and (rows == c.N or nchunks > 1)
        assert grid == c.B * -(-c.K // tc) * nchunks
        assert threads == (1024 if rows * tc * cell > sc.T80 else 512 if rows * tc * cell > sc.T40 else 256)
        assert flags == int(c.K == 1 and c.E % 4 == 0 and c.dt == "f32" and c.src_off == 0 and c.idx_off == 0)
    else:
        assert c.ib == 8 and c.ab == 8 and d[SLOT["grid"]] == min(-(-c.B * c.E * c.K // 256), 4096)


@pytest.mark.parametrize("c,status", sc.refusal_cases(), ids=[c.name for c, _ in sc.refusal_cases()])
def test_refusals_launch_nothing(c, status):
    assert sc.query(c) == (NONE, [0] * 8)
    if status == sc.EUNSUPPORTED:                         # the same shape with int64 ids and arg rows is taken, by the atomics
        assert sc.query(c._replace(ib=8, ab=8))[0] == ATOMICS


def _lds_bytes(c):
    d = sc.query(c)[1]
    return d[SLOT["rows"]] * d[SLOT["tc"]] * d[SLOT["cell"]]


def _cell(c):
    return sc.query(c)[1][SLOT["cell"]]


# label -> predicate on the case's own numbers: a case that claims the label must stand exactly there
SIDES = {
    "one.k2+": lambda c: c.K >= 2 and c.N * _cell(c) == BG // 2,
    "one.k2-": lambda c: c.K >= 2 and c.N * _cell(c) == BG // 2 + _cell(c),
    "one.k1+": lambda c: c.K == 1 and c.N * _cell(c) == BG,
    "one.k1-": lambda c: c.K == 1 and c.N * _cell(c) == BG + _cell(c),
    "c16+": lambda c: c.N == 16 * (BG // (_cell(c) * min(c.K, 4))),
    "c16-": lambda c: c.N == 16 * (BG // (_cell(c) * min(c.K, 4))) + 1,
    "cellw+": lambda c: c.E == 65534 and sc.EB[c.dt] == 2 and c.red in ("min", "max"),
    "cellw-": lambda c: c.E == 65535 and sc.EB[c.dt] == 2 and c.red in ("min", "max"),
    "t40-": lambda c: c.N * c.K * _cell(c) == 40960,
    "t40+": lambda c: 40960 < c.N * c.K * _cell(c) <= 40960 + c.K * _cell(c),
    "t80-": lambda c: c.N * c.K * _cell(c) == 81920,
    "t80+": lambda c: 81920 < c.N * c.K * _cell(c) <= 81920 + c.K * _cell(c),
    "narrow-": lambda c: c.B * -(-c.K // 8) == 192,
    "narrow+": lambda c: c.B * -(-c.K // 8) == 191,
    "vec4+": lambda c: c.K == 1 and c.dt == "f32" and c.E % 4 == 0 and c.src_off == 0 and c.idx_off == 0,
    "vec4-": lambda c: c.K == 1 and c.dt == "f32" and c.E % 4 == 1 and c.src_off == 0 and c.idx_off == 0,
}


def test_every_threshold_has_a_case_on_each_side():
    claimed = {}
    for c in CASES:
        for label in c.sides:
            assert SIDES[label](c), f"{c.name} claims {label}"
            claimed.setdefault(label, []).append(sc.query(c))
    assert set(claimed) == set(SIDES), sorted(set(SIDES) - set(claimed))
    for label in SIDES:                                   # a pair is a seam: route or geometry differs across it
        if label.endswith("+"):
            assert all(p != m for p in claimed[label] for m in claimed[label[:-1] + "-"]), label


def test_seams_sit_where_the_code_puts_them():
    N = {c.name: c.N for c in CASES}
    assert (N["one-k2-at-sum-f32"], N["one-k2-over-sum-f32"]) == (20416, 20417)           # N * 4 = 81664 | 81668
    assert (N["one-k2-at-max-f32"], N["one-k2-over-max-f32"]) == (10208, 10209)           # N * 8
    assert (N["one-k2-at-min-f16"], N["one-k2-at-mean-f32"]) == (20416, 10208)
    assert (N["one-k1-at-sum-f32"], N["one-k1-over-sum-f32"]) == (40832, 40833)           # N * 4 = 163328 | 163332
    assert (N["one-k1-at-max-f32"], N["one-k1-over-max-f32"]) == (20416, 20417)
    assert (N["c16-at-k4-sum-f32"], N["c16-over-k4-sum-f32"]) == (163328, 163329)         # rows 10208
    assert (N["c16-at-k4-min-f32"], N["c16-over-k4-min-f32"]) == (81664, 81665)           # rows 5104
    assert (N["c16-at-k3-sum-f16"], N["c16-ragged-k3-sum-f16"]) == (16 * 13610, 15 * 13610 + 7)
    assert (N["c16-at-k1-sum-f32"], N["c16-over-k1-sum-f32"]) == (653312, 653313)         # rows 40832
    assert [N[f"threads-{t}-{s}-k4-sum-f32"] for t in ("t40", "t80") for s in ("at", "over")] == [2560, 2561, 5120, 5121]
    assert [N[f"threads-{t}-{s}-k4-max-f32"] for t in ("t40", "t80") for s in ("at", "over")] == [1280, 1281, 2560, 2561]
    assert [N[f"threads-{t}-{s}-k1-sum-f32"] for t in ("t40", "t80") for s in ("at", "over")] == [10240, 10241, 20480, 20481]
    by = {c.name: c for c in CASES}
    assert sc.chunks_of(by["edges-sum-f32"]) == [(0, 40832), (40832, 40832), (81664, 1)]   # a last chunk of one destination
    assert sc.edge_destinations(by["edges-sum-f32"]) == [0, 40831, 40832, 81663, 81664]
    assert sc.empty_destinations(by["edges-sum-f32"]) == [1, 40833]
    assert {c.E for c in CASES if c.name.startswith("sweep-") and c.name.endswith("sum-f16-k1")} == {1, 2047, 2048, 2049}
    assert {c.E for c in CASES if c.name.startswith("vec4-E") and c.name.endswith("-sum")} == {4, 4092, 4096, 4100}
    assert sc.narrow_lengths() == (0, 1, 2, 4095, 4096, 4097, 8191, 8192, 8193)


def test_table_covers_every_form():
    seen = {}
    for c in CASES:
        r, d = sc.query(c)
        key = (r, c.red, c.dt)
        seen.setdefault(key, []).append((c, d))
        seen.setdefault(r, []).append((c, d))
    for dt in ("f32", "f16", "bf16"):
        for red in ("sum", "mean", "mul", "min", "max"):
            assert {c.K for c, _ in seen[(ATOMICS, red, dt)]} >= {1, 2}, (red, dt)
        assert any(c.init for c, _ in seen[(ATOMICS, "sum", dt)]) and any(c.init for c, _ in seen[(ATOMICS, "min", dt)])
        assert {(c.B * c.N * c.K) % 2 for c, _ in seen[(ATOMICS, "min", dt)]} | {(c.N * c.K) % 2 for c, _ in seen[(ATOMICS, "min", dt)]} == {0, 1}
    lds = seen[LDS] + seen[CHUNKS]
    assert {d[SLOT["tc"]] for _, d in lds} >= {1, 2, 3, 4, 8, 12, 64}
    assert {d[SLOT["threads"]] for _, d in lds} == {256, 512, 1024}
    assert {d[SLOT["nchunks"]] for _, d in seen[CHUNKS]} >= {2, 3, 16}
    for cellb in (4, 8):
        for ib in (8, 4, 2):
            for r in (LDS, CHUNKS):
                assert any(c.ib == ib and d[SLOT["cell"]] == cellb and c.dropped for c, d in seen[r]), (cellb, ib, r)
    assert {c.ab for c, _ in lds if c.red in ("min", "max")} == {4, 8}
    assert all(r in (LDS, CHUNKS) for c in CASES if c.dropped for r in [sc.query(c)[0]])      # ids outside [0, N): LDS routes only
    assert any(c.K == 1 and c.B == 3 and d[SLOT["flags"]] == 1 for c, d in lds)
    assert {c.N for c in CASES if c.ib == 2} >= {65535, 65536}
    assert any(c.B == 1 and c.K > 1 for c, _ in seen[ATOMICS]) and any(c.init and c.B == 1 and c.K > 1 for c, _ in seen[ATOMICS])
    assert any(c.init for c, _ in seen[CHUNKS])
    ragged = [c for c, d in lds if c.K % d[SLOT["tc"]]]
    assert any(c.K == 70 for c in ragged)


def test_hand_worked_queries(lib):
    f32, f16, bf16, SUM, MEAN, MIN, MAX, MUL = 0, 1, 2, 0, 1, 2, 3, 4
    # (6708, 6708) fp16 sum along dim 1: 6708 rows of K = 1; 6708 * 4 = 26832 bytes of LDS -> 256 threads, one per source row
    assert _q(lib, 6708, 6708, 1, 6708, f16, SUM, 8, 8, 0, 0) == (LDS, [1, 6708, 1, 256, 4, 0, 6708, 0])
    # the same along dim 0: B = 1, K = 6708; 163328 / 26832 = 6 columns -> 4; 1677 strips, 6708 * 4 * 4 = 107328 bytes -> 1024
    assert _q(lib, 1, 6708, 6708, 6708, f16, SUM, 8, 8, 0, 0) == (LDS, [4, 6708, 1, 1024, 4, 2, 1677, 0])
    # (1000, 1000) fp32 max along dim 0: 8-byte cells, 163328 / 8000 = 20 columns; 50 strips < 192 -> 8 (125 strips) -> 4 (250)
    assert _q(lib, 1, 1000, 1000, 1000, f32, MAX, 8, 8, 0, 0) == (LDS, [4, 1000, 1, 256, 8, 2, 250, 0])
    # (7, 60000) along dim 1 to 50001 destinations: fp32 sums 200004 bytes > budget -> two chunks of 163328 / 4 = 40832
    assert _q(lib, 7, 60000, 1, 50001, f32, SUM, 8, 8, 0, 0) == (CHUNKS, [1, 40832, 2, 1024, 4, 0, 14, 1])
    # its fp32 max: 8-byte cells, chunks of 20416 -> three; fp16 max: 60000 < 65535 positions pack into 4 bytes -> two
    assert _q(lib, 7, 60000, 1, 50001, f32, MAX, 8, 8, 0, 0) == (CHUNKS, [1, 20416, 3, 1024, 8, 0, 21, 1])
    assert _q(lib, 7, 60000, 1, 50001, f16, MAX, 8, 8, 0, 0) == (CHUNKS, [1, 40832, 2, 1024, 4, 0, 14, 0])
    # (50000, 6) along dim 0 to 45001 destinations: 180004 bytes; strips of 4 columns, rows = 163328 / 16 = 10208 -> 5 chunks x 2 strips
    assert _q(lib, 1, 50000, 6, 45001, f32, SUM, 8, 8, 0, 0) == (CHUNKS, [4, 10208, 5, 1024, 4, 2, 10, 0])
    # (700000, 2) to 690001 destinations: rows = 163328 / 8 = 20416, 34 chunks > 16 -> atomics, 1400000 / 256 = 5469 -> 4096 workgroups
    assert _q(lib, 1, 700000, 2, 690001, f32, SUM, 8, 8, 0, 0) == (ATOMICS, [0, 0, 0, 256, 4, 0, 4096, 0])
    # (38000, 38000) fp32 max transposed: 38000 rows, K = 1, 304000 bytes of 8-byte cells -> 2 chunks; int32 ids and arg rows
    assert _q(lib, 38000, 38000, 1, 38000, f32, MAX, 4, 4, 0, 0) == (CHUNKS, [1, 20416, 2, 1024, 8, 0, 76000, 1])
    # a mean keeps a count next to each sum: 8 bytes; 3000 destinations x 24 columns: 163328 / 24000 = 6 -> 4; 96 * 6 = 576 strips
    assert _q(lib, 96, 30, 24, 3000, bf16, MEAN, 8, 8, 0, 0) == (LDS, [4, 3000, 1, 1024, 8, 2, 576, 0])
    # products use 4-byte cells: 163328 / 12000 = 13 -> 12 columns, 16 lanes per row; 96 * 2 = 192 strips: not narrowed
    assert _q(lib, 96, 30, 24, 3000, f32, MUL, 8, 8, 0, 0) == (LDS, [12, 3000, 1, 1024, 4, 4, 192, 0])
    # E = 65535 no longer fits 16 bits next to the "out won" mark: 8-byte cells; an index 8 bytes off leaves the four-per-lane path
    assert _q(lib, 1, 65535, 1, 3000, f16, MIN, 8, 8, 0, 0)[1][4] == 8 and _q(lib, 1, 65534, 1, 3000, f16, MIN, 8, 8, 0, 0)[1][4] == 4
    assert _q(lib, 1, 64, 1, 3000, f32, MIN, 8, 8, 0, 8)[1][7] == 0 and _q(lib, 1, 64, 1, 3000, f32, MIN, 8, 8, 16, 32)[1][7] == 1
    # nothing to launch, or nothing the entry point accepts
    for args in ((0, 5, 1, 10, f32, SUM, 8, 8), (1, 5, 1, 0, f32, SUM, 8, 8), (1, 5, 1, 10, 3, SUM, 8, 8), (1, 5, 1, 10, f32, 5, 8, 8),
                 (1, 5, 1, 10, f32, SUM, 3, 8), (1, 5, 1, 65537, f32, SUM, 2, 8), (1, 5, 1, 10, f32, SUM, 8, 4), (-1, 5, 1, 10, f32, SUM, 8, 8)):
        assert _q(lib, *args, 0, 0) == (NONE, [0] * 8), args
    assert _q(lib, 1, 0, 1, 10, f32, SUM, 8, 8, 0, 0)[0] == LDS                     # E == 0 still initialises out
    assert lib.gnnops_scatter_elementwise_route(1, 5, 1, 10, f32, SUM, 8, 8, 0, 0, None) == LDS      # detail may be NULL


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_workspace_bytes(lib, c):
    up = lambda b: -(-b // 256) * 256
    nout = c.B * c.N * c.K
    want = (up(nout * 4) if (c.red in ("sum", "mean", "mul") and c.dt != "f32") else 0) + (up(nout * 4) if c.red == "mean" else 0)
    assert lib.gnnops_scatter_elementwise_workspace_bytes(c.B, c.N, c.K, sc.DT[c.dt], sc.RED[c.red]) == want


def test_python_agrees_with_the_library_on_the_transposed_route():
    """ops.scatter sends a dim-0 call (B == 1, K > 1) through the transposes exactly where one column's destinations no
    longer fit an LDS strip: where the query stops answering "one chunk" for a single column of the same N."""
    from gnnops import ops

    for red in ("sum", "mean", "mul", "min", "max"):
        for dt in ("f32", "f16", "bf16"):
            for E in (300, 65534, 65535, 65536):
                for cellb in (4, 8):
                    for N in (BG // cellb - 1, BG // cellb, BG // cellb + 1, BG // cellb + 2):
                        one_strip = sc.route(1, E, 1, N, dt, red)[0] == LDS
                        assert ops._strip_overflows(N, red, sc.EB[dt], E) == (not one_strip), (red, dt, E, N)
    assert ops._strip_overflows(BG // 4 + 1, "add", 4, 300) and not ops._strip_overflows(BG // 4, "add", 4, 300)


SUMS = [c for c in CASES if c.red in ("sum", "mean", "mul")]


@pytest.mark.parametrize("c", SUMS, ids=[c.name for c in SUMS])
def test_inputs_are_exact_in_any_order(c):
    """float64 result == the oracle's sequential fp32 result, at most 60 contributions per destination, |log2| sums < 100."""
    most, logs = sc.exactness(c.name)
    assert most <= sc.MAX_CONTRIB and logs < 100


MINMAX = [c for c in CASES if c.red in ("min", "max")]


@pytest.mark.parametrize("c", MINMAX, ids=[c.name for c in MINMAX])
def test_inputs_of_min_max_cases(c):
    """What the min / max inputs promise: few distinct values, both zeros, NaNs and the identity; an empty destination per
    chunk with arg = E; positions 0 and E - 1 of column 0 each the only winner of a destination; in every case that starts
    from `out`, a destination where out ties with its best contribution and is kept (arg = E)."""
    import numpy as np

    inp = sc.inputs(c.name)
    v = sc.widen(inp.src, c.dt)
    ident = np.inf if c.red == "min" else -np.inf
    assert len(np.unique(v[~np.isnan(v)])) <= 8
    if v.size >= 400:
        assert np.isnan(v).any() and (v == ident).any(), c.name
        assert (v.view(np.uint32) == 0x80000000).any() and (v.view(np.uint32) == 0).any(), c.name     # atomic cases included
    out, arg = sc.expected(c.name)
    for n in sc.empty_destinations(c):
        assert (arg[:, n, :] == c.E).all(), c.name
    first, last = inp.index[0, 0, 0], inp.index[0, c.E - 1, 0]
    best = -8.0 if c.red == "min" else 8.0
    assert arg[0, first, 0] == 0 and sc.widen(out, c.dt)[0, first, 0] == best
    if last != first:
        assert arg[0, last, 0] == c.E - 1 and sc.widen(out, c.dt)[0, last, 0] == best
        col = v[0, :, 0]
        assert (col[inp.index[0, :, 0] == last] == best).sum() == 1 and (col[inp.index[0, :, 0] == first] == best).sum() == 1
    if c.init:
        t = sc.tie_position(inp.index)
        assert t is not None, c.name
        d = inp.index[0, t, 0]
        fed = v[0, inp.index[0, :, 0] == d, 0]
        fed = fed[~np.isnan(fed) & ~np.isinf(fed)]
        assert fed.size, c.name
        kept = sc.widen(inp.out_init, c.dt)[0, d, 0]
        assert kept == (fed.min() if c.red == "min" else fed.max()) and arg[0, d, 0] == c.E, c.name      # out wins the tie
        assert out.view(f"u{out.itemsize}")[0, d, 0] == inp.out_init.view(f"u{out.itemsize}")[0, d, 0]
