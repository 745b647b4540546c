"""The case tables of gather_cases.py against the route queries of csrc/gather.hip, without a device: every case lands
on the route and geometry it aims at, every route of every entry point occurs, every dispatch threshold has a case on
each side (the side a case claims is re-derived here from its numbers), and the geometry takes every value the
dispatch can produce."""
import ctypes

import pytest

import gather_cases as gc
from gather_cases import EB, ELEMS, K1, LDS, LONGROWS, ROWS


@pytest.fixture(scope="module")
def lib():
    import gnnops

    return gnnops.load_library()


def _q(lib, fn, *args):
    d = (ctypes.c_int * 4)()
    return getattr(lib, fn)(*args, d), list(d)


@pytest.mark.parametrize("c", gc.all_cases(), ids=[f"{c.op}-{c.name}" for c in gc.all_cases()])
def test_case_takes_its_route(lib, c):
    gc.check_route(lib, c)
    # only the low four bits of an address matter
    assert gc.query(lib, c, c.off + (1 << 40)) == gc.query(lib, c)


def test_case_names_are_unique():
    for cases in (gc.select_cases() + gc.select_wrap_cases() + gc.push_cases(), gc.gather_cases(), gc.sum_cases()):
        names = [c.name for c in cases]
        assert len(set(names)) == len(names)


def test_every_route_of_every_entry_point_occurs():
    seen = {op: {c.route for c in gc.all_cases() if c.op == op} for op in ("select", "gather", "sum")}
    assert seen["select"] == {ROWS, K1, LDS, LONGROWS, ELEMS}
    assert seen["gather"] == {LDS, ELEMS}
    assert seen["sum"] == {ROWS, LDS, LONGROWS, ELEMS}


def _rb(c):
    return c.K * EB[c.dt]


def _k1_others(c, skip):
    """The K1 condition with one clause left out."""
    nb = c.N * EB[c.dt]
    cl = {"K": c.K == 1, "B": c.B > 1, "N": c.N >= 512, "E": c.E >= 256, "bytes": nb <= 65536, "sel": c.E * 32 >= nb}
    not_rows = not (_rb(c) % 16 == 0 and c.off % 16 == 0)
    return not_rows and all(v for k, v in cl.items() if k != skip)


def _lds_bytes(c, tc):
    """LDS a strip of tc columns takes: N * tc * eb, what the 40 KiB / 80 KiB thread-count thresholds look at."""
    return c.N * tc * EB[c.dt]


def _near(x, threshold, tc=1):
    """Within one table row (tc elements) of the threshold."""
    return abs(x - threshold) <= tc * 4


# label -> (op, predicate): the numbers of a case that claims the label must put it exactly there
SIDES = {
    "rows.whole+": ("select", lambda c: c.B == 1 and _rb(c) in (16, 32, 64, 128, 256, 512, 1024)),
    "rows.whole-": ("select", lambda c: _rb(c) % 16 == 0 and not (c.B == 1 and _rb(c) in (16, 32, 64, 128, 256, 512, 1024))),
    "rows.base+": ("select", lambda c: c.off % 16 == 0 and _rb(c) % 16 == 0),
    "rows.base-": ("select", lambda c: c.off % 16 != 0 and _rb(c) % 16 == 0),
    "rows.mult16+": ("select", lambda c: _rb(c) % 16 == 0 and c.off % 16 == 0),
    "rows.mult16-": ("select", lambda c: _rb(c) % 16 != 0 and c.off % 16 == 0),
    "k1.N+": ("select", lambda c: c.N == 512 and _k1_others(c, "N")),
    "k1.N-": ("select", lambda c: c.N == 511 and _k1_others(c, "N")),
    "k1.E+": ("select", lambda c: c.E == 256 and _k1_others(c, "E")),
    "k1.E-": ("select", lambda c: c.E == 255 and _k1_others(c, "E")),
    "k1.B+": ("select", lambda c: c.B == 2 and _k1_others(c, "B")),
    "k1.B-": ("select", lambda c: c.B == 1 and _k1_others(c, "B")),
    "k1.bytes+": ("select", lambda c: c.N * EB[c.dt] == 65536 and _k1_others(c, "bytes")),
    "k1.bytes-": ("select", lambda c: c.N * EB[c.dt] == 65540 and _k1_others(c, "bytes")),
    "k1.sel+": ("select", lambda c: c.E * 32 == c.N * EB[c.dt] and _k1_others(c, "sel")),
    "k1.sel-": ("select", lambda c: (c.E + 1) * 32 == c.N * EB[c.dt] and _k1_others(c, "sel")),
    "lds.wide+": ("select", lambda c: _rb(c) == 8),
    "lds.wide-": ("select", lambda c: 8 < _rb(c) <= 12 and c.E * 32 >= c.N * EB[c.dt]),
    "lds.t40-": ("select", lambda c: _near(_lds_bytes(c, c.K), 40960) and _lds_bytes(c, c.K) <= 40960),
    "lds.t40+": ("select", lambda c: _near(_lds_bytes(c, c.K), 40960) and _lds_bytes(c, c.K) > 40960),
    "lds.t80-": ("select", lambda c: _near(_lds_bytes(c, c.K), 81920) and _lds_bytes(c, c.K) <= 81920),
    "lds.t80+": ("select", lambda c: _near(_lds_bytes(c, c.K), 81920) and _lds_bytes(c, c.K) > 81920),
    "lds.budget+": ("select", lambda c: c.N * EB[c.dt] == gc.GL_BUDGET and c.E * 32 >= c.N * EB[c.dt]),
    "lds.budget-": ("select", lambda c: c.N * EB[c.dt] == gc.GL_BUDGET + 4 and c.E * 32 >= c.N * EB[c.dt]),
    "lds.sel+": ("select", lambda c: c.E * 32 == c.N * EB[c.dt] and _rb(c) <= 8),
    "lds.sel-": ("select", lambda c: (c.E + 1) * 32 == c.N * EB[c.dt] and _rb(c) <= 8),
    "long.min+": ("select", lambda c: c.K == gc.LONGROW_MIN_UNITS),
    "long.min-": ("select", lambda c: c.K == gc.LONGROW_MIN_UNITS - 1),
    "g.narrow-": ("gather", lambda c: c.K >= 64 and c.B * -(-c.K // 64) == 256),
    "g.narrow+": ("gather", lambda c: c.K >= 64 and c.B * -(-c.K // 64) < 256 <= c.B * -(-c.K // 32)),
    "g.t40-": ("gather", lambda c: _near(_lds_bytes(c, 8), 40960, 8) and _lds_bytes(c, 8) <= 40960),
    "g.t40+": ("gather", lambda c: _near(_lds_bytes(c, 8), 40960, 8) and _lds_bytes(c, 8) > 40960),
    "g.t80-": ("gather", lambda c: _near(_lds_bytes(c, 8), 81920, 8) and _lds_bytes(c, 8) <= 81920),
    "g.t80+": ("gather", lambda c: _near(_lds_bytes(c, 8), 81920, 8) and _lds_bytes(c, 8) > 81920),
    "g.budget+": ("gather", lambda c: c.N * EB[c.dt] == gc.GL_BUDGET and c.E * 32 >= c.N * EB[c.dt]),
    "g.budget-": ("gather", lambda c: c.N * EB[c.dt] == gc.GL_BUDGET + 4 and c.E * 32 >= c.N * EB[c.dt]),
    "g.sel+": ("gather", lambda c: c.E * 32 == c.N * EB[c.dt]),
    "g.sel-": ("gather", lambda c: (c.E + 1) * 32 == c.N * EB[c.dt]),
    "g.thin+": ("gather", lambda c: _rb(c) >= 8 and gc.GL_BUDGET // (c.N * EB[c.dt]) * EB[c.dt] == 8),
    "g.thin-": ("gather", lambda c: _rb(c) >= 8 and gc.GL_BUDGET // (c.N * EB[c.dt]) * EB[c.dt] < 8 and c.E * 32 >= c.N * EB[c.dt]),
    "sum.whole+": ("sum", lambda c: c.B == 1 and _rb(c) in (16, 32, 64, 128, 256, 512, 1024) and c.off % 16 == 0),
    "sum.whole-": ("sum", lambda c: c.B == 1 and _rb(c) % 16 == 0 and _rb(c) < 1024 and _rb(c) not in (16, 32, 64, 128, 256, 512)),
    "sum.base-": ("sum", lambda c: _rb(c) % 16 == 0 and c.off % 16 != 0),
    "sum.vec-": ("sum", lambda c: _rb(c) % 16 != 0 and c.off % 16 == 0),
    "sum.sel+": ("sum", lambda c: c.K == 1 and c.E * 32 == c.N * EB[c.dt]),
    "sum.sel-": ("sum", lambda c: c.K == 1 and (c.E + 1) * 32 == c.N * EB[c.dt]),
    "sum.budget+": ("sum", lambda c: c.K == 1 and c.N * EB[c.dt] <= gc.GL_BUDGET),
    "sum.budget-": ("sum", lambda c: c.K == 1 and c.N * EB[c.dt] == gc.GL_BUDGET + 4 and c.E * 32 >= c.N * EB[c.dt]),
    "sum.long+": ("sum", lambda c: c.K == gc.LONGROW_MIN_UNITS + 1 and _rb(c) % 16 != 0),
    "sum.long-": ("sum", lambda c: c.K == gc.LONGROW_MIN_UNITS - 1 and _rb(c) % 16 != 0),
}


def test_every_threshold_has_a_case_on_each_side():
    claimed = {}
    for c in gc.all_cases():
        for label in c.sides:
            op, pred = SIDES[label]
            assert c.op == op and pred(c), f"{c.op} {c.name} claims {label}"
            claimed.setdefault(label, []).append(c.name)
    assert set(claimed) == set(SIDES), sorted(set(SIDES) - set(claimed))
    for label in SIDES:                                      # the labels come in pairs
        assert label[:-1] + ("-" if label.endswith("+") else "+") in SIDES or label in ("sum.base-", "sum.vec-"), label


def test_sides_change_the_route(lib):
    """A threshold's two sides differ in route or geometry: the pair is a seam, not two points on one side."""
    by_label = {}
    for c in gc.all_cases():
        for label in c.sides:
            by_label.setdefault(label, []).append(gc.query(lib, c))
    for label in SIDES:
        if not label.endswith("+") or label[:-1] + "-" not in SIDES:
            continue
        plus, minus = by_label[label], by_label[label[:-1] + "-"]
        assert all(p != m for p in plus for m in minus), label


def test_detail_takes_every_value(lib):
    got = {}
    for c in gc.all_cases():
        r, d = gc.query(lib, c)
        for slot in range(4):
            got.setdefault((c.op, r, slot), set()).add(d[slot])
    assert got[("select", ROWS, 0)] == {0, 1, 2, 6} and got[("select", ROWS, 1)] == {1, 2} and got[("select", ROWS, 2)] == {0, 1}
    assert gc.ROWS_GRID_CAP in got[("select", ROWS, 3)] and 1 in got[("select", ROWS, 3)]
    assert got[("select", K1, 0)] == {1, 2, 3, 4}
    assert got[("select", LDS, 0)] == {1, 2, 3, 4}                       # K*eb <= 8: at most four columns
    assert got[("select", LDS, 1)] == {256, 512, 1024} == got[("gather", LDS, 1)]
    assert got[("select", LONGROWS, 0)] == {1, 2, 4, 8} == got[("select", ELEMS, 0)]
    assert got[("select", LONGROWS, 1)] >= {512, 513, 1024, 1025} and 511 in got[("select", ELEMS, 1)]
    assert got[("gather", LDS, 0)] >= {1, 3, 4, 5, 6, 8, 16, 32, 64}
    assert got[("gather", LDS, 3)] == {0, 2, 3, 4, 5, 6}
    assert {s % 8 for s in got[("gather", LDS, 2)]} >= {0, 1, 2, 3, 5, 7}    # strips alone; B * strips: the GPU file
    assert got[("gather", ELEMS, 0)] == {1, 2, 4, 8}
    assert got[("sum", ROWS, 0)] == {0, 2, 3, 6} and got[("sum", ROWS, 1)] == {1, 2}
    assert got[("sum", ROWS, 2)] == {0, 2, 3}                             # guarded, simple, simple and whole
    assert got[("sum", LONGROWS, 0)] == {1, 2}
    for route in (LDS, LONGROWS, ELEMS):
        assert gc.FUSED_BLOCKS in got[("sum", route, 2)]
    # B * strips of the LDS launches: every residue class gl_xcd_contiguous treats differently
    for op in ("select", "gather"):
        totals = {c.B * gc.query(lib, c)[1][2] for c in gc.all_cases() if c.op == op and c.route == LDS}
        assert {t for t in totals if t < 8} and {t % 8 for t in totals if t >= 8} >= {0, 1, 7}, (op, sorted(totals))


def test_hand_worked_queries(lib):
    sel, gat, fus = "gnnops_index_select_route", "gnnops_gather_route", "gnnops_fused_select_sum_route"
    # 1000 fp32 per row, 500 rows, along the last dim: 16 rows of 4000 bytes fit 64 KiB, capped at 4 -> 125 workgroups
    assert _q(lib, sel, 500, 1000, 1, 1000, 4, 0, 0) == (K1, [4, 125, 0, 0])
    # config-2 rows of 64 fp32 = 256 bytes: 16 lanes per row, 16 rows per workgroup, 4 in flight each -> 64 rows per step
    assert _q(lib, sel, 1, 1000, 64, 6400, 4, 0, 0) == (ROWS, [4, 1, 1, 100])
    # an output 8 bytes off: no 16-byte stores; 32 eight-byte units are too few for a wave per row
    assert _q(lib, sel, 1, 1000, 64, 6400, 4, 0, 8) == (ELEMS, [8, 32, 1600, 0])
    # (14142, 14142) fp16 along dim 0: 28284-byte rows, 4 divides them and 8 does not -> 7071 four-byte units
    assert _q(lib, sel, 1, 14142, 14142, 14142, 2, 0, 0) == (LONGROWS, [4, 7071, 8192, 0])
    # the same along dim 1: rows of 28284 bytes fit 64 KiB twice
    assert _q(lib, sel, 14142, 14142, 1, 14142, 2, 0, 0) == (K1, [2, 7071, 0, 0])
    # gather over (1224, 1224) fp16 along dim 0: 64 columns would make 20 workgroups; narrowed to 8 -> 153 strips
    assert _q(lib, gat, 1, 1224, 1224, 1224, 2) == (LDS, [8, 256, 153, 3])
    assert _q(lib, gat, 1224, 1224, 1, 1224, 2) == (LDS, [1, 256, 1, 0])
    # fused sum over (2738, 2738) fp16: dim 0 has rows of 2738 = 2 * 1369 halves -> pairs; dim 1 parks a row per step
    assert _q(lib, fus, 1, 2738, 2738, 2738, 1, 0) == (LONGROWS, [2, 1369, 685, 0])
    assert _q(lib, fus, 2738, 2738, 1, 2738, 1, 0) == (LDS, [1, 1024, 2048, 0])
    assert _q(lib, fus, 1, 1000, 64, 4096, 0, 0) == (ROWS, [4, 1, 3, 64])
    # nothing to launch, or nothing the entry point accepts
    assert _q(lib, sel, 1, 10, 4, 0, 4, 0, 0)[0] == -1 and _q(lib, sel, 1, 10, 4, 5, 3, 0, 0)[0] == -1
    assert _q(lib, gat, 0, 10, 4, 5, 4)[0] == -1 and _q(lib, fus, 1, 10, 4, 5, 7, 0)[0] == -1
    assert lib.gnnops_index_select_route(1, 10, 4, 5, 4, 0, 0, None) == ROWS      # detail may be NULL
