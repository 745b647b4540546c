"""Case tables for csrc/gather.hip, shared by test_gather_routes_cpu.py (route queries only, no device) and
test_gather_routes_gpu.py (the kernels, bit for bit). The tables are built from the constants of gather.hip, restated
here once; every case names the route it aims at, the geometry the route query must report (`detail`) and the side of
the dispatch thresholds it stands on (`sides`), and both files refuse a case that lands elsewhere.

A case views its input as [B, N, K] around the indexed dimension (include/gnnops.h):
  layout "3d"  input [B, N, K], dim 1          "1d"  input [N], dim 0 (B = K = 1)
         "2d0" input [N, K], dim 0 (B = 1)     "2d1" input [B, N], dim 1 (K = 1)
`off` is the byte offset of the input inside a 16-byte aligned flat buffer, `idx_off` the offset of the index inside an
int64 buffer (1: 8- but not 16-byte aligned), `pmap` the value of GNNOPS_PULL_MAP, `plan` a push-form index pattern.
"""
from collections import namedtuple

ROWS, K1, LDS, LONGROWS, ELEMS = 0, 1, 2, 3, 4     # enum gnnops_route
ROUTE_NAME = {ROWS: "ROWS", K1: "K1", LDS: "LDS", LONGROWS: "LONGROWS", ELEMS: "ELEMS"}

# constants of csrc/gather.hip
RIF = 4                       # ROWS_IN_FLIGHT
ROWS_GRID_CAP = 256 * 64      # select_rows_kernel
FUSED_BLOCKS = 256 * 8
GL_BUDGET = 160 * 1024 - 512
SK1_THREADS, SK1_MAX_TB, SK1_UNR, SK1_LDS = 512, 4, 8, 64 * 1024
LONGROW_MIN_UNITS = 512
PUSH_PU = 8                   # positions per step of select_rows_push_kernel
T_HUB = 8192                  # csrc/hub.h

EB = {"u8": 1, "f16": 2, "bf16": 2, "f32": 4, "i64": 8, "f64": 8}
DTYPE_CODE = {"f32": 0, "f16": 1, "bf16": 2}     # enum gnnops_dtype

Case = namedtuple("Case", "op name dt B N K E layout off idx_off pmap plan route detail sides")


def case(op, name, dt, B, N, K, E, route, detail=None, layout="3d", off=0, idx_off=0, pmap=None, plan=None, sides=()):
    if layout == "1d":
        assert B == 1 and K == 1
    elif layout == "2d0":
        assert B == 1
    elif layout == "2d1":
        assert K == 1
    assert off % EB[dt] == 0
    return Case(op, name, dt, B, N, K, E, layout, off, idx_off, pmap, plan, route, dict(detail or {}), tuple(sides))


def step_items(gshift):
    """Items (output row pieces) one workgroup step of the row kernels covers."""
    return (256 >> gshift) * RIF


def _rows_dt(rowbytes):
    """(dtype, K) for a row of `rowbytes` bytes; the element width rotates through 1, 2, 4 and 8 bytes."""
    return {16: ("f32", 4), 48: ("f32", 12), 64: ("f16", 32), 1024: ("i64", 128), 1040: ("f16", 520), 2048: ("f32", 512)}[rowbytes]


def _gshift(rowbytes):
    vecs, g = rowbytes // 16, 0
    while (1 << g) < vecs and g < 6:
        g += 1
    return g, -(-vecs // (1 << g))


# ------------------------------------------------------------------------------------------------ index_select
def select_cases():
    C = []
    # ROWS, whole: B = 1, one chunk, every lane of a group on the row
    for rb in (16, 64, 1024):
        dt, K = _rows_dt(rb)
        g, ch = _gshift(rb)
        S = step_items(g)
        for E in (1, S - 1, S, S + 1, 3 * S + 1):
            for pmap in (None, "g"):
                C.append(case("select", f"rows-whole-rb{rb}-E{E}-map{pmap or 'b'}", dt, 1, 37, K, E, ROWS,
                              {0: g, 1: 1, 2: 1, 3: -(-E // S)}, pmap=pmap, sides=("rows.whole+",)))
    C.append(case("select", "rows-whole-u8", "u8", 1, 37, 16, 70, ROWS, {0: 0, 2: 1}, sides=("rows.whole+",)))
    # ROWS, guarded
    for rb, B, why in ((48, 1, "idle-lane"), (1040, 1, "chunk2-one-lane"), (2048, 1, "two-chunks"), (64, 3, "batch")):
        dt, K = _rows_dt(rb) if B == 1 else ("u8", 64)
        g, ch = _gshift(rb)
        S = step_items(g)
        for E in (1, 5, S + 1):
            for pmap in (None, "g"):
                C.append(case("select", f"rows-guard-{why}-E{E}-map{pmap or 'b'}", dt, B, 29, K, E, ROWS,
                              {0: g, 1: ch, 2: 0, 3: -(-B * ch * E // S)}, pmap=pmap, sides=("rows.whole-",)))
    # ROWS, base 16-byte aligned or not, rows a multiple of 16 bytes or not
    C.append(case("select", "rows-align-base8", "f32", 1, 29, 8, 40, ELEMS, {0: 8, 1: 4}, off=8, sides=("rows.base-",)))
    C.append(case("select", "rows-align-base0", "f32", 1, 29, 8, 40, ROWS, {0: 1, 2: 1}, sides=("rows.base+", "rows.mult16+")))
    C.append(case("select", "rows-rowbytes-24", "f32", 1, 29, 6, 40, ELEMS, {0: 8, 1: 3}, sides=("rows.mult16-",)))

    # K1: K == 1 && B > 1 && N >= 512 && E >= 256 && N*eb <= 65536 && E*32 >= N*eb
    def k1(name, dt, B, N, E, route=K1, detail=None, sides=(), idx_off=0):
        if route == K1 and detail is None:
            tb = min(max(SK1_LDS // (N * EB[dt]), 1), SK1_MAX_TB, B)
            detail = {0: tb, 1: -(-B // tb)}
        C.append(case("select", "k1-" + name, dt, B, N, 1, E, route, detail, layout="2d1", idx_off=idx_off, sides=sides))

    k1("N511", "f16", 4, 511, 256, LDS, {0: 1}, sides=("k1.N-",))
    k1("N512", "f16", 4, 512, 256, sides=("k1.N+", "k1.E+"))
    k1("E255", "f16", 4, 512, 255, LDS, {0: 1}, sides=("k1.E-",))
    k1("bytes65536", "f32", 3, 16384, 2100, detail={0: 1, 1: 3}, sides=("k1.bytes+",))
    k1("bytes65540", "f32", 3, 16385, 2100, LDS, {0: 1}, sides=("k1.bytes-",))
    k1("E32-at", "f32", 3, 16384, 2048, detail={0: 1, 1: 3}, sides=("k1.sel+",))
    k1("E32-below", "f32", 3, 16384, 2047, ELEMS, {0: 4, 1: 1}, sides=("k1.sel-",))
    k1("B1", "f16", 1, 512, 256, LDS, {0: 1}, sides=("k1.B-",))
    for B, tb in ((2, 2), (4, 4), (5, 4), (9, 4)):     # tb clamped to B, exact fit, ragged last tiles of 1
        k1(f"tb-B{B}", "f16", B, 512, 300, detail={0: tb, 1: -(-B // tb)}, sides=(("k1.B+",) if B == 2 else ()))
    # staging: odd N with 2-byte elements (every other tile starts off 16 bytes: scalar copy; tb*N*2 = 4104 bytes: a vector
    # tail of 4 elements on the aligned tiles); nvec = tb*N*eb/16 below, at and above 4 * 512
    k1("stage-odd", "f16", 9, 513, 300, detail={0: 4, 1: 3})
    k1("stage-odd-bf16", "bf16", 5, 515, 301, detail={0: 4, 1: 2})
    for N in (2047, 2048, 2049):
        k1(f"stage-nvec{N}", "f32", 4, N, 300, detail={0: 4, 1: 1})
    # paired 16-bit stores: one sweep is SK1_THREADS * UNR pairs = 8192 outputs
    sweep = 2 * SK1_THREADS * SK1_UNR
    for E in (256, 258, sweep, sweep + 2):
        k1(f"pair-E{E}", "f16", 4, 512, E)
    k1("pair-E8194-bf16-ragged", "bf16", 5, 640, sweep + 2)
    for E in (257, sweep + 1):
        k1(f"unpaired-oddE{E}", "f16", 4, 512, E)
    k1("unpaired-index8", "f16", 4, 512, 256, idx_off=1)
    k1("unpaired-index8-E8194", "f16", 3, 512, sweep + 2, idx_off=1)
    for E in (4095, 4096, 4097):                        # unpaired loop: SK1_THREADS * UNR outputs per sweep
        k1(f"unpaired-f32-E{E}", "f32", 4, 512, E)
    k1("u8", "u8", 5, 1024, 300, detail={0: 4, 1: 2})
    k1("f32-tb3", "f32", 3, 4096, 600, detail={0: 3, 1: 1})
    k1("i64", "i64", 3, 512, 300, detail={0: 3, 1: 1})
    k1("i64-tb2", "i64", 5, 4096, 1100, detail={0: 2, 1: 3})

    # LDS: K*eb <= 8 and not K1
    def lds(name, dt, B, N, K, E, detail, layout="3d", route=LDS, sides=()):
        C.append(case("select", "lds-" + name, dt, B, N, K, E, route, detail, layout=layout, sides=sides))

    lds("1d", "f32", 1, 1000, 1, 500, {0: 1, 1: 256, 2: 1, 3: 0}, layout="1d")
    lds("K2-f32", "f32", 1, 300, 2, 100, {0: 2, 1: 256, 2: 1, 3: 1}, layout="2d0", sides=("lds.wide+",))
    lds("K2-f32-B3", "f32", 3, 300, 2, 100, {0: 2, 2: 1, 3: 1})
    lds("K4-f16", "f16", 3, 301, 4, 77, {0: 4, 2: 1, 3: 2})
    lds("K3-f16", "f16", 3, 301, 3, 77, {0: 3, 2: 1, 3: 2})              # tshift 2: column 3 idles
    lds("K1-u8", "u8", 3, 301, 1, 77, {0: 1, 2: 1, 3: 0})
    lds("K1-i64", "i64", 3, 301, 1, 77, {0: 1, 2: 1, 3: 0})
    lds("K3-f32-12bytes", "f32", 1, 300, 3, 100, {0: 4, 1: 3}, layout="2d0", route=ELEMS, sides=("lds.wide-",))
    for N, thr in ((10240, 256), (10241, 512), (20480, 512), (20481, 1024)):   # N*tc*eb against 40 KiB and 80 KiB
        lds(f"threads-N{N}", "f32", 1, N, 1, 2600, {0: 1, 1: thr}, layout="1d",
            sides=((f"lds.t40{'+' if N * 4 > 40960 else '-'}",) if N < 15000 else (f"lds.t80{'+' if N * 4 > 81920 else '-'}",)))
    lds("budget-at", "f32", 1, GL_BUDGET // 4, 1, 5200, {0: 1, 1: 1024}, layout="1d", sides=("lds.budget+",))
    lds("budget-over", "f32", 1, GL_BUDGET // 4 + 1, 1, 5200, {0: 4, 1: 1}, layout="1d", route=ELEMS, sides=("lds.budget-",))
    lds("E32-at", "f32", 1, 1000, 1, 125, {0: 1}, layout="1d", sides=("lds.sel+",))
    lds("E32-below", "f32", 1, 1000, 1, 124, {0: 4, 1: 1}, layout="1d", route=ELEMS, sides=("lds.sel-",))
    for B in (3, 9, 16):                                # K == 1, odd N: the strip base is 16-byte aligned for b % 8 == 0 only
        lds(f"K1-oddN-B{B}", "f16", B, 511, 1, 300, {0: 1, 2: 1}, layout="2d1")
    for B in (1, 7, 8, 9, 15, 17):                      # gl_xcd_contiguous: q = 0, r = 0, r = 1, r = 7
        lds(f"xcd-{B}", "f32", B, 300, 1, 100, {0: 1, 2: 1}, layout="2d1")
    lds("xcd-K2-B5", "f16", 5, 300, 2, 100, {0: 2, 2: 1})

    # LONGROWS / ELEMS: the copy unit is the widest of 8 / 4 / 2 / 1 that divides base addresses and row length
    for unit, dt in ((8, "i64"), (4, "f32"), (2, "f16"), (1, "u8")):
        for KU in (511, 512, 513, 1024, 1025):
            for B in (1, 3):
                odd = KU % 2 == 1
                off = 0 if odd else unit                # an even row length needs a base `unit` bytes off to keep the unit
                route = LONGROWS if KU >= LONGROW_MIN_UNITS else ELEMS
                C.append(case("select", f"long-u{unit}-KU{KU}-B{B}", dt, B, 7, KU, 9, route, {0: unit, 1: KU}, off=off,
                              sides=(("long.min+",) if KU == 512 else ("long.min-",) if KU == 511 else ())))
    for off, unit in ((0, 8), (2, 2), (4, 4), (8, 8), (6, 2)):   # 4104-byte fp16 rows fall to the unit the base allows
        C.append(case("select", f"long-4104-off{off}", "f16", 1, 7, 2052, 9, LONGROWS, {0: unit, 1: 4104 // unit}, off=off))
    C.append(case("select", "long-u8-off1-rows-1026", "u8", 3, 7, 1026, 9, LONGROWS, {0: 1, 1: 1026}, off=1))
    C.append(case("select", "elems-K7-f32", "f32", 3, 50, 7, 33, ELEMS, {0: 4, 1: 7}))
    C.append(case("select", "elems-K3-u8", "u8", 3, 1000, 3, 20, ELEMS, {0: 1, 1: 3}))
    C.append(case("select", "elems-K5-i64", "i64", 3, 50, 5, 33, ELEMS, {0: 8, 1: 5}))
    C.append(case("select", "elems-K9-f16", "f16", 2, 50, 9, 33, ELEMS, {0: 2, 1: 9}))
    return C


def select_wrap_cases():
    """The two large ones: the grid is capped at 16384 workgroups and the loop takes a second trip."""
    return [case("select", "rows-wrap-whole-rb1024", "f32", 1, 64, 256, 262144 + 17, ROWS, {0: 6, 1: 1, 2: 1, 3: ROWS_GRID_CAP}),
            case("select", "rows-wrap-guard-rb1040", "f16", 1, 64, 520, 131100, ROWS, {0: 6, 1: 2, 2: 0, 3: ROWS_GRID_CAP})]


def push_cases():
    """Planned push form. plan: "small" = empty segments at the front, in the middle and at the end, rows selected 7, 8
    and 9 times; ("hub", c) = one row selected c times next to ordinary rows."""
    C = []
    for rb in (16, 48, 1024, 1040):
        dt, K = _rows_dt(rb)
        for B in (1, 3):
            C.append(case("select", f"push-rb{rb}-B{B}", dt, B, 41, K, 0, ROWS, plan="small"))
    for rb in (16, 1040):
        dt, K = _rows_dt(rb)
        for count in (T_HUB, T_HUB + 1):
            C.append(case("select", f"push-hub{count}-rb{rb}", dt, 1, 41, K, 0, ROWS, plan=("hub", count)))
    return C


# ------------------------------------------------------------------------------------------------------ gather
def gather_cases():
    C = []

    def g(name, dt, B, N, K, E, detail, layout="3d", route=LDS, sides=()):
        C.append(case("gather", name, dt, B, N, K, E, route, detail, layout=layout, sides=sides))

    # dimension and index length
    g("dim0-E<N", "f32", 1, 300, 24, 100, {0: 8, 2: 3, 3: 3}, layout="2d0")
    g("dim0-E>N", "f16", 1, 100, 24, 300, {0: 8, 2: 3, 3: 3}, layout="2d0")
    g("last-E<N", "f32", 7, 300, 1, 100, {0: 1, 2: 1, 3: 0}, layout="2d1")
    g("last-E>N", "u8", 9, 100, 1, 300, {0: 1, 2: 1, 3: 0}, layout="2d1")
    g("mid-E<N", "i64", 3, 50, 5, 20, {0: 5, 2: 1, 3: 3})
    g("mid-E>N", "bf16", 3, 20, 6, 50, {0: 6, 2: 1, 3: 3})
    # strip width: 64 needs 256 workgroups, else it is halved down to 8; the ragged last strip
    g("tc64", "f32", 256, 16, 64, 8, {0: 64, 1: 256, 2: 1, 3: 6}, sides=("g.narrow-",))
    g("tc32", "f16", 128, 16, 64, 8, {0: 32, 2: 2, 3: 5}, sides=("g.narrow+",))
    g("tc16", "f16", 64, 16, 64, 8, {0: 16, 2: 4, 3: 4})
    g("tc8-narrowed", "f32", 1, 40, 64, 30, {0: 8, 2: 8, 3: 3}, layout="2d0")
    g("tc8-narrowed-B3", "u8", 3, 40, 64, 30, {0: 8, 2: 8, 3: 3})
    g("tc64-K65", "f16", 256, 16, 65, 8, {0: 64, 2: 2, 3: 6})
    g("tc64-K70", "f32", 128, 16, 70, 8, {0: 64, 2: 2, 3: 6})
    g("tc8-K9", "f32", 1, 40, 9, 30, {0: 8, 2: 2, 3: 3}, layout="2d0")
    g("tc8-K12", "i64", 2, 40, 12, 30, {0: 8, 2: 2, 3: 3})
    g("tc1-K1", "f16", 3, 301, 1, 77, {0: 1, 2: 1, 3: 0}, layout="2d1")
    # B * strips mod 8 in {0, 1, 7}, and below 8
    g("strips8", "f16", 1, 40, 64, 30, {0: 8, 2: 8}, layout="2d0")
    g("strips9", "f16", 1, 40, 72, 30, {0: 8, 2: 9}, layout="2d0")
    g("strips15", "f16", 1, 40, 120, 30, {0: 8, 2: 15}, layout="2d0")
    g("strips15-B3x5", "f32", 3, 40, 40, 30, {0: 8, 2: 5})
    g("strips3", "f16", 1, 40, 24, 30, {0: 8, 2: 3}, layout="2d0")
    # workgroup size by N*tc*eb against 40 KiB and 80 KiB
    for N, thr in ((1280, 256), (1281, 512), (2560, 512), (2561, 1024)):
        g(f"threads-N{N}", "f32", 1, N, 16, 330, {0: 8, 1: thr, 2: 2}, layout="2d0",
          sides=((f"g.t40{'+' if N * 32 > 40960 else '-'}",) if N < 2000 else (f"g.t80{'+' if N * 32 > 81920 else '-'}",)))
    # element route
    g("budget-at", "f32", 2, GL_BUDGET // 4, 1, 5200, {0: 1, 1: 1024, 2: 1}, layout="2d1", sides=("g.budget+",))
    g("elems-budget", "f32", 2, GL_BUDGET // 4 + 1, 1, 5200, {0: 4, 1: 1}, layout="2d1", route=ELEMS, sides=("g.budget-",))
    g("sel-at", "f32", 2, 1000, 3, 125, {0: 3}, sides=("g.sel+",))
    g("elems-sel", "f32", 2, 1000, 3, 124, {0: 4, 1: 3}, route=ELEMS, sides=("g.sel-",))
    g("elems-u8", "u8", 2, 1000, 3, 20, {0: 1, 1: 3}, route=ELEMS)
    g("elems-f16", "f16", 2, 1000, 3, 20, {0: 2, 1: 3}, route=ELEMS)
    g("elems-i64", "i64", 2, 1000, 3, 20, {0: 8, 1: 3}, route=ELEMS)
    # a strip under 8 bytes of a row of 8 bytes or more is refused
    g("elems-thin-strip-u8", "u8", 1, 30000, 64, 1000, {0: 1, 1: 64}, layout="2d0", route=ELEMS, sides=("g.thin-",))   # tc 5
    g("elems-thin-strip-f16", "f16", 1, 30000, 64, 2000, {0: 2, 1: 64}, layout="2d0", route=ELEMS, sides=("g.thin-",))  # tc 2
    g("thin-strip-8-bytes", "f16", 1, 20000, 64, 1300, {0: 4, 1: 1024, 2: 16, 3: 2}, layout="2d0", sides=("g.thin+",))
    return C


# ------------------------------------------------------------------------------------------- index_select_sum
def sum_cases():
    C = []

    def s(name, dt, B, N, K, E, route, detail, layout="3d", off=0, sides=()):
        assert 3 * B * E * K < 2 ** 24, name          # |v| <= 3: the fp32 sum is exact in any order
        C.append(case("sum", name, dt, B, N, K, E, route, detail, layout=layout, off=off, sides=sides))

    # whole: E around ngroups * RIF, the items one pass of the grid covers, with the grid the query reports for a probe
    # length of a few workgroups (3000 rows); one row more is one workgroup more
    lib = _library()
    for K in (8, 64, 512):
        r, d = query(lib, case("sum", "probe", "f16", 1, 23, K, 3000, ROWS, layout="2d0"))
        assert r == ROWS and d[2] == 3, (K, r, d)
        gshift, grid = d[0], d[3]
        full = ((grid * 256) >> gshift) * RIF
        s(f"rows-whole-K{K}-E1", "f16", 1, 23, K, 1, ROWS, {0: gshift, 1: 1, 2: 3, 3: 1}, layout="2d0", sides=("sum.whole+",))
        for tag, E, want in (("below", full - 1, grid), ("at", full, grid), ("above", full + 1, grid + 1)):
            s(f"rows-whole-K{K}-pass-{tag}", "f16", 1, 23, K, E, ROWS, {0: gshift, 1: 1, 2: 3, 3: want}, layout="2d0",
              sides=("sum.whole+",))
    s("rows-whole-bf16", "bf16", 1, 23, 64, 500, ROWS, {0: 3, 1: 1, 2: 3}, layout="2d0")
    s("rows-whole-f32", "f32", 1, 23, 32, 500, ROWS, {0: 3, 1: 1, 2: 3}, layout="2d0")
    for E in (1, 5, 257, 769):
        s(f"rows-simple-K24-E{E}", "f16", 1, 23, 24, E, ROWS, {0: 2, 1: 1, 2: 2}, layout="2d0", sides=("sum.whole-",))
        s(f"rows-chunked-K520-E{E}", "f16", 1, 23, 520, E, ROWS, {0: 6, 1: 2, 2: 0}, layout="2d0")
        s(f"rows-batched-K64-E{E}", "f16", 3, 23, 64, E, ROWS, {0: 3, 1: 1, 2: 0})
    s("rows-f32-K12", "f32", 1, 23, 12, 300, ROWS, {0: 2, 1: 1, 2: 2}, layout="2d0")
    s("rows-off8-f16-K64", "f16", 1, 23, 64, 300, ELEMS, {0: 1, 1: 64}, layout="2d0", off=8, sides=("sum.base-",))
    s("rows-K60-f16", "f16", 1, 23, 60, 300, ELEMS, {0: 1, 1: 60}, layout="2d0", sides=("sum.vec-",))
    s("lds-at", "f32", 5, 1000, 1, 125, LDS, {0: 1, 1: 1024, 2: 5}, layout="2d1", sides=("sum.sel+", "sum.budget+"))
    s("lds-below", "f32", 5, 1000, 1, 124, ELEMS, {0: 1, 1: 1}, layout="2d1", sides=("sum.sel-",))
    s("lds-f16-oddN", "f16", 9, 1237, 1, 400, LDS, {0: 1, 1: 1024, 2: 9}, layout="2d1")
    s("lds-1d-bf16", "bf16", 1, 3000, 1, 2000, LDS, {0: 1, 2: 1}, layout="1d")
    s("lds-budget-over", "f32", 1, GL_BUDGET // 4 + 1, 1, 5200, ELEMS, {0: 1, 1: 1}, layout="1d", sides=("sum.budget-",))
    s("long-pair2-K514", "f16", 1, 9, 514, 13, LONGROWS, {0: 2, 1: 257}, layout="2d0")
    s("long-pair2-K1026", "f16", 3, 9, 1026, 13, LONGROWS, {0: 2, 1: 513})
    s("long-pair2-K1026-bf16", "bf16", 1, 9, 1026, 13, LONGROWS, {0: 2, 1: 513}, layout="2d0")
    s("long-pair1-K513", "f16", 1, 9, 513, 13, LONGROWS, {0: 1, 1: 513}, layout="2d0")
    s("long-pair1-K514-off2", "f16", 1, 9, 514, 13, LONGROWS, {0: 1, 1: 514}, layout="2d0", off=2)
    s("long-pair1-f32-K513", "f32", 3, 9, 513, 13, LONGROWS, {0: 1, 1: 513}, sides=("sum.long+",))
    s("long-K511", "f32", 3, 9, 511, 13, ELEMS, {0: 1, 1: 511}, sides=("sum.long-",))
    s("elems-K7", "f32", 3, 50, 7, 33, ELEMS, {0: 1, 1: 7})
    s("elems-K7-f16", "f16", 3, 50, 7, 33, ELEMS, {0: 1, 1: 7})
    # 2048 partials: the element kernel and the long-row kernel wrap their grids; the LDS kernel takes one row per block
    s("grid2048-elems", "f32", 1, 50, 7, 300000, ELEMS, {0: 1, 1: 7, 2: FUSED_BLOCKS}, layout="2d0")
    s("grid2048-long", "f16", 1, 9, 514, 8200, LONGROWS, {0: 2, 2: FUSED_BLOCKS}, layout="2d0")
    s("grid2048-lds", "f16", 2049, 64, 1, 64, LDS, {0: 1, 2: FUSED_BLOCKS}, layout="2d1")
    s("grid600-rows", "f16", 1, 23, 8, 600 * 1024 + 3, ROWS, {0: 0, 1: 1, 2: 3, 3: 601}, layout="2d0")
    return C


def _library():
    import gnnops

    return gnnops.load_library()      # loads without a device; the route queries touch none


ALL_QUERY_CASES = None


def all_cases():
    """Every case a route query applies to (the push form has no dispatch)."""
    global ALL_QUERY_CASES
    if ALL_QUERY_CASES is None:
        ALL_QUERY_CASES = select_cases() + select_wrap_cases() + gather_cases() + sum_cases()
    return ALL_QUERY_CASES


def query(lib, c, input_addr=None):
    """(route, detail) the library reports for a case; input_addr defaults to the case's offset from an aligned base."""
    import ctypes

    d = (ctypes.c_int * 4)()
    addr = c.off if input_addr is None else input_addr
    if c.op == "select":
        r = lib.gnnops_index_select_route(c.B, c.N, c.K, c.E, EB[c.dt], addr, 0, d)
    elif c.op == "gather":
        r = lib.gnnops_gather_route(c.B, c.N, c.K, c.E, EB[c.dt], d)
    else:
        r = lib.gnnops_fused_select_sum_route(c.B, c.N, c.K, c.E, DTYPE_CODE[c.dt], addr, d)
    return r, list(d)


def check_route(lib, c, input_addr=None):
    """Assert that a case takes the route and geometry it aims at; returns the detail."""
    r, d = query(lib, c, input_addr)
    assert r == c.route, f"{c.op} {c.name}: route {ROUTE_NAME.get(r, r)}, aimed at {ROUTE_NAME[c.route]} (detail {d})"
    for slot, want in c.detail.items():
        assert d[slot] == want, f"{c.op} {c.name}: detail[{slot}] = {d[slot]}, expected {want} (detail {d})"
    return d
