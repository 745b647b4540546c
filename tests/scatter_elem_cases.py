"""Case table for csrc/scatter_elem.hip (layout-F scatter), shared by test_scatter_elem_routes_cpu.py (route queries and
the exactness of the inputs, no device) and test_scatter_elem_gpu.py (the kernels through the C entry points, bit for bit).

Nothing here copies a dispatch threshold of scatter_elem.hip: the LDS budget is read once from the route query
(`budget()`, 163328 bytes) and every seam is derived from it and from what the query reports (`rows`, `threads`, `tshift`).
The two thread-class bounds, 40 KiB and 80 KiB of LDS, are restated once (T40, T80). Each case names the route and the
geometry (`detail`, by name) it expects and the side of each threshold it stands on (`sides`); both test files refuse a
case that lands elsewhere.

A case is a direct call of gnnops_scatter_elementwise_ixa: src, index [B, E, K] -> out [B, N, K]. `ib` / `ab` are the
bytes per index / arg element, `init` is init_from_out, `src_off` / `idx_off` place the operand that many ELEMENTS off a
16-byte boundary, `dropped` puts ids outside [0, N) into the index (LDS routes only: the atomic kernels do not check ids,
`inputs()` asserts the route), `edges` asks that every chunk edge is fed from position 0 and from position E - 1.

Inputs make every comparison exact in any arrival order (checked by `exactness()` on the CPU): sums and means add whole
numbers in [-4, 4], at most 60 per destination (the fp32 accumulator is exact, |sum| <= 240 is a bf16 value; the mean is one
fp32 division and the storage rounding, as in the kernel); products multiply values of {1, -1, 2, 0.5}; min / max draw
from a few values (ties everywhere), both zeros, 2 % NaNs and the reduce's identity, with one empty destination per chunk.
"""
import ctypes
import functools
import zlib
from collections import namedtuple

import numpy as np

NONE, LDS, CHUNKS, ATOMICS = -1, 2, 5, 6            # enum gnnops_route
ROUTE_NAME = {NONE: "NONE", LDS: "LDS", CHUNKS: "LDS_CHUNKS", ATOMICS: "ATOMICS"}
SLOT = {"tc": 0, "rows": 1, "nchunks": 2, "threads": 3, "cell": 4, "tshift": 5, "grid": 6, "flags": 7}
DT = {"f32": 0, "f16": 1, "bf16": 2}                # enum gnnops_dtype
EB = {"f32": 4, "f16": 2, "bf16": 2}
RED = {"sum": 0, "mean": 1, "min": 2, "max": 3, "mul": 4}
OK, EINVAL, EUNSUPPORTED = 0, 1, 4
T40, T80 = 40 * 1024, 80 * 1024                     # LDS bytes above which a strip gets 512 / 1024 threads
MAX_CHUNKS = 16
MAX_CONTRIB = 60

Case = namedtuple("Case", "name B E K N dt red ib ab init route detail sides src_off idx_off dropped edges")


def library():
    import gnnops

    return gnnops.load_library()      # loads without a device; the route query touches none


def route(B, E, K, N, dt, red, ib=8, ab=8, src_addr=0, idx_addr=0):
    d = (ctypes.c_int64 * 8)()
    r = library().gnnops_scatter_elementwise_route(B, E, K, N, DT[dt], RED[red], ib, ab, src_addr, idx_addr, d)
    return r, list(d)


def query(c, src_addr=None, idx_addr=None):
    sa = c.src_off * EB[c.dt] if src_addr is None else src_addr
    ia = c.idx_off * c.ib if idx_addr is None else idx_addr
    return route(c.B, c.E, c.K, c.N, c.dt, c.red, c.ib, c.ab, sa, ia)


def check_route(c, src_addr=None, idx_addr=None):
    """Assert that a case takes the route and geometry it names; returns the detail."""
    r, d = query(c, src_addr, idx_addr)
    assert r == c.route, f"{c.name}: route {ROUTE_NAME.get(r, r)}, aimed at {ROUTE_NAME[c.route]} (detail {d})"
    for k, want in c.detail.items():
        assert d[SLOT[k]] == want, f"{c.name}: {k} = {d[SLOT[k]]}, expected {want} (detail {d})"
    return d


@functools.lru_cache(None)
def budget():
    """LDS_BUDGET of scatter_elem.hip, read from the query: a single fp32 sum column is cut into chunks of budget / 4
    destinations as soon as it does not fit, whatever N is."""
    r, d = route(1, 8, 1, 1 << 19, "f32", "sum")
    assert r == CHUNKS and d[SLOT["tc"]] == 1 and d[SLOT["cell"]] == 4
    return d[SLOT["rows"]] * 4


def cell(dt, red, E):
    """LDS bytes per destination and column, as the query reports them (any shape of that dtype / reduce / E)."""
    return route(1, E, 1, 64, dt, red)[1][SLOT["cell"]]


def rpi(B, K, N, dt, red, E=64):
    """Source rows one sweep of a workgroup covers: threads >> tshift, from the query."""
    r, d = route(B, E, K, N, dt, red)
    assert r in (LDS, CHUNKS)
    return d[SLOT["threads"]] >> d[SLOT["tshift"]]


def _cases():
    C = []

    def add(name, B, E, K, N, dt, red, route, detail=None, sides=(), ib=8, ab=8, init=0, src_off=0, idx_off=0,
            dropped=False, edges=False):
        assert not (red == "mean" and init), name
        assert ab == 8 or red in ("min", "max"), name
        C.append(Case(name, B, E, K, N, dt, red, ib, ab, init, route, dict(detail or {}), tuple(sides), src_off, idx_off,
                      dropped, edges))

    BG = budget()
    # one cell width per entry: (tag, dtype, reduce, E) — E < 65535 keeps 16-bit min / max in 4-byte cells
    widths = (("sum-f32", "f32", "sum", 600), ("max-f32", "f32", "max", 600), ("min-f16", "f16", "min", 600),
              ("mean-f32", "f32", "mean", 600), ("mul-bf16", "bf16", "mul", 600))

    # ---- one chunk or chunked: N * cell against budget / 2 (K >= 2: the narrowest strip is two columns) and budget (K == 1)
    for tag, dt, red, E in widths:
        cb = cell(dt, red, E)
        n2, n1 = BG // (2 * cb), BG // cb
        add(f"one-k2-at-{tag}", 1, E, 2, n2, dt, red, LDS, {"tc": 2, "rows": n2, "nchunks": 1, "cell": cb}, ("one.k2+",), dropped=True)
        add(f"one-k2-over-{tag}", 1, E, 2, n2 + 1, dt, red, CHUNKS, {"tc": 2, "rows": n2, "nchunks": 2, "cell": cb}, ("one.k2-",))
        add(f"one-k1-at-{tag}", 1, E, 1, n1, dt, red, LDS, {"tc": 1, "rows": n1, "nchunks": 1, "cell": cb}, ("one.k1+",))
        add(f"one-k1-over-{tag}", 1, E, 1, n1 + 1, dt, red, CHUNKS, {"tc": 1, "rows": n1, "nchunks": 2, "cell": cb}, ("one.k1-",),
            dropped=True)

    # ---- 16 chunks or atomics (the output is what is large here: a few MB; E stays small)
    for tag, dt, red, K in (("k4-sum-f32", "f32", "sum", 4), ("k4-min-f32", "f32", "min", 4), ("k3-sum-f16", "f16", "sum", 3),
                            ("k1-sum-f32", "f32", "sum", 1), ("k1-mul-bf16", "bf16", "mul", 1)):
        cb = cell(dt, red, 300)
        tc = min(K, 4)
        rows = BG // (cb * tc)
        top = MAX_CHUNKS * rows
        add(f"c16-at-{tag}", 1, 300, K, top, dt, red, CHUNKS, {"tc": tc, "rows": rows, "nchunks": 16, "cell": cb}, ("c16+",))
        add(f"c16-over-{tag}", 1, 300, K, top + 1, dt, red, ATOMICS, {"tc": 0, "nchunks": 0, "threads": 256}, ("c16-",))
        if K == 3:
            add(f"c16-ragged-{tag}", 2, 300, K, top - rows + 7, dt, red, CHUNKS, {"tc": 3, "rows": rows, "nchunks": 16, "tshift": 2},
                dropped=True)

    # ---- chunk edges: n_lo - 1, n_lo, n_lo + rows - 1 and N - 1 fed from position 0 and from position E - 1; a last chunk of one
    for tag, dt, red, B, K in (("sum-f32", "f32", "sum", 8, 1), ("min-f32", "f32", "min", 4, 2), ("max-f16", "f16", "max", 3, 3),
                               ("mean-f16", "f16", "mean", 2, 4), ("mul-f32", "f32", "mul", 8, 1), ("max-bf16", "bf16", "max", 8, 1)):
        cb = cell(dt, red, 500)
        rows = BG // (cb * min(K, 4))
        add(f"edges-{tag}", B, 500, K, 2 * rows + 1, dt, red, CHUNKS, {"rows": rows, "nchunks": 3}, edges=True, dropped=True)

    # ---- cell width: 16-bit min / max pack value image and position + 1 into 32 bits while E < 65535
    for E in (65534, 65535, 65536):
        for dt, red in (("f16", "min"), ("f16", "max"), ("bf16", "min"), ("bf16", "max")):
            cb = 4 if E == 65534 else 8
            side = {65534: "cellw+", 65535: "cellw-"}.get(E)
            add(f"cellw-E{E}-{red}-{dt}", 1, E, 1, 3000, dt, red, LDS, {"tc": 1, "cell": cb, "flags": 0}, (side,) if side else (),
                ab=4 if dt == "bf16" else 8)
        add(f"cellw-E{E}-min-f16-init", 1, E, 1, 3000, "f16", "min", LDS, {"cell": 4 if E == 65534 else 8}, init=1)
        add(f"cellw-E{E}-max-bf16-init", 1, E, 1, 3000, "bf16", "max", LDS, {"cell": 4 if E == 65534 else 8}, init=1, ib=4)

    # ---- thread classes: rows * tc * cell against 40 KiB and 80 KiB
    for tag, dt, red, B, K in (("k4-sum-f32", "f32", "sum", 2, 4), ("k4-max-f32", "f32", "max", 2, 4), ("k1-sum-f32", "f32", "sum", 3, 1),
                               ("k1-mean-f16", "f16", "mean", 3, 1)):
        cb = cell(dt, red, 300)
        for T, below, above, lab in ((T40, 256, 512, "t40"), (T80, 512, 1024, "t80")):
            n = T // (K * cb)
            add(f"threads-{lab}-at-{tag}", B, 300, K, n, dt, red, LDS, {"tc": K, "threads": below, "cell": cb}, (lab + "-",))
            add(f"threads-{lab}-over-{tag}", B, 300, K, n + 1, dt, red, LDS, {"tc": K, "threads": above, "cell": cb}, (lab + "+",))

    # ---- strip geometry
    for K, tsh in ((1, 0), (2, 1), (3, 2), (4, 2)):
        add(f"strip-tc{K}-sum-f16", 5, 200, K, 301, "f16", "sum", LDS, {"tc": K, "tshift": tsh, "grid": 5}, dropped=True)
        add(f"strip-tc{K}-max-f32", 5, 200, K, 301, "f32", "max", LDS, {"tc": K, "tshift": tsh, "grid": 5}, init=1)
    n12 = BG // (4 * 13)                                 # budget / (N * 4) = 13: twelve columns, sixteen lanes per row
    add("strip-tc12-sum-f32", 96, 30, 24, n12, "f32", "sum", LDS, {"tc": 12, "tshift": 4, "grid": 192})
    add("strip-tc12-min-f16", 96, 30, 24, n12, "f16", "min", LDS, {"tc": 12, "tshift": 4, "grid": 192})
    add("strip-tc64-ragged-sum-f32", 200, 40, 70, 9, "f32", "sum", LDS, {"tc": 64, "tshift": 6, "grid": 400})
    add("strip-tc64-ragged-max-f16", 200, 40, 70, 9, "f16", "max", LDS, {"tc": 64, "tshift": 6, "grid": 400}, init=1)
    add("strip-tc64-ragged-mean-bf16", 200, 40, 70, 9, "bf16", "mean", LDS, {"tc": 64, "tshift": 6, "grid": 400})
    # the narrowing loop halves tc while B * ceil(K / tc) < 192: not running, ending at 4, ending at 8
    add("narrow-192-stays-8", 192, 30, 8, 100, "f32", "sum", LDS, {"tc": 8, "grid": 192}, ("narrow-",))
    add("narrow-191-ends-at-4", 191, 30, 8, 100, "f32", "sum", LDS, {"tc": 4, "grid": 382}, ("narrow+",))
    add("narrow-ends-at-8", 24, 30, 64, 100, "f16", "mul", LDS, {"tc": 8, "grid": 192})
    add("narrow-64-to-4", 23, 30, 64, 100, "f32", "min", LDS, {"tc": 4, "grid": 368})
    add("narrow-B3-two-strips", 3, 200, 8, 100, "bf16", "sum", LDS, {"tc": 4, "grid": 6})

    # ---- sweeps: E around one unrolled sweep of the scalar loops (8 rows per lane) and of the four-per-lane loops (16 elements)
    for tag, dt, red, B, K, N in (("sum-f16-k1", "f16", "sum", 1, 1, 700), ("min-f16-k1", "f16", "min", 1, 1, 700),
                                  ("mean-f32-k2", "f32", "mean", 1, 2, 700), ("max-f32-k3", "f32", "max", 2, 3, 5000)):
        r8 = rpi(B, K, N, dt, red) * 8
        for E in (1, r8 - 1, r8, r8 + 1):
            add(f"sweep-E{E}-{tag}", B, E, K, N, dt, red, LDS, {"flags": 0})
    for tag, red in (("sum", "sum"), ("max", "max"), ("mul", "mul")):
        r16 = rpi(1, 1, 700, "f32", red) * 16
        for E in (4, r16 - 4, r16, r16 + 4):
            add(f"vec4-E{E}-{tag}", 1, E, 1, 700, "f32", red, LDS, {"flags": 1}, ("vec4+",) if E == r16 else ())
        for E in (r16 + 1, r16 + 2, r16 + 3):
            add(f"vec4-off-E{E}-{tag}", 1, E, 1, 700, "f32", red, LDS, {"flags": 0}, ("vec4-",) if E == r16 + 1 else ())
        add(f"vec4-off-src-{tag}", 1, r16, 1, 700, "f32", red, LDS, {"flags": 0}, src_off=1)
        add(f"vec4-off-index-{tag}", 1, r16, 1, 700, "f32", red, LDS, {"flags": 0}, idx_off=1)
        add(f"vec4-off-index4-{tag}", 1, r16, 1, 700, "f32", red, LDS, {"flags": 0}, idx_off=1, ib=4)
        add(f"vec4-B3-{tag}", 3, r16 + 4, 1, 700, "f32", red, LDS, {"flags": 1}, dropped=True)
        add(f"vec4-B3-index2-{tag}", 3, r16 + 4, 1, 700, "f32", red, LDS, {"flags": 1}, dropped=True, ib=2)

    # ---- index and arg widths: every LDS case class with 8-, 4- and 2-byte ids (narrowed by gnnops_narrow_index), dropped ids
    n1 = BG // 4
    classes = (("sumk-scalar", 3, 900, 3, 500, "f16", "sum", LDS), ("sumk-vec4", 2, 1200, 1, 500, "f32", "sum", LDS),
               ("sumk-mean", 3, 900, 2, 500, "bf16", "mean", LDS), ("mm-cell4", 3, 900, 3, 500, "f16", "min", LDS),
               ("mm-cell8", 3, 900, 3, 500, "f32", "max", LDS), ("mm-vec4", 2, 1200, 1, 500, "f32", "min", LDS),
               ("chunks-sum", 2, 900, 1, n1 + 5, "f32", "sum", CHUNKS), ("chunks-max", 2, 900, 2, n1 // 4 + 5, "f32", "max", CHUNKS))
    for tag, B, E, K, N, dt, red, rt in classes:
        if rt == CHUNKS and N > 65535:
            N2 = 65535                                   # two-byte ids: the largest N they can name and still drop an id
            assert route(B, E, K, N2, dt, red)[0] == CHUNKS
        else:
            N2 = N
        for ib in (8, 4, 2):
            for ab in ((8, 4) if red in ("min", "max") else (8,)):
                add(f"width-{tag}-i{ib}-a{ab}", B, E, K, N2 if ib == 2 else N, dt, red, rt, ib=ib, ab=ab, dropped=True,
                    init=1 if (ib == 4 and red != "mean") else 0)
    add("width-i2-N65535-sum-f16", 1, 2000, 1, 65535, "f16", "sum", CHUNKS, {"nchunks": 2}, ib=2, dropped=True)
    add("width-i2-N65536-sum-f16", 1, 2000, 1, 65536, "f16", "sum", CHUNKS, {"nchunks": 2}, ib=2)   # 0xFFFF is a valid id here
    add("width-i2-N65536-max-bf16", 1, 2000, 1, 65536, "bf16", "max", CHUNKS, {"nchunks": 2, "cell": 4}, ib=2, ab=4)

    # ---- memory-side atomics: every reduce at K = 1 and K = 2 for every dtype; N * K even and odd (the 16-bit CAS works
    # on the 32-bit word a destination shares with its neighbour: a batch's base offset B * N * K is then odd or even)
    na = MAX_CHUNKS * (BG // 4) + 88
    for dt in ("f32", "f16", "bf16"):
        for red in ("sum", "mean", "mul", "min", "max"):
            for K in (1, 2):
                N = na + (1 if (K == 1 and red in ("min", "mul")) else 0)
                add(f"atomics-{red}-{dt}-k{K}", 2, 1500, K, N, dt, red, ATOMICS, {"threads": 256, "grid": -(-2 * 1500 * K // 256)})
        add(f"atomics-sum-{dt}-init", 2, 1500, 1, na + 1, dt, "sum", ATOMICS, init=1)
        add(f"atomics-min-{dt}-init", 2, 1500, 1, na + 1, dt, "min", ATOMICS, init=1)
        add(f"atomics-max-{dt}-init-k2", 1, 1500, 2, na, dt, "max", ATOMICS, init=1)
    add("atomics-sum-f32-dim0", 1, 1500, 2, na, "f32", "sum", ATOMICS)          # B == 1: dim 0 of a matrix through gnnops.scatter
    add("atomics-min-f16-dim0", 1, 1500, 3, na, "f16", "min", ATOMICS)
    return C


@functools.lru_cache(None)
def all_cases():
    C = _cases()
    names = [c.name for c in C]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return tuple(C)


# Refusals: host-side checks of the entry point, nothing is launched. (case, status): the query answers NONE for all.
def refusal_cases():
    na = MAX_CHUNKS * (budget() // 4) + 1
    mk = lambda name, N, red, ib, ab: Case(name, 1, 64, 1, N, "f32", red, ib, ab, 0, NONE, {}, (), 0, 0, False, False)
    return ((mk("refuse-atomics-index4", na, "sum", 4, 8), EUNSUPPORTED),
            (mk("refuse-atomics-arg4", na, "min", 8, 4), EUNSUPPORTED),
            (mk("refuse-index2-N65537", 65537, "sum", 2, 8), EINVAL),
            (mk("refuse-arg4-sum", 100, "sum", 8, 4), EINVAL))


# ------------------------------------------------------------------------------------------------------------- inputs
def chunks_of(c):
    """[(n_lo, nloc)] of the destinations as the case's route cuts them (one piece for LDS and ATOMICS)."""
    r, d = query(c)
    rows = d[SLOT["rows"]] if r == CHUNKS else c.N
    return [(lo, min(rows, c.N - lo)) for lo in range(0, c.N, rows)]


def edge_destinations(c):
    out = []
    for lo, n in chunks_of(c):
        out += [lo - 1] if lo > 0 else []
        out += [lo, lo + n - 1]
    return sorted(set(out + [c.N - 1]))


def empty_destinations(c):
    return [lo + 1 for lo, n in chunks_of(c) if n >= 3]


_MINMAX_VALUES = {"min": (-2.0, -1.0, -0.0, 0.0, 1.0, 2.0, np.inf), "max": (-2.0, -1.0, -0.0, 0.0, 1.0, 2.0, -np.inf)}


def _store(a32, dt):
    """float32 array of values exact in `dt` -> the storage array (bf16: uint16 bit patterns)."""
    a32 = np.ascontiguousarray(a32, dtype=np.float32)
    if dt == "f32":
        return a32
    if dt == "f16":
        return a32.astype(np.float16)
    u = a32.view(np.uint32)
    assert ((u & 0xffff) == 0).all()
    return (u >> 16).astype(np.uint16)


def widen(a, dt):
    return (a.astype(np.uint32) << 16).view(np.float32) if dt == "bf16" else a.astype(np.float32)


def round_to(a32, dt):
    """fp32 -> storage type, round to nearest even (no NaNs)."""
    a32 = np.ascontiguousarray(a32, dtype=np.float32)
    if dt != "bf16":
        return _store(a32, dt) if dt == "f32" else a32.astype(np.float16)
    u = a32.view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _values(rng, shape, c):
    if c.red in ("sum", "mean"):
        return rng.integers(-4, 5, shape).astype(np.float32)
    if c.red == "mul":
        return rng.choice(np.array([1.0, -1.0, 2.0, 0.5], np.float32), shape)
    vals = np.array(_MINMAX_VALUES[c.red], np.float32)
    p = np.full(len(vals), 0.95 / (len(vals) - 1))
    p[-1] = 0.03                                          # the reduce's identity
    v = rng.choice(vals, shape, p=p / p.sum()).astype(np.float32)
    v[rng.random(shape) < 0.02] = np.nan
    return v


Inputs = namedtuple("Inputs", "src index out_init")


def tie_position(index):
    """A position of column (0, :, 0) whose destination is fed neither from position 0 nor from position E - 1 and is a
    valid id: where an init case makes `out` tie with the best contribution. None if there is none."""
    E = index.shape[1]
    col0 = index[0, :, 0]
    for t in range(4, E - 1):
        if col0[t] >= 0 and col0[t] != col0[0] and col0[t] != col0[E - 1] and not (col0[1:4] == col0[t]).any():
            return t
    return None


@functools.lru_cache(None)
def inputs(name):
    c = by_name(name)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    B, E, K, N = c.B, c.E, c.K, c.N
    r, _ = query(c)
    assert r == c.route, name
    assert not c.dropped or r in (LDS, CHUNKS), f"{name}: ids outside [0, N) on a route that does not check them"
    empties = empty_destinations(c)
    elig = np.setdiff1d(np.arange(N, dtype=np.int64), np.array(empties, dtype=np.int64))
    U = min(len(elig), max(1, -(-E // 8)))
    sel = rng.choice(elig, max(1, U // 2), replace=False)
    used = np.setdiff1d(np.union1d(sel, np.minimum(sel + 1, N - 1)), np.array(empties, dtype=np.int64))   # neighbours share a word
    base = rng.permutation(np.arange(E) % len(used))
    shift = rng.integers(0, len(used), (B, 1, K))
    index = used[(base[None, :, None] + shift) % len(used)]
    src = _values(rng, (B, E, K), c)
    L = edge_destinations(c)
    col = np.arange(B * K).reshape(B, K)
    index[:, 0, :] = np.array(L)[col % len(L)]
    if E > 1:
        index[:, E - 1, :] = np.array(L)[(col + len(L) // 2) % len(L)]
    if c.red in ("min", "max"):                           # even columns: positions 0 and E - 1 are the only winners of their destinations
        best = np.float32(-8.0 if c.red == "min" else 8.0)
        src[:, 0, :] = np.where(col % 2 == 0, best, src[:, 0, :])
        src[:, E - 1, :] = np.where(col % 2 == 0, best, src[:, E - 1, :])
    if c.dropped and E >= 6:
        bad = np.array([-1, N, N + 65541], dtype=np.int64)
        for j in range(3):
            index[:, 1 + j, :] = bad[(col + j) % 3]
    out_init = _values(rng, (B, N, K), c) if c.init else None
    if c.init and c.red in ("min", "max"):
        # the forced winners of the even columns beat whatever out holds, a NaN excepted: none there
        bb, kk = np.nonzero(col % 2 == 0)
        for e in (0, E - 1):
            out_init[bb, index[bb, e, kk], kk] = 1.0
        # and `out` ties with the best contribution of one destination per column: out is kept, arg = E
        t = tie_position(index)
        if t is not None:
            v = src[0, :, 0].copy()
            v[(index[0, :, 0] != index[0, t, 0]) | np.isnan(v) | np.isinf(v)] = np.nan
            if not np.isnan(v).all():
                out_init[0, index[0, t, 0], 0] = np.nanmin(v) if c.red == "min" else np.nanmax(v)
    out_init = _store(out_init, c.dt) if c.init else None
    if c.edges:
        fed0 = set(index[:, 0, :].ravel().tolist())
        fedl = set(index[:, E - 1, :].ravel().tolist())
        assert fed0 >= set(L) and fedl >= set(L), f"{name}: {B * K} columns do not cover the {len(L)} chunk edges"
    assert not (set(empties) & set(index.ravel().tolist())), name
    return Inputs(_store(src, c.dt), np.ascontiguousarray(index), out_init)


@functools.lru_cache(None)
def _by_name():
    return {c.name: c for c in all_cases() + tuple(rc for rc, _ in refusal_cases())}


def by_name(name):
    return _by_name()[name]


def _clean(c, inp):
    """Ids outside [0, N) sent to one more destination, N, which is cut off again: every position keeps its number."""
    valid = (inp.index >= 0) & (inp.index < c.N)
    return np.where(valid, inp.index, c.N), valid


@functools.lru_cache(None)
def expected(name):
    """(out, arg or None) of the sequential oracle, arg as int64."""
    from oracle import oracle

    c, inp = by_name(name), inputs(name)
    idx, valid = _clean(c, inp)
    extra = 0 if valid.all() else 1
    assert extra == 0 or c.dropped
    kw = {"dim_size": c.N + extra}
    if c.init:
        pad = np.zeros((c.B, extra, c.K), dtype=inp.out_init.dtype)
        kw = {"out": np.concatenate([inp.out_init, pad], axis=1)}
    res = oracle.scatter(inp.src, idx, dim=1, reduce=c.red, dtype=c.dt, **kw)
    if isinstance(res, tuple):
        return np.ascontiguousarray(res[0][:, :c.N]), np.ascontiguousarray(res[1][:, :c.N])
    return np.ascontiguousarray(res[:, :c.N]), None


def exactness(name):
    """The two conditions under which a sum / mean / product is the same in any order; returns (max contributions, max |log2| sum)."""
    c, inp = by_name(name), inputs(name)
    assert c.red in ("sum", "mean", "mul")
    idx, valid = _clean(c, inp)
    B, E, K, N = c.B, c.E, c.K, c.N + 1
    b, _, k = np.meshgrid(np.arange(B), np.arange(E), np.arange(K), indexing="ij")
    flat = ((b * N + idx) * K + k).ravel()
    v = widen(inp.src, c.dt).astype(np.float64).ravel()
    cnt = np.bincount(flat, minlength=B * N * K).reshape(B, N, K)[:, :c.N]
    init = widen(inp.out_init, c.dt).astype(np.float64) if c.init else None
    if c.red == "mul":
        acc = np.ones(B * N * K)
        np.multiply.at(acc, flat, v)
        logs = np.bincount(flat, weights=np.abs(np.log2(np.abs(v))), minlength=B * N * K).reshape(B, N, K)[:, :c.N]
        acc = acc.reshape(B, N, K)[:, :c.N]
        if c.init:
            acc, logs = acc * init, logs + np.abs(np.log2(np.abs(init)))
        worst = float(logs.max())
        assert worst < 100, name
    else:
        acc = np.bincount(flat, weights=v, minlength=B * N * K).reshape(B, N, K)[:, :c.N]
        if c.init:
            acc = acc + init
        worst = 0.0
        assert np.abs(acc).max() <= 4 * (MAX_CONTRIB + 1)
        if c.red == "mean":
            acc = (acc / np.maximum(cnt, 1)).astype(np.float32)
    assert cnt.max() + (1 if c.init else 0) <= MAX_CONTRIB, f"{name}: {cnt.max()} contributions to one destination"
    want = round_to(acc.astype(np.float32), c.dt)
    got = expected(name)[0]
    assert np.array_equal(want.view(f"u{want.itemsize}"), got.view(f"u{got.itemsize}")), f"{name}: the oracle's result depends on the order"
    return int(cnt.max()), worst


# -------------------------------------------------------------------------------------------------- gnnops_narrow_index
def narrow_sweep(n):
    """Ids one eight-load sweep of narrow_index_kernel's grid covers: ceil(n / 4096) workgroups (at most 2048) of 256
    lanes, eight 16-byte loads of two ids each."""
    return min(-(-n // 4096), 2048) * 256 * 8 * 2


def narrow_lengths():
    full = next(n for n in range(4097, 1 << 20) if narrow_sweep(n) == n)      # the shortest input beyond one workgroup's
    assert narrow_sweep(full - 1) > full - 1                                  # that is exactly one full sweep
    return (0, 1, 2, 4095, 4096, 4097, full - 1, full, full + 1)
