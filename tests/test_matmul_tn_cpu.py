"""Host side of gnnops_gemm_tn (csrc/gemm_tn.hip): geometry and workspace over a grid of shapes. No GPU: the library loads without one
(test_abi_cpu.py) and these entry points touch no device."""
import ctypes
import itertools

import pytest

from gnnops import _lib

ROWS = [0, 1, 7, 2047, 2048, 2049, 70001, 10 ** 5, 10 ** 6, 6 * 10 ** 6, 10 ** 8]
WIDTHS = [1, 8, 11, 44, 127, 128, 129, 259, 512, 1024, 2048]
DTYPES = [_lib.F32, _lib.F16, _lib.BF16]
CAP_BYTES = 64 << 20    # include/gnnops.h: max(64 MiB, one fp32 output padded to whole tiles); 2048 x 2048 x 4 = 16 MiB


@pytest.fixture(scope="module")
def L():
    return _lib.load()


def _geometry(L, R, P, Q, dt):
    v = [ctypes.c_int64(-1) for _ in range(4)]
    rc = L.gnnops_gemm_tn_geometry(R, P, Q, dt, *[ctypes.byref(x) for x in v])
    return rc, tuple(x.value for x in v)


def _cdiv(a, b):
    return -(-a // b)


def test_geometry_and_workspace_over_the_grid(L):
    for (R, P, Q), dt in itertools.product(itertools.product(ROWS, WIDTHS, WIDTHS), DTYPES):
        rc, (tp, tq, sr, slabs) = _geometry(L, R, P, Q, dt)
        assert rc == _lib.OK, (R, P, Q, dt)
        assert tp >= 1 and tq >= 1 and sr >= 1, (R, P, Q, dt)
        assert slabs == _cdiv(R, sr), (R, P, Q, dt, sr, slabs)
        ws = L.gnnops_gemm_tn_workspace_bytes(R, P, Q, dt)
        assert ws >= slabs * _cdiv(P, tp) * tp * _cdiv(Q, tq) * tq * 4, (R, P, Q, dt)
        assert ws <= CAP_BYTES, (R, P, Q, dt, ws)
        assert _geometry(L, R, P, Q, dt) == (rc, (tp, tq, sr, slabs)) and L.gnnops_gemm_tn_workspace_bytes(R, P, Q, dt) == ws


def test_slabs_fill_the_machine_at_the_recorded_shapes(L):
    """tiles x slabs: a few workgroups per CU (256 CUs) at the shapes the issue names, never more than 1024 partial tiles."""
    for R, P, Q in [(6 * 10 ** 6, 8, 128), (6 * 10 ** 6, 128, 1024), (6 * 10 ** 6, 11, 2048)]:
        _, (tp, tq, sr, slabs) = _geometry(L, R, P, Q, _lib.F32)
        wgs = slabs * _cdiv(P, tp) * _cdiv(Q, tq)
        assert 512 <= wgs <= 1024, (R, P, Q, wgs)


def test_error_codes(L):
    for bad in [(-1, 8, 8), (8, -1, 8), (8, 8, -1)]:
        assert _geometry(L, *bad, _lib.F32)[0] == _lib.EINVAL
        assert L.gnnops_gemm_tn_workspace_bytes(*bad, _lib.F32) == 0
        assert L.gnnops_gemm_tn(None, None, None, *bad, _lib.F32, None, 0, None) == _lib.EINVAL
    for dt in (-1, 3, 99):
        assert _geometry(L, 100, 8, 8, dt)[0] == _lib.EUNSUPPORTED
        assert L.gnnops_gemm_tn_workspace_bytes(100, 8, 8, dt) == 0
        assert L.gnnops_gemm_tn(None, None, None, 100, 8, 8, dt, None, 0, None) == _lib.EUNSUPPORTED
    # an empty output returns at once, whatever the pointers; a missing one is refused before anything is launched
    assert L.gnnops_gemm_tn(None, None, None, 100, 0, 8, _lib.F32, None, 0, None) == _lib.OK
    assert L.gnnops_gemm_tn(None, None, None, 100, 8, 0, _lib.F32, None, 0, None) == _lib.OK
    assert L.gnnops_gemm_tn(None, None, None, 100, 8, 8, _lib.F32, None, 0, None) == _lib.EINVAL
    buf = (ctypes.c_float * 64)()
    assert L.gnnops_gemm_tn(buf, buf, buf, 100, 8, 8, _lib.F32, None, 0, None) == _lib.EWORKSPACE


def test_python_geometry_and_predicate_are_pure(L):
    import torch

    from gnnops import ops

    geo = ops.matmul_tn_geometry(6 * 10 ** 6, 8, 128, torch.float32)
    assert set(geo) == {"tile_p", "tile_q", "slab_rows", "slabs", "workspace_bytes"}
    assert geo["slabs"] == _cdiv(6 * 10 ** 6, geo["slab_rows"])
    for R, (P, Q), dt in itertools.product([10 ** 3, 10 ** 5, 6 * 10 ** 6], [(8, 128), (128, 1024), (512, 512)], [torch.float32, torch.bfloat16]):
        first = ops.matmul_tn_preferred(R, P, Q, dt)
        assert isinstance(first, bool) and ops.matmul_tn_preferred(R, P, Q, dt) is first
    with pytest.raises(NotImplementedError):
        ops.matmul_tn_geometry(10, 8, 8, torch.float64)
