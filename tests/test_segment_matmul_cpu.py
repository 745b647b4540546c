"""segment_matmul without a GPU: the C ABI's host-only entry points and the argument checks of the Python op."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gnnops_segment_matmul", "gnnops_segment_matmul_workspace_bytes", "gnnops_segment_matmul_geometry")


@pytest.fixture(scope="module")
def lib():
    import gnnops

    return gnnops.load_library()


def test_new_names_are_declared_and_exported(lib):
    from gnnops import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gnnops.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gnnops_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/gnnops.h"
        assert hasattr(lib, name), f"{name} is not exported by libgnnops.so"
        assert name in _lib.SIGNATURES
    for name in declared:
        assert hasattr(lib, name), f"{name} declared but not exported"
    assert lib.gnnops_version() == 3


def test_geometry_and_workspace(lib):
    from gnnops import _lib, ops

    for code, dtype in ((_lib.F32, torch.float32), (_lib.F16, torch.float16), (_lib.BF16, torch.bfloat16)):
        v = [ctypes.c_int64(-1) for _ in range(3)]
        assert lib.gnnops_segment_matmul_geometry(code, *[ctypes.byref(x) for x in v]) == _lib.OK
        assert all(x.value > 0 for x in v)
        geo = ops.segment_matmul_geometry(dtype)
        assert (geo["tile_m"], geo["tile_n"], geo["k_step"]) == tuple(x.value for x in v)
        assert lib.gnnops_segment_matmul_geometry(code, None, None, None) == _lib.OK
    assert lib.gnnops_segment_matmul_geometry(77, None, None, None) == _lib.EUNSUPPORTED
    with pytest.raises(NotImplementedError):
        ops.segment_matmul_geometry(torch.float64)
    ws = lib.gnnops_segment_matmul_workspace_bytes
    last = 0
    for T in (0, 1, 2, 63, 64, 65, 1000, 1 << 20):
        assert ws(T) >= (T + 1) * 4
        assert ws(T) >= last
        last = ws(T)
    assert ws(-1) == 0


def test_abi_refuses_bad_arguments_before_any_launch(lib):
    from gnnops import _lib

    f = lib.gnnops_segment_matmul
    one = ctypes.c_void_p(256)       # never dereferenced: every call below returns before a launch
    assert f(one, one, one, None, one, -1, 4, 4, 1, _lib.F32, one, 1024, None) == _lib.EINVAL
    assert f(one, one, one, None, one, 4, 4, 4, -1, _lib.F32, one, 1024, None) == _lib.EINVAL
    assert f(one, one, one, None, one, 4, 4, 4, 1, 9, one, 1024, None) == _lib.EUNSUPPORTED
    assert f(None, one, one, None, one, 4, 4, 4, 1, _lib.F32, one, 1024, None) == _lib.EINVAL
    assert f(one, None, one, None, one, 4, 4, 4, 1, _lib.F32, one, 1024, None) == _lib.EINVAL
    assert f(one, one, one, None, None, 4, 4, 4, 1, _lib.F32, one, 1024, None) == _lib.EINVAL
    assert f(one, one, one, None, one, 4, 4, 4, 1, _lib.F32, one, 4, None) == _lib.EWORKSPACE
    assert f(one, one, one, None, one, 4, 4, 4, 1, _lib.F32, None, 0, None) == _lib.EWORKSPACE
    assert b"workspace" in lib.gnnops_last_error()
    # nothing to do: OK without a look at the pointers
    assert f(None, None, None, None, None, 0, 4, 4, 3, _lib.F32, None, 0, None) == _lib.OK
    assert f(None, None, None, None, None, 4, 4, 0, 3, _lib.F32, None, 0, None) == _lib.OK


def test_python_op_checks_a_cpu_ptr_and_its_operands():
    import gnnops
    from gnnops import autograd, ops

    assert gnnops.segment_matmul is autograd.segment_matmul
    x, w = torch.rand(6, 4), torch.rand(3, 4, 5)
    good = torch.tensor([0, 2, 2, 6])
    for ptr, what in ((torch.tensor([1, 2, 2, 6]), "start at 0"), (torch.tensor([0, 2, 2, 5]), "end at"),
                      (torch.tensor([0, 4, 2, 6]), "not decrease"), (torch.tensor([0, 2, 6]), "entries"),
                      (torch.tensor([0, 1, 2, 2, 6]), "entries")):
        with pytest.raises(RuntimeError, match=what):
            ops.segment_matmul(x, ptr, w)
    with pytest.raises(RuntimeError, match="int64"):
        ops.segment_matmul(x, good.int(), w)
    with pytest.raises(RuntimeError, match="same dtype"):
        ops.segment_matmul(x, good, w.half())
    with pytest.raises(RuntimeError, match="same dtype"):
        ops.segment_matmul(x, good, w, torch.rand(3, 5).bfloat16())
    with pytest.raises(RuntimeError, match="columns"):
        ops.segment_matmul(x, good, torch.rand(3, 7, 5))
    with pytest.raises(RuntimeError, match="bias must be"):
        ops.segment_matmul(x, good, w, torch.rand(2, 5))
    with pytest.raises(NotImplementedError, match="requires grad"):
        ops.segment_matmul(x.clone().requires_grad_(True), good, w)
    with pytest.raises(NotImplementedError, match="requires grad"):
        ops.segment_matmul(x, good, w.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="requires grad"):
        ops.segment_matmul(x, good, w, torch.rand(3, 5, requires_grad=True))
    # and with everything in order, CPU tensors are refused, not emulated
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.segment_matmul(x, good, w)
    with pytest.raises(RuntimeError, match="no CPU path"):
        gnnops.segment_matmul(x, good, w)


def test_layers_carry_pyg_parameter_names():
    from gnnops import conv

    lin = conv.HeteroLinear(11, 44, 5)
    assert {k: tuple(v.shape) for k, v in lin.state_dict().items()} == {"weight": (5, 11, 44), "bias": (5, 44)}
    assert set(conv.HeteroLinear(11, 44, 5, bias=False).state_dict()) == {"weight"}
    full = conv.RGCNConv(11, 44, 5)
    assert {k: tuple(v.shape) for k, v in full.state_dict().items()} == {"weight": (5, 11, 44), "root": (11, 44), "bias": (44,)}
    based = conv.RGCNConv(11, 44, 5, num_bases=2, root_weight=False, bias=False)
    assert {k: tuple(v.shape) for k, v in based.state_dict().items()} == {"weight": (2, 11, 44), "comp": (5, 2)}
    with pytest.raises(NotImplementedError):
        conv.RGCNConv(4, 4, 2, aggr="max")
