"""CPU suite: the host-only contract of the five attention entry points of include/gnnops.h. Every argument check of
gnnops_edge_attention, gnnops_edge_attention_backward, gnnops_edge_attention_v1 and gnnops_edge_attention_v1_backward runs before
the first GPU call, so the calls below — return code and gnnops_last_error() — need no GPU: their pointers are dummy addresses
that are never dereferenced, and every case ends in a check (or in the N == 0 early-out), none in a launch."""
import pytest

OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, 1, 2, 4   # enum gnnops_status
PTR = 0x10000                                       # a 16-byte-aligned address nobody reads

# argument order of include/gnnops.h; the message prefix of each entry point
ENTRIES = {
    "gnnops_edge_attention": ("edge_attention", "q ldq p ldp att u rowptr perm col out ldo lse N E H C negative_slope dtype stream"),
    "gnnops_edge_attention_backward": ("edge_attention_backward", "q ldq p ldp att u out ldo lse grad_out ldg rowptr perm col grad_p gq gu grad_att "
                                       "N E H C negative_slope dtype workspace workspace_bytes stream"),
    "gnnops_edge_attention_v1": ("edge_attention_v1", "q ldq d ldd att u c edge_scale rowptr perm col out ldo lse N E H C has_row_slope row_slope "
                                 "negative_slope dtype stream"),
    "gnnops_edge_attention_v1_backward": ("edge_attention_v1_backward", "q ldq d ldd att u c edge_scale out ldo lse grad_out ldg rowptr perm col "
                                          "grad_d gq gc grad_att N E H C has_row_slope row_slope negative_slope dtype workspace workspace_bytes "
                                          "stream"),
}
FORWARD = ["gnnops_edge_attention", "gnnops_edge_attention_v1"]
BACKWARD = ["gnnops_edge_attention_backward", "gnnops_edge_attention_v1_backward"]
SECOND_FAMILY = ["gnnops_edge_attention_v1", "gnnops_edge_attention_v1_backward"]
WORKSPACE_BYTES = "gnnops_edge_attention_backward_workspace_bytes"
OPTIONAL = ("u", "c", "edge_scale", "gu", "gc", "stream")


@pytest.fixture(scope="module")
def lib():
    import gnnops

    return gnnops.load_library()


def call(lib, entry, **over):
    """(return code, last error) of one call: a valid call on N = 4, E = 8, H = 2, C = 4 in fp32 without optional operands, every
    pitch the row's width, the workspace as large as asked for — with the named arguments replaced."""
    prefix, order = ENTRIES[entry]
    H, C = over.get("H", 2), over.get("C", 4)
    args = {"N": 4, "E": 8, "H": H, "C": C, "ldq": H * C, "ldp": H * C, "ldo": H * C, "ldg": H * C, "ldd": H, "negative_slope": 0.2,
            "has_row_slope": 0, "row_slope": 0.0, "dtype": 0, "workspace_bytes": 1 << 30}
    args.update(over)
    values = [args[name] if name in args else (None if name in OPTIONAL else PTR) for name in order.split()]
    rc = getattr(lib, entry)(*values)
    return rc, lib.gnnops_last_error().decode(), prefix


@pytest.mark.parametrize("entry", FORWARD + BACKWARD)
def test_size_checks_come_before_any_gpu_call(lib, entry):
    rc, _, _ = call(lib, entry, N=0)
    assert rc == OK                                              # no destination: nothing is read or written
    for over, code, fragment in (
            (dict(H=1, C=8193), EINVAL, "heads * channels <= 8192 (got 1 x 8193)"),
            (dict(H=0), EINVAL, "needs heads >= 1"),
            (dict(dtype=7), EINVAL, "unknown dtype 7"),
            (dict(ldq=7), EINVAL, "a row pitch is shorter than the row"),
            (dict(E=2 ** 31), EUNSUPPORTED, "N, E and the row pitch must be < 2^31")):
        rc, msg, prefix = call(lib, entry, **over)
        assert rc == code, (over, rc, msg)
        assert msg.startswith(prefix + ": ") and fragment in msg, (over, msg)


@pytest.mark.parametrize("entry", SECOND_FAMILY)
def test_u_and_c_together_are_refused(lib, entry):
    rc, msg, prefix = call(lib, entry, u=PTR, c=PTR, gc=PTR)
    assert rc == EUNSUPPORTED and msg.startswith(prefix + ": ") and "together have no kernel instance" in msg, (rc, msg)


@pytest.mark.parametrize("entry", BACKWARD)
def test_backward_needs_grad_att_and_its_workspace(lib, entry):
    rc, msg, prefix = call(lib, entry, grad_att=None)
    assert rc == EINVAL and msg == prefix + ": null pointer", (rc, msg)
    need = getattr(lib, WORKSPACE_BYTES)(4, 2, 4)
    assert need == 4 * 8 * 4
    for over in (dict(workspace=None), dict(workspace_bytes=need - 1), dict(workspace=PTR + 8, workspace_bytes=need)):
        rc, msg, prefix = call(lib, entry, **over)
        assert rc == EWORKSPACE and msg.startswith(prefix + ": workspace "), (over, rc, msg)
    rc, msg, _ = call(lib, entry, workspace_bytes=need - 1)
    assert msg.endswith(f"workspace {need - 1} < {need}"), msg


def test_workspace_bytes_serves_both_families(lib):
    ws = getattr(lib, WORKSPACE_BYTES)
    assert ws(0, 4, 64) == 0
    assert ws(100, 8, 1025) == 0 and ws(100, 1, 8193) == 0     # H * C > 8192
    for N, H, C in ((1, 1, 1), (300, 4, 64), (5000, 8, 1024)):
        rows = min(max((1 << 22) // (H * C), 256), 2048, N)      # 16 MiB of fp32 partials at the most, 256 .. 2048 rows, never more than N
        assert ws(N, H, C) == rows * H * C * 4, (N, H, C)
