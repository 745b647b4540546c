"""CPU suite: the host-only contract of gnnops_edge_attention_dot and gnnops_edge_attention_dot_backward (include/gnnops.h). Every
argument check runs before the first GPU call, so the calls below — return code and gnnops_last_error() — need no GPU: their pointers
are dummy addresses that are never dereferenced, and every case ends in a check (or in the N == 0 early-out), none in a launch.
The layout of test_attention_abi_cpu.py, which covers the four older entry points."""
import pytest

OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, 1, 2, 4   # enum gnnops_status
PTR = 0x10000                                       # a 16-byte-aligned address nobody reads

# argument order of include/gnnops.h; the message prefix of each entry point
ENTRIES = {
    "gnnops_edge_attention_dot": ("edge_attention_dot", "qry ldq k v ldkv u edge_scale rowptr perm col out ldo lse N E H C scale dtype stream"),
    "gnnops_edge_attention_dot_backward": ("edge_attention_dot_backward", "qry ldq k v ldkv u edge_scale out ldo lse grad_out ldg rowptr perm col "
                                           "grad_qry gkv gu N E H C scale dtype stream"),
}
OPTIONAL = ("u", "edge_scale", "gu", "stream")


@pytest.fixture(scope="module")
def lib():
    import gnnops

    return gnnops.load_library()


def call(lib, entry, **over):
    """(return code, last error) of one call: a valid call on N = 4, E = 8, H = 2, C = 4 in fp32 without optional operands, every
    pitch the row's width — with the named arguments replaced."""
    prefix, order = ENTRIES[entry]
    H, C = over.get("H", 2), over.get("C", 4)
    args = {"N": 4, "E": 8, "H": H, "C": C, "ldq": H * C, "ldkv": H * C, "ldo": H * C, "ldg": H * C, "scale": 0.5, "dtype": 0}
    args.update(over)
    values = [args[name] if name in args else (None if name in OPTIONAL else PTR) for name in order.split()]
    rc = getattr(lib, entry)(*values)
    return rc, lib.gnnops_last_error().decode(), prefix


def test_both_symbols_are_exported(lib):
    for entry in ENTRIES:
        assert callable(getattr(lib, entry))
    assert lib.gnnops_version() == 3                                 # additive: no existing signature changed


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_size_checks_come_before_any_gpu_call(lib, entry):
    rc, _, _ = call(lib, entry, N=0)
    assert rc == OK                                              # no destination: nothing is read or written
    for over, code, fragment in (
            (dict(H=1, C=8193), EINVAL, "heads * channels <= 8192 (got 1 x 8193)"),
            (dict(H=0), EINVAL, "needs heads >= 1"),
            (dict(N=-1), EINVAL, "negative size"),
            (dict(E=-1), EINVAL, "negative size"),
            (dict(dtype=7), EINVAL, "unknown dtype 7"),
            (dict(ldq=7), EINVAL, "a row pitch is shorter than the row"),
            (dict(ldkv=7), EINVAL, "a row pitch is shorter than the row"),
            (dict(ldo=7), EINVAL, "a row pitch is shorter than the row"),
            (dict(E=2 ** 31), EUNSUPPORTED, "N, E and the row pitch must be < 2^31"),
            (dict(ldkv=2 ** 31), EUNSUPPORTED, "N, E and the row pitch must be < 2^31"),
            (dict(ldq=2 ** 31), EUNSUPPORTED, "N, E and the row pitch must be < 2^31")):
        rc, msg, prefix = call(lib, entry, **over)
        assert rc == code, (over, rc, msg)
        assert msg.startswith(prefix + ": ") and fragment in msg, (over, msg)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_null_pointers_are_refused(lib, entry):
    for name in ("qry", "rowptr", "out", "lse", "k", "v", "col"):
        rc, msg, prefix = call(lib, entry, **{name: None})
        assert rc == EINVAL and msg == prefix + ": null pointer", (name, rc, msg)


def test_backward_pitch_and_pointers(lib):
    entry = "gnnops_edge_attention_dot_backward"
    rc, msg, prefix = call(lib, entry, ldg=7)
    assert rc == EINVAL and "a row pitch is shorter than the row" in msg, (rc, msg)
    for name in ("grad_out", "grad_qry", "gkv"):
        rc, msg, prefix = call(lib, entry, **{name: None})
        assert rc == EINVAL and msg == prefix + ": null pointer", (name, rc, msg)


def test_u_without_gu_is_refused(lib):
    rc, msg, prefix = call(lib, "gnnops_edge_attention_dot_backward", u=PTR)
    assert rc == EINVAL and msg == prefix + ": u without a place for its gradient", (rc, msg)
    rc, _, _ = call(lib, "gnnops_edge_attention_dot_backward", u=PTR, N=0)
    assert rc == OK
