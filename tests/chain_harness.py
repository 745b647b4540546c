"""What the chain tests share: the rule by which a GPU result passes against a float64 chain, the choice of its bar, and the
builder / writer / reader of the self-error tables the bars come from. A chain module (tests/*_chain.py) restates one op; its GPU
test runs the device and hands every tensor to ``judge_case``; its CPU test pins the recorded table with
``check_self_error_table``. Nothing here touches the GPU or loads the library at import time.

The measure is per tensor, max |got - want| / max |want| (``rel_err``). The bar is the project's (``PROJECT_BAR``: fp32 3e-5, fp16
1e-2, from test_conv_train_gpu.py) where the project has a precedent, and 4 x the chain's recorded distance from itself — the same
chain run in float32 with the library's roundings against the float64 one, never the kernels — where it has none (bf16, and the
cases a table marks ``bar="self"``)."""
import json

import torch

F32, F16, BF16 = DTYPES = [torch.float32, torch.float16, torch.bfloat16]
DNAME = {F32: "f32", F16: "f16", BF16: "bf16"}
PROJECT_BAR = {F32: 3e-5, F16: 1e-2}


def rel_err(got, want):
    if want.numel() == 0:
        return 0.0
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-6)


# ---- the pass rule ------------------------------------------------------------------------------------------------------------
def judge(label, name, got, want, project_bar, self_bar=False, key=None, recorded=None, transform=None):
    """One tensor of one case: ``got`` (a device tensor or None) against ``want`` (float64, CPU). The bar is 4 x recorded[key] when
    ``self_bar``, else ``project_bar``; a key the recorded table lacks raises, no other bar stands in for it. ``transform`` is applied
    to both sides before the measure (a mean's gradients are compared degree-scaled)."""
    assert got is not None, f"{name}: no gradient"
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{label} {name}: not finite"
    err = rel_err(got, want) if transform is None else rel_err(transform(got), transform(want))
    if self_bar:
        bar, why = 4 * recorded[key], f"4 x self error, {key}"
    else:
        bar, why = project_bar, "the project's bar"
    print(f"{label} {name}: {err:.3e} (bar {bar:.3e}: {why})")
    assert err <= bar, f"{label} {name}: error {err:.3e} of scale exceeds {bar:.3e} ({why})"


def judge_case(case, dtype, name, got, want, recorded, key=None, transform=None):
    """``judge`` for a case of a chain module's tables (a ``CaseBars``); ``key`` where the table's key is not case.key(dtype, name)."""
    self_bar = case.self_bar(dtype)
    judge(case.id(dtype), name, got, want, None if self_bar else case.project_bar(dtype), self_bar,
          case.key(dtype, name) if key is None else key, recorded, transform)


class CaseBars:
    """The naming and the bar choice of a chain module's Case dataclass (fields ``table``, ``name``, ``bar``: project | self)."""

    def id(self, dtype):
        return f"{self.name}-{DNAME[dtype]}"

    def key(self, dtype, tensor):
        return f"{self.table}/{self.name}/{DNAME[dtype]}/{tensor}"

    def self_bar(self, dtype):
        return self.bar == "self" or dtype == BF16

    def project_bar(self, dtype):
        return PROJECT_BAR[dtype]


# ---- what the GPU test files share --------------------------------------------------------------------------------------------
def params(table):
    """pytest.mark.parametrize("case,dtype", **params(table))"""
    pairs = [(c, d) for c in table for d in c.dtypes]
    return {"argvalues": pairs, "ids": [c.id(d) for c, d in pairs]}


class Reference:
    """The float64 chain of a case, computed once per (table, name, dtype, further arguments) and shared; nobody writes to it."""

    def __init__(self, case_grads):
        self.case_grads, self.cache = case_grads, {}

    def __call__(self, case, dtype, *more):
        key = (case.table, case.name, dtype) + more
        if key not in self.cache:
            self.cache[key] = self.case_grads(case, dtype, *more)
        return self.cache[key]


def load_conv():
    """The body of the module-scoped ``conv`` fixture: gnnops.conv with the library loaded."""
    import gnnops
    from gnnops import conv

    gnnops.load_library()
    return conv


# ---- the self-error tables ----------------------------------------------------------------------------------------------------
def self_error(case_grads, case, dtype):
    """{"out" | operand: rel_err of the chain run with ``rnd=dtype`` against the float64 one}; case_grads returns (out, grads)."""
    out, grads = case_grads(case, dtype)
    out_r, grads_r = case_grads(case, dtype, rnd=dtype)
    err = {"out": rel_err(out_r, out)}
    for k in grads:
        err[k] = rel_err(grads_r[k], grads[k])
    return err


def self_bar_cases(tables):
    return [(c, d) for t in tables.values() for c in t for d in c.dtypes if c.self_bar(d)]


def build_table(cases, self_error, key=lambda case, dtype, tensor: case.key(dtype, tensor)):
    """{key: self error} over ``cases`` (the argument tuples of a chain module's own ``self_error``; (case, dtype) in most)."""
    table = {}
    for case in cases:
        for tensor, err in self_error(*case).items():
            table[key(*case, tensor)] = err
    return table


def write_table(table, path):
    with open(path, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    return table


def load_table(path):
    with open(path) as f:
        return json.load(f)


def recomputed_table(chain, capsys, what="library-order float32 chain against the float64 chain"):
    """(table recomputed from the chain alone, the committed one) of a chain module, with the same keys; prints the worst entry per
    table and type (a key is [family/]table/case/type/tensor)."""
    recorded = chain.load_self_error()
    table = chain.self_error_table()
    with capsys.disabled():
        worst = {}
        for k, v in table.items():
            *group, _, d, _ = k.split("/")
            worst[(*group, d)] = max(worst.get((*group, d), (0.0, "")), (v, k))
        width = max(6, max(len(g[-2]) for g in worst))
        print(f"\nself error of tests/{chain.__name__}.py ({what})")
        for (*lead, t, d), (v, k) in sorted(worst.items()):
            print("  worst of " + "".join(f"{f} " for f in lead) + f"{t:{width}s} {d:4s} {v:.3e}  ({k})")
    assert set(recorded) == set(table)
    return table, recorded


def check_self_error_table(chain, bound, capsys):
    """The numbers the bars of the GPU tests are 4 x of: recomputed, each in [0, bound) and equal to the committed JSON."""
    table, recorded = recomputed_table(chain, capsys)
    for k, v in table.items():
        assert v == v and 0 <= v < bound, (k, v)
        assert v == recorded[k], (k, v, recorded[k])
