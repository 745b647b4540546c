"""tests/chain_harness.py on tiny CPU tensors: the one pass rule every chain GPU test goes through, its choice of bar, and the table
helpers. want = [1, 2] has max |want| = 2, so got = want + [0, 2 d] is exactly d from it in the harness's measure; the self error
2^-10 makes the bar 4 x 2^-10 = 2^-8, and every number here is exact in float64."""
from dataclasses import dataclass

import pytest
import torch

import chain_harness as ch
from chain_harness import BF16, DTYPES, F16, F32

WANT = torch.tensor([1.0, 2.0], dtype=torch.float64)
BAR = 2.0 ** -8


@dataclass(frozen=True)
class Case(ch.CaseBars):
    table: str
    name: str
    bar: str = "project"
    dtypes: tuple = tuple(DTYPES)


SELF, PROJECT = Case("t", "self", bar="self"), Case("t", "project")
RECORDED = {SELF.key(d, "out"): BAR / 4 for d in DTYPES}
RECORDED[PROJECT.key(BF16, "out")] = BAR / 4


def off_by(d):
    return WANT + torch.tensor([0.0, 2 * d], dtype=torch.float64)


def test_the_measure():
    assert ch.rel_err(off_by(BAR), WANT) == BAR
    assert ch.rel_err(torch.zeros(0), torch.zeros(0)) == 0.0
    assert ch.rel_err(torch.tensor([2.0 ** -30], dtype=torch.float64), torch.zeros(1, dtype=torch.float64)) == 2.0 ** -30 / 1e-6      # the denominator's floor


def test_passes_at_the_bar_and_fails_just_above(capsys):
    ch.judge_case(SELF, F32, "out", off_by(BAR), WANT, RECORDED)
    assert capsys.readouterr().out == f"self-f32 out: {BAR:.3e} (bar {BAR:.3e}: 4 x self error, t/self/f32/out)\n"
    with pytest.raises(AssertionError, match="exceeds"):
        ch.judge_case(SELF, F32, "out", off_by(BAR + 2.0 ** -41), WANT, RECORDED)


def test_fails_on_none_a_wrong_shape_and_a_value_that_is_not_finite():
    with pytest.raises(AssertionError, match="no gradient"):
        ch.judge_case(SELF, F32, "out", None, WANT, RECORDED)
    with pytest.raises(AssertionError):
        ch.judge_case(SELF, F32, "out", WANT.view(1, 2), WANT, RECORDED)
    with pytest.raises(AssertionError):
        ch.judge_case(SELF, F32, "out", WANT[:1], WANT, RECORDED)          # would broadcast
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(AssertionError, match="not finite"):
            ch.judge_case(SELF, F32, "out", torch.tensor([1.0, bad], dtype=torch.float64), WANT, RECORDED)
    # a NaN in the reference is no pass either: the comparison with the bar is false
    with pytest.raises(AssertionError, match="exceeds"):
        ch.judge_case(SELF, F32, "out", WANT, torch.tensor([1.0, float("nan")], dtype=torch.float64), RECORDED)


def test_a_key_the_recorded_table_lacks_raises():
    with pytest.raises(KeyError):
        ch.judge_case(SELF, F32, "q", WANT, WANT, RECORDED)
    with pytest.raises(KeyError):
        ch.judge_case(SELF, F32, "out", WANT, WANT, RECORDED, key="v2/t/self/f32/out")
    with pytest.raises(KeyError):
        ch.judge("label", "out", WANT, WANT, 1.0, self_bar=True, key="absent", recorded={})


@pytest.mark.parametrize("dtype,passes,fails", [(F32, 2.0 ** -16, 2.0 ** -14), (F16, 2.0 ** -7, 2.0 ** -6)], ids=["f32", "f16"])
def test_project_cases_take_the_projects_bar_for_fp32_and_fp16(dtype, passes, fails, capsys):
    assert ch.PROJECT_BAR == {F32: 3e-5, F16: 1e-2} and passes < ch.PROJECT_BAR[dtype] < fails
    assert not PROJECT.self_bar(dtype) and PROJECT.project_bar(dtype) == ch.PROJECT_BAR[dtype]
    ch.judge_case(PROJECT, dtype, "out", off_by(passes), WANT, {})             # the recorded table is not consulted
    assert f"(bar {ch.PROJECT_BAR[dtype]:.3e}: the project's bar)" in capsys.readouterr().out
    with pytest.raises(AssertionError, match="the project's bar"):
        ch.judge_case(PROJECT, dtype, "out", off_by(fails), WANT, {})


def test_bf16_and_self_cases_take_four_times_the_self_error(capsys):
    assert PROJECT.self_bar(BF16) and all(SELF.self_bar(d) for d in DTYPES)
    for case, dtype in [(PROJECT, BF16)] + [(SELF, d) for d in DTYPES]:
        ch.judge_case(case, dtype, "out", off_by(BAR), WANT, RECORDED)
        assert f"(bar {BAR:.3e}: 4 x self error, {case.key(dtype, 'out')})" in capsys.readouterr().out
        with pytest.raises(AssertionError, match="4 x self error"):
            ch.judge_case(case, dtype, "out", off_by(BAR + 2.0 ** -41), WANT, RECORDED)
    # an own project bar (conv_chain's film cases) is what a project case is held to
    film = type("Film", (Case,), {"project_bar": lambda self, dtype: 2.0 ** -5})("t", "film")
    ch.judge_case(film, F16, "out", off_by(2.0 ** -5), WANT, {})
    with pytest.raises(AssertionError):
        ch.judge_case(film, F16, "out", off_by(2.0 ** -4), WANT, {})


def test_the_transform_is_applied_to_both_sides():
    want = torch.tensor([1.0, 1000.0], dtype=torch.float64)
    first = lambda t: t * torch.tensor([1.0, 0.0], dtype=torch.float64)   # noqa: E731
    got = torch.tensor([1.0, 7.0], dtype=torch.float64)
    with pytest.raises(AssertionError, match="exceeds"):
        ch.judge_case(SELF, F32, "out", got, want, RECORDED)
    ch.judge_case(SELF, F32, "out", got, want, RECORDED, transform=first)      # on got alone 0 would face 1000, on want alone 7 would face 0
    # and it is the measure that is transformed: 0.5 / 1000 passes, 500 / 1000 does not
    got = torch.tensor([1.5, 1000.0], dtype=torch.float64)
    ch.judge_case(SELF, F32, "out", got, want, RECORDED)
    with pytest.raises(AssertionError, match="exceeds"):
        ch.judge_case(SELF, F32, "out", got, want, RECORDED, transform=lambda t: t * torch.tensor([1000.0, 1.0], dtype=torch.float64))
    # finiteness is asked of what the device returned, before any transform
    with pytest.raises(AssertionError, match="not finite"):
        ch.judge_case(SELF, F32, "out", torch.tensor([1.0, float("inf")], dtype=torch.float64), want, RECORDED, transform=first)


def test_names_params_and_the_reference_cache():
    assert SELF.id(BF16) == "self-bf16" and SELF.key(F16, "d x") == "t/self/f16/d x"
    one = Case("t", "one", dtypes=(F32, BF16))
    assert ch.params([one, SELF]) == {"argvalues": [(one, F32), (one, BF16)] + [(SELF, d) for d in DTYPES],
                                      "ids": ["one-f32", "one-bf16", "self-f32", "self-f16", "self-bf16"]}
    assert ch.self_bar_cases({"a": [one], "b": [SELF]}) == [(one, BF16)] + [(SELF, d) for d in DTYPES]
    calls = []
    ref = ch.Reference(lambda case, dtype, flag=False: calls.append((case.name, dtype, flag)) or len(calls))
    assert (ref(one, F32), ref(one, F32), ref(one, F32, True), ref(one, BF16), ref(one, F32, True)) == (1, 1, 2, 3, 2)
    assert calls == [("one", F32, False), ("one", F32, True), ("one", BF16, False)]


def test_tables(tmp_path):
    def case_grads(case, dtype, rnd=None):
        shift = 0.0 if rnd is None else (0.25 if rnd == BF16 else 0.125)
        return WANT + shift, {"q": WANT * 2 + shift, "p": torch.zeros(0, dtype=torch.float64)}

    assert ch.self_error(case_grads, SELF, BF16) == {"out": 0.125, "q": 0.0625, "p": 0.0}
    assert list(ch.self_error(case_grads, SELF, F16)) == ["out", "q", "p"]
    table = ch.build_table(ch.self_bar_cases({"t": [SELF, PROJECT]}), lambda c, d: ch.self_error(case_grads, c, d))
    assert set(table) == {c.key(d, t) for c, d in [(SELF, F32), (SELF, F16), (SELF, BF16), (PROJECT, BF16)] for t in ("out", "q", "p")}
    assert table["t/project/bf16/q"] == 0.0625 and table["t/self/f16/out"] == 0.0625
    keyed = ch.build_table([("v2", SELF, F32)], lambda f, c, d: {"out": 0.5}, lambda f, c, d, t: f"{f}/{c.key(d, t)}")
    assert keyed == {"v2/t/self/f32/out": 0.5}
    path = tmp_path / "table.json"
    assert ch.write_table({"b": 0.5, "a": 1e-7}, path) == {"b": 0.5, "a": 1e-7}
    assert path.read_text() == '{\n"a": 1e-07,\n"b": 0.5\n}\n'
    assert ch.load_table(path) == {"a": 1e-7, "b": 0.5}
