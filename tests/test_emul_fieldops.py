"""CPU tier: every field primitive on the emulator build, through ark355_diag_field_ops, against the plain-integer reference of
tests/fieldops_cases.py.  The emulator build compiles the PORTABLE flavour of csrc/field.cuh (no inline assembly; the adc / sbb
of g++), so this module proves the harness, the reference, the operand classes with their preconditions (the emulator build
aborts on a violated Fp28 bound) and every refusal -- the flavour word it reads back must be 0.  The device flavour is what
tests/test_gpu_fieldops.py runs, on the same cases."""
import pytest

import fieldops_cases as fc

FLAVOUR = 0


@pytest.fixture(scope="module")
def run(emul_lib, emul_ctx):
    return fc.Runner(emul_lib, emul_ctx, FLAVOUR)


def test_table_is_complete():
    assert fc.table_is_complete() == len(fc.TABLE) == 128


@pytest.mark.parametrize("name", list(fc.FP_FIELDS))
def test_fp_ops(run, name):
    """Unary ops on the 17 images and 4096 random operands, binary ops on all 289 ordered pairs, mul2sum / mul_sub on all 17^4
    ordered quadruples (the portable multiplier takes them in well under a second, so this tier runs the full sweep too)"""
    before = len(run.ran)
    fc.fp_case(run, name)
    assert set(run.ran[before:]) == {t for t in fc.TABLE if t[0] == name}


@pytest.mark.parametrize("name", list(fc.FP2_FIELDS))
def test_fp2_ops(run, name):
    before = len(run.ran)
    fc.fp2_case(run, name)
    assert set(run.ran[before:]) == {t for t in fc.TABLE if t[0] == name}


@pytest.mark.parametrize("name", list(fc.FP28_FIELDS))
def test_fp28_ops(run, name):
    before = len(run.ran)
    fc.fp28_case(run, name)
    assert set(run.ran[before:]) == {t for t in fc.TABLE if t[0] == name}


def test_pd_filter_range():
    fc.pd_filter_case()


@pytest.mark.parametrize("name", list(fc.TAIL_OPS))
def test_tails(run, name):
    fc.tail_case(run, name)


def test_refusals(run):
    fc.refusal_cases(run)


def test_comparer_bites():
    fc.comparer_bites()


def test_every_combination_is_driven():
    """Nothing is skipped: every field of the table has its parametrised test above, and each of those asserts that the
    combinations it drove are exactly the table's for its field -- 128 in all (this holds per test, so also when the module's
    tests run on several workers)"""
    fields = list(fc.FP_FIELDS) + list(fc.FP2_FIELDS) + list(fc.FP28_FIELDS)
    assert sorted({f for f, op in fc.TABLE}) == sorted(fields) == sorted(fc.TAIL_OPS)
    assert sum(len([t for t in fc.TABLE if t[0] == f]) for f in fields) == len(fc.TABLE) == 128
