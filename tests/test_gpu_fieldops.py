"""GPU tier (-m gpu): every device field primitive -- Fp with its inline-assembly column chains (mul, the dual-product mul2sum /
mul_sub, the 12-limb multi-chunk statements of BLS12-381 Fq), the __builtin_addc / __builtin_subc flavour of add / sub / neg /
reduce_once, Fp2, and the radix-2^28 Fp28 with its Karatsuba level, bias classes, filter and conversions -- through
ark355_diag_field_ops against the plain-integer reference of tests/fieldops_cases.py, at designed operands: all 17^4 ordered
quadruples of the Montgomery-image patterns for the dual product, all 289^2 ordered pairs of Fp2 elements, every form of k p and
its neighbours for the filter.  The flavour word the kernel writes must be 1: the assembly multiplier ran.
CPU twin (portable flavour): tests/test_emul_fieldops.py."""
import pytest

import fieldops_cases as fc

pytestmark = pytest.mark.gpu
FLAVOUR = 1


@pytest.fixture(scope="module")
def run(gpu_lib, gpu_ctx):
    return fc.Runner(gpu_lib, gpu_ctx, FLAVOUR)


def test_table_is_complete():
    assert fc.table_is_complete() == len(fc.TABLE) == 128


@pytest.mark.parametrize("name", list(fc.FP_FIELDS))
def test_fp_ops(run, name):
    before = len(run.ran)
    fc.fp_case(run, name, full_quads=True)          # always the full 17^4 sweep here: this is where the assembly is
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
