"""finalize() on the device -- cases shared by the CPU-emulator tier and the GPU tier (tests/test_emul_lcmap.py,
tests/test_gpu_lcmap.py): ark355_gr1cs_from_lcs (include/ark355.h "finalize() on the device", snark_amd.LcSystem) against
oracle/r1cs.py.  A circuit is built on the oracle's ConstraintSystem; its lc_map, argument_lcs, ell and w are snapshotted into the
flat arrays of the entry; then the oracle's own finalize() and to_matrices() give the expected value.  Instance outlining is
transliterated here onto that class from relations/src/gr1cs/constraint_system.rs:826-863 and instance_outliner.rs:41-81: it
allocates the witnesses, rewrites lc_map and enforces the outliner's constraints through the class, and knows nothing of the
closed-form rows the kernels append.  The library is never its own expected value."""
from __future__ import annotations

import ctypes
import random

import numpy as np

from gr1cs_cases import CIRCUIT1_W, CIRCUIT1_X
from helpers import z_bytes
from oracle import r1cs as R, synthetic as S
from snark_amd import LcSystem, outlined_assignment, _binding as B
from snark_amd.lcmap import pack_variable
from sr1cs_cases import linear_forms, rows_from_csr, sr1cs_terms

SR1CS_LABEL = "SR1CS"
LDS_MAX = 1024                     # the default of policy LCS_ROW_LDS_MAX (snark_amd/csrc/policy.h)


# ---- building blocks -----------------------------------------------------------------------------------------------------------
def new_cs(C, sr1cs=False):
    """matrices are constructed, LC assignments are not: values of LCs are always evaluated through the (inlined) map"""
    cs = R.ConstraintSystem(C.r)
    cs.set_mode_prove(construct_matrices=True, generate_lc_assignments=False)
    if sr1cs:
        cs.register_predicate(SR1CS_LABEL, R.PredicateCS(R.PolynomialPredicate(C.r, 2, sr1cs_terms(C.r))))
    return cs


def raw_lc(cs, terms):
    """an LC pushed as it is (LcMap::push), without the shortcuts of new_lc_add_helper"""
    cs.lc_map.append(list(terms))
    cs.num_linear_combinations += 1
    return R.symbolic_lc(cs.num_linear_combinations - 1)


def raw_row(cs, label, *args):
    """a constraint over Variables as they are (PredicateConstraintSystem::enforce_constraint)"""
    cs.predicates[label].enforce_constraint(list(args))


def value_of(cs, v):
    """after finalize(): the value of an argument under the current assignment"""
    return cs._eval_terms(cs.get_lc(v))


def lc_references(cs):
    return sum(1 for lc in cs.lc_map for _, v in lc if v[0] == R.LC_T)


# ---- the reference side of outlining -------------------------------------------------------------------------------------------
def outline_reference(cs, mode):
    """finalize()'s second half (constraint_system.rs:698-704) after inline_all_lcs: perform_instance_outlining (:826-863) with
    outline_r1cs (mode 1) or outline_sr1cs (mode 2) of instance_outliner.rs:41-81"""
    label = R.R1CS_PREDICATE_LABEL if mode == 1 else SR1CS_LABEL
    if label not in cs.predicates:                                        # has_predicate
        return
    p = cs.p
    one_witness_var = cs.new_witness_variable(lambda: 1)                  # :834
    instance_to_witness_map = [one_witness_var]
    instance_assignment = list(cs.instance_assignment)
    for i in range(1, cs.num_instance_variables):                         # :838-843
        instance_to_witness_map.append(cs.new_witness_variable(lambda i=i: instance_assignment[i]))
    for lc in cs.lc_map:                                                  # :852-860: the map only
        for t, (c, var) in enumerate(lc):
            if var[0] == R.INSTANCE_T:
                lc[t] = (c, instance_to_witness_map[var[1]])
            elif var[0] == R.ONE_T:
                lc[t] = (c, one_witness_var)
    try:
        if mode == 1:                                                     # outline_r1cs
            one = instance_to_witness_map[0]
            cs.enforce_r1cs_constraint(lambda: R.sum_vars(p, [one]), lambda: R.sum_vars(p, [one]), lambda: R.sum_vars(p, [R.VAR_ONE]))
            for inst, wit in list(enumerate(instance_to_witness_map))[1:]:
                cs.enforce_r1cs_constraint(lambda: R.sum_vars(p, [one]), lambda wit=wit: R.sum_vars(p, [wit]),
                                           lambda inst=inst: R.sum_vars(p, [R.instance(inst)]))
        else:                                                             # outline_sr1cs: lc_diff![instance, witness], lc![]
            for inst, wit in enumerate(instance_to_witness_map):
                cs.enforce_constraint(SR1CS_LABEL, lambda inst=inst, wit=wit: R.LC(p, [(1, R.instance(inst)), (p - 1, wit)]),
                                      lambda: R.LC(p))
    except R.SynthesisError:                                              # finalize drops the outliner's error (:702)
        pass


# ---- the comparison ------------------------------------------------------------------------------------------------------------
def read_back(g):
    """{label: [(row_ptr, col, coeff bytes)]} of the resident system"""
    return {p.label: g.matrices(p.label) for p in g.predicates}


def finalize_both(lib, ctx, C, cs, outline=0):
    """snapshot, device finalize, then the oracle's finalize (+ the transliterated outlining) on the same object"""
    system = LcSystem.from_constraint_system(C.curve_id, cs)
    ell = cs.num_instance_variables
    g = system.finalize(lib, ctx, {0: None, 1: "R1CS", 2: "SR1CS"}[outline])
    cs.finalize()
    z_before = cs.full_assignment()
    if outline:
        outline_reference(cs, outline)
        if ("R1CS" if outline == 1 else SR1CS_LABEL) in cs.predicates:
            assert outlined_assignment(z_before, ell) == cs.full_assignment()
    return system, g


def check_against_oracle(lib, ctx, C, cs, outline=0, perturb=()):
    """dims; every matrix equal to the oracle's as linear forms and in canonical form; which_is_unsatisfied on the oracle's
    assignment and on one with witness `j` changed, for every j of `perturb`, equal to the oracle's.  Returns the read-back."""
    p = C.r
    system, g = finalize_both(lib, ctx, C, cs, outline)
    try:
        assert (g.ell, g.w) == (cs.num_instance_variables, cs.num_witness_variables), (g.ell, g.w)
        assert lib.gr1cs_dims(g.handle) == (g.ell, g.w, len(cs.predicates))
        assert g.num_constraints() == cs.num_constraints()
        want = cs.to_matrices()
        got = read_back(g)
        for i, (label, pcs) in enumerate(cs.predicates.items()):
            arity, n, nnz = lib.gr1cs_pred_dims(g.handle, i)
            assert (arity, n) == (pcs.predicate.arity, pcs.num_constraints), (label, arity, n)
            for k in range(arity):
                rp, col, coeff = got[label][k]
                assert len(rp) == n + 1 and int(rp[0]) == 0 and int(rp[-1]) == nnz[k] == len(col)
                rows = rows_from_csr(C, rp, col, coeff)
                for r, row in enumerate(rows):                            # canonical form
                    cols = [j for _, j in row]
                    assert all(a < b for a, b in zip(cols, cols[1:])), (label, k, r, "columns not strictly ascending")
                    assert all(c != 0 for c, _ in row), (label, k, r, "a zero coefficient is stored")
                    assert all(j < g.ell + g.w for j in cols)
                forms, ref = linear_forms(p, rows), linear_forms(p, want[label][k])
                assert forms == ref, (C.name, label, k, [r for r in range(n) if forms[r] != ref[r]][:5])
        labels = list(cs.predicates)

        def verdicts():
            bad = cs.which_is_unsatisfied()
            dev = g.which_is_unsatisfied(cs.full_assignment())
            assert (None if dev is None else "%s - %d" % dev) == bad, (C.name, dev, bad)
            return bad
        verdicts()
        for j in perturb:
            old = cs.witness_assignment[j]
            cs.witness_assignment[j] = (old + 1) % p
            verdicts()
            cs.witness_assignment[j] = old
        assert labels == [q.label for q in g.predicates]
        return got
    finally:
        g.free()


# ---- reference circuits --------------------------------------------------------------------------------------------------------
def circuit2_cs(C, sr1cs=False):
    """gr1cs/tests/circuit2.rs:46-60 (depth 2: e = d + d, d = a + b); with sr1cs, three rows of x0^2 - x1 over its LCs beside it"""
    cs = new_cs(C, sr1cs)
    R.circuit2(cs, 3, 5, 30)
    if sr1cs:
        p = C.r
        d, e = R.symbolic_lc(1), R.symbolic_lc(2)
        sq = cs.new_witness_variable(lambda: 64)                          # (a + b)^2
        raw_row(cs, SR1CS_LABEL, d, sq)
        raw_row(cs, SR1CS_LABEL, e, raw_lc(cs, [(4, sq)]))
        raw_row(cs, SR1CS_LABEL, R.instance(1), raw_lc(cs, [(9, R.VAR_ONE)]))      # a bare instance: never remapped
        assert p > 64
    return cs


def circuit1_cs(C):
    cs = new_cs(C)
    R.circuit1(cs, CIRCUIT1_X, CIRCUIT1_W)
    return cs


def example_cs(C, satisfiable=True):
    cs = new_cs(C)
    R.example_circuit(cs, satisfiable)
    return cs


def reference_circuit_case(lib, ctx, C, which):
    if which == 0:
        cs = circuit2_cs(C)
        assert lc_references(cs) == 2                                   # e = d + d
        check_against_oracle(lib, ctx, C, cs, perturb=[0, 1])
    elif which == 1:
        cs = circuit1_cs(C)
        assert cs.predicates["R1CS"].num_constraints == 0 and [q.predicate.arity for q in cs.predicates.values()] == [3, 4, 3, 3]
        check_against_oracle(lib, ctx, C, cs, perturb=[3, 7])
    else:
        check_against_oracle(lib, ctx, C, example_cs(C), perturb=[0, 10])
        check_against_oracle(lib, ctx, C, example_cs(C, satisfiable=False))


# ---- the circuit of relations/examples/bench.rs ---------------------------------------------------------------------------------
NUM_COEFFS_IN_LC = 10


def bench_rs_cs(C, num_constraints, seed=0):
    """BenchCircuit::generate_constraints (examples/bench.rs:22-83) line by line, with its new_lc extras on the even rows;
    Python's generator stands in for StdRng"""
    p = C.r
    cs = new_cs(C)
    rnd = random.Random(0xBE7C4 + seed)
    va, vb, vc = (rnd.randrange(p) for _ in range(3))
    a = cs.new_witness_variable(lambda: va)
    b = cs.new_witness_variable(lambda: vb)
    c = cs.new_witness_variable(lambda: vc)
    variables = [a, b, c]
    rng_a = random.Random(seed)
    rng_b = random.Random(rng_a.getrandbits(64))
    rng_c = random.Random(rng_a.getrandbits(64))
    for i in range(num_constraints):
        cur_num_vars = min(len(variables), 10)
        lower = max(0, len(variables) - cur_num_vars)
        upper = len(variables)
        a_i_lc_size = rng_a.randint(1, NUM_COEFFS_IN_LC)

        def a_i():
            return R.LC(p, [(1, variables[rng_a.randrange(lower, upper)]) for _ in range(a_i_lc_size)])
        b_i_lc_size = rng_b.randint(1, NUM_COEFFS_IN_LC)

        def b_i():
            return R.LC(p, [(1, variables[rng_b.randrange(lower, upper)]) for _ in range(b_i_lc_size)])
        c_i = variables[rng_c.randrange(lower, upper)]
        if i % 2 == 0:
            extra_lc = cs.new_lc(lambda: R.LC(p, [(1, variables[rng_c.randrange(lower, upper)]) for _ in range(a_i_lc_size)]))
            cs.enforce_r1cs_constraint(lambda: a_i() + extra_lc, b_i, lambda: R.LC(p) + c_i)
        else:
            cs.enforce_r1cs_constraint(a_i, b_i, lambda: R.LC(p) + c_i)
        for _ in range(3):
            variables.append(cs.new_witness_variable(lambda: va))
    return cs


def bench_rs_case(lib, ctx, C, rows):
    assert lc_references(S.bench_lc_cs(C.r, 20)) == 0                     # the oracle's bench-LC circuit has no extras
    cs = bench_rs_cs(C, rows)
    assert lc_references(cs) >= rows // 4                                 # depth 1
    check_against_oracle(lib, ctx, C, cs, perturb=[0])


# ---- the hand-made system --------------------------------------------------------------------------------------------------------
def handmade_cs(C, long_row=LDS_MAX + 1):
    """ell = 3, and every shape the kernels treat differently; see the issue's list in the comments below.  Returns the
    system and the witnesses whose change must move the verdict."""
    p = C.r
    rnd = random.Random(0x4A11D)
    cs = new_cs(C)
    x1 = cs.new_input_variable(lambda: 11)
    x2 = cs.new_input_variable(lambda: 13)
    ws = [cs.new_witness_variable(lambda v=rnd.randrange(p): v) for _ in range(80 + long_row)]
    lc0 = R.symbolic_lc(0)
    # a doubling chain d <- d + d of depth 40: 2^41 on one column, one entry per LC once each level is compacted
    d = raw_lc(cs, [(1, ws[0]), (1, ws[0])])
    doubling = [d]
    for _ in range(40):
        d = raw_lc(cs, [(1, d), (1, d)])
        doubling.append(d)
    # an accumulator of depth 64 with alternating signs: one more term per level
    acc = raw_lc(cs, [(1, ws[1])])
    accs = [acc]
    for k in range(1, 65):
        acc = raw_lc(cs, [(1, acc), (p - 1 if k & 1 else 1, ws[1 + k])])
        accs.append(acc)
    general = rnd.randrange(2, p - 1)
    specials = [
        raw_lc(cs, [(general, accs[5]), (1, ws[2])]),                     # a reference with a general coefficient
        raw_lc(cs, [(p - 1, accs[7]), (3, x1)]),                          # ... with -1 (pool index 1)
        raw_lc(cs, [(0, accs[9]), (1, ws[3])]),                           # ... with a zero coefficient
        raw_lc(cs, [(5, R.VAR_ZERO), (2, ws[4])]),                        # Zero inside an LC
        raw_lc(cs, [(7, lc0), (1, ws[5])]),                               # Lc(0) inside an LC
        raw_lc(cs, [(1, ws[6]), (p - 1, ws[6])]),                         # x - x: the row cancels to empty
        raw_lc(cs, [(2, R.VAR_ONE), (1, x2), (general, R.instance(0)), (p - 2, R.VAR_ONE)]),     # One and Instance(0) share column 0
        raw_lc(cs, [(1, doubling[-1]), (p - pow(2, 41, p), ws[0])]),      # 2^41 w0 - 2^41 w0 through a reference
    ]
    raw_lc(cs, [(3, ws[7])])                                              # an LC no argument reaches
    # one LC of long_row distinct columns, with repeats, in no order
    base = 80
    terms = [(rnd.choice([1, p - 1, rnd.randrange(p)]), ws[base + j]) for j in range(long_row)]
    terms += [(rnd.randrange(1, p), ws[base + rnd.randrange(long_row)]) for _ in range(40)]
    rnd.shuffle(terms)
    long_lc = raw_lc(cs, terms)
    through = raw_lc(cs, [(1, accs[20]), (general, long_lc), (1, x1)])    # above the threshold through a reference
    shared = raw_lc(cs, [(general, accs[20]), (1, x1), (p - 1, ws[9])])
    one = R.VAR_ONE
    for v in doubling[-2:] + accs[-3:] + specials + [long_lc, through, shared, lc0]:
        raw_row(cs, "R1CS", v, one, v)                                    # v * 1 = v
    raw_row(cs, "R1CS", one, x1, x1)                                      # One, an instance, a witness and Zero as bare arguments
    raw_row(cs, "R1CS", ws[8], R.VAR_ZERO, R.VAR_ZERO)
    raw_row(cs, "R1CS", R.VAR_ZERO, ws[8], lc0)
    for _ in range(1000):                                                 # one LC used by 1 000 rows
        raw_row(cs, "R1CS", shared, one, shared)
    # rows that a changed witness breaks: t = the accumulator's value, u = (the long LC)^2 / itself
    tail = len(ws)
    t = cs.new_witness_variable(lambda: 0)
    u = cs.new_witness_variable(lambda: 0)
    raw_row(cs, "R1CS", accs[-1], one, t)
    raw_row(cs, "R1CS", long_lc, long_lc, u)
    return cs, tail


def handmade_settle(cs, tail):
    """after finalize(): give the two determined witnesses their values"""
    rows = cs.predicates["R1CS"]
    n = rows.num_constraints
    cs.witness_assignment[tail] = value_of(cs, rows.argument_lcs[0][n - 2])
    cs.witness_assignment[tail + 1] = value_of(cs, rows.argument_lcs[0][n - 1]) ** 2 % cs.p


def handmade_case(lib, ctx, C, policy, outline=0):
    """the hand-made system with LCS_ROW_LDS_MAX at its default (the long LC alone takes the any-length path) and lowered to 8
    (every LC of more than 8 entries does): the two read-backs are byte-identical"""
    seen = []
    for knob in (None, 8):
        if knob is not None:
            policy.setenv("ARK355_LCS_ROW_LDS_MAX", knob)
        cs, tail = handmade_cs(C)
        snap_finalize = cs.finalize

        def finalize_and_settle(cs=cs, tail=tail, snap_finalize=snap_finalize):
            snap_finalize()
            handmade_settle(cs, tail)
        cs.finalize = finalize_and_settle
        got = check_against_oracle(lib, ctx, C, cs, outline, perturb=[1, 80 + 17, tail])
        inlined = sum(len(lc) for lc in cs.lc_map)
        # compaction per level: 41 + 1 entries for the doubling chain, 1 + .. + 65 for the accumulator
        assert all(len(cs.lc_map[k]) == 1 for k in range(1, 42)) and inlined < 2 * (LDS_MAX + 1) + 2145 + 400, inlined
        seen.append({label: [(rp.tobytes(), col.tobytes(), cf) for rp, col, cf in mats] for label, mats in got.items()})
    assert seen[0] == seen[1], "the two compaction paths disagree"


# ---- random systems --------------------------------------------------------------------------------------------------------------
def random_cs(C, n_lcs, seed, ell=None, max_depth=12, fan_in=6):
    """n_lcs LCs of depth <= 12 and 1..6 entries over a palette that includes 0, 1 and -1; rows of "R1CS" (a, b, fresh witness)
    and of "SR1CS" (a, fresh witness) over LCs and bare variables.  The fresh witnesses are settled after finalize()."""
    p = C.r
    rnd = random.Random(seed)
    cs = new_cs(C, sr1cs=True)
    ell = rnd.randrange(1, 6) if ell is None else ell
    for _ in range(ell - 1):
        cs.new_input_variable(lambda: rnd.randrange(p))
    base_w = max(4, n_lcs // 2)
    ws = [cs.new_witness_variable(lambda: rnd.randrange(p)) for _ in range(base_w)]
    leaves = [R.VAR_ONE, R.VAR_ZERO] + [R.instance(i) for i in range(ell)] + ws
    palette = [0, 1, p - 1, 2, rnd.randrange(p), rnd.randrange(p), rnd.randrange(p)]
    depth = [0]
    lcs = [R.symbolic_lc(0)]
    for _ in range(n_lcs):
        terms, dmax = [], 0
        for _ in range(rnd.randrange(1, fan_in + 1)):
            c = rnd.choice(palette) if rnd.random() < 0.8 else rnd.randrange(p)
            if rnd.random() < 0.25:
                j = rnd.randrange(len(lcs))
                if depth[j] < max_depth:
                    terms.append((c, lcs[j]))
                    dmax = max(dmax, depth[j] + 1)
                    continue
            terms.append((c, rnd.choice(leaves)))
        lcs.append(raw_lc(cs, terms))
        depth.append(dmax)

    def arg():
        return rnd.choice(lcs) if rnd.random() < 0.8 else rnd.choice(leaves)
    fresh = []
    for _ in range(max(3, n_lcs // 2)):
        f = cs.new_witness_variable(lambda: 0)
        fresh.append(("R1CS", f))
        raw_row(cs, "R1CS", arg(), arg(), f)
    for _ in range(max(2, n_lcs // 4)):
        f = cs.new_witness_variable(lambda: 0)
        fresh.append((SR1CS_LABEL, f))
        raw_row(cs, SR1CS_LABEL, arg(), f)
    plain_finalize = cs.finalize

    def finalize_and_settle():
        plain_finalize()
        count = {"R1CS": 0, SR1CS_LABEL: 0}
        for label, f in fresh:
            cols, i = cs.predicates[label].argument_lcs, count[label]
            a = value_of(cs, cols[0][i])
            cs.witness_assignment[f[1]] = a * value_of(cs, cols[1][i]) % p if label == "R1CS" else a * a % p
            count[label] += 1
    cs.finalize = finalize_and_settle
    return cs, max(depth), base_w


def random_case(lib, ctx, C, n_lcs, seed, outline=0, ell=None):
    cs, depth, base_w = random_cs(C, n_lcs, seed + C.curve_id, ell)
    assert depth >= (4 if n_lcs >= 70 else 0), depth
    check_against_oracle(lib, ctx, C, cs, outline, perturb=[0, base_w, cs.num_witness_variables - 1])


# ---- outlining -------------------------------------------------------------------------------------------------------------------
def outline_case(lib, ctx, C, mode, n_random=70):
    """circuit2 (with rows of SR1CS beside it), a random system, the kept quirk, the absent label, the wrong arity"""
    check_against_oracle(lib, ctx, C, circuit2_cs(C, sr1cs=True), mode, perturb=[0, 1])
    random_case(lib, ctx, C, n_random, 0x0071 + mode, outline=mode)
    random_case(lib, ctx, C, 12, 0x0072 + mode, outline=mode, ell=1)      # ell = 1: the copy of One alone
    # the quirk: an instance handed directly to the predicate stays an instance, the same one inside an LC becomes its copy
    label = "R1CS" if mode == 1 else SR1CS_LABEL
    cs = new_cs(C, sr1cs=True)
    x = cs.new_input_variable(lambda: 6)
    w = cs.new_witness_variable(lambda: 36)
    inside = raw_lc(cs, [(1, x), (1, R.VAR_ZERO)])
    if mode == 1:
        raw_row(cs, label, x, inside, w)
    else:
        raw_row(cs, label, x, w)
        raw_row(cs, label, inside, w)
    got = check_against_oracle(lib, ctx, C, cs, mode, perturb=[0])
    first = [int(c) for c in got[label][0][1]]                             # columns of the first matrix, row by row
    assert first[0] == 1 and (2 + 1 + 1) in [int(c) for M in got[label] for c in M[1]]     # x bare: column 1; inside an LC: ell + w + 1
    # the label is absent: nothing at all happens
    absent = _without_r1cs if mode == 1 else circuit2_cs
    plain = check_against_oracle(lib, ctx, C, absent(C), 0)
    same = check_against_oracle(lib, ctx, C, absent(C), mode)
    assert _bytes_of(plain) == _bytes_of(same)
    # the label is there with another arity: refused (the reference remaps and drops the ArityMismatch)
    cs = new_cs(C)
    if mode == 1:
        cs.predicates["R1CS"] = R.PredicateCS(R.PolynomialPredicate(C.r, 2, sr1cs_terms(C.r)))
    else:
        cs.register_predicate(SR1CS_LABEL, R.PredicateCS.new_r1cs(C.r))
    system = LcSystem.from_constraint_system(C.curve_id, cs)
    try:
        system.finalize(lib, ctx, label).free()
        assert False, "must refuse"
    except B.Ark355Error as e:
        assert e.code == B.EINVAL and label in str(e) and "arity" in str(e), str(e)


def _without_r1cs(C):
    """a system whose only predicate is SR1CS: outline_r1cs finds no label"""
    cs = new_cs(C, sr1cs=True)
    del cs.predicates["R1CS"]
    x = cs.new_input_variable(lambda: 5)
    w = cs.new_witness_variable(lambda: 49)
    raw_row(cs, SR1CS_LABEL, raw_lc(cs, [(1, x), (2, R.VAR_ONE)]), w)
    return cs


def _bytes_of(got):
    return {label: [(rp.tobytes(), col.tobytes(), cf) for rp, col, cf in mats] for label, mats in got.items()}


# ---- edges -----------------------------------------------------------------------------------------------------------------------
def edges_case(lib, ctx, C):
    p = C.r
    # n_lcs = 0 (not even the empty LC of ConstraintSystem::new), bare arguments only
    cs = new_cs(C)
    cs.lc_map, cs.num_linear_combinations = [], 0
    a, b = cs.new_witness_variable(lambda: 3), cs.new_witness_variable(lambda: 9)
    raw_row(cs, "R1CS", a, a, b)
    raw_row(cs, "R1CS", R.VAR_ONE, R.VAR_ZERO, R.VAR_ZERO)
    system = LcSystem.from_constraint_system(C.curve_id, cs)
    assert system.n_lcs == 0 and len(system.lc_vars) == 0
    check_against_oracle(lib, ctx, C, cs, perturb=[1])
    # ell = 1, a predicate without rows next to one with rows, an empty system
    cs = new_cs(C, sr1cs=True)
    a = cs.new_witness_variable(lambda: 4)
    raw_row(cs, SR1CS_LABEL, raw_lc(cs, [(2, a), (p - 2, a), (1, a)]), raw_lc(cs, [(16, R.VAR_ONE)]))
    assert cs.predicates["R1CS"].num_constraints == 0
    check_against_oracle(lib, ctx, C, cs, perturb=[0])
    check_against_oracle(lib, ctx, C, new_cs(C))
    for mode in (1, 2):
        check_against_oracle(lib, ctx, C, new_cs(C, sr1cs=True), mode)   # outlining a system without rows: ell = 1 row appears


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def refusal_case(lib, ctx, C):
    """every refusal of the header: ARK355_EINVAL and a message that names the array and the index; the context works after"""
    p = C.r
    cs = circuit2_cs(C, sr1cs=True)
    good = LcSystem.from_constraint_system(C.curve_id, cs)
    pool = good.pool_bytes()
    descs = good._descs()
    ell, w = good.ell, good.w
    V = pack_variable

    def call(off=good.lc_offsets, vars_=good.lc_vars, coeffs=good.lc_coeffs, pool=pool, preds=descs, ell=ell, w=w, **kw):
        return lib.gr1cs_from_lcs(ctx, C.curve_id, ell, w, off, vars_, coeffs, pool, preds, **kw)

    def refused(needles, **kw):
        try:
            h = call(**kw)
        except B.Ark355Error as e:
            assert e.code == B.EINVAL, (e.code, str(e))
            for needle in needles:
                assert needle in str(e), (needle, str(e))
            return
        lib.gr1cs_free(h)
        assert False, ("accepted", needles)

    def with_var(i, v):
        a = good.lc_vars.copy()
        a[i] = v
        return a

    def with_arg(pred, k, i, v):
        out = []
        for q, d in enumerate(descs):
            args = [a.copy() for a in d[7]]
            if q == pred:
                args[k][i] = v
            out.append(d[:7] + (args,))
        return out
    lib.gr1cs_free(call())                                                # the arrays as they are: accepted
    n_lcs, T = good.n_lcs, len(good.lc_vars)
    # a NULL where a count is non-zero
    refused(["lc_offsets is NULL"], off=None, n_lcs=n_lcs)
    refused(["lc_vars / lc_coeffs is NULL"], vars_=None)
    refused(["lc_vars / lc_coeffs is NULL"], coeffs=None)
    refused(["pool is NULL"], pool=None, n_pool=len(pool) // 32)
    refused(["preds is NULL"], preds=None, n_preds=2)
    assert lib.dll.ark355_gr1cs_from_lcs(ctx, C.curve_id, None, None, 0, ctypes.byref(ctypes.c_void_p())) == B.EINVAL
    refused(['"R1CS"', "args is NULL"], preds=[descs[0][:7] + (None,)] + descs[1:])
    refused(['"R1CS"', "args[1] is NULL"], preds=[descs[0][:7] + ([descs[0][7][0], None, descs[0][7][2]],)] + descs[1:])
    # offsets
    bad = good.lc_offsets.copy()
    bad[0] = 1
    refused(["lc_offsets[0]"], off=bad)
    bad = good.lc_offsets.copy()
    bad[3] = bad[2] - 1
    refused(["lc_offsets[3]", "below lc_offsets[2]"], off=bad)
    # variables inside the map: entry 0 is the first entry of LC 1 (d = a + b)
    refused(["lc_vars[1]", "tag above 4"], vars_=with_var(1, V(5, 0)))
    refused(["lc_vars[0]", "instance index"], vars_=with_var(0, V(B.VAR_INSTANCE, ell)))
    refused(["lc_vars[%d]" % (T - 1), "witness index"], vars_=with_var(T - 1, V(B.VAR_WITNESS, w)))
    refused(["lc_vars[2]", "LC index >= n_lcs"], vars_=with_var(2, V(B.VAR_LC, n_lcs)))
    refused(["lc_vars[2]", "not below"], vars_=with_var(2, V(B.VAR_LC, 2)))             # LC 2 references itself
    refused(["lc_vars[0]", "not below"], vars_=with_var(0, V(B.VAR_LC, 3)))             # LC 1 references LC 3
    bad = good.lc_coeffs.copy()
    bad[3] = len(pool) // 32
    refused(["lc_coeffs[3]", "coefficient index"], coeffs=bad)
    # ... and as arguments
    refused(['"R1CS"', "args[2][1]", "tag above 4"], preds=with_arg(0, 2, 1, V(7, 0)))
    refused(['"R1CS"', "args[0][0]", "instance index"], preds=with_arg(0, 0, 0, V(B.VAR_INSTANCE, ell)))
    refused(['"SR1CS"', "args[1][2]", "witness index"], preds=with_arg(1, 1, 2, V(B.VAR_WITNESS, w + 5)))
    refused(['"SR1CS"', "args[0][1]", "LC index"], preds=with_arg(1, 0, 1, V(B.VAR_LC, n_lcs)))
    # the pool
    refused(["n_pool below 2"], n_pool=1)
    two = C.r - 2
    refused(["pool[0] is not 1"], pool=z_bytes(C, [two]) + pool[32:])
    refused(["pool[1] is not -1"], pool=pool[:32] + z_bytes(C, [1]) + pool[64:])
    # labels and polynomials
    refused(["duplicate label"], preds=[descs[0], descs[0]])
    refused(["label is NULL"], preds=[(None,) + descs[0][1:]] + descs[1:])
    refused(["arity 0"], preds=[(descs[0][0], 0) + descs[0][2:]] + descs[1:])
    refused(["arity above"], preds=[(descs[0][0], 17) + descs[0][2:]] + descs[1:])
    refused(["term_ptr must start at 0"], preds=[descs[0][:4] + (np.array([1, 2, 3], np.uint32),) + descs[0][5:]] + descs[1:])
    refused(["non-decreasing"], preds=[descs[0][:4] + (np.array([0, 2, 1], np.uint32),) + descs[0][5:]] + descs[1:])
    refused(["variable >= arity"], preds=[descs[0][:5] + (np.array([0, 1, 3], np.uint32),) + descs[0][6:]] + descs[1:])
    refused(["term_var / term_exp is NULL"], preds=[descs[0][:5] + (None,) + descs[0][6:]] + descs[1:])
    refused(["outline"], outline=3)
    # a matrix above ARK355_GR1CS_MAX_ROWS non-zeros: one LC of 2^16 columns used by 2^16 + 1 rows; refused from the row lengths,
    # before the matrix is allocated
    big, rows = 1 << 16, (1 << 16) + 1
    zero = np.full(rows, V(B.VAR_ZERO, 0), dtype=np.uint64)
    wide = [(descs[0][:2] + (rows,) + descs[0][3:7] + ([np.full(rows, V(B.VAR_LC, 0), dtype=np.uint64), zero, zero],))]
    refused(['"R1CS"', "matrix 0", "ARK355_GR1CS_MAX_ROWS"], off=np.array([0, big], dtype=np.uint64),
            vars_=np.arange(big, dtype=np.uint64) | np.uint64(B.VAR_WITNESS << B.VAR_TAG_SHIFT), coeffs=np.zeros(big, dtype=np.uint32),
            pool=pool[:64], preds=wide, w=big)
    refused(["num_instance"], ell=0)
    # the context still works, and so does the system
    check_against_oracle(lib, ctx, C, circuit2_cs(C, sr1cs=True), perturb=[0])
