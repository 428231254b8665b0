"""CPU: every case of tests/train_cases.py is well conditioned.

tests/test_gpu_train_forms.py holds csrc/bnn_train.hip to rtol 2e-5 / atol 2e-5 max(1, max|ref|) against the
fp64 oracle after several Adam steps.  That bound is honest only where fp32 arithmetic alone stays far inside
it: Adam moves a variable by about lr whatever the gradient's size, so a gradient near zero can flip sign under
rounding and shift its variable by 2 lr = 100 tolerances.  Here the oracle itself takes each case's steps once in
fp64 and once in fp32 on the same minibatches; the two must agree to 0.1 of the GPU tolerance, element-wise.
A case that does not gets another data seed in train_cases.py, never a looser bound.
"""
import time

import numpy as np
import pytest

import train_cases as tc

CONDITION = 0.1   # fp32 oracle vs fp64 oracle, in units of the GPU tolerance


def test_case_table_names_every_form_and_edge():
    """The table holds what the GPU file promises to run: all ten row forms, a partial last block of 4, 8 and
    12 units, E in {1, 8, 9, 16}, the generic shapes, every geometry; no case twice."""
    forms = {c.form for c in tc.CASES if c.form}
    older = {(1, 2, 2), (2, 13, 3), (2, 8, 3), (3, 13, 4), (3, 4, 4)}
    assert forms == older | {(1, 13, 2), (2, 2, 3), (2, 16, 3), (1, 16, 2), (1, 8, 2)}
    assert {c.H % 16 for c in tc.CASES if c.form} == {0, 4, 8, 12}
    assert {4, 12} <= {c.H % 16 for c in tc.CASES if c.group == 'b'}
    assert {1, 8, 9, 16} <= {c.E for c in tc.CASES if c.group == 'c'}
    generic = [c for c in tc.CASES if c.group == 'd']
    assert all(c.form is None for c in generic)
    listed = {(3, 11, 3, 64), (3, 10, 3, 32), (3, 10, 3, 50), (3, 11, 3, 30), (2, 3, 1, 8), (2, 17, 6, 400)}
    assert listed <= {c[1:5] for c in generic}
    assert {9, 16} <= {c.E for c in generic}   # more than 8 members: more problems than one grouped launch holds
    assert {c.geometry for c in tc.CASES} == set(tc.GEOMETRY)
    ids = [tc.case_id(c) for c in tc.CASES]
    assert len(set(ids)) == len(ids)
    for c in tc.CASES:   # a named form is the shape's block counts, and only H % 4 == 0 with even D has one
        if c.form:
            assert c.form == (-(-(c.o + c.a) // 16), -(-c.H // 16), -(-2 * (c.o + 1) // 16))
            assert c.H % 4 == 0 and (c.o + 1) % 2 == 0


@pytest.mark.parametrize('case', tc.CASES, ids=tc.case_id)
def test_case_is_well_conditioned(case):
    mats, X, Y, idxs = tc.case_inputs(case)
    batch = tc.GEOMETRY[case.geometry][1]
    assert len(mats) == 16 and mats[2].shape == (case.E, case.o + case.a, case.H)
    np.testing.assert_allclose(mats[0], X.mean(0, keepdims=True), rtol=1e-6, atol=1e-7)   # the scaler is X's
    t0 = time.perf_counter()
    ref = tc.oracle_steps(mats, X, Y, idxs, batch, np.float64)
    f32 = tc.oracle_steps(mats, X, Y, idxs, batch, np.float32)
    dt = time.perf_counter() - t0
    assert all(v.dtype == np.float64 for v in ref) and all(v.dtype == np.float32 for v in f32)
    ratios = [tc.tol_ratio(g, r) for g, r in zip(f32, ref)]
    k = int(np.argmax(ratios))
    print('%-26s %-9s fp32/fp64 worst d/tol %.4f (%s)  oracle %.2f s'
          % (tc.case_id(case), tc.form_name(case.form), ratios[k], tc.NAMES[k], dt))
    assert len(ratios) == 14 and ratios[k] <= CONDITION, (tc.NAMES[k], ratios[k])
    # the steps moved every variable: a parity test on parameters that stood still would prove nothing
    start = mats[2:]
    for name, s, r in zip(tc.NAMES, start, ref):
        assert np.abs(r.reshape(s.shape) - s).max() > 1e-4, name


@pytest.mark.parametrize('E,o,a,H,named', tc.LOSS_CASES, ids=['E%d-%d+%d-H%d' % c[:4] for c in tc.LOSS_CASES])
def test_loss_case_is_well_conditioned(E, o, a, H, named):
    """The loss value the GPU file compares to rel 1e-5: its two terms have opposite signs, so the sum must not
    cancel -- the fp32 oracle's value stays within 0.1 of that bound of the fp64 one, and the decays and bound
    terms the log leaves out are far larger than the bound (a log that included them would fail)."""
    from oracle import bnn as obnn
    from oracle import bnn_train as ot
    mats, X, Y, idx = tc.loss_inputs(E, o, a, H)
    p = obnn.from_mat_list(mats)
    ref = tc.data_loss(p, X[idx], Y[idx])
    f32 = tc.data_loss(p, X[idx], Y[idx], np.float32)
    full, _ = ot.loss_and_grads(p, X[idx].astype(np.float64), Y[idx].astype(np.float64))
    print('E=%d %d+%d H=%d %s: data loss %.6f, fp32 rel %.2e, full loss %.6f' % (E, o, a, H, tc.form_name(named), ref,
                                                                               abs(f32 - ref) / abs(ref), full))
    assert abs(f32 - ref) <= CONDITION * 1e-5 * abs(ref)
    assert abs(full - ref) > 100 * 1e-5 * abs(ref)
