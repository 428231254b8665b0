"""CPU: tests/sac_cases.py holds the shapes it promises, and every case is well conditioned.

tests/test_gpu_sac_shapes.py holds csrc/sac.hip to the SAC tolerances of tests/test_gpu_sac.py (gradients within
1e-4 max|g| + 1e-7 per tensor, ...) against the fp64 oracle.  Those bounds are honest only where fp32 arithmetic
alone stays far inside them: a relu pre-activation, the min(Q1, Q2) selection or a log-std clip that sits within
rounding of its kink decides differently in fp32, and then a correct kernel misses the bound by two orders of
magnitude.  Here the oracle itself runs each case once in fp64 and once in fp32 on the same inputs; the two must
agree to CONDITION of every GPU tolerance, and the two discrete decisions must keep a margin.  A case that does
not gets another data seed in sac_cases.py, never a looser bound.
"""
import numpy as np
import pytest

import sac_cases as sc

CONDITION = 0.1   # fp32 oracle vs fp64 oracle, in units of the GPU tolerance (test_train_cases.py's bound)
SENSITIVITY = 100.0   # a broken rule vs the rule, in the same units (test_dim_cases.py (c))


def test_case_table_names_every_width_and_edge():
    A, B, C, D, E = (sc.by_group(g) for g in 'ABCDE')
    sq = {c.hidden: (c.o, c.a, c.n) for c in A if np.isscalar(c.hidden)}
    assert sq == {16: (1, 1, 1), 32: (31, 8, 16), 48: (11, 3, 17), 64: (17, 6, 15), 80: (11, 3, 100), 96: (27, 8, 40),
                  112: (17, 6, 33), 128: (8, 8, 64), 144: (17, 6, 257), 160: (31, 1, 48), 176: (11, 3, 31),
                  192: (24, 8, 100), 208: (17, 6, 250), 224: (3, 2, 130), 240: (31, 8, 1000), 256: (17, 6, 1024)}
    assert {sc.device_width(c.hidden) for c in A} == set(range(16, 257, 16))          # all 16 device widths
    assert {c.hidden for c in A if not np.isscalar(c.hidden)} == {(200, 48), (16, 256), (100, 100)}
    assert all((c.o, c.a, c.n) == (11, 3, 100) for c in A if not np.isscalar(c.hidden))
    assert sc.device_width((100, 100)) == 112 and sc.device_width((200, 48)) == 208
    one = A + B
    assert {c.o + c.a > 31 for c in one} == {False, True}                             # narrow and wide layer 1
    assert min(c.o + c.a for c in one if c.o + c.a > 31) == 32
    assert {0, 1, 15} <= {c.n % 16 for c in one}
    assert {-(-c.n // sc.WG_KC) for c in one} == {1, 2, 3, 4}                         # weight-gradient K passes
    assert {c.n % sc.WG_KC == 0 for c in one if c.n > sc.WG_KC} == {False, True}      # full / partial last chunk
    assert any(-(-c.n // 16) > 32 for c in one) and any(16 < -(-c.n // 16) <= 32 for c in one)
    assert {(c.o, c.a, c.hidden, c.n) for c in B if c.prior == 'uniform'} == \
        {(17, 6, 256, n) for n in (257, 511, 512, 513, 768, 769, 1024)} | {(11, 3, 80, n) for n in (272, 528, 1023)} | \
        {(27, 8, 256, 513), (27, 8, 256, 1024), (3, 1, 16, 1024)}
    assert [(c.o, c.a, c.hidden, c.n) for c in B if c.prior == 'normal'] == [(17, 6, 256, 513)]
    assert all(c.steps == 0 and c.n_env == int(c.n * 0.05) for c in one)
    # the pool split: perf mode, 3 steps
    assert [(c.o, c.a, c.hidden, c.n, c.n_env) for c in C] == \
        [(17, 6, 64, 40, 0), (17, 6, 64, 40, 40), (11, 3, 48, 17, 1), (17, 6, 256, 300, 150)]
    assert [sc.real_ratio(c) for c in C][:2] == [0.0, 1.0] and sc.real_ratio(C[3]) == 0.5
    assert all(c.steps == 3 for c in C)
    for c in sc.CASES:
        assert int(c.n * sc.real_ratio(c)) == c.n_env, sc.case_id(c)
    # perf-mode steps; K may be lowered for conditioning, not below 4
    assert [(c.o, c.a, c.hidden, c.n) for c in D] == \
        [(17, 6, 256, 1024), (11, 3, 80, 528), (27, 8, 256, 1000), (11, 3, (48, 200), 300), (3, 1, 16, 1), (11, 3, 64, 16),
         (11, 3, 32, 9)]
    assert all(4 <= c.steps <= 10 for c in D)
    single = [c for c in D if -(-sc.device_width(c.hidden) // 64) * -(-c.n // 16) < 2]   # one B1 block
    assert len(single) == 3
    assert [(c.o, c.a, c.hidden, c.n, c.head) for c in E] == \
        [(17, 6, 256, 1024, ''), (27, 8, 240, 1000, ''), (11, 3, 80, 528, ''), (17, 6, 64, 40, 'even')]
    # saturated heads: nowhere but in G and its copy in E
    G = sc.by_group('G')
    assert [(c.o, c.a, c.hidden, c.n, c.head, c.prior, c.steps) for c in G] == \
        [(3, 1, 16, 17, 'upper', 'uniform', 0), (3, 1, 16, 17, 'lower', 'uniform', 0), (11, 3, 64, 40, 'mixed', 'uniform', 0),
         (17, 6, 256, 100, 'mixed', 'uniform', 0), (17, 6, 256, 100, 'cross', 'uniform', 0),
         (27, 8, 96, 40, 'mixed', 'normal', 0), (17, 6, 256, 513, 'mixed', 'uniform', 0),
         (11, 3, (48, 200), 100, 'mixed', 'uniform', 0), (17, 6, 64, 40, 'even', 'uniform', 3)]
    assert all(c.n_env == int(c.n * 0.05) for c in G)
    assert [c for c in sc.CASES if c.head and c.group != 'G'] == [G[-1]._replace(group='E', steps=0)]
    assert all(c.head in sc.HEAD_MODES for c in G)
    assert max(-(-c.n // sc.WG_KC) for c in G) == 3                                   # the clamp recomputed per chunk
    assert len(sc.REFUSALS) == 4
    ids = [sc.case_id(c) for c in sc.CASES]
    assert len(set(ids)) == len(ids)


def _check_margins(margins):
    dq, qmax, clip = margins
    assert dq > 1e-5 * (1 + qmax), 'min |Q1(s,pi) - Q2(s,pi)| %.3g: the min-Q selection may flip' % dq
    assert clip > 1e-5, 'a raw log-std lies %.3g from a clip bound' % clip


@pytest.mark.parametrize('case', sc.by_group('A', 'B', 'C', 'G'), ids=sc.case_id)
def test_one_step_is_well_conditioned(case):
    ci, ref = sc.reference_step(case)
    f32 = sc.oracle_step(ci, np.float32)
    assert all(np.array_equal(p, p.astype(np.float32)) for p in ci['params'])
    assert len(ref['grads']) == 20 and ref['params'].size == sc.flat(ci['params']).size + 1
    ratios = sc.step_ratios(f32, ref)
    name, w = sc.worst(ratios)
    print('%-34s fp32/fp64 worst d/tol %.4f (%s)  min|dQ| %.2e clip %.2e' % ((sc.case_id(case), w, name) + ref['margins'][::2]))
    assert w <= CONDITION, (name, w)
    _check_margins(ref['margins'])
    if case.n_env in (0, case.n):    # the unused pool is NaN: the oracle never reads it either
        assert all(np.isfinite(v) for v in ref['logs'].values())
    # the step moved the parameters: a parity test on parameters that stood still would prove nothing
    assert np.abs(ref['params'][:-1] - sc.flat(ci['params'])).max() > 0.5 * sc.LR_T


@pytest.mark.parametrize('case', [c for c in sc.by_group('C', 'D', 'G') if c.steps], ids=sc.case_id)
def test_perf_steps_are_well_conditioned(case):
    ref = sc.reference_steps(case)
    f32 = sc.oracle_steps(case, dtype=np.float32)
    np.testing.assert_array_equal(f32['idx'], ref['idx'])
    assert ref['idx'].shape == (case.steps, case.n)
    ratios = sc.multi_ratios(f32, ref)
    name, w = sc.worst(ratios)
    print('%-34s K=%d fp32/fp64 worst d/tol %.4f (%s)' % (sc.case_id(case), case.steps, w, name))
    assert w <= CONDITION, (name, w)
    assert all(np.isfinite(v) for v in ref['logs'].values())


def _raw_of_every_step(case):
    """The raw log-std of pi(s) and pi(s') [steps, 2, n, a] (fp64 oracle, pre-step parameters) and the noise
    of the injected step."""
    ci, ref = sc.reference_step(case)
    raw = sc.reference_steps(case)['ls_raw'] if case.steps else ref['ls_raw'][None]
    if case.steps:
        np.testing.assert_array_equal(raw[0], ref['ls_raw'])
    assert raw.shape == (max(case.steps, 1), 2, case.n, case.a)
    return ci, raw


@pytest.mark.parametrize('case', sc.by_group('G'), ids=sc.case_id)
def test_saturated_heads_hold_their_classes(case):
    """Group G, over pi(s) and pi(s') of every step: (a) every class the mode names holds at least a quarter of
    the (row, column) entries ('cross': of the rows of the crossing column, on each side); (b) every raw value
    lies at least CLIP_MARGIN from both bounds; (c) below the lower bound the noise is exactly 0, elsewhere it
    is not."""
    ci, raw = _raw_of_every_step(case)
    lo, hi = sc.osac.LOG_STD_MIN, sc.osac.LOG_STD_MAX
    assert (lo, hi) == (-20.0, 2.0)
    cls = sc.head_classes(case)
    above, below = raw > hi, raw < lo
    print('%-36s raw in [%.2f, %.2f], nearest to a bound %.2f; above %.2f below %.2f of the entries' % (
        sc.case_id(case), raw.min(), raw.max(), min(np.abs(raw - lo).min(), np.abs(raw - hi).min()),
        above.mean(), below.mean()))
    assert min(np.abs(raw - lo).min(), np.abs(raw - hi).min()) >= sc.CLIP_MARGIN                 # (b)
    if case.head == 'cross':
        col = raw[:, :, :, sc.CROSS_COL]
        for k in range(raw.shape[0]):
            for side in range(2):                                                                  # (a)
                assert 0.25 <= (col[k, side] > hi).mean() <= 0.75, (k, side)
        assert not below.any() and raw.min() >= -sc.INSIDE
        assert not np.delete(above, sc.CROSS_COL, axis=3).any()
    else:
        assert set(cls.tolist()) == {'upper': {1}, 'lower': {-1}, 'mixed': {1, -1, 0}, 'even': {1, 0}}[case.head]
        for v in set(cls.tolist()):                                                                # (a)
            assert (cls == v).mean() >= 0.25, v
        # the class of a column is the class of each of its entries, at every step
        assert (above == (cls > 0)).all() and (below == (cls < 0)).all()
        assert np.abs(raw[..., cls == 0]).max(initial=0) <= 2.0          # 'inside' stays where std is not tiny
    if not case.steps:
        for e, b in ((ci['eps_s'], below[0, 0]), (ci['eps_n'], below[0, 1])):                     # (c)
            assert (e[b] == 0).all() and (e[~b] != 0).all()
    else:
        assert not below.any()


@pytest.mark.parametrize('case', sc.by_group('G'), ids=sc.case_id)
def test_saturated_heads_tell_the_rule_from_its_mutations(case):
    """Group G (d): the fp64 oracle re-run with the clip rule broken -- no forward clamp, each bound moved by 0.5
    either way, no gradient mask, the mask on one side only -- moves at least one compared quantity by at
    least SENSITIVITY times its tolerance (the figure dim_cases.FACTOR was chosen by), and the unbroken re-run
    moves none at all: a kernel with any of these mutations fails the GPU comparison outright.  The perf-mode
    case is measured on its first step in the one-step units: three Adam steps cannot move a parameter by 100
    times the several-step bound (1e-2), so the several-step comparison sees a broken mask only through
    exact_zero_columns' assertions in tests/test_gpu_sac_shapes.py."""
    ci, ref = sc.reference_step(case)
    same = sc.step_ratios(sc.oracle_step(ci), ref)
    assert sc.worst(same)[1] == 0.0
    assert not sc.worst(same)[1] >= SENSITIVITY           # the assertion below fails where no break is applied
    names = sc.breaks_of(case)
    assert {'no clamp', 'no mask'} < set(names) and len(names) in (5, 8)
    if case.head == 'mixed':
        assert len(names) == len(sc.BREAKS)
    for name in names:
        moved = sc.step_ratios(sc.oracle_step(ci, rule=sc.BREAKS[name][0]), ref)
        k, w = sc.worst(moved)
        print('%-36s %-18s moves %s by %.3g tolerances' % (sc.case_id(case), name, k, w))
        assert w >= SENSITIVITY, (name, k, w)
    assert (sc.osac.LOG_STD_MIN, sc.osac.LOG_STD_MAX) == (-20.0, 2.0)      # broken_rule put the bounds back


def test_fp64_oracle_is_unchanged_by_the_dtype_argument():
    """SACState's default stays fp64 end to end, and an fp32 run really is fp32 (oracle_step asserts it)."""
    c = sc.by_group('A')[2]
    ci, ref = sc.reference_step(c)
    assert ref['params'].dtype == np.float64 and all(g.dtype == np.float64 for g in ref['grads'])
    f32 = sc.oracle_step(ci, np.float32)
    assert f32['params'].dtype == np.float32 and all(g.dtype == np.float32 for g in f32['grads'])
    assert not np.array_equal(f32['params'], ref['params'])
