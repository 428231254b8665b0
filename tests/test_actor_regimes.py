"""CPU: tests/actor_regimes.py's regimes are what they say, are well conditioned, and show the clip bound.

tests/test_gpu_actor_regimes.py holds the actor kernels to 2e-5 (1 + |ref|) against the fp64 oracle in the clipped
regimes.  That is honest only where fp32 arithmetic alone stays a tenth inside it, which (b) measures with the
oracle run in fp32; and it watches the clamp only if a clamp at another value would miss the bound by far, which
(c) measures.  The scaled regimes are compared with the fp32 actor's own error on the GPU; (d) holds their data to
a conditioning at which that comparison is about the number formats, not about the data's cancellations.
"""
import numpy as np
import pytest

import actor_regimes as ar
from oracle import sac as osac

CASES = [(r, O, A, H) for r in ar.REGIMES for (O, A) in ar.SHAPES for H in ar.WIDTHS]
ids = lambda cs: ['%s-%d+%d-H%d' % c for c in cs]


def test_table():
    assert ar.SHAPES == ((3, 1), (11, 3), (17, 6), (27, 8)) and ar.WIDTHS == (32, 96, 256) and ar.DTYPES == (0, 3, 4)
    assert ar.B == 37 and ar.TOL == 2e-5
    assert set(ar.CLIPPED) == {'upper', 'lower', 'lower100', 'mixed', 'squashed', 'dead'}
    assert set(ar.SCALED) == {'scales-20', 'scales10', 'scales17', 'outlier'}
    assert (osac.LOG_STD_MIN, osac.LOG_STD_MAX) == (-20.0, 2.0)


@pytest.mark.parametrize('regime,O,A,H', CASES, ids=ids(CASES))
def test_regime_is_what_it_says(regime, O, A, H):
    """(a) The class shares: every class a regime names holds at least a quarter of the (row, column) entries,
    every raw log-std lies at least 0.5 from both bounds, and each regime's own promise holds."""
    c = ar.case(regime, O, A, H)
    raw, cls = c['c']['ls_raw'], ar.head_classes(regime, A)
    assert raw.shape == (ar.B, A) and c['flat'].size == sum(int(np.prod(s)) for s in osac.param_shapes(O, A, H))
    above, below = raw > osac.LOG_STD_MAX, raw < osac.LOG_STD_MIN
    if regime in ('upper', 'lower', 'lower100', 'mixed'):
        assert (above == (cls > 0)).all() and (below == (cls < 0)).all()
        for v in set(cls.tolist()):
            assert (cls == v).mean() >= 0.25, v
        assert (cls != 0).any()
        assert min(np.abs(raw - osac.LOG_STD_MAX).min(), np.abs(raw - osac.LOG_STD_MIN).min()) >= 0.5
        if regime == 'lower100':
            assert raw[below].max() < -87.4 and np.exp(np.float32(raw[below].max())) < np.finfo(np.float32).tiny
        if (cls > 0).any():      # the clamp value shows in the action: u is off tanh's plateau on most clipped entries
            assert (np.abs(c['c']['u'][above]) < 3).mean() > 0.75
    elif regime == 'squashed':
        for v in (c['act'], c['mu']):
            assert (np.abs(v) <= 1).all() and np.isfinite(v).all()
        assert (np.abs(np.float32(c['mu'])) == 1).all()              # f32's tanh(12) is 1 exactly
        assert (np.sign(c['mu']) == np.where(np.arange(A) % 2 == 0, 1, -1)).all()
        assert (np.abs(np.float32(c['act'])) == 1).mean() >= 0.25
    elif regime == 'dead':
        assert (c['P'][1] < 0).all()
        assert (c['obs'][:ar.DEAD_ROWS] == 0).all() and (c['c']['h1'][:ar.DEAD_ROWS] == 0).all()
        assert ((c['c']['h1'][ar.DEAD_ROWS:] > 0).sum(1) >= 2).all() and (c['obs'][ar.DEAD_ROWS:] != 0).all()
        assert ((c['c']['h2'][ar.DEAD_ROWS:] > 0).sum(1) >= 2).all()
    elif regime.startswith('scales'):
        s = 2.0 ** int(regime[6:])
        ref = ar.case('scales10', O, A, H)
        # the same function of the same rows, exactly: only the power of two differs between the three
        np.testing.assert_array_equal(c['obs'] / np.float32(s), ref['obs'] / np.float32(2.0 ** 10))
        np.testing.assert_array_equal(c['P'][0] * np.float32(s), ref['P'][0] * np.float32(2.0 ** 10))
        np.testing.assert_array_equal(c['act'], ref['act'])
        far = np.abs(c['obs']).max(1) / np.median(np.abs(c['obs']).max(1))
        assert (far[::7] > 1e3).all() and (np.delete(far, np.s_[::7]) < 1e2).all()
    elif regime == 'outlier':
        for t in (0, 2, 4):
            w = np.abs(c['P'][t])
            assert w.max() >= 4096 * np.sort(w.ravel())[-2]        # one entry, 12 bits above the rest of its matrix
        assert np.isfinite(c['act']).all()


COND = [c for c in CASES if c[0] in ar.CLIPPED]


@pytest.mark.parametrize('regime,O,A,H', COND, ids=ids(COND))
def test_clipped_regimes_are_well_conditioned(regime, O, A, H):
    """(b) upper, lower, squashed, dead (and lower100, mixed): the fp32 oracle within a tenth of 2e-5 (1 + |ref|)."""
    r = ar.fp32_oracle_ratio(regime, O, A, H)
    print('%-9s %d+%d H%-3d fp32/fp64 oracle %.4f of the tolerance' % (regime, O, A, H, r))
    assert r <= ar.CONDITION


SENS = [c for c in CASES if c[0] in ('upper', 'mixed')]


@pytest.mark.parametrize('regime,O,A,H', SENS, ids=ids(SENS))
def test_upper_clip_shows_in_the_action(regime, O, A, H):
    """(c) A clamp at 2.5 or at 1.5 moves the action by at least 100 tolerances on at least a quarter of the
    clipped entries; the rule itself moves none (so the comparison fails where no break is applied)."""
    c = ar.case(regime, O, A, H)
    above = c['c']['ls_raw'] > osac.LOG_STD_MAX
    assert above.any()
    for hi in (None, 2.5, 1.5):
        act, mu = ar.actor(c['P'], c['obs'], c['eps'], hi=hi)
        moved = np.abs(act - c['act']) / (ar.TOL * (1 + np.abs(c['act'])))
        share = (moved[above] >= ar.SENSITIVITY).mean()
        print('%-6s %d+%d H%-3d clamp at %s: %.2f of the clipped entries move >= 100 tol' % (regime, O, A, H, hi or 2.0, share))
        np.testing.assert_array_equal(mu, c['mu'])
        if hi is None:
            assert moved.max() == 0 and not share >= 0.25
        else:
            assert share >= 0.25, (hi, share)
    assert osac.LOG_STD_MAX == 2.0


def test_lower_clip_shows_in_the_action():
    """Below the lower bound std = e^-20 moves u by less than an ulp: the action cannot tell the clamp from its
    absence, only from a clamp high enough to matter.  What the GPU test can and does show there is that the
    action is the oracle's and finite (lower100: where an unclamped expf underflows); the lower bound's value is
    watched by the SAC step (tests/sac_cases.py group G), through logp."""
    c = ar.case('lower', 17, 6, 256)
    below = c['c']['ls_raw'] < osac.LOG_STD_MIN
    np.testing.assert_allclose(c['act'][below], c['mu'][below], rtol=0, atol=1e-7)


SCALED = [c for c in CASES if c[0] in ar.SCALED]


def test_scaled_regimes_are_well_conditioned():
    """(d) The scaled regimes amplify rounding by the data's luck; the relative rule of the GPU test binds on the
    16-bit formats only where fp32 rounding alone stays within SCALED_CONDITION of 2e-5 (actor_regimes.SEEDS:
    a case that does not gets another data seed).  There the fp32 actor is held to 2e-5 outright as well."""
    rs = {c: ar.fp32_oracle_ratio(*c) for c in SCALED}
    for c, r in rs.items():
        print('%-9s %d+%d H%-3d fp32/fp64 oracle %8.4f of the tolerance' % (c + (r,)))
    assert ar.SCALED_CONDITION <= ar.CONDITION
    assert max(rs.values()) <= ar.SCALED_CONDITION, max(rs, key=rs.get)
    # the table names only cases whose default seed is not conditioned, and the first seed above it that is
    for (fam, O, A, H), seed in ar.SEEDS.items():
        regs = [r for r in ar.SCALED if ar.family(r) == fam]
        d = ar.default_seed(O, A, H)
        assert regs and seed > d
        for s in range(d, seed):
            assert max(ar.fp32_oracle_ratio(r, O, A, H, s) for r in regs) > ar.SEED_SEARCH, (fam, O, A, H, s)


def test_rollout_policy_is_saturated_at_every_step():
    """The ring actor's rollout (actor_regimes.rollout_case): at both steps the 'mixed' classes hold on every
    row, 0.5 from the bounds, and the upper entries' actions are off tanh's plateau."""
    from mopo_amd.rollout import split_params
    c = ar.rollout_case()
    r = ar.ROLLOUT
    assert c['steps'] == [r['B']] * r['horizon'] and r['B'] < 4096
    P = [p.astype(np.float64) for p in split_params(c['flat'], 17, 6)[:8]]
    obs = c['pool'].return_all_samples()['observations']
    assert obs.shape == (r['B'] * r['horizon'], 17)
    eps = c['eps_act'].reshape(-1, 6).astype(np.float64)
    _, act, _, _, cache = osac.pi_forward(P, obs.astype(np.float32).astype(np.float64), eps)
    raw, cls = cache['ls_raw'], ar.head_classes('mixed', 6)
    assert ((raw > osac.LOG_STD_MAX) == (cls > 0)).all() and ((raw < osac.LOG_STD_MIN) == (cls < 0)).all()
    assert min(np.abs(raw - osac.LOG_STD_MAX).min(), np.abs(raw - osac.LOG_STD_MIN).min()) >= 0.5
    assert (np.abs(cache['u'][:, cls > 0]) < 3).mean() > 0.75
    np.testing.assert_allclose(act, c['pool'].return_all_samples()['actions'], rtol=0, atol=1e-6)
    for hi in (2.5, 1.5):           # a clamp elsewhere moves a quarter of the clipped actions by 100 x 5e-5 (1 + |ref|)
        moved, _ = ar.actor(P, obs.astype(np.float32), eps, hi=hi)
        far = np.abs(moved - act) / (5e-5 * (1 + np.abs(act))) >= ar.SENSITIVITY
        assert far[:, cls > 0].mean() >= 0.25, hi
