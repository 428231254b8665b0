"""GPU: the ensemble forward, FakeEnv.step, the fused rollout, evaluate, validate and the actor at every obs / act
block shape of tests/dim_cases.py, against the f64 (FakeEnv: the reference-following f32 / f64) oracle.

The cases, their parameters (spread biases, log-variance bounds different in every column, weights x
dim_cases.FACTOR) and why a kernel that misplaces a feature, a hidden unit or a head column cannot pass them are
in tests/dim_cases.py and tests/test_dim_cases.py.  Which kernel form runs a case is mopo_bnn_forward_form's answer.

Tolerances (the project's own, tests/test_gpu_rollout.py and tests/test_gpu_ref.py):
  * ensemble mean / log-variance:  |d| <= 2e-5 (1 + |ref|) in fp32, bf16x6, f16x3; 2e-3 bf16x3; 3e-2 bf16
  * next_obs / rewards / pool floats:  5e-5 (1 + |ref|);  penalty: rel 1e-5
  * actor pi / mu:  2e-5 (1 + |ref|)
  * member choice, step counts, pool pointer and size, terminals (the rollout cases keep every row 1e-3 away from
    a termination bound: test_dim_cases.py): bit-exact
"""
import itertools

import numpy as np
import pytest

import dim_cases as dc
from oracle import bnn as obnn
from oracle import fake_env as ofe
from oracle import sac as osac

pytestmark = pytest.mark.gpu
WORST = {}


def scaled_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    return float((np.abs(a - b) / (1 + np.abs(b))).max(initial=0))


def note(group, err, tol):
    """Keeps the worst ratio to tolerance per group and prints the figure before the caller asserts."""
    WORST[group] = max(WORST.get(group, 0.0), err / tol)
    return err


def make_model(mats, O, A, H, dtype, E=dc.E, elites=dc.ELITES):
    from mopo_amd.bnn import BNN
    m = BNN({'name': 'dims', 'num_networks': E, 'num_elites': len(elites), 'separate_mean_var': True, 'obs_dim': O,
             'act_dim': A, 'hidden_dim': H, 'dtype': dtype}).set_params(mats)
    m.set_elites(elites)
    return m


# ---- predict ---------------------------------------------------------------------------------------------------------
def _predict_check(c, O, A, H, dtype, label):
    p = c['params']
    model = make_model(c['mats'], O, A, H, dtype)
    tol = dc.TOL[dtype]
    runs = [(c['x'][:B].astype(np.float32), 'B=%d f32' % B) for B in dc.BATCHES] + [(c['x'], 'B=%d f64' % len(c['x']))]
    for x, what in runs:
        mean, var = model.predict(x, factored=True)
        rm, rl = obnn.forward(p, x, dtype=np.float64, ret_log_var=True)
        assert mean.shape == rm.shape == (dc.E, len(x), O + 1) and var.shape == rm.shape
        assert (var > 0).all()
        em, el = scaled_err(mean, rm), scaled_err(np.log(var.astype(np.float64)), rl)
        print('%s %s: mean %.3g, log-var %.3g (x tol: %.3g, %.3g)' % (label, what, em, el, em / tol, el / tol))
        note('predict ' + dtype, max(em, el), tol)
        assert em <= tol and el <= tol, (label, what, em, el)


@pytest.mark.parametrize('O,A,H,dtype', dc.predict_cases(), ids=[dc.case_id(c) for c in dc.predict_cases()])
def test_predict_vs_f64_oracle(O, A, H, dtype):
    _predict_check(dc.case(O, A, H), O, A, H, dtype, dc.case_id((O, A, H, dtype)))


SATURATED = [(O, A, dt) for (O, A) in dc.SATURATED_SHAPES for dt in dc.MAIN_DTYPES]


@pytest.mark.parametrize('O,A,dtype', SATURATED, ids=[dc.case_id(c) for c in SATURATED])
def test_predict_saturated_clamp(O, A, dtype):
    """The log-variance more than 14 above max_logvar in some columns, more than 14 below min_logvar in others:
    both outer branches of the kernels' softplus."""
    _predict_check(dc.case(O, A, 64, saturated=True), O, A, 64, dtype, 'saturated ' + dc.case_id((O, A, 64, dtype)))


# ---- FakeEnv.step ----------------------------------------------------------------------------------------------------
STEP = [(O, A, H, dt) for (O, A) in dc.SHAPES for H in dc.HIDDEN_ALL_SHAPES for dt in dc.MAIN_DTYPES]


@pytest.mark.parametrize('O,A,H,dtype', STEP, ids=[dc.case_id(c) for c in STEP])
def test_fakeenv_step_vs_oracle(O, A, H, dtype):
    from mopo_amd.fake_env import FakeEnv
    from mopo_amd.static import static_fns
    c = dc.case(O, A, H)
    p = c['params']
    model = make_model(c['mats'], O, A, H, dtype)
    x = c['x'].astype(np.float32)
    coeff = 1.5
    for learned_var, det, B in ((True, False, 37), (False, False, 37), (True, True, 37), (False, True, 37),
                                (True, False, 1)):
        obs, act = x[:B, :O], x[:B, O:]
        env = FakeEnv(model, static_fns['halfcheetah'], penalty_coeff=coeff, penalty_learned_var=learned_var)
        np.random.seed(5 + B)
        nobs, rew, term, info = env.step(obs, act, deterministic=det)
        used = np.random.get_state()[1:3]
        np.random.seed(5 + B)
        rn, rr, rt, ri = ofe.step(p, dc.ELITES, obs, act, ofe.term_halfcheetah, penalty_coeff=coeff,
                                  penalty_learned_var=learned_var, deterministic=det)
        # the member choice: numpy's global stream consumed exactly as the oracle (and the reference) consumes it
        assert used[1] == np.random.get_state()[2] and np.array_equal(used[0], np.random.get_state()[1])
        en, er = scaled_err(nobs, rn), scaled_err(rew, rr)
        ep = float((np.abs(info['penalty'] - ri['penalty']) / np.abs(ri['penalty'])).max())
        print('%s lv=%d det=%d B=%d: next_obs %.3g, rewards %.3g (x 5e-5: %.3g), penalty rel %.3g'
              % (dc.case_id((O, A, H, dtype)), learned_var, det, B, en, er, max(en, er) / 5e-5, ep))
        note('step ' + dtype, max(en, er), 5e-5)
        note('step penalty ' + dtype, ep, 1e-5)
        assert en <= 5e-5 and er <= 5e-5 and ep <= 1e-5
        assert scaled_err(info['unpenalized_rewards'], ri['unpenalized_rewards']) <= 5e-5
        assert scaled_err(info['mean'], ri['mean']) <= 5e-5 and scaled_err(info['std'], ri['std']) <= 5e-5
        np.testing.assert_array_equal(term, rt)
        if not det:   # the selected member's own mean is what info['mean'] carries: a wrong member is a large error
            other = ofe.step(p, dc.ELITES, obs, act, ofe.term_halfcheetah, deterministic=False,
                             noise=np.zeros((dc.E, B, O + 1)), model_inds=1 - ri['model_inds'])[3]['mean']
            assert scaled_err(other, ri['mean']) > 100 * 5e-5


# ---- fused rollout ---------------------------------------------------------------------------------------------------
def _run_rollout(c, domain, O, A, H, dtype):
    import torch
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    B, horizon = dc.ROLLOUT_B, dc.ROLLOUT_HORIZON
    model = make_model(c['mats'], O, A, H, dtype, E=dc.ROLLOUT_E, elites=c['elites'])
    dev = torch.device('cuda')
    pool = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=B * horizon + 7)
    ro = ModelRollout(model, B, horizon)
    steps = ro.run(torch.from_numpy(c['env_obs']).to(dev), torch.from_numpy(c['flat']).to(dev), pool, B, horizon,
                   static_fns[domain].term_kind, c['coeff'], c['elites'], start_idx=c['start'], eps_act=c['eps_act'],
                   eps_obs=c['eps_obs'], model_inds=c['inds'])
    return steps.cpu().numpy(), pool, ro, model


@pytest.mark.parametrize('domain,O,A,H,dtype', dc.rollout_cases(), ids=[dc.case_id(c) for c in dc.rollout_cases()])
def test_fused_rollout_parity(domain, O, A, H, dtype):
    c = dc.rollout_case(domain, O, A, H)
    steps, pool, _, _ = _run_rollout(c, domain, O, A, H, dtype)
    exp = np.zeros(dc.ROLLOUT_HORIZON, np.int64)
    exp[:len(c['steps'])] = c['steps']
    np.testing.assert_array_equal(steps, exp)
    op = c['pool']
    assert pool.size == op.size and pool._pointer == op._pointer
    got, ref = pool.return_all_samples(as_numpy=True), op.return_all_samples()
    np.testing.assert_array_equal(got['terminals'], ref['terminals'])
    worst = 0.0
    for k in ('observations', 'actions', 'next_observations', 'rewards'):
        assert got[k].shape == ref[k].shape
        worst = max(worst, scaled_err(got[k], ref[k]))
    print('%s: pool floats %.3g (x 5e-5: %.3g), steps %s' % (dc.case_id((domain, O, A, H, dtype)), worst, worst / 5e-5,
                                                           steps.tolist()))
    note('rollout ' + dtype, worst, 5e-5)
    assert worst <= 5e-5


def test_rollout_refuses_two_observation_rules_on_a_one_observation_model():
    """1 + 1 rolls out under a rule that reads observation 0 alone; walker2d's and hopper's are refused by name."""
    import torch
    from mopo_amd import _lib as L
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout, init_sac_params
    O, A, H, B = 1, 1, 64, 40
    rs = np.random.RandomState(1)
    env = rs.normal(size=(200, O)).astype(np.float32)
    p = obnn.init_params(dc.E, O, A, hidden=H, seed=2, inputs=rs.normal(size=(100, 2)), bias_std=dc.BIAS_STD)
    model = make_model(obnn.to_mat_list(p), O, A, H, 'f16x3')
    dev = torch.device('cuda')
    pool = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=4 * B)
    ro = ModelRollout(model, B, 2)
    args = (torch.from_numpy(env).to(dev), torch.from_numpy(init_sac_params(O, A)).to(dev), pool, B, 2)
    for kind in (1, 2):
        with pytest.raises(L.MopoError, match='obs_dim must be >= 2'):
            ro.run(*args, kind, 1.0, dc.ELITES, seed=3)
    assert pool.size == 0
    steps = ro.run(*args, 4, 1.0, dc.ELITES, seed=3).cpu().numpy()     # humanoid's rule: observation 0 alone
    assert steps[0] == B and pool.size == int(steps.sum())
    assert torch.isfinite(pool.fields['next_observations'][:pool.size]).all()


def test_evaluate_at_pendulum_dims():
    """ModelRollout.evaluate at 3 + 1 under walker2d's rule, sampled policy, against the episode sums rebuilt from
    the oracle pool (tests/test_gpu_model_eval.py's host restatement)."""
    import torch
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    from test_gpu_model_eval import _check_against_pool, _host
    domain, O, A, H = 'walker2d', 3, 1, 64
    c = dc.rollout_case(domain, O, A, H)
    B, T = dc.ROLLOUT_B, dc.ROLLOUT_HORIZON
    for dtype in ('fp32', 'f16x3'):
        model = make_model(c['mats'], O, A, H, dtype, E=dc.ROLLOUT_E, elites=c['elites'])
        dev = torch.device('cuda')
        got = _host(ModelRollout(model, B, 1).evaluate(
            torch.from_numpy(c['env_obs']).to(dev), torch.from_numpy(c['flat']).to(dev), B, T,
            static_fns[domain].term_kind, c['coeff'], c['elites'], start_idx=c['start'], eps_obs=c['eps_obs'],
            model_inds=c['inds'], penalty_learned_var=c['learned_var'], deterministic=c['det'],
            policy_deterministic=False, eps_act=c['eps_act']))
        _check_against_pool(got, c, B, T)
        assert 0 < got['terminated'].sum() and got['lengths'].min() < T


def test_validate_at_pendulum_dims(monkeypatch):
    """ModelRollout.validate at 3 + 1 (never done), K = 5, B in {1, 65, 257}, against the host loop of
    tests/test_gpu_model_val.py over its own kind of dataset."""
    import test_gpu_model_val as tv
    from mopo_amd.rollout import ModelRollout
    monkeypatch.setitem(tv.SHAPES, 'pendulum', (3, 1, 64))
    d = tv._dataset('pendulum')
    assert d['observations'].shape[1] == 3 and d['actions'].shape[1] == 1
    try:
        for dtype in ('fp32', 'f16x3'):
            ro, pool = ModelRollout(tv._model('pendulum', dtype), 257, 1), tv._device_pool(d)
            for B, (learned_var, det) in itertools.product((1, 65, 257), ((True, True), (False, False))):
                key = ('pendulum', B, learned_var, det)
                ref = dict(tv._parity_oracle(*key), starts=tv._starts(d, B))
                got = tv._validate('pendulum', dtype, B, ref, learned_var, det, ro=ro, pool=pool)
                np.testing.assert_array_equal(got['start_rows'], ref['starts'])
                tv._compare(got, ref, 'pendulum %s B=%d' % (dtype, B))
    finally:
        for cache in (tv._POOLS, tv._ORACLES, tv._MODELS):
            for k in [k for k in cache if 'pendulum' in (k if isinstance(k, tuple) else (k,))]:
                del cache[k]


# ---- actor -----------------------------------------------------------------------------------------------------------
ACTOR_SHAPES = ((1, 1), (16, 8), (17, 1), (20, 8), (21, 3), (31, 8), (32, 1))
ACTOR = [(H, dt) for H in (32, 96, 256) for dt in (0, 3, 4)]


@pytest.mark.parametrize('H,dtype', ACTOR, ids=['H%d-dt%d' % c for c in ACTOR])
def test_actor_forward_vs_oracle(H, dtype):
    import torch
    from mopo_amd import _lib as L
    from mopo_amd.rollout import init_sac_params, split_params
    dev = torch.device('cuda')
    for O, A in ACTOR_SHAPES:
        flat = init_sac_params(O, A, H, seed=4)
        rs = np.random.RandomState(H + 3 * O + A)
        flat = flat + (rs.normal(size=flat.shape) * 0.01).astype(np.float32)   # non-zero biases
        P = [p.astype(np.float64) for p in split_params(flat, O, A, H)[:8]]
        obs_all = rs.normal(size=(37, O))
        eps_all = rs.normal(size=(37, A)).astype(np.float32)
        tp = torch.from_numpy(flat).to(dev)
        for B in (1, 37):
            obs, eps = obs_all[:B], eps_all[:B]
            to, te = torch.from_numpy(obs.copy()).to(dev), torch.from_numpy(eps.copy()).to(dev)
            act = torch.full((B, A), float('nan'), device=dev)
            mu = torch.full((B, A), float('nan'), device=dev)
            L.check(L.lib().mopo_actor_forward_dtype(L.ptr(tp), O, A, H, L.ptr(to), 1, B, L.ptr(te), 0, 0, L.ptr(act),
                                                     L.ptr(mu), dtype, L.stream_ptr()))
            ra, rmu = osac.actor_act(P, obs.astype(np.float32).astype(np.float64), eps.astype(np.float64))
            ea, em = scaled_err(act.cpu().numpy(), ra), scaled_err(mu.cpu().numpy(), rmu)
            print('actor %d+%d H=%d dtype %d B=%d: act %.3g, mu %.3g (x 2e-5: %.3g)' % (O, A, H, dtype, B, ea, em,
                                                                                     max(ea, em) / 2e-5))
            note('actor dtype %d' % dtype, max(ea, em), 2e-5)
            assert ea <= 2e-5 and em <= 2e-5, (O, A, B)


# ---- dispatch sweep --------------------------------------------------------------------------------------------------
SWEEP_HIDDEN = (16, 32, 48, 64, 100, 128, 200, 208, 220, 256, 400, 416)


def dispatch_classes(dtype):
    """One representative (O, A, H) -- the smallest -- of every distinct form the form function accepts in a dtype."""
    reps = {}
    for O in range(1, 32):
        for A in range(1, 64 - O + 1):
            for H in SWEEP_HIDDEN:
                form = dc.forward_form(O, A, H, dtype)
                if form is not None:
                    key = form + (H % 16 != 0,)
                    reps[key] = min(reps.get(key, (O + A, H, O, A)), (O + A, H, O, A))
    return sorted((o, a, h) + k[:4] for k, (_, h, o, a) in reps.items())


@pytest.mark.parametrize('dtype', list(dc.DTYPE_IDS))
def test_every_accepted_form_launches(dtype):
    """One predict of B = 5 per (KG0, hidden form, NBO, wide) class of the dtype, whole and partial last hidden
    block apart: a form the form function accepts has a kernel behind it, and its outputs are the oracle's."""
    classes = dispatch_classes(dtype)
    assert len(classes) >= 8
    tol = dc.TOL[dtype]
    for O, A, H, kg0, nbh, nbo, wide in classes:
        rs = np.random.RandomState(O + 64 * A + H)
        fit = rs.normal(size=(100, O + A)) * 1.5 + 0.2
        p = obnn.init_params(1, O, A, hidden=H, seed=3, inputs=fit, bias_std=dc.BIAS_STD)
        x = (rs.normal(size=(5, O + A)) * 1.5 + 0.2).astype(np.float32)
        mean, var = make_model(obnn.to_mat_list(p), O, A, H, dtype, E=1, elites=[0]).predict(x, factored=True)
        assert mean.shape == var.shape == (1, 5, O + 1)
        assert np.isfinite(mean).all() and np.isfinite(var).all() and (var > 0).all()
        rm, rl = obnn.forward(p, x, dtype=np.float64, ret_log_var=True)
        em, el = scaled_err(mean, rm), scaled_err(np.log(var.astype(np.float64)), rl)
        print('%s %d+%d H=%d form (KG0 %d, NBH %d, NBO %d, wide %d): mean %.3g, log-var %.3g'
              % (dtype, O, A, H, kg0, nbh, nbo, wide, em, el))
        assert em <= tol and el <= tol, (O, A, H, kg0, nbh, nbo, wide)


def test_print_worst_ratios():
    """Last in the file: the worst ratio to tolerance per group over the tests that ran before it."""
    for k in sorted(WORST):
        print('worst %-22s %.3g x tol' % (k, WORST[k]))
