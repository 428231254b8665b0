"""GPU: the penalty kinds max_pairwise and ensemble_std (csrc/penalty.hip) through every caller.

The reference is tests/penalty_kinds.py: the definitions in numpy f64 and the shared cases (H = 32, members with
spread-out biases; tests/test_penalty_kinds.py shows on the CPU that every case tells the four kinds apart by
more than 100 x the tolerance used here).  Tolerances:
  * the kernel against f64 on the device's own member outputs:  rel 1e-5 (the project's penalty tolerance)
  * against the f64 oracle:  |u - u_ref| <= 2 sqrt(D) 2e-5 (1 + max |ref|)  (penalty_kinds.oracle_bound: derived)
  * next_obs / rewards / penalized rewards:  5e-5 (1 + |ref|); integer work and the old kinds: bit-exact
"""
import ctypes as C

import numpy as np
import pytest

import penalty_kinds as pk

pytestmark = pytest.mark.gpu
NEW_KINDS = ('max_pairwise', 'ensemble_std')


def make_model(mats, E, O, A, smv=True, dtype='fp32'):
    from mopo_amd.bnn import BNN
    m = BNN({'name': 't', 'num_networks': E, 'num_elites': min(5, E), 'separate_mean_var': smv, 'obs_dim': O,
             'act_dim': A, 'hidden_dim': pk.H, 'dtype': dtype})
    m.set_params(mats)
    m.set_elites([4, 1, 0, 6, 2][:min(5, E)] if E >= 7 else list(range(E)))
    return m


def close(a, b, tol=5e-5):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b) / (1 + np.abs(b))
    assert err.max(initial=0) <= tol, 'max scaled err %.3g > %.3g' % (err.max(), tol)


# ---- 1. the kernel's arithmetic alone --------------------------------------------------------------------------
def _c_step(model, obs, act, kind, coeff=1.0):
    """mopo_fakeenv_step (deterministic) with caller-owned member outputs; returns d_penalty, d_ens_mean, d_ens_var."""
    import torch
    from mopo_amd import _lib as L
    dev = torch.device('cuda')
    B, E, O = len(obs), model.num_nets, model.obs_dim
    o, a = torch.from_numpy(obs).to(dev), torch.from_numpy(act).to(dev)
    nobs = torch.empty((B, O), dtype=torch.float64, device=dev)
    rew = torch.empty(B, dtype=torch.float64, device=dev)
    term = torch.empty(B, dtype=torch.uint8, device=dev)
    pen = torch.full((B,), -1.0, dtype=torch.float32, device=dev)
    em = torch.empty((E, B, O + 1), dtype=torch.float32, device=dev)
    ev = torch.empty((E, B, O + 1), dtype=torch.float32, device=dev)
    args = L.FakeEnvArgs(d_obs=L.ptr(o), obs_f64=0, d_act=L.ptr(a), B=B, deterministic=1, penalty_coeff=coeff,
                         penalty_learned_var=kind, term_kind=0, d_next_obs=L.ptr(nobs), d_rewards=L.ptr(rew),
                         d_terminals=L.ptr(term), d_penalty=L.ptr(pen), d_ens_mean=L.ptr(em), d_ens_var=L.ptr(ev))
    L.check(L.lib().mopo_fakeenv_step(model.handle, args, L.stream_ptr()))
    torch.cuda.synchronize()
    return pen.cpu().numpy(), em.cpu().numpy(), ev.cpu().numpy()


def _c_penalty(params, obs, act, kind):
    """mopo_penalty_from_predictions on the oracle's f32 member outputs (the same kernel, the predict layout)."""
    import torch
    from mopo_amd import _lib as L
    from oracle import bnn as obnn
    mean, var = obnn.forward(params, np.concatenate([obs, act], 1))
    dev = torch.device('cuda')
    em, ev = torch.from_numpy(np.ascontiguousarray(mean)).to(dev), torch.from_numpy(np.ascontiguousarray(var)).to(dev)
    E, B, D = mean.shape
    pen = torch.full((B,), -1.0, dtype=torch.float32, device=dev)
    L.check(L.lib().mopo_penalty_from_predictions(kind, L.ptr(em), L.ptr(ev), E, D - 1, B, L.ptr(pen), L.stream_ptr()))
    torch.cuda.synchronize()
    return pen.cpu().numpy(), mean, var


@pytest.mark.parametrize('smv', pk.KERNEL_SMV, ids=['smv', 'joint'])
@pytest.mark.parametrize('OA', pk.KERNEL_OA, ids=lambda oa: 'O%d' % oa[0])
@pytest.mark.parametrize('E', pk.KERNEL_E)
def test_kernel_against_f64_on_the_device_outputs(E, OA, smv):
    """Through mopo_fakeenv_step on the device's own member outputs, at every shape ((3, 1), D = 4, runs on a
    two-block head: mopo_bnn_forward_form).  At (3, 1) the same kernel is also reached through
    mopo_penalty_from_predictions, on the oracle's f32 forward of the same weights in the predict layout."""
    O, A = OA
    c = pk.kernel_case(E, O, A, smv)
    model = make_model(c['mats'], E, O, A, smv=smv)
    for B in pk.KERNEL_B:
        for kind in (2, 3):
            runs = [_c_step(model, c['obs'][:B], c['act'][:B], kind)]
            if O + 1 < 9:
                runs.append(_c_penalty(c['params'], c['obs'][:B], c['act'][:B], kind))
            for pen, em, ev in runs:
                ref = pk.penalty(kind, em, ev)
                err = np.abs(pen - ref) / np.where(ref > 0, ref, 1)
                print('E=%d O=%d smv=%d B=%d kind=%d: max rel err %.3g' % (E, O, smv, B, kind, err.max()))
                assert (pen >= 0).all() and err.max() <= pk.KERNEL_RTOL
                if E == 1 and kind == 2:
                    assert not pen.any()
                if E > 1:   # and not the penalty the field's old reading gave (any non-zero value: max_aleatoric)
                    old = pk.penalty(1, em, ev)
                    assert np.mean(np.abs(pen - old) > 100 * pk.KERNEL_RTOL * old) >= 0.9


# ---- 2. FakeEnv.step against the f64 oracle ----------------------------------------------------------------------
@pytest.mark.parametrize('kind', NEW_KINDS)
@pytest.mark.parametrize('dtype', ['fp32', 'bf16x6', 'f16x3'])
def test_fakeenv_step_against_the_f64_oracle(dtype, kind):
    from mopo_amd.fake_env import FakeEnv
    from mopo_amd.static import static_fns
    c = pk.step_case()
    E, O, A = (pk.STEP_SHAPE[k] for k in 'EOA')
    model = make_model(c['mats'], E, O, A, dtype=dtype)
    lam = 1.5
    env = FakeEnv(model, static_fns['walker2d'], penalty_coeff=lam, penalty_kind=kind)
    obs = c['obs'].astype(np.float64)
    nobs, rew, term, info = env.step(obs, c['act'], noise=c['noise'], model_inds=c['inds'])
    ref = pk.penalty(kind, c['mean'], c['var'])
    bound = pk.oracle_bound(c['mean'], c['var'])
    err = np.abs(info['penalty'].ravel() - ref)
    print('%s %s: max |u - u_ref| / bound = %.3g' % (dtype, kind, (err / bound).max()))
    assert (err <= bound).all()
    close(rew, info['unpenalized_rewards'] - lam * info['penalty'].astype(np.float64))
    env0 = FakeEnv(model, static_fns['walker2d'], penalty_coeff=0.0, penalty_kind=kind)
    nobs0, rew0, term0, info0 = env0.step(obs, c['act'], noise=c['noise'], model_inds=c['inds'])
    np.testing.assert_array_equal(nobs, nobs0)
    np.testing.assert_array_equal(term, term0)
    np.testing.assert_array_equal(info['mean'], info0['mean'])
    np.testing.assert_array_equal(info['unpenalized_rewards'], rew0)
    assert info0['penalty'] is None


# ---- 3. the fused rollout, parity mode -----------------------------------------------------------------------
def _run_rollout(c, det, **kw):
    import torch
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    dev = torch.device('cuda')
    O, A, B, h = c['O'], c['A'], c['B'], c['horizon']
    model = make_model(c['mats'], pk.ROLLOUT_E, O, A)
    pool = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=B * h + 7)
    ro = ModelRollout(model, B, h)
    steps = ro.run(torch.from_numpy(c['env_obs']).to(dev), torch.from_numpy(c['flat']).to(dev), pool, B, h,
                   static_fns[c['domain']].term_kind, kw.pop('coeff', 1.0), c['elites'], start_idx=c['start'],
                   eps_act=c['eps_act'], eps_obs=c['eps_obs'], model_inds=c['inds'], deterministic=det, **kw)
    return steps.cpu().numpy(), pool


@pytest.mark.parametrize('kind', NEW_KINDS)
@pytest.mark.parametrize('det', [False, True], ids=['sampled', 'det'])
@pytest.mark.parametrize('name', sorted(pk.ROLLOUT_CASES))
def test_fused_rollout_parity(name, det, kind):
    c = pk.rollout_case(name, det)
    lam = 1.0
    steps, pool = _run_rollout(c, det, coeff=lam, penalty_kind=kind)
    exp = np.zeros(c['horizon'], np.int64)
    exp[:len(c['steps'])] = c['steps']
    np.testing.assert_array_equal(steps, exp)
    op, ref = c['pool'], c['ref']
    assert pool.size == op.size and pool._pointer == op._pointer
    got = pool.return_all_samples(as_numpy=True)
    np.testing.assert_array_equal(got['terminals'], ref['terminals'])
    np.testing.assert_array_equal(got['observations'][:c['B']], c['env_obs'][c['start']])     # the start rows
    for k in ('observations', 'actions', 'next_observations'):
        close(got[k], ref[k])
    u = pk.penalty(kind, c['mean'], c['var'])
    want = np.asarray(ref['rewards'], np.float64).ravel() - lam * u
    tol = 5e-5 * (1 + np.abs(want)) + lam * pk.oracle_bound(c['mean'], c['var'])
    err = np.abs(got['rewards'].ravel() - want)
    print('%s det=%d %s: max err / tol = %.3g' % (name, det, kind, (err / tol).max()))
    assert (err <= tol).all()


# ---- 4. the old kinds, by name: bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize('name,learned_var', [('max_aleatoric', True), ('mean_distance', False)])
def test_old_kinds_by_name_are_bit_identical(name, learned_var):
    from mopo_amd.fake_env import FakeEnv
    from mopo_amd.static import static_fns
    for case, det in (('halfcheetah-4096', False), ('walker2d-300', False), ('walker2d-300', True)):
        c = pk.rollout_case(case, det)
        s1, p1 = _run_rollout(c, det, coeff=2.0, penalty_kind=name)
        s0, p0 = _run_rollout(c, det, coeff=2.0, penalty_learned_var=learned_var)
        np.testing.assert_array_equal(s1, s0)
        a, b = p1.return_all_samples(as_numpy=True), p0.return_all_samples(as_numpy=True)
        for k in a:
            np.testing.assert_array_equal(a[k].view(np.uint8), b[k].view(np.uint8), err_msg=k)
    c = pk.step_case()
    model = make_model(c['mats'], *(pk.STEP_SHAPE[k] for k in 'EOA'))
    outs = []
    for kw in (dict(penalty_kind=name), dict(penalty_learned_var=learned_var)):
        env = FakeEnv(model, static_fns['walker2d'], penalty_coeff=2.0, **kw)
        nobs, rew, term, info = env.step(c['obs'], c['act'], noise=c['noise'], model_inds=c['inds'])
        outs.append(dict(info, next_obs=nobs, rew=rew, term=term))
    for k in outs[0]:
        np.testing.assert_array_equal(outs[0][k], outs[1][k], err_msg=k)


# ---- 5. evaluate ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', NEW_KINDS)
def test_evaluate_equals_the_host_loop(kind):
    """64 episodes x 5 steps of tanh(mu) on halfcheetah against DevicePolicy.actions + FakeEnv.step under the same
    kind with the same injected FakeEnv streams: the penalized returns at 5e-5 sum_t (1 + |r_t|), the penalty
    sums at 5e-5 sum_t (1 + u_t) (the same rule: r - u is held to it)."""
    import torch
    from mopo_amd.evaluation import DevicePolicy
    from mopo_amd.fake_env import FakeEnv
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    c = pk.rollout_case('halfcheetah-300', False)
    B, T, E, O, A = 64, 5, pk.ROLLOUT_E, c['O'], c['A']
    model = make_model(c['mats'], E, O, A)
    dev = torch.device('cuda')
    pi = torch.from_numpy(c['flat']).to(dev)
    env = FakeEnv(model, static_fns['halfcheetah'], penalty_coeff=1.0, penalty_kind=kind)
    policy = DevicePolicy(pi, O, A, 256)
    rs = np.random.RandomState(77)
    start = c['start'][:B]
    obs = c['env_obs'][start].astype(np.float64)
    eps_obs, inds_all = np.zeros((T, B, O + 1)), np.zeros((T, B), np.int32)
    pret, psum, scale, uscale = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros(B)
    for i in range(T):
        act = policy.actions(obs)
        noise, inds = rs.normal(size=(E, B, O + 1)), rs.choice(c['elites'], size=B)
        obs, rew, term, info = env.step(obs, act, noise=noise, model_inds=inds)
        eps_obs[i], inds_all[i] = noise[inds, np.arange(B)], inds
        u = info['penalty'].ravel().astype(np.float64)
        pret += rew.ravel(); psum += u
        scale += 1 + np.abs(info['unpenalized_rewards'].ravel()); uscale += 1 + u
    out = ModelRollout(model, B, 1).evaluate(torch.from_numpy(c['env_obs']).to(dev), pi, B, T, 0, 1.0, c['elites'],
                                            policy_deterministic=True, start_idx=start, eps_obs=eps_obs,
                                            model_inds=inds_all, penalty_kind=kind)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert (got['lengths'] == T).all()
    e1, e2 = np.abs(got['penalty_sums'] - psum) / uscale, np.abs(got['penalized_returns'] - pret) / scale
    print('%s: penalty sums %.3g, penalized returns %.3g (of 5e-5)' % (kind, e1.max(), e2.max()))
    assert e1.max() <= 5e-5 and e2.max() <= 5e-5
    np.testing.assert_allclose(got['returns'] - got['penalty_sums'], got['penalized_returns'], rtol=0,
                               atol=1e-9 * scale.max())


# ---- 6. validate ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', NEW_KINDS)
def test_validate_tables_and_correlation(kind):
    """64 segments x 4 steps on a synthetic trajectory pool (episodes of 4 rows, next_obs[j] == obs[j + 1] bit for
    bit inside an episode): the [K][B] penalty table is FakeEnv.step's penalty per step (deterministic, fed its
    own predictions) at 5e-5 (1 + u), and penalty-error-corr is Pearson's coefficient with err_obs for
    max_pairwise, with err for ensemble_std, recomputed from the returned tables."""
    import torch
    from mopo_amd.fake_env import FakeEnv
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    c = pk.rollout_case('halfcheetah-300', False)
    B, K, E, O, A = 64, 4, pk.ROLLOUT_E, c['O'], c['A']
    rs = np.random.RandomState(9)
    chain = (rs.normal(size=(B, 1, O)) + np.cumsum(rs.normal(size=(B, K + 1, O)) * 0.05, 1)).astype(np.float32)
    term = np.zeros((B, K), np.uint8)
    term[:, -1] = 1
    data = {'observations': chain[:, :-1].reshape(-1, O), 'next_observations': chain[:, 1:].reshape(-1, O),
            'actions': rs.uniform(-1, 1, (B * K, A)).astype(np.float32),
            'rewards': rs.normal(size=(B * K, 1)).astype(np.float32), 'terminals': term.reshape(-1)}
    pool = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=B * K)
    pool.add_samples(data)
    model = make_model(c['mats'], E, O, A)
    starts = np.arange(B) * K
    out = ModelRollout(model, B, 1).validate(pool, B, K, 0, c['elites'], start_idx=starts, penalty_kind=kind)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert (got['lengths'] == K).all() and not got['end_reasons'].any()
    env = FakeEnv(model, static_fns['halfcheetah'], penalty_coeff=1.0, penalty_kind=kind)
    other = FakeEnv(model, static_fns['halfcheetah'], penalty_coeff=1.0, penalty_learned_var=True)
    obs = data['observations'][starts].astype(np.float64)
    for k in range(K):
        act = data['actions'][starts + k]
        old = other.step(obs, act, deterministic=True)[3]['penalty'].ravel()
        obs, _, _, info = env.step(obs, act, deterministic=True)
        u = info['penalty'].ravel().astype(np.float64)
        assert (np.abs(got['penalties'][k] - u) <= 5e-5 * (1 + u)).all(), k
        assert np.mean(np.abs(u - old) > 100 * 5e-5 * (1 + u)) >= 0.9      # not the field's old reading
    u = got['penalties'].astype(np.float64).ravel()
    e = (got['obs_errors'] if kind == 'max_pairwise' else got['errors']).ravel()
    corr = np.corrcoef(u, e)[0, 1]
    print('%s: penalty-error-corr device %.12g numpy %.12g' % (kind, got['stats'][K, 8], corr))
    assert abs(got['stats'][K, 8] - corr) <= 1e-9
    wrong = np.corrcoef(u, (got['errors'] if kind == 'max_pairwise' else got['obs_errors']).ravel())[0, 1]
    assert abs(wrong - corr) > 1e-6                                         # the two errors are told apart
    assert got['stats'][K, 9] == np.mean(u >= e)


# ---- 7. MOPO ------------------------------------------------------------------------------------------------------
def _mopo(coeff):
    import torch
    from mopo_amd.mopo import MOPO
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.static import static_fns
    rs = np.random.RandomState(2)
    n = 3000
    obs = rs.normal(size=(n, 17)).astype(np.float32)
    pool = SimpleReplayPool(obs_dim=17, act_dim=6, max_size=n)
    pool.add_samples({'observations': obs, 'actions': rs.uniform(-1, 1, (n, 6)), 'rewards': rs.normal(size=(n, 1)),
                      'terminals': np.zeros((n, 1), bool), 'next_observations': obs + 0.1})
    np.random.seed(123)
    algo = MOPO(pool, static_fns['halfcheetah'], 17, 6, hidden_dim=pk.H, rollout_batch_size=500, rollout_length=2,
                epoch_length=20, model_train_freq=20, separate_mean_var=True, penalty_coeff=coeff,
                penalty_kind='max_pairwise', real_ratio=0.05, target_entropy=-3, seed=5, ensemble_dtype='fp32',
                model_eval_episodes=8, model_eval_length=5)
    algo._model.set_elites([0, 1, 2, 3, 4])
    algo._model_train_metrics = {}                     # the model is given (no BNN.train in this epoch)
    d = list(algo.train(1))[0]
    torch.cuda.synchronize()
    mp = algo._model_pool
    return algo, d, {k: v[:mp.size].cpu().numpy() for k, v in mp.fields.items()}


def test_mopo_epoch_with_a_named_kind():
    from mopo_amd.fake_env import FakeEnv
    a1, d1, p1 = _mopo(1.0)
    a0, d0, p0 = _mopo(0.0)
    assert a1.fake_env.penalty_kind == 'max_pairwise' and len(p1['rewards']) == 1000
    for k in ('observations', 'actions', 'next_observations', 'terminals'):
        np.testing.assert_array_equal(p1[k], p0[k], err_msg=k)
    env = FakeEnv(a1._model, a1._static_fns, penalty_coeff=1.0, penalty_kind='max_pairwise')
    _, _, _, info = env.step(p1['observations'].astype(np.float64), p1['actions'], deterministic=True)
    mean, var = a1._model.predict(np.concatenate([p1['observations'], p1['actions']], 1), factored=True)
    r1, r0 = p1['rewards'].ravel().astype(np.float64), p0['rewards'].ravel().astype(np.float64)
    tol = pk.oracle_bound(mean, var) + 2.0 ** -23 * (np.abs(r0) + np.abs(r1))      # the pool's rewards are f32
    err = np.abs((r0 - r1) - info['penalty'].ravel())
    print('max err / tol = %.3g, mean penalty %.3g' % ((err / tol).max(), info['penalty'].mean()))
    # a freshly constructed model's members all but agree: the penalty is small, yet well above the tolerance
    assert (err <= tol).all() and info['penalty'].mean() > 10 * tol.mean()
    assert d1['model_eval/penalty-average'] > 0


# ---- 8. refusals --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', [4, -1])
def test_unknown_kinds_are_refused(bad):
    import torch
    from mopo_amd import _lib as L
    from mopo_amd.fake_env import FakeEnv
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    c = pk.step_case()
    model = make_model(c['mats'], *(pk.STEP_SHAPE[k] for k in 'EOA'))
    ro = ModelRollout(model, 8, 2)
    lib = L.lib()
    fa = L.FakeEnvArgs(B=1, penalty_learned_var=bad, term_kind=0)
    ra = L.RolloutArgs(B=1, horizon=1, term_kind=0, penalty_learned_var=bad)
    desc, ev, va = L.PoolDesc(), L.EvalArgs(), L.ValArgs()
    calls = [lambda: lib.mopo_penalty_from_predictions(bad, None, None, 7, 17, 1, None, None),
             lambda: lib.mopo_fakeenv_step(model.handle, fa, None),
             lambda: lib.mopo_rollout_run(ro._h, ra, desc, None),
             lambda: lib.mopo_rollout_run_staged(ro._h, ra, desc, None),
             lambda: lib.mopo_rollout_run_staged_steps(ro._h, ra, desc, 0, 1, None),
             lambda: lib.mopo_rollout_evaluate(ro._h, ra, ev, None),
             lambda: lib.mopo_rollout_validate(ro._h, ra, desc, va, None)]
    for call in calls:
        assert call() == -1
        msg = lib.mopo_last_error().decode()
        assert 'penalty kind' in msg and all(k in msg for k in pk.PENALTY_KINDS), msg
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        FakeEnv(model, static_fns['halfcheetah'], penalty_kind='nope')
