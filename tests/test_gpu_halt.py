"""GPU: hard truncation (MOReL's HALT) on every rollout path, and the penalty over a dataset.

The reference is tests/halt_cases.py: the oracle's FakeEnv.step / rollout loop with the rule restated on top, and
cases whose thresholds lie in a gap of the oracle's sorted u at least 10 device tolerances wide on either side
(tests/test_halt_cases.py checks that on the CPU).  So halted sets, terminals and step counts are compared exactly,
with no row excluded; halted rewards must equal the halt reward exactly.  Everything else is held to the existing
tolerances: states, actions and rewards 5e-5 (1 + |ref|) (tests/test_gpu_rollout.py), u of kinds 0 and 1 rel 1e-5,
u of kinds 2 and 3 penalty_kinds.oracle_bound.  E = 7, H = 64.
"""
import functools

import numpy as np
import pytest

import halt_cases as hc
import penalty_kinds as pk

pytestmark = pytest.mark.gpu
KIND_NAMES = pk.PENALTY_KINDS
R = hc.HALT_REWARD


def make_model(mats, O, A, dtype='fp32'):
    from mopo_amd.bnn import BNN
    m = BNN({'name': 't', 'num_networks': hc.E, 'num_elites': 5, 'separate_mean_var': True, 'obs_dim': O,
             'act_dim': A, 'hidden_dim': hc.H, 'dtype': dtype})
    m.set_params(mats)
    m.set_elites(hc.ELITES)
    return m


def scaled(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / (1 + np.abs(b))


def close(a, b, tol=5e-5):
    err = scaled(a, b)
    assert err.max(initial=0) <= tol, 'max scaled err %.3g > %.3g' % (err.max(), tol)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


# ---- 1. FakeEnv.step ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', hc.KINDS, ids=KIND_NAMES)
@pytest.mark.parametrize('shape', sorted(hc.STEP_SHAPES), ids=lambda s: 'O%d' % s[0])
def test_fakeenv_step(shape, kind):
    from mopo_amd.fake_env import FakeEnv
    from mopo_amd.static import static_fns
    O, A = shape
    c = hc.step_case(O, A)
    model = make_model(c['mats'], O, A)
    thr = hc.THRESHOLDS[('step', O, A, kind)]
    bound = pk.oracle_bound(c['mean'], c['var'])
    n_halted = 0
    for B in hc.STEP_B:
        obs, act = c['obs'][:B].astype(np.float64), c['act'][:B]
        for det in (False, True):
            for coeff in (0.0, 1.0):
                kw = dict(deterministic=True) if det else dict(noise=c['noise'][:, :B], model_inds=c['inds'][:B])
                fns = static_fns[c['domain']]
                on = FakeEnv(model, fns, penalty_coeff=coeff, penalty_kind=kind, halt_threshold=thr, halt_reward=R)
                off = FakeEnv(model, fns, penalty_coeff=coeff, penalty_kind=kind)
                nobs, rew, term, info = on.step(obs, act, **kw)
                nobs0, rew0, term0, info0 = off.step(obs, act, **kw)
                ref = hc.step_reference(O, A, kind, B, det, coeff)
                h = ref['halted']
                n_halted += int(h.sum())
                tag = 'O=%d kind=%d B=%d det=%d coeff=%g' % (O, kind, B, det, coeff)
                # exact: the halted set, the terminals, the halted rewards
                np.testing.assert_array_equal(rew[:, 0] == R, h, err_msg=tag)
                np.testing.assert_array_equal(term, ref['term'], err_msg=tag)
                np.testing.assert_array_equal(term0, ref['rule'], err_msg=tag)
                np.testing.assert_array_equal(info['mean'][:, 1], term[:, 0].astype(np.float32), err_msg=tag)
                # everything else is what the step returns without the fields, bit for bit: every output of a
                # row that does not halt, and of a halted row all but its terminal and penalized reward
                np.testing.assert_array_equal(bits(rew[~h]), bits(rew0[~h]), err_msg=tag)
                for k, a, b in (('next_obs', nobs, nobs0), ('unpen', info['unpenalized_rewards'],
                                                            info0['unpenalized_rewards']),
                                ('std', info['std'], info0['std']), ('mean', np.delete(info['mean'], 1, 1),
                                                                     np.delete(info0['mean'], 1, 1)),
                                ('log_prob', info['log_prob'], info0['log_prob']), ('dev', info['dev'], info0['dev'])):
                    np.testing.assert_array_equal(bits(a), bits(b), err_msg=tag + ' ' + k)
                if coeff:
                    np.testing.assert_array_equal(bits(info['penalty']), bits(info0['penalty']), err_msg=tag)
                    err = np.abs(info['penalty'].ravel() - ref['u'])
                    assert (err <= (1e-5 * (1 + ref['u']) if kind < 2 else bound[:B])).all(), tag
                else:
                    assert info['penalty'] is None
                # against the oracle, at the existing tolerances
                close(nobs, ref['next_obs'])
                close(info['unpenalized_rewards'], ref['unpen'])
                tol = 5e-5 * (1 + np.abs(ref['rew'][:, 0])) + coeff * (bound[:B] if kind >= 2 else 0.0)
                assert (np.abs(rew[:, 0] - ref['rew'][:, 0]) <= tol).all(), tag
    assert n_halted > 0


# ---- 2. the fused rollout, parity mode ---------------------------------------------------------------------------
def _run(c, dtype='fp32', horizon=None, streams=None, **kw):
    import torch
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    dev = torch.device('cuda')
    O, A, B = c['O'], c['A'], c['B']
    h = horizon or c['horizon']
    s = streams or c
    model = make_model(c['mats'], O, A, dtype)
    pool = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=B * h + 7)
    ro = ModelRollout(model, B, h)
    steps = ro.run(torch.from_numpy(c['env_obs']).to(dev), torch.from_numpy(c['flat']).to(dev), pool, B, h,
                   static_fns[c['domain']].term_kind, kw.pop('coeff', hc.ROLLOUT_COEFF), hc.ELITES,
                   start_idx=c['start'], eps_act=s['eps_act_c'][:h], eps_obs=s['eps_obs_c'][:h],
                   model_inds=s['inds_c'][:h], **kw)
    torch.cuda.synchronize()
    halted = None if ro.last_halted is None else ro.last_halted.cpu().numpy()
    return steps.cpu().numpy(), halted, pool


@functools.lru_cache(None)
def _pool_bound(name, kind):
    c = hc.rollout_case(name, kind)
    return pk.oracle_bound(*hc.member_outputs(c['params'], c['ref']['observations'], c['ref']['actions']))


@pytest.mark.parametrize('kind', hc.ROLLOUT_KINDS, ids=[KIND_NAMES[k] for k in hc.ROLLOUT_KINDS])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16x6'])
@pytest.mark.parametrize('name', sorted(hc.ROLLOUT_CASES))
def test_fused_rollout_parity(name, dtype, kind):
    c = hc.rollout_case(name, kind)
    thr = hc.THRESHOLDS[('rollout', name, kind)]
    steps, halted, pool = _run(c, dtype, penalty_kind=kind, halt_threshold=thr, halt_reward=R)
    exp = np.zeros(c['horizon'], np.int64)
    exp[:len(c['steps'])] = c['steps']
    exph = np.zeros(c['horizon'], np.int64)
    exph[:len(c['halted_n'])] = c['halted_n']
    print('%s %s kind %d: steps %s halted %s' % (name, dtype, kind, steps.tolist(), halted.tolist()))
    np.testing.assert_array_equal(steps, exp)
    np.testing.assert_array_equal(halted, exph)
    op, ref = c['pool'], c['ref']
    assert pool.size == op.size and pool._pointer == op._pointer
    got = pool.return_all_samples(as_numpy=True)
    np.testing.assert_array_equal(got['terminals'], ref['terminals'])
    h = ref['rewards'][:, 0] == R
    assert h.sum() == sum(c['halted_n'])
    np.testing.assert_array_equal(got['rewards'][:, 0] == np.float32(R), h)          # halted rewards: exact
    for k in ('observations', 'actions', 'next_observations'):
        close(got[k], ref[k])
    want = np.asarray(ref['rewards'], np.float64).ravel()
    tol = 5e-5 * (1 + np.abs(want)) + (hc.ROLLOUT_COEFF * _pool_bound(name, kind) if kind >= 2 else 0.0)
    err = np.abs(got['rewards'].ravel() - want)
    print('max err / tol = %.3g' % (err / tol).max())
    assert (err <= tol).all()


# ---- 3. off means off ----------------------------------------------------------------------------------------------
def _same_pools(a, b):
    sa, _, pa = a
    sb, _, pb = b
    np.testing.assert_array_equal(sa, sb)
    assert pa.size == pb.size and pa._pointer == pb._pointer
    x, y = pa.return_all_samples(as_numpy=True), pb.return_all_samples(as_numpy=True)
    for k in x:
        np.testing.assert_array_equal(bits(x[k]), bits(y[k]), err_msg=k)


@pytest.mark.parametrize('name,horizon', [('halfcheetah-4100', 3), ('walker2d-300', 4)])
def test_off_means_off(name, horizon, monkeypatch):
    """halt = 0 with garbage in the other two fields, and halt = 1 with threshold +inf, are bit for bit the call
    that never sets the fields -- for halfcheetah-4100 that is the compacting path against the split path."""
    import mopo_amd.fake_env as fe
    for kind in hc.ROLLOUT_KINDS:
        c = hc.rollout_unhalted(name, kind)
        plain = _run(c, horizon=horizon, penalty_kind=kind)
        assert plain[1] is None
        if c['domain'] == 'halfcheetah':
            assert plain[0].tolist() == [c['B']] * horizon
        inf = _run(c, horizon=horizon, penalty_kind=kind, halt_threshold=float('inf'), halt_reward=R)
        _same_pools(plain, inf)
        assert inf[1].tolist() == [0] * horizon
        with monkeypatch.context() as m:
            m.setattr(fe, 'halt_fields', lambda *a: (0, float('nan'), float('-inf')))
            _same_pools(plain, _run(c, horizon=horizon, penalty_kind=kind))
            m.setattr(fe, 'halt_fields', lambda *a: (0, -1.0, 12345.0))
            _same_pools(plain, _run(c, horizon=horizon, penalty_kind=kind))


@pytest.mark.parametrize('name', ['halfcheetah-300', 'walker2d-300'])
def test_threshold_below_every_penalty_halts_every_row(name):
    c = hc.rollout_unhalted(name, 1)
    B, h = c['B'], c['horizon']
    for kind, coeff in ((0, 0.0), (1, 1.0), (2, 0.0), (3, 1.0)):
        steps, halted, pool = _run(c, penalty_kind=kind, coeff=coeff, halt_threshold=-1.0, halt_reward=R)
        assert steps.tolist() == [B] + [0] * (h - 1) and halted.tolist() == [B] + [0] * (h - 1)
        got = pool.return_all_samples(as_numpy=True)
        assert pool.size == B and got['terminals'].all() and (got['rewards'] == np.float32(R)).all()


# ---- 4. evaluate --------------------------------------------------------------------------------------------------
def _actions(pi, O, A, obs, eps):
    import torch
    from mopo_amd import _lib as L
    o = torch.as_tensor(np.ascontiguousarray(obs, np.float64)).cuda()
    e = None if eps is None else torch.as_tensor(np.ascontiguousarray(eps, np.float32)).cuda()
    B = len(obs)
    act = torch.empty((B, A), dtype=torch.float32, device=o.device)
    mu = torch.empty_like(act)
    L.check(L.lib().mopo_actor_forward_dtype(L.ptr(pi), O, A, 256, L.ptr(o), 1, B, L.ptr(e), 0, 0, L.ptr(act),
                                             L.ptr(mu), 0, L.stream_ptr()))
    return (mu if eps is None else act).cpu().numpy()


@pytest.mark.parametrize('policy_det', [True, False], ids=['tanh-mu', 'sampled'])
def test_evaluate(policy_det):
    """64 episodes x 6 steps under walker2d's rule, kind max_pairwise, against the host loop of the device actor and
    FakeEnv.step WITHOUT the fields, with the rule applied by halt_cases.apply_halt.  The threshold is the gap rule's
    on that loop's own u over every (step, episode) an unhalted episode visits; the test first holds it to the
    margin of tests/test_halt_cases.py."""
    import torch
    from mopo_amd.fake_env import FakeEnv
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    s = hc.rollout_setup('walker2d-300')
    B, T, O, A, kind, coeff = 64, 6, s['O'], s['A'], 2, 1.0
    model = make_model(s['mats'], O, A)
    dev = torch.device('cuda')
    pi = torch.from_numpy(s['flat']).to(dev)
    env = FakeEnv(model, static_fns['walker2d'], penalty_coeff=coeff, penalty_kind=kind)
    rs = np.random.RandomState(5)
    eps_act = rs.normal(size=(T, B, A)).astype(np.float32)
    eps_sel, inds = rs.normal(size=(T, B, O + 1)), rs.choice(hc.ELITES, size=(T, B)).astype(np.int32)
    start = s['start'][:B]

    def loop(thr):
        ids, obs = np.arange(B), s['env_obs'][start].astype(np.float64)
        out = dict(ret=np.zeros(B), pret=np.zeros(B), psum=np.zeros(B), length=np.zeros(B, np.int32),
                   halted=np.zeros(B, np.uint8), terminated=np.zeros(B, np.uint8), scale=np.zeros(B), u=[], m=[])
        ea_c, eo_c, in_c = np.zeros_like(eps_act), np.zeros_like(eps_sel), np.zeros_like(inds)
        for i in range(T):
            n = len(ids)
            if n == 0:
                break
            ea_c[i, :n], eo_c[i, :n], in_c[i, :n] = eps_act[i, ids], eps_sel[i, ids], inds[i, ids]
            act = _actions(pi, O, A, obs, None if policy_det else eps_act[i, ids])
            noise = np.zeros((hc.E, n, O + 1))
            noise[inds[i, ids], np.arange(n)] = eps_sel[i, ids]
            nobs, rew, term, info = env.step(obs, act, noise=noise, model_inds=inds[i, ids])
            u = info['penalty'].ravel().astype(np.float64)
            mean, var = model.predict(np.concatenate([obs, act], 1), factored=True)
            out['u'].append(u)
            out['m'].append(hc.margin(kind, u, mean, var))
            rule = term[:, 0].copy()
            if thr is not None:
                rew, term, h = hc.apply_halt(rew, term, u, thr)
                out['halted'][ids[h]] = 1
            out['terminated'][ids[rule]] = 1
            out['ret'][ids] += info['unpenalized_rewards'].ravel()
            out['pret'][ids] += rew.ravel()
            out['psum'][ids] += u
            out['scale'][ids] += 1 + np.abs(info['unpenalized_rewards'].ravel())
            out['length'][ids] += 1
            keep = ~term[:, 0]
            obs, ids = nobs[keep], ids[keep]
        out.update(eps_act=ea_c, eps_obs=eo_c, inds=in_c)
        return out

    free = loop(None)
    u, m = np.concatenate(free['u']), np.concatenate(free['m'])
    thr = hc.gap_threshold(u)
    assert (np.abs(u - thr) > m).all()                        # the condition: the threshold lies in a wide gap
    ref = loop(thr)
    assert ref['halted'].any() and ref['terminated'].any() and (ref['length'] == T).any()
    ro = ModelRollout(model, B, 1)
    args = (torch.from_numpy(s['env_obs']).to(dev), pi, B, T, static_fns['walker2d'].term_kind, coeff, hc.ELITES)
    kw = dict(policy_deterministic=policy_det, start_idx=start, eps_act=ref['eps_act'], eps_obs=ref['eps_obs'],
              model_inds=ref['inds'], penalty_kind=kind, actor_dtype='fp32')
    got = {k: v.cpu().numpy() for k, v in ro.evaluate(*args, halt_threshold=thr, halt_reward=R, **kw).items()}
    print('halted %.3f terminated %.3f mean length %.3f' % (got['halted'].mean(), got['terminated'].mean(),
                                                            got['lengths'].mean()))
    np.testing.assert_array_equal(got['lengths'], ref['length'])
    np.testing.assert_array_equal(got['halted'], ref['halted'])
    np.testing.assert_array_equal(got['terminated'], ref['terminated'])
    assert (np.abs(got['penalized_returns'] - ref['pret']) <= 5e-5 * ref['scale']).all()
    assert (np.abs(got['returns'] - ref['ret']) <= 5e-5 * ref['scale']).all()
    assert got['stats'][12] == got['halted'].mean() and got['stats'][10] == got['terminated'].mean()
    assert not got['stats'][13:].any()
    off = {k: v.cpu().numpy() for k, v in ro.evaluate(*args, **dict(kw, eps_act=free['eps_act'],
                                                                    eps_obs=free['eps_obs'],
                                                                    model_inds=free['inds'])).items()}
    assert not off['stats'][12:].any() and not off['halted'].any()
    np.testing.assert_array_equal(off['lengths'], free['length'])


# ---- 5. penalty_profile ----------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _profile_data(name):
    s = hc.rollout_setup(name)
    rs = np.random.RandomState(77)
    n = 1000
    obs = s['env_obs'][:n]
    act = rs.uniform(-1, 1, (n, s['A'])).astype(np.float32)
    mean, var = hc.member_outputs(s['params'], obs, act)
    return dict(obs=obs, act=act, mean=mean, var=var)


@pytest.mark.parametrize('name', ['halfcheetah-300', 'ant-300'], ids=['narrow', 'wide'])
def test_penalty_profile(name):
    import torch
    from mopo_amd.fake_env import FakeEnv
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    s, d = hc.rollout_setup(name), _profile_data(name)
    O, A, n = s['O'], s['A'], 1000
    model = make_model(s['mats'], O, A)
    pool = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=n + 5)
    pool.add_samples({'observations': d['obs'], 'actions': d['act'], 'rewards': np.zeros((n, 1)),
                      'terminals': np.zeros((n, 1), bool), 'next_observations': d['obs']})
    before = {k: v.clone() for k, v in pool.fields.items()}
    ro = ModelRollout(model, 300, 1)
    bound = pk.oracle_bound(d['mean'], d['var'])
    for kind in hc.KINDS:
        env = FakeEnv(model, static_fns['halfcheetah'], penalty_coeff=1.0, penalty_kind=kind)
        step_u = env.step(d['obs'].astype(np.float64), d['act'], deterministic=True)[3]['penalty'].ravel()
        ref = pk.penalty(kind, d['mean'], d['var'])
        for N in (1, 300, 1000):     # one row; one full chunk; three chunks and a partial fourth
            u = ro.penalty_profile(pool, kind, n_rows=N)
            torch.cuda.synchronize()
            assert u.dtype == torch.float32 and tuple(u.shape) == (N,)
            u = u.cpu().numpy()
            e1 = np.abs(u - step_u[:N]) / step_u[:N]
            e2 = np.abs(u - ref[:N])
            print('%s kind %d N %d: rel to FakeEnv.step %.3g, to the f64 oracle / bound %.3g'
                  % (name, kind, N, e1.max(), (e2 / bound[:N]).max()))
            assert e1.max() <= 1e-5
            assert (e2 <= (1e-5 * (1 + ref[:N]) if kind < 2 else bound[:N])).all()
        assert np.array_equal(ro.penalty_profile(pool, KIND_NAMES[kind]).cpu().numpy(), u)   # by name, the pool's size
        if kind == 0:
            # the u a one-step rollout from those rows on the dataset's actions stores (the open-loop validation's
            # [1][B] penalty table): the same f32 order, the same bits
            for lo in (0, 300, 900):
                m = min(300, n - lo)
                val = ro.validate(pool, m, 1, 0, hc.ELITES, start_idx=np.arange(lo, lo + m), penalty_kind=0)
                np.testing.assert_array_equal(bits(val['penalties'][0].cpu().numpy()), bits(u[lo:lo + m]))
    for k, v in pool.fields.items():
        assert torch.equal(v, before[k]), k


# ---- 6. MOPO ---------------------------------------------------------------------------------------------------
def test_mopo_run_with_a_halt_quantile():
    import torch
    from mopo_amd.evaluation import halt_threshold_from_quantile
    from mopo_amd.mopo import MOPO
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    rs = np.random.RandomState(2)
    n = 3000
    obs = rs.normal(size=(n, 17)).astype(np.float32)
    pool = SimpleReplayPool(obs_dim=17, act_dim=6, max_size=n)
    pool.add_samples({'observations': obs, 'actions': rs.uniform(-1, 1, (n, 6)), 'rewards': rs.normal(size=(n, 1)),
                      'terminals': np.zeros((n, 1), bool), 'next_observations': obs + 0.1})
    np.random.seed(123)
    algo = MOPO(pool, static_fns['halfcheetah'], 17, 6, hidden_dim=32, rollout_batch_size=500, rollout_length=3,
                epoch_length=20, model_train_freq=20, separate_mean_var=True, penalty_coeff=1.0,
                penalty_kind='max_pairwise', real_ratio=0.05, target_entropy=-3, seed=5, ensemble_dtype='fp32',
                model_eval_episodes=8, model_eval_length=5, halt_quantile=0.9, halt_reward=R)
    algo._model.set_elites([0, 1, 2, 3, 4])
    algo._model_train_metrics = {}                     # the model is given (no BNN.train in this run)
    u = ModelRollout(algo._model, 1024, 1).penalty_profile(pool, 'max_pairwise')
    want = halt_threshold_from_quantile(u, 0.9)
    assert want == np.sort(u.cpu().numpy())[int(np.ceil(0.9 * n)) - 1]
    seen = 0
    for e, d in enumerate(algo.train(2)):
        torch.cuda.synchronize()
        assert d['model/halt-threshold'] == want and algo._halt_threshold == want
        mp = algo._model_pool
        rew = mp.fields['rewards'][seen:mp.size].cpu().numpy().ravel()
        term = mp.fields['terminals'][seen:mp.size].cpu().numpy().ravel()
        share = float(np.mean((term != 0) & (rew == np.float32(R))))
        print('epoch %d: rows %d halted-fraction %.4f (pool %.4f) eval %.3f' % (
            e, mp.size - seen, d['model/halted-fraction'], share, d['model_eval/halted-fraction']))
        assert mp.size - seen > 0 and d['model/halted-fraction'] == share and 0 < share < 1
        assert (rew[term != 0] == np.float32(R)).all()        # halfcheetah: nothing else ends a row
        assert 0.0 <= d['model_eval/halted-fraction'] <= 1.0
        seen = mp.size
    with pytest.raises(ValueError):
        MOPO(pool, static_fns['halfcheetah'], 17, 6, hidden_dim=32, halt_quantile=0.9, halt_threshold=1.0,
             halt_reward=R)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    import torch
    from mopo_amd import _lib as L
    from mopo_amd.fake_env import FakeEnv
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    c = hc.step_case(17, 6)
    model = make_model(c['mats'], 17, 6)
    ro = ModelRollout(model, 8, 2)
    lib = L.lib()
    desc, ev = L.PoolDesc(), L.EvalArgs()
    el = torch.zeros(1, dtype=torch.int32, device='cuda')
    bad = [(dict(halt=2), 'halt must be'), (dict(halt=-1), 'halt must be'),
           (dict(halt=1, halt_threshold=1.0, halt_reward=float('inf')), 'halt_reward'),
           (dict(halt=1, halt_threshold=1.0, halt_reward=float('nan')), 'halt_reward'),
           (dict(halt=1, halt_threshold=float('nan'), halt_reward=-1.0), 'halt_threshold')]
    for fields, word in bad:
        fa = L.FakeEnvArgs(B=1, penalty_learned_var=1, term_kind=0, **fields)
        ra = L.RolloutArgs(B=1, horizon=1, term_kind=0, penalty_learned_var=1, n_elites=1, d_elites=L.ptr(el), **fields)
        for call in (lambda: lib.mopo_fakeenv_step(model.handle, fa, None),
                     lambda: lib.mopo_rollout_run(ro._h, ra, desc, None),
                     lambda: lib.mopo_rollout_run_staged(ro._h, ra, desc, None),
                     lambda: lib.mopo_rollout_run_staged_steps(ro._h, ra, desc, 0, 1, None),
                     lambda: lib.mopo_rollout_evaluate(ro._h, ra, ev, None)):
            assert call() == -1
            msg = lib.mopo_last_error().decode()
            assert word in msg, msg
    u = torch.zeros(8, device='cuda')
    full = L.PoolDesc(d_obs=L.ptr(u), d_act=L.ptr(u), max_size=1)
    for call, word in ((lambda: lib.mopo_rollout_penalty_profile(ro._h, full, 1, 4, L.ptr(u), None), 'penalty kind'),
                       (lambda: lib.mopo_rollout_penalty_profile(ro._h, full, 1, -1, L.ptr(u), None), 'penalty kind'),
                       (lambda: lib.mopo_rollout_penalty_profile(ro._h, full, -1, 1, L.ptr(u), None), 'n_rows'),
                       (lambda: lib.mopo_rollout_penalty_profile(ro._h, full, 2, 1, L.ptr(u), None), 'max_size'),
                       (lambda: lib.mopo_rollout_penalty_profile(ro._h, full, 1, 1, None, None), 'd_u'),
                       (lambda: lib.mopo_rollout_penalty_profile(ro._h, desc, 1, 1, L.ptr(u), None), 'pool field'),
                       (lambda: lib.mopo_rollout_penalty_profile(ro._h, None, 1, 1, L.ptr(u), None), 'NULL')):
        assert call() == -1
        assert word in lib.mopo_last_error().decode(), lib.mopo_last_error().decode()
    assert lib.mopo_rollout_penalty_profile(ro._h, desc, 0, 1, None, None) == 0      # nothing to do: nothing read
    with pytest.raises(ValueError):
        FakeEnv(model, static_fns['halfcheetah'], halt_threshold=1.0)
    with pytest.raises(ValueError):
        ro.run(u, u, desc, 1, 1, 0, 0.0, hc.ELITES, halt_threshold=1.0)
    torch.cuda.synchronize()


def test_validate_ignores_the_fields(monkeypatch):
    """A segment ends where the data does: fields that would halt every row leave every output as it was."""
    import mopo_amd.fake_env as fe
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout
    s, d = hc.rollout_setup('halfcheetah-300'), _profile_data('halfcheetah-300')
    n, K = 256, 3
    pool = SimpleReplayPool(obs_dim=s['O'], act_dim=s['A'], max_size=n)
    nxt = np.roll(d['obs'][:n], -1, 0)
    pool.add_samples({'observations': d['obs'][:n], 'actions': d['act'][:n], 'rewards': np.zeros((n, 1)),
                      'terminals': np.zeros((n, 1), bool), 'next_observations': nxt})
    ro = ModelRollout(make_model(s['mats'], s['O'], s['A']), 64, 1)
    run = lambda: {k: v.cpu().numpy() for k, v in ro.validate(pool, 64, K, 0, hc.ELITES, start_idx=np.arange(64) * 3,
                                                               penalty_kind=2).items()}
    plain = run()
    assert (plain['lengths'] == K).all()
    for garbage in ((1, -1.0, -5.0), (7, float('nan'), float('inf'))):
        monkeypatch.setattr(fe, 'halt_fields', lambda *a, g=garbage: g)
        got = run()
        for k in plain:
            np.testing.assert_array_equal(bits(got[k]), bits(plain[k]), err_msg=k)
