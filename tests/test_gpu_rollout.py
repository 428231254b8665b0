"""GPU parity: HIP ensemble forward, FakeEnv.step, actor, pool and fused rollout vs the oracle.

Tolerances (fp32 device vs reference dtypes; the reference mixes f32 GEMMs with f64 sampling):
  * ensemble mean/var (f32 GEMM order differs from TF/BLAS):   |d| <= 2e-5 * (1 + |ref|)
  * next_obs / rewards / penalized rewards:                      |d| <= 5e-5 * (1 + |ref|)
  * penalty:                                                     rel 1e-5
  * log_prob (where finite):                                     |d| <= 1e-4 * (1 + |ref|)
  * integer work (model_inds consumed, terminals, pool pointer/size, compaction order): bit-exact
"""
import glob
import os

import numpy as np
import pytest

from oracle import bnn as obnn
from oracle import fake_env as ofe
from oracle import replay_pool as opool
from oracle import sac as osac

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
CASES = sorted(glob.glob(os.path.join(GOLD, 'fakeenv_*.npz')))


def close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b) / (1 + np.abs(b))
    assert np.all(np.isfinite(a) == np.isfinite(b))
    m = np.isfinite(b)
    assert err[m].max(initial=0) <= tol, 'max scaled err %.3g > %.3g' % (err[m].max(), tol)


def golden_params(E, H):
    z = np.load(os.path.join(GOLD, 'bnn_E%d_H%d.npz' % (E, H)))
    return [z['w%d' % i] for i in range(16)]


def make_model(mats, E, H, O=17, A=6, dtype='fp32'):
    from mopo_amd.bnn import BNN
    m = BNN({'name': 't', 'num_networks': E, 'num_elites': 5, 'separate_mean_var': True, 'obs_dim': O,
             'act_dim': A, 'hidden_dim': H, 'dtype': dtype})
    return m.set_params(mats)


@pytest.mark.parametrize('E,H,B,f64', [(7, 64, 257, False), (32, 32, 100, True), (7, 200, 4099, False),
                                       (7, 200, 33, True), (3, 400, 500, False), (7, 200, 1, False)])
def test_bnn_predict_vs_oracle(E, H, B, f64):
    rs = np.random.RandomState(E * 1000 + H)
    if (E, H) in ((7, 64), (32, 32)):
        mats = golden_params(E, H)
    else:
        mats = obnn.to_mat_list(obnn.init_params(E, 17, 6, hidden=H, seed=3, inputs=rs.normal(size=(300, 23)) * 3))
    p = obnn.from_mat_list(mats)
    x = rs.normal(size=(B, 23)) * 2
    x = x if f64 else x.astype(np.float32)
    model = make_model(mats, E, H)
    mean, var = model.predict(x, factored=True)
    rm, rv = obnn.forward(p, x, dtype=np.float64)
    close(mean, rm, 2e-5)
    close(var, rv, 2e-5)


@pytest.mark.parametrize('path', CASES, ids=[os.path.basename(c) for c in CASES])
def test_fakeenv_step_vs_reference_golden(path):
    from mopo_amd.fake_env import FakeEnv
    from mopo_amd.static import static_fns
    c = dict(np.load(path))
    E, H = int(c['E']), int(c['H'])
    model = make_model(golden_params(E, H), E, H)
    model.set_elites(list(c['elites']))
    env = FakeEnv(model, static_fns[str(c['domain'])], penalty_coeff=float(c['penalty_coeff']),
                  penalty_learned_var=bool(c['learned_var']))
    det = bool(c['deterministic'])
    np.random.seed(int(c['seed']))
    nobs, rew, term, info = env.step(c['obs'], c['act'], deterministic=det)
    # numpy's global stream consumed exactly like the reference (normal then choice)
    np.random.seed(int(c['seed']))
    if not det:
        np.random.normal(size=(E, int(c['B']), 18))
        np.testing.assert_array_equal(np.random.choice(list(c['elites']), size=int(c['B'])), c['model_inds'])
    close(nobs, c['next_obs'], 5e-5)
    close(rew, c['rew'], 5e-5)
    close(info['unpenalized_rewards'], c['unpenalized'], 5e-5)
    close(info['penalty'], c['penalty'], 1e-5)
    close(info['mean'], c['info_mean'], 5e-5)
    close(info['std'], c['info_std'], 5e-5)
    close(info['dev'], c['dev'], 1e-4)
    lp = c['log_prob']
    fin = np.isfinite(lp)
    close(info['log_prob'][fin], lp[fin], 1e-4)
    # terminals bit-exact except where the f32-vs-f64 threshold operand is within 1e-4 of a bound
    bad = term[:, 0] != c['term'][:, 0]
    if bad.any():
        h, a = c['next_obs'][bad, 0], c['next_obs'][bad, 1]
        bounds = np.array([0.7, 0.8, 2.0])
        near = (np.abs(h[:, None] - bounds).min(1) < 1e-4) | (np.abs(np.abs(a)[:, None] - np.array([0.2, 1.0])).min(1) < 1e-4)
        assert near.all()


@pytest.mark.parametrize('dtype', [0, 3, 4])   # fp32, bf16x6, f16x3
def test_actor_forward_vs_oracle(dtype):
    import torch
    from mopo_amd import _lib as L
    from mopo_amd.rollout import init_sac_params, split_params
    O, A, H, B = 17, 6, 256, 1000
    flat = init_sac_params(O, A, H, seed=4)
    rs = np.random.RandomState(0)
    flat = flat + (rs.normal(size=flat.shape) * 0.01).astype(np.float32)   # non-zero biases
    P = [p.astype(np.float64) for p in split_params(flat, O, A, H)[:8]]
    obs = rs.normal(size=(B, O))
    eps = rs.normal(size=(B, A)).astype(np.float32)
    dev = torch.device('cuda')
    tp, to, te = (torch.from_numpy(x).to(dev) for x in (flat, obs, eps))
    act = torch.empty((B, A), device=dev)
    mu = torch.empty((B, A), device=dev)
    L.check(L.lib().mopo_actor_forward_dtype(L.ptr(tp), O, A, H, L.ptr(to), 1, B, L.ptr(te), 0, 0, L.ptr(act),
                                             L.ptr(mu), dtype, L.stream_ptr()))
    ra, rmu = osac.actor_act(P, obs.astype(np.float32).astype(np.float64), eps.astype(np.float64))
    close(act.cpu().numpy(), ra, 2e-5)
    close(mu.cpu().numpy(), rmu, 2e-5)


def test_pool_vs_reference_trace():
    import torch
    from mopo_amd.replay_pool import SimpleReplayPool
    z = np.load(os.path.join(GOLD, 'pool_trace.npz'))
    pool = SimpleReplayPool(obs_dim=17, act_dim=6, max_size=int(z['max_size']))
    for i, n in enumerate(z['adds']):
        if n == 0:
            continue
        pool.add_samples({k: z['add%d_%s' % (i, k)] for k in opool.FIELDS})
        assert pool._pointer == int(z['add%d_ptr' % i]) and pool.size == int(z['add%d_size' % i])
        np.random.seed(50 + i)
        b = pool.random_batch(33, as_numpy=True)
        for k in opool.FIELDS:
            np.testing.assert_array_equal(b[k], z['add%d_batch_%s' % (i, k)].astype(b[k].dtype))
    for k, v in pool.return_all_samples(as_numpy=True).items():
        np.testing.assert_array_equal(v, z['final_' + k].astype(v.dtype))
    # a single add larger than the pool keeps only the last max_size rows, like the reference ring
    p2 = SimpleReplayPool(obs_dim=17, act_dim=6, max_size=10)
    o2 = opool.Pool(17, 6, 10)
    s = {'observations': np.arange(25 * 17, dtype=np.float32).reshape(25, 17), 'actions': np.zeros((25, 6)),
         'next_observations': np.zeros((25, 17)), 'rewards': np.arange(25.).reshape(25, 1),
         'terminals': np.zeros((25, 1), bool)}
    p2.add_samples(s); o2.add_samples(s)
    assert p2._pointer == o2._pointer and p2.size == o2.size
    np.testing.assert_array_equal(p2.fields['rewards'].cpu().numpy(), o2.fields['rewards'])
    torch.cuda.synchronize()


def _rollout_case(domain, E, H, B, horizon, seed, coeff=1.0, O=17, A=6, height=None, learned_var=True, det=False,
                  rand_act=False, policy=None):
    """Oracle rollout with every random stream drawn in the reference order; returns inputs,
    injected streams and the oracle pool.  ``height``: fixed walker height (50: every row done).
    ``learned_var`` / ``det``: FakeEnv's penalty and deterministic modes (fake_env.py:69-110);
    ``rand_act``: rollout_random (mopo.py:736-738: uniform actions drawn after get_action_meta);
    ``policy``: a function (flat, O, A) -> (flat, factor [A]) that restates the 256-wide policy and scales the
    policy noise per action column (tests/actor_regimes.py rollout_policy)."""
    rs = np.random.RandomState(seed)
    env_n = 3000
    env_obs = rs.normal(size=(env_n, O)).astype(np.float32)
    if domain == 'walker2d':
        env_obs[:, 0] = rs.uniform(0.9, 1.9, env_n) if height is None else height
        env_obs[:, 1] = rs.uniform(-0.9, 0.9, env_n)
    if domain in ('ant', 'antangle'):
        env_obs[:, 0] = rs.uniform(0.25, 0.95, env_n)
    if domain == 'humanoid':
        env_obs[:, 0] = rs.uniform(1.05, 1.95, env_n)
    mats = obnn.to_mat_list(obnn.init_params(E, O, A, hidden=H, seed=seed + 1,
                                             inputs=np.concatenate([env_obs, rs.uniform(-1, 1, (env_n, A))], 1)))
    p = obnn.from_mat_list(mats)
    # keep the model's predicted change small so walker rows terminate at a moderate rate
    flat = __import__('mopo_amd.rollout', fromlist=['x']).init_sac_params(O, A, 256, seed=seed + 2)
    eps_factor = np.ones(A, np.float32)
    if policy is not None:
        flat, eps_factor = policy(flat, O, A)
    P = [q.astype(np.float64) for q in __import__('mopo_amd.rollout', fromlist=['x']).split_params(flat, O, A)[:8]]
    elites = [4, 1, 0, 6, 2][:min(5, E)]
    env_pool = opool.Pool(O, A, env_n)
    env_pool.add_samples({'observations': env_obs, 'actions': np.zeros((env_n, A)), 'rewards': np.zeros((env_n, 1)),
                          'terminals': np.zeros((env_n, 1), bool), 'next_observations': env_obs})
    model_pool = opool.Pool(O, A, B * horizon + 7)
    np.random.seed(seed)
    start = env_pool.random_indices(B)
    obs = env_obs[start]
    act_rs = np.random.RandomState(seed + 99)    # stands in for TF's policy noise stream
    eps_act = np.zeros((horizon, B, A), np.float32)
    eps_obs = np.zeros((horizon, B, O + 1))
    inds_all = np.zeros((horizon, B), np.int32)
    act_uni = np.zeros((horizon, B, A), np.float32)
    steps = []
    for i in range(horizon):
        Bi = len(obs)
        ea = act_rs.normal(size=(Bi, A)).astype(np.float32) * eps_factor
        act, _ = osac.actor_act(P, obs.astype(np.float32).astype(np.float64), ea.astype(np.float64))
        act = act.astype(np.float32)
        if rand_act:
            act = np.random.uniform(low=-1, high=1, size=act.shape).astype(np.float32)    # mopo.py:738
            act_uni[i, :Bi] = act
        if det:
            nobs, rew, term, info = ofe.step(p, elites, obs, act, ofe.TERMINATION[domain], penalty_coeff=coeff,
                                             penalty_learned_var=learned_var, deterministic=True)
        else:
            noise = np.random.normal(size=(E, Bi, O + 1))
            inds = np.random.choice(elites, size=Bi)
            nobs, rew, term, info = ofe.step(p, elites, obs, act, ofe.TERMINATION[domain], penalty_coeff=coeff,
                                             penalty_learned_var=learned_var, noise=noise, model_inds=inds)
            eps_obs[i, :Bi] = noise[inds, np.arange(Bi)]
            inds_all[i, :Bi] = inds
        eps_act[i, :Bi] = ea
        steps.append(Bi)
        model_pool.add_samples({'observations': obs, 'actions': act, 'next_observations': nobs,
                                'rewards': rew, 'terminals': term})
        nt = ~term[:, 0]
        if nt.sum() == 0:
            break
        obs = nobs[nt]
    return dict(env_obs=env_obs, mats=mats, flat=flat, elites=elites, start=start, eps_act=eps_act,
                eps_obs=eps_obs, inds=inds_all, steps=steps, pool=model_pool, coeff=coeff, act_uni=act_uni,
                learned_var=learned_var, det=det, rand_act=rand_act)


@pytest.mark.parametrize('domain,E,H,B,horizon,dtype', [
    c if len(c) == 6 else c + ('fp32',) for c in [
                                                  ('halfcheetah', 7, 200, 1000, 5), ('walker2d', 7, 200, 777, 5),
                                                  ('hopper', 7, 64, 300, 4), ('halfcheetah', 32, 32, 64, 3),
                                                  ('halfcheetah', 7, 200, 5000, 3),   # B >= 4096: split rollout
                                                  ('walker2d', 7, 200, 4500, 1),      # one step: no compaction
                                                  # f32 via 3 bf16 parts (f32-accurate), same tolerances
                                                  ('halfcheetah', 7, 200, 1000, 5, 'bf16x6'),
                                                  ('walker2d', 7, 200, 777, 5, 'bf16x6'),
                                                  ('hopper', 7, 64, 300, 4, 'bf16x6'),
                                                  ('halfcheetah', 7, 200, 5000, 3, 'bf16x6'),
                                                  ('halfcheetah', 7, 200, 1000, 5, 'f16x3'),
                                                  ('walker2d', 7, 200, 777, 5, 'f16x3'),
                                                  ('halfcheetah', 7, 200, 5000, 3, 'f16x3'),
                                                  # ant.py / antangle.py / humanoid.py termination rules
                                                  ('ant', 7, 200, 777, 5), ('antangle', 7, 64, 300, 4, 'bf16x6'),
                                                  ('humanoid', 7, 200, 777, 5), ('humanoid', 7, 200, 5000, 3, 'bf16x6'),
                                                  ('pendulum', 7, 64, 300, 3)]])
def test_fused_rollout_parity(domain, E, H, B, horizon, dtype):
    import torch
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    c = _rollout_case(domain, E, H, B, horizon, seed=11)
    model = make_model(c['mats'], E, H, dtype=dtype)
    dev = torch.device('cuda')
    pool = SimpleReplayPool(obs_dim=17, act_dim=6, max_size=B * horizon + 7)
    ro = ModelRollout(model, B, horizon)
    env = torch.from_numpy(c['env_obs']).to(dev)
    pi = torch.from_numpy(c['flat']).to(dev)
    steps = ro.run(env, pi, pool, B, horizon, static_fns[domain].term_kind, c['coeff'], c['elites'],
                   start_idx=c['start'], eps_act=c['eps_act'], eps_obs=c['eps_obs'], model_inds=c['inds'])
    st = steps.cpu().numpy()
    exp = np.zeros(horizon, np.int64)
    exp[:len(c['steps'])] = c['steps']
    np.testing.assert_array_equal(st, exp)                         # compaction counts bit-exact
    op = c['pool']
    assert pool.size == op.size and pool._pointer == op._pointer
    got = pool.return_all_samples(as_numpy=True)
    ref = op.return_all_samples()
    np.testing.assert_array_equal(got['terminals'], ref['terminals'])
    close(got['observations'], ref['observations'], 5e-5)
    close(got['actions'], ref['actions'], 5e-5)
    close(got['next_observations'], ref['next_observations'], 5e-5)
    close(got['rewards'], ref['rewards'], 5e-5)


@pytest.mark.parametrize('domain,E,H,B,horizon,dtype,learned_var,det,rand_act', [
    ('walker2d', 7, 200, 777, 5, 'fp32', False, False, False),     # mean-distance penalty (fake_env.py:98-108)
    ('halfcheetah', 7, 200, 5000, 3, 'bf16x6', False, False, False),  # ... through the split rollout
    ('hopper', 7, 64, 300, 4, 'fp32', True, True, False),           # deterministic (fake_env.py:69-70, 84-86)
    ('walker2d', 7, 200, 777, 4, 'bf16x6', False, True, False),     # deterministic + mean-distance
    ('halfcheetah', 7, 200, 1000, 3, 'fp32', True, False, True),    # rollout_random (mopo.py:736-738)
    ('walker2d', 32, 32, 300, 3, 'fp32', False, False, True)])
def test_fused_rollout_modes_parity(domain, E, H, B, horizon, dtype, learned_var, det, rand_act):
    """The fused rollout's FakeEnv modes vs the oracle (which follows the reference FakeEnv.step,
    pinned by the golden fixtures covering both penalty modes and deterministic)."""
    import torch
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    c = _rollout_case(domain, E, H, B, horizon, seed=13, coeff=2.0, learned_var=learned_var, det=det,
                      rand_act=rand_act)
    model = make_model(c['mats'], E, H, dtype=dtype)
    dev = torch.device('cuda')
    pool = SimpleReplayPool(obs_dim=17, act_dim=6, max_size=B * horizon + 7)
    ro = ModelRollout(model, B, horizon)
    steps = ro.run(torch.from_numpy(c['env_obs']).to(dev), torch.from_numpy(c['flat']).to(dev), pool, B, horizon,
                   static_fns[domain].term_kind, c['coeff'], c['elites'], start_idx=c['start'], eps_act=c['eps_act'],
                   eps_obs=c['eps_obs'], model_inds=c['inds'], penalty_learned_var=learned_var, deterministic=det,
                   rollout_random=rand_act, act_uniform=c['act_uni'] if rand_act else None)
    exp = np.zeros(horizon, np.int64)
    exp[:len(c['steps'])] = c['steps']
    np.testing.assert_array_equal(steps.cpu().numpy(), exp)
    op = c['pool']
    assert pool.size == op.size and pool._pointer == op._pointer
    got, ref = pool.return_all_samples(as_numpy=True), op.return_all_samples()
    np.testing.assert_array_equal(got['terminals'], ref['terminals'])
    for k in ('observations', 'actions', 'next_observations', 'rewards'):
        close(got[k], ref[k], 5e-5)


def test_fused_rollout_random_actions_perf_mode():
    """rollout_random with Philox uniforms: actions in [-1, 1), roughly uniform, deterministic per seed."""
    import torch
    from mopo_amd.bnn import construct_model
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout, init_sac_params
    dev = torch.device('cuda')
    model = construct_model(obs_dim=17, act_dim=6, hidden_dim=200, num_networks=7, num_elites=5,
                            separate_mean_var=True, seed=0)
    B, h = 4000, 2
    pool = SimpleReplayPool(obs_dim=17, act_dim=6, max_size=B * h)
    ro = ModelRollout(model, B, h)
    env = torch.randn(10000, 17, device=dev)
    pi = torch.from_numpy(init_sac_params(17, 6)).to(dev)
    ro.run(env, pi, pool, B, h, 0, 1.0, [0, 1, 2, 3, 4], seed=3, rollout_random=True)
    a = pool.return_all_samples(as_numpy=True)['actions']
    assert a.min() >= -1 and a.max() < 1 and abs(a.mean()) < 0.02 and abs(a.std() - 1 / np.sqrt(3)) < 0.01


def test_fused_rollout_perf_mode_runs():
    import torch
    from mopo_amd.bnn import construct_model
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout, init_sac_params
    dev = torch.device('cuda')
    model = construct_model(obs_dim=17, act_dim=6, hidden_dim=200, num_networks=7, num_elites=5,
                            separate_mean_var=True, seed=0)
    B, h = 5000, 5
    pool = SimpleReplayPool(obs_dim=17, act_dim=6, max_size=3 * B * h)
    ro = ModelRollout(model, B, h)
    env = torch.randn(20000, 17, device=dev)
    pi = torch.from_numpy(init_sac_params(17, 6)).to(dev)
    for ep in range(3):
        steps = ro.run(env, pi, pool, B, h, 0, 1.0, [0, 1, 2, 3, 4], seed=7, epoch=ep)
        assert steps.cpu().tolist() == [B] * h
    assert pool.size == min(3 * B * h, pool._max_size)
    f = pool.return_all_samples(as_numpy=True)
    assert np.isfinite(f['next_observations']).all() and np.isfinite(f['rewards']).all()
    # Philox noise is standard normal: next_obs - mean has unit-ish spread (sanity, not parity)
    assert 0.1 < np.std(f['next_observations'] - f['observations']) < 100
    # determinism: same seed/epoch -> identical transitions
    p2 = SimpleReplayPool(obs_dim=17, act_dim=6, max_size=B * h)
    ro.run(env, pi, p2, B, h, 0, 1.0, [0, 1, 2, 3, 4], seed=7, epoch=0)
    np.testing.assert_array_equal(p2.fields['next_observations'].cpu().numpy(), f['next_observations'][:B * h])


@pytest.mark.parametrize('E,H,B', [(7, 200, 3000), (7, 64, 257), (32, 32, 100), (32, 400, 300)])
def test_bnn_predict_bf16_vs_oracle(E, H, B):
    """bf16 weights/activations, f32 accumulate: |d| <= 3e-2 * (1 + |ref|) against the f32 oracle."""
    from mopo_amd.bnn import BNN
    rs = np.random.RandomState(E + H)
    mats = obnn.to_mat_list(obnn.init_params(E, 17, 6, hidden=H, seed=3, inputs=rs.normal(size=(300, 23)) * 3))
    p = obnn.from_mat_list(mats)
    x = (rs.normal(size=(B, 23)) * 2).astype(np.float32)
    m = BNN({'name': 'b', 'num_networks': E, 'num_elites': 5, 'separate_mean_var': True, 'obs_dim': 17,
             'act_dim': 6, 'hidden_dim': H, 'dtype': 'bf16'}).set_params(mats)
    mean, var = m.predict(x)
    rm, rv = obnn.forward(p, x)
    close(mean, rm, 3e-2)
    close(var, rv, 3e-2)
    # and it is genuinely a different (reduced-precision) path: not bit-identical to fp32
    m32 = make_model(mats, E, H)
    assert not np.array_equal(mean, m32.predict(x)[0])


@pytest.mark.parametrize('dtype,tol', [('bf16x6', 2e-5), ('f16x3', 2e-5), ('bf16x3', 1e-4)])
@pytest.mark.parametrize('E,H,B', [(7, 200, 4099), (7, 64, 257), (32, 32, 100), (32, 400, 300), (7, 200, 1)])
def test_bnn_predict_split_vs_oracle(E, H, B, dtype, tol):
    """f32 operands split into bf16 parts, f32 accumulate.  bf16x6 (3 parts, 6 products) holds the
    fp32 path's tolerance, 2e-5 * (1 + |ref|) against the f64 oracle; bf16x3 (2 parts, 3 products,
    ~17 significand bits) is held to 1e-4 * (1 + |ref|)."""
    rs = np.random.RandomState(E + H + B)
    mats = obnn.to_mat_list(obnn.init_params(E, 17, 6, hidden=H, seed=3, inputs=rs.normal(size=(300, 23)) * 3))
    p = obnn.from_mat_list(mats)
    x = (rs.normal(size=(B, 23)) * 2).astype(np.float32)
    if dtype == 'bf16x6' and H > 256:   # no bf16x6 kernel above H = 256 (its layer loop would not unroll)
        with pytest.raises(RuntimeError, match='bf16x6'):
            make_model(mats, E, H, dtype=dtype)
        return
    mean, var = make_model(mats, E, H, dtype=dtype).predict(x)
    rm, rv = obnn.forward(p, x, dtype=np.float64)
    close(mean, rm, tol)
    close(var, rv, tol)
    if dtype in ('bf16x6', 'f16x3'):   # f32-class: no worse than the f32-MFMA path's own rounding (x2, floor 2e-6)
        m32, v32 = make_model(mats, E, H).predict(x)
        err = lambda a, b: float(np.max(np.abs(np.float64(a) - b) / (1 + np.abs(b))))
        assert err(mean, rm) <= max(2 * err(m32, rm), 2e-6), (err(mean, rm), err(m32, rm))
        assert err(var, rv) <= max(2 * err(v32, rv), 2e-6), (err(var, rv), err(v32, rv))


def test_ensemble_dtypes_no_pathological_slowdown():
    """Guard against a code-generation cliff (a split kernel whose part loops stop unrolling turns
    register arrays into select chains and ran 70x slower while still passing parity): every split
    dtype's predict of 50k rows (device in / out) takes at most the fp32 kernel's time, 1.5x."""
    import torch
    E, H, B = 7, 200, 50000
    rs = np.random.RandomState(11)
    mats = obnn.to_mat_list(obnn.init_params(E, 17, 6, hidden=H, seed=3, inputs=rs.normal(size=(300, 23))))
    x = torch.from_numpy(rs.normal(size=(B, 23)).astype(np.float32)).cuda()
    ms = {}
    for dt in ('fp32', 'bf16x6', 'f16x3', 'bf16x3', 'bf16'):
        m = make_model(mats, E, H, dtype=dt)
        for _ in range(3):
            m.predict(x)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(10):
            m.predict(x)
        t1.record()
        torch.cuda.synchronize()
        ms[dt] = t0.elapsed_time(t1) / 10
    for dt, v in ms.items():
        assert v <= 1.5 * ms['fp32'], ms


@pytest.mark.parametrize('scale', [1e-6, 1.0, 1e3, 1e5])
def test_f16x3_dynamic_range(scale):
    """f16x3 carries fp16 parts under power-of-two scales (per row for activations, per layer and member
    for weights): inputs and weights far outside fp16's range give the f32 kernel's answer, no inf/NaN."""
    rs = np.random.RandomState(17)
    E, H, B = 7, 200, 640
    p = obnn.init_params(E, 17, 6, hidden=H, seed=4, inputs=rs.normal(size=(300, 23)))
    p['W'] = [w * np.float32(scale if i == 0 else 1.0) for i, w in enumerate(p['W'])]   # layer-0 weights x scale
    mats = obnn.to_mat_list(p)
    x = (rs.normal(size=(B, 23)) * 3).astype(np.float32)
    x[::7] *= np.float32(1e4)                                                              # far-out rows
    mean, var = make_model(mats, E, H, dtype='f16x3').predict(x)
    rm, rv = obnn.forward(p, x, dtype=np.float64)
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    # within 2x the exact-f32 MFMA kernel's own error against the f64 oracle (adversarial scales make
    # cancellations that amplify every kernel's rounding alike), and at the fp32 parity tolerance (2e-5,
    # test_bnn_predict_split_vs_oracle) outright wherever the fp32 kernel itself meets it
    err = lambda a, b: float(np.max(np.abs(np.float64(a) - b) / (1 + np.abs(b))))
    mo, vo = make_model(mats, E, H, dtype='fp32').predict(x)
    e32m, e32v = err(mo, rm), err(vo, rv)
    assert err(mean, rm) <= max(2 * e32m, 2e-6), (err(mean, rm), e32m)
    assert err(var, rv) <= max(2 * e32v, 2e-6), (err(var, rv), e32v)
    if e32m <= 1e-5:
        assert err(mean, rm) <= 2e-5, err(mean, rm)
    if e32v <= 1e-5:
        assert err(var, rv) <= 2e-5, err(var, rv)


def test_fused_rollout_bf16_walker_runs():
    import torch
    from mopo_amd.bnn import construct_model
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout, init_sac_params
    model = construct_model(obs_dim=17, act_dim=6, hidden_dim=200, num_networks=7, num_elites=5,
                            separate_mean_var=True, seed=0, dtype='bf16')
    B = 4000
    pool = SimpleReplayPool(obs_dim=17, act_dim=6, max_size=B)
    env = torch.randn(9000, 17, device='cuda')
    env[:, 0] = 1.3
    env[:, 1] = 0.0
    ro = ModelRollout(model, B, 1)
    steps = ro.run(env, torch.from_numpy(init_sac_params(17, 6)).cuda(), pool, B, 1, 1, 1.0, [0, 1, 2, 3, 4], seed=3)
    assert steps.cpu().tolist() == [B] and pool.size == B
    f = pool.return_all_samples(as_numpy=True)
    assert np.isfinite(f['next_observations']).all()
    # walker2d termination (walker2d.py:10-16) applied to the stored next_obs
    h, a = f['next_observations'][:, 0], f['next_observations'][:, 1]
    exp = ~((h > 0.8) & (h < 2.0) & (a > -1.0) & (a < 1.0))
    near = (np.abs(h - 0.8) < 1e-5) | (np.abs(h - 2.0) < 1e-5) | (np.abs(np.abs(a) - 1.0) < 1e-5)
    assert (f['terminals'][:, 0] == exp)[~near].all()


def test_rollout_stops_when_every_row_is_done():
    """mopo.py:754-756: the horizon loop breaks once all rows are terminal -- walker2d rows at height
    50 all terminate in step 0, so only step 0's transitions enter the pool and the rest add 0."""
    import torch
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    B, horizon = 300, 4
    c = _rollout_case('walker2d', 7, 64, B, horizon, seed=5, height=50.0)
    assert c['steps'] == [B]                                       # the oracle broke after step 0
    model = make_model(c['mats'], 7, 64)
    pool = SimpleReplayPool(obs_dim=17, act_dim=6, max_size=B * horizon + 7)
    ro = ModelRollout(model, B, horizon)
    dev = torch.device('cuda')
    steps = ro.run(torch.from_numpy(c['env_obs']).to(dev), torch.from_numpy(c['flat']).to(dev), pool, B, horizon,
                   static_fns['walker2d'].term_kind, c['coeff'], c['elites'], start_idx=c['start'],
                   eps_act=c['eps_act'], eps_obs=c['eps_obs'], model_inds=c['inds'])
    np.testing.assert_array_equal(steps.cpu().numpy(), [B, 0, 0, 0])
    assert pool.size == B and pool._pointer == B
    got = pool.return_all_samples(as_numpy=True)
    assert got['terminals'].all()
    close(got['next_observations'], c['pool'].return_all_samples()['next_observations'], 5e-5)


@pytest.mark.parametrize('domain', ['ant', 'antangle', 'humanoid', 'walker2d', 'hopper', 'halfcheetahveljump',
                                    'point2dwallenv', 'pendulum'])
def test_fakeenv_termination_rules_on_device(domain):
    """FakeEnv.step's device termination (csrc/internal.h term_fn_at) applied to its own next_obs equals
    the oracle rule (pinned to mopo/static/<domain>.py by tests/golden/termination*.npz), including rows
    made non-finite outside column 0 and rows near every bound."""
    from mopo_amd.fake_env import FakeEnv
    from mopo_amd.static import static_fns
    rs = np.random.RandomState(5)
    B = 4096
    mats = obnn.to_mat_list(obnn.init_params(7, 17, 6, hidden=64, seed=8))
    model = make_model(mats, 7, 64)
    obs = rs.normal(size=(B, 17)).astype(np.float32)
    obs[:, 0] = rs.uniform(-0.5, 2.5, B)
    obs[:, 1] = rs.uniform(-1.5, 1.5, B)
    obs[:8, 5] = np.nan
    obs[8:16, 16] = np.inf
    obs[16:24, 3] = -np.inf
    obs[24:32, 0] = np.nan
    act = rs.uniform(-1, 1, (B, 6)).astype(np.float32)
    env = FakeEnv(model, static_fns[domain], penalty_coeff=1.0, penalty_learned_var=True)
    np.random.seed(3)
    with np.errstate(invalid='ignore'):
        nobs, rew, term, info = env.step(obs, act)
        exp = ofe.TERMINATION[domain](obs, act, nobs)
    assert term.shape == (B, 1) and term.dtype == bool
    np.testing.assert_array_equal(term, exp)
    if domain in ('ant', 'antangle', 'humanoid', 'walker2d', 'hopper'):
        assert 0 < term.sum() < B                     # both outcomes exercised
    else:
        assert not term.any()


def test_unknown_term_kind_rejected():
    from mopo_amd.fake_env import FakeEnv
    from mopo_amd.static import StaticFns
    mats = obnn.to_mat_list(obnn.init_params(7, 17, 6, hidden=64, seed=8))
    env = FakeEnv(make_model(mats, 7, 64), StaticFns('bogus', 9), penalty_coeff=1.0)
    with pytest.raises(RuntimeError, match='term_kind'):
        env.step(np.zeros((4, 17), np.float32), np.zeros((4, 6), np.float32))


def test_empty_batches():
    """Zero rows through every entry point: numpy-shaped empty outputs, pool unchanged (the
    reference's numpy code returns empty arrays for empty inputs)."""
    import torch
    from mopo_amd.fake_env import FakeEnv
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout, init_sac_params
    from mopo_amd.static import static_fns
    rs = np.random.RandomState(2)
    mats = obnn.to_mat_list(obnn.init_params(7, 17, 6, hidden=64, seed=3))
    model = make_model(mats, 7, 64)
    mean, var = model.predict(np.zeros((0, 23), np.float32), factored=True)
    assert mean.shape == (7, 0, 18) and var.shape == (7, 0, 18)
    env = FakeEnv(model, static_fns['halfcheetah'], penalty_coeff=1.0, penalty_learned_var=True)
    nobs, rew, term, info = env.step(np.zeros((0, 17), np.float32), np.zeros((0, 6), np.float32))
    assert nobs.shape == (0, 17) and rew.shape == (0, 1) and term.shape == (0, 1)
    pool = SimpleReplayPool(obs_dim=17, act_dim=6, max_size=100)
    pool.add_samples({'observations': np.zeros((0, 17)), 'actions': np.zeros((0, 6)), 'rewards': np.zeros((0, 1)),
                      'terminals': np.zeros((0, 1), bool), 'next_observations': np.zeros((0, 17))})
    assert pool.size == 0
    ro = ModelRollout(model, 64, 3)
    dev = torch.device('cuda')
    steps = ro.run(torch.from_numpy(rs.normal(size=(50, 17)).astype(np.float32)).to(dev),
                   torch.from_numpy(init_sac_params(17, 6)).to(dev), pool, 0, 3, 0, 1.0, [0, 1, 2, 3, 4])
    assert steps.cpu().numpy().tolist() == [0, 0, 0] and pool.size == 0


# the C2 workload itself (halfcheetah, E=7, H=200, B=50,000, h=5) is compared row for row over the whole pool
# below (test_full_pool_c2_rollout_vs_oracle); these sample 192 rows of the other full-size workloads
FULL_SIZE = [
    ('walker2d', 'fp32', 7, 200, 50000, 5, 1.0, 40000), ('walker2d', 'bf16x6', 7, 200, 50000, 5, 1.0, 40000),
    ('walker2d', 'f16x3', 7, 200, 50000, 5, 1.0, 40000),
    ('walker2d', 'bf16', 7, 200, 100000, 1, 1.0, 40000),                                     # C3
    ('halfcheetah', 'f16x3', 7, 200, 50000, 5, 5.0, 1000000),     # C4 per GPU: medium-expert, 1e6-row env pool
    ('halfcheetah', 'f16x3', 7, 200, 100000, 5, 1.0, 101000),     # N2: north_star's 100k rows, horizon 5
    ('halfcheetah', 'fp32', 32, 400, 125000, 5, 1.0, 40000), ('halfcheetah', 'f16x3', 32, 400, 125000, 5, 1.0, 40000),
    ('halfcheetah', 'bf16', 32, 400, 125000, 5, 1.0, 40000)]    # C5 per GPU


@pytest.mark.parametrize('domain,dtype,E,H,B,h,coeff,env_n', FULL_SIZE,
                         ids=['%s-%s-E%d-H%d-B%d-h%d-c%g-env%d' % c for c in FULL_SIZE])
def test_full_size_perf_mode_rows_vs_oracle(domain, dtype, E, H, B, h, coeff, env_n):
    """BASELINE workloads at full size (C2: E=7, H=200, B=50,000, h=5; C3: walker2d, bf16, B=100,000, h=1;
    C4: one GPU's share of halfcheetah-medium-expert, penalty_coeff 5 (halfcheetah_medium_expert.py:12-13),
    B=50,000 of 400k, h=5, from a 1e6-row env pool; N2: north_star's halfcheetah-mixed B=100,000, h=5;
    C5: one GPU's share, E=32, H=400, B=125,000, h=5, in fp32, f16x3 and bf16), learned-var penalty,
    perf-mode Philox streams
    (halfcheetah: split rollout, walker2d: order-preserving compaction between steps): 192 sampled rows
    are recomputed end to end by the oracle from the restated Philox streams (oracle/rng.py) and
    compared at their pool positions.  Start rows bit-exact, terminals bit-exact (bf16: except where the
    oracle's next state is within the bf16 tolerance of a walker bound), floats at the parity tolerance
    (5e-5; bf16 3e-2).  Under compaction a row's position at step i+1 is its rank among step i's
    survivors (mopo.py:758), taken from the device's own terminal flags of the other rows (the sampled
    rows' flags are checked against the oracle)."""
    _full_size_rows(domain, dtype, E, H, B, h, coeff, env_n)


_POOL_ERRS = {}


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x6', 'f16x3'])
def test_full_pool_c2_rollout_vs_oracle(dtype):
    """C2 at full size (halfcheetah-mixed: E=7, H=200, B=50,000, h=5, learned-var penalty, perf-mode Philox
    streams, split rollout): EVERY one of the 250,000 pool rows is recomputed by the oracle from the restated
    streams (oracle/rng.py) -- start rows bit-exact, terminals bit-exact, observations, actions, next
    observations and rewards within the fp32 parity tolerance 5e-5 (1 + |ref|) -- in exact-f32 MFMA, the
    exact-split bf16x6 and the f16x3 default."""
    _POOL_ERRS[dtype] = _full_pool_c2(dtype)


def test_full_size_16bit_error_distributions_match_fp32():
    """The C2 pool's scaled next-state errors against the f64 oracle (all 250,000 rows) in bf16x6 and f16x3
    have quantiles (50 / 90 / 99 / 100 %) within 2x of the exact-f32 MFMA kernel's, floor 2^-23."""
    for d in ('fp32', 'bf16x6', 'f16x3'):
        if d not in _POOL_ERRS:
            _POOL_ERRS[d] = _full_pool_c2(d)
    q32 = np.quantile(_POOL_ERRS['fp32'], (0.5, 0.9, 0.99, 1.0))
    for d in ('bf16x6', 'f16x3'):
        q = np.quantile(_POOL_ERRS[d], (0.5, 0.9, 0.99, 1.0))
        assert np.all(q <= np.maximum(2 * q32, 2.0 ** -23)), (d, q, q32)


C2_FULL = dict(O=17, A=6, E=7, H=200, B=50000, h=5, env_n=40000, coeff=1.0, seed=0x1234567890ab, epoch=3,
               elites=[4, 1, 0, 6, 2])
_C2_ORACLE = {}


def _c2_inputs():
    from mopo_amd.rollout import init_sac_params
    c = C2_FULL
    rs = np.random.RandomState(21)
    env_obs = rs.normal(size=(c['env_n'], c['O'])).astype(np.float32)
    mats = obnn.to_mat_list(obnn.init_params(c['E'], c['O'], c['A'], hidden=c['H'], seed=22,
                                             inputs=np.concatenate([env_obs[:2000], rs.uniform(-1, 1, (2000, c['A']))], 1)))
    return env_obs, mats, init_sac_params(c['O'], c['A'], 256, seed=23)


def _c2_oracle(chunk=12500):
    """The oracle's C2 rollout of all B rows (same inputs and streams for every dtype: computed once)."""
    if _C2_ORACLE:
        return _C2_ORACLE
    from oracle import rng as orng
    from mopo_amd.rollout import split_params
    c = C2_FULL
    O, A, E, B, h, seed, epoch = c['O'], c['A'], c['E'], c['B'], c['h'], c['seed'], c['epoch']
    env_obs, mats, flat = _c2_inputs()
    p = obnn.from_mat_list(mats)
    P = [q.astype(np.float64) for q in split_params(flat, O, A)[:8]]
    out = {k: [[] for _ in range(h)] for k in ('obs', 'act', 'nobs', 'rew', 'term')}
    for c0 in range(0, B, chunk):
        rows = np.arange(c0, min(B, c0 + chunk))
        obs = env_obs[orng.start_rows(rows, seed, epoch * 4096, c['env_n'])].astype(np.float64)
        for i in range(h):
            st = epoch * 4096 + 1 + i
            ea = orng.act_noise(rows, seed, st, A).astype(np.float64)
            act, _ = osac.actor_act(P, obs.astype(np.float32).astype(np.float64), ea)
            act = act.astype(np.float32)
            sel = orng.model_choice(rows, seed, st, c['elites'])
            noise = np.broadcast_to(orng.obs_noise(rows, seed, st, O + 1).astype(np.float64), (E, len(rows), O + 1))
            nobs, rew, term, _ = ofe.step(p, c['elites'], obs, act, ofe.TERMINATION['halfcheetah'],
                                          penalty_coeff=c['coeff'], penalty_learned_var=True, noise=noise, model_inds=sel)
            for k, v in (('obs', obs), ('act', act), ('nobs', nobs), ('rew', rew), ('term', term)):
                out[k][i].append(v)
            obs = nobs
    for k in out:
        _C2_ORACLE[k] = [np.concatenate(v) for v in out[k]]
    return _C2_ORACLE


def _full_pool_c2(dtype):
    """One full-size C2 rollout, every pool row against the oracle; returns the next-state scaled errors."""
    import torch
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    c = C2_FULL
    B, h, tol = c['B'], c['h'], 5e-5
    env_obs, mats, flat = _c2_inputs()
    model = make_model(mats, c['E'], c['H'], dtype=dtype)
    pool = SimpleReplayPool(obs_dim=c['O'], act_dim=c['A'], max_size=B * h)
    ro = ModelRollout(model, B, h)
    steps = ro.run(torch.from_numpy(env_obs).cuda(), torch.from_numpy(flat).cuda(), pool, B, h,
                   static_fns['halfcheetah'].term_kind, c['coeff'], c['elites'], seed=c['seed'],
                   epoch=c['epoch']).cpu().numpy()
    assert steps.tolist() == [B] * h and pool.size == B * h    # halfcheetah never terminates: no compaction
    dev = {k: v[:pool.size].cpu().numpy() for k, v in pool.fields.items()}
    ref = _c2_oracle()
    errs = []
    for i in range(h):
        got = {k: v[i * B:(i + 1) * B] for k, v in dev.items()}
        obs, act, nobs = ref['obs'][i], ref['act'][i], ref['nobs'][i]
        if i == 0:   # the start rows: an exact copy of the Philox-chosen env rows
            np.testing.assert_array_equal(got['observations'], obs.astype(np.float32))
        close(got['observations'], obs, tol)
        close(got['actions'], act, 5e-5 if i == 0 else tol)
        close(got['next_observations'], nobs, tol)
        close(got['rewards'], ref['rew'][i], tol)
        np.testing.assert_array_equal(got['terminals'], ref['term'][i])
        errs.append((np.abs(got['next_observations'] - nobs) / (1 + np.abs(nobs))).ravel())
    return np.concatenate(errs)


def _full_size_rows(domain, dtype, E, H, B, h, coeff, env_n):
    """Runs one full-size perf-mode rollout and checks 192 sampled rows against the oracle (see the
    test above); returns the per-step arrays of the rows' next-state scaled errors."""
    import torch
    from oracle import rng as orng
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout, init_sac_params, split_params
    from mopo_amd.static import static_fns
    O, A = 17, 6
    tol = 3e-2 if dtype == 'bf16' else 5e-5
    seed, epoch = 0x1234567890ab, 3
    rs = np.random.RandomState(21)
    env_obs = rs.normal(size=(env_n, O)).astype(np.float32)
    if domain == 'walker2d':
        env_obs[:, 0] = rs.uniform(0.9, 1.9, env_n)
        env_obs[:, 1] = rs.uniform(-0.9, 0.9, env_n)
    if domain in ('ant', 'antangle'):
        env_obs[:, 0] = rs.uniform(0.25, 0.95, env_n)
    if domain == 'humanoid':
        env_obs[:, 0] = rs.uniform(1.05, 1.95, env_n)
    mats = obnn.to_mat_list(obnn.init_params(E, O, A, hidden=H, seed=22,
                                             inputs=np.concatenate([env_obs[:2000], rs.uniform(-1, 1, (2000, A))], 1)))
    p = obnn.from_mat_list(mats)
    flat = init_sac_params(O, A, 256, seed=23)
    P = [q.astype(np.float64) for q in split_params(flat, O, A)[:8]]
    elites = [4, 1, 0, 6, 2]
    model = make_model(mats, E, H, dtype=dtype)
    pool = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=B * h)
    ro = ModelRollout(model, B, h)
    steps = ro.run(torch.from_numpy(env_obs).cuda(), torch.from_numpy(flat).cuda(), pool, B, h,
                   static_fns[domain].term_kind, coeff, elites, seed=seed, epoch=epoch).cpu().numpy()
    assert steps[0] == B and pool.size == steps.sum()
    if domain == 'halfcheetah':
        assert steps.tolist() == [B] * h
    term_dev = pool.fields['terminals'][:pool.size, 0].cpu().numpy()
    rows = np.sort(rs.choice(B, 192, replace=False))   # uids (global row ids) of the sampled rows
    idx = rows.copy()                                   # their positions within the current step
    obs = env_obs[orng.start_rows(rows, seed, epoch * 4096, env_n)].astype(np.float64)
    base, checked, errs = 0, 0, []
    for i in range(h):
        if len(rows) == 0:
            break
        st = epoch * 4096 + 1 + i
        ea = orng.act_noise(rows, seed, st, A).astype(np.float64)
        act, _ = osac.actor_act(P, obs.astype(np.float32).astype(np.float64), ea)
        act = act.astype(np.float32)
        sel = orng.model_choice(rows, seed, st, elites)
        noise = np.broadcast_to(orng.obs_noise(rows, seed, st, O + 1).astype(np.float64), (E, len(rows), O + 1))
        nobs, rew, term, _ = ofe.step(p, elites, obs, act, ofe.TERMINATION[domain], penalty_coeff=coeff,
                                      penalty_learned_var=True, noise=noise, model_inds=sel)
        pos = torch.from_numpy(base + idx).cuda()
        got = {k: v[pos].cpu().numpy() for k, v in pool.fields.items()}
        if i == 0:   # the start rows: an exact copy of the Philox-chosen env rows
            np.testing.assert_array_equal(got['observations'], obs.astype(np.float32))
        close(got['observations'], obs, tol)
        close(got['actions'], act, 5e-5 if i == 0 else tol)
        close(got['next_observations'], nobs, tol)
        errs.append((np.abs(got['next_observations'] - nobs) / (1 + np.abs(nobs))).ravel())
        close(got['rewards'], rew, tol)
        bad = got['terminals'][:, 0] != term[:, 0]
        if dtype == 'bf16' and bad.any():   # a bf16 next state may land on the other side of a bound
            hh, an = nobs[bad, 0], nobs[bad, 1]
            near = (np.abs(hh[:, None] - np.array([0.8, 2.0])).min(1) < tol * (1 + np.abs(hh))) | \
                   (np.abs(np.abs(an) - 1.0) < tol * (1 + np.abs(an)))
            assert near.all()
        else:
            np.testing.assert_array_equal(got['terminals'], term)
        checked += len(rows)
        live = ~term[:, 0]
        keep = ~term_dev[base:base + steps[i]]
        rank = np.cumsum(keep) - keep
        base += steps[i]
        rows, idx, obs = rows[live], rank[idx[live]], nobs[live]
    assert checked >= (192 * h if domain == 'halfcheetah' else min(192 * h, 192 + 64))   # walker: >= 1 compacted step
    return errs
