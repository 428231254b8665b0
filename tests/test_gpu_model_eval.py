"""GPU: model-based policy evaluation (ModelRollout.evaluate, csrc/rollout_eval.hip) against the oracle, against
the training rollout it must retrace, and through a MOPO epoch.

Tolerance: the project's per-step reward tolerance 5e-5 (1 + |r_t|) (test_gpu_rollout.py), summed over an
episode's steps: |d return| <= 5e-5 sum_t (1 + |r_t|).  Lengths and the terminated flags are bit-exact."""
import numpy as np
import pytest

from oracle import bnn as obnn
from oracle import fake_env as ofe
from oracle import sac as osac
from test_gpu_rollout import _rollout_case, make_model

pytestmark = pytest.mark.gpu
_CASES = {}


def _case(*a, **k):
    """_rollout_case, computed once per argument set (the dtypes share it; nothing modifies it)."""
    key = (a, tuple(sorted(k.items())))
    if key not in _CASES:
        _CASES[key] = _rollout_case(*a, **k)
    return _CASES[key]


def episode_sums(rew, term, steps, B):
    """Per-episode reward sum, sum of 1 + |r|, length and terminated flag from a rollout's pool rows
    (step-major; step i holds steps[i] rows, the survivors of step i - 1 in order: mopo.py:750-758)."""
    ret, scale = np.zeros(B), np.zeros(B)
    length, done = np.zeros(B, np.int32), np.zeros(B, np.uint8)
    ids, base = np.arange(B), 0
    for n in steps:
        n = int(n)
        if n == 0:
            break
        assert n == len(ids)
        r, t = np.asarray(rew[base:base + n], np.float64).ravel(), np.asarray(term[base:base + n]).ravel().astype(bool)
        ret[ids] += r
        scale[ids] += 1 + np.abs(r)
        length[ids] += 1
        done[ids[t]] = 1
        ids, base = ids[~t], base + n
    return ret, scale, length, done


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _evaluate_case(c, domain, E, H, B, T, dtype, **kw):
    import torch
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    model = make_model(c['mats'], E, H, dtype=dtype)
    dev = torch.device('cuda')
    ro = ModelRollout(model, B, 1)
    return _host(ro.evaluate(torch.from_numpy(c['env_obs']).to(dev), torch.from_numpy(c['flat']).to(dev), B, T,
                             static_fns[domain].term_kind, c['coeff'], c['elites'], start_idx=c['start'],
                             eps_obs=c['eps_obs'], model_inds=c['inds'], penalty_learned_var=c['learned_var'],
                             deterministic=c['det'], **kw))


def _check_against_pool(got, c, B, T):
    """The evaluation's penalized returns against the oracle pool's (penalized) rewards per episode."""
    ref = c['pool'].return_all_samples()
    ret, scale, length, done = episode_sums(ref['rewards'], ref['terminals'], c['steps'], B)
    exp_steps = np.zeros(T, np.int64)
    exp_steps[:len(c['steps'])] = c['steps']
    np.testing.assert_array_equal(got['steps'], exp_steps)
    np.testing.assert_array_equal(got['lengths'], length)
    np.testing.assert_array_equal(got['terminated'], done)
    err = np.abs(got['penalized_returns'] - ret) / scale
    print('max |d penalized return| / sum(1 + |r|) = %.3g' % err.max())
    assert err.max() <= 5e-5
    # reward = unpenalized - coeff * penalty at every step (fake_env.py:115), so the same of the sums
    np.testing.assert_allclose(got['returns'] - c['coeff'] * got['penalty_sums'], got['penalized_returns'],
                               rtol=0, atol=1e-9 * scale.max())
    assert (got['penalty_sums'] > 0).all()


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x6'])
@pytest.mark.parametrize('domain,E,H,B,T', [('walker2d', 7, 200, 777, 5), ('hopper', 7, 64, 300, 4),
                                            ('halfcheetah', 7, 200, 1000, 5)])
def test_sampled_policy_parity(domain, E, H, B, T, dtype):
    """policy_deterministic=False with the oracle rollout's injected streams: every episode's return and
    length equal the ones rebuilt from the oracle pool (the survivors followed through compaction)."""
    c = _case(domain, E, H, B, T, seed=11)
    got = _evaluate_case(c, domain, E, H, B, T, dtype, policy_deterministic=False, eps_act=c['eps_act'])
    _check_against_pool(got, c, B, T)
    if domain == 'halfcheetah':
        assert (got['lengths'] == T).all() and not got['terminated'].any()
    else:
        assert 0 < got['terminated'].sum() and got['lengths'].min() < T   # compaction exercised


def _det_oracle(domain, E, H, B, T, O=17, A=6):
    """Host loop of the oracle actor with zero policy noise (tanh(mu)) and the oracle FakeEnv.step; the numpy
    draws in the reference's order (normal, then choice) from a stream of its own."""
    from mopo_amd.rollout import split_params
    c = _case(domain, E, H, B, 1, seed=11)                  # inputs only: env pool, model, policy, start rows
    p = obnn.from_mat_list(c['mats'])
    P = [q.astype(np.float64) for q in split_params(c['flat'], O, A)[:8]]
    rs = np.random.RandomState(4711)
    eps_obs, inds_all = np.zeros((T, B, O + 1)), np.zeros((T, B), np.int32)
    ret, pret, scale = np.zeros(B), np.zeros(B), np.zeros(B)
    length, done, near = np.zeros(B, np.int32), np.zeros(B, np.uint8), np.zeros(B, bool)
    ids, obs = np.arange(B), c['env_obs'][c['start']]
    for i in range(T):
        n = len(ids)
        act, _ = osac.actor_act(P, obs.astype(np.float32).astype(np.float64), np.zeros((n, A)))
        noise = rs.normal(size=(E, n, O + 1))
        inds = rs.choice(c['elites'], size=n)
        nobs, rew, term, info = ofe.step(p, c['elites'], obs, act.astype(np.float32), ofe.TERMINATION[domain],
                                         penalty_coeff=1.0, penalty_learned_var=True, noise=noise, model_inds=inds)
        eps_obs[i, :n], inds_all[i, :n] = noise[inds, np.arange(n)], inds
        r = np.asarray(info['unpenalized_rewards'], np.float64).ravel()
        ret[ids] += r
        pret[ids] += np.asarray(rew, np.float64).ravel()
        scale[ids] += 1 + np.abs(r)
        length[ids] += 1
        hh, an = nobs[:, 0], nobs[:, 1]
        near[ids] |= (np.abs(hh[:, None] - np.array([0.8, 2.0])).min(1) < 1e-3) | (np.abs(np.abs(an) - 1.0) < 1e-3)
        t = term[:, 0]
        done[ids[t]] = 1
        if t.all():
            break
        ids, obs = ids[~t], nobs[~t]
    return dict(c=dict(c, eps_obs=eps_obs, inds=inds_all), ret=ret, pret=pret, scale=scale, length=length, done=done,
                near=near)


def test_deterministic_policy_parity():
    """policy_deterministic=True (tanh(mu): zero policy noise) on walker2d E=7, H=200, B=777, T=6 against a
    host loop of the oracle actor and oracle FakeEnv.step, summing info['unpenalized_rewards'].  An episode
    whose oracle height or angle comes within 1e-3 of a walker threshold (walker2d.py:10-16) at any step is
    excluded from the comparison; at most 1 % may be."""
    domain, E, H, B, T = 'walker2d', 7, 200, 777, 6
    o = _det_oracle(domain, E, H, B, T)
    ret, pret, scale, length, done, near, cc = (o[k] for k in ('ret', 'pret', 'scale', 'length', 'done', 'near', 'c'))
    print('oracle: %d of %d episodes near a threshold, lengths %d..%d, %d terminated'
          % (near.sum(), B, length.min(), length.max(), done.sum()))
    assert near.sum() <= B // 100
    assert length.min() < length.max() and done.sum() > B // 2    # the batch compacts at several steps
    got = _evaluate_case(cc, domain, E, H, B, T, 'fp32', policy_deterministic=True)
    ok = ~near
    np.testing.assert_array_equal(got['lengths'][ok], length[ok])
    np.testing.assert_array_equal(got['terminated'][ok], done[ok])
    err = np.abs(got['returns'] - ret)[ok] / scale[ok]
    perr = np.abs(got['penalized_returns'] - pret)[ok] / scale[ok]
    print('max |d return| / sum(1 + |r|) = %.3g (penalized %.3g)' % (err.max(), perr.max()))
    assert err.max() <= 5e-5 and perr.max() <= 5e-5


@pytest.mark.parametrize('learned_var,det', [(False, False), (True, True), (False, True)])
def test_modes_parity(learned_var, det):
    """The mean-distance penalty and FakeEnv's deterministic mode (fake_env.py:69-70, 84-86, 98-108) on
    halfcheetah E=32, H=32, B=64, T=3 against the oracle."""
    domain, E, H, B, T = 'halfcheetah', 32, 32, 64, 3
    c = _case(domain, E, H, B, T, seed=13, coeff=2.0, learned_var=learned_var, det=det)
    got = _evaluate_case(c, domain, E, H, B, T, 'fp32', policy_deterministic=False, eps_act=c['eps_act'])
    _check_against_pool(got, c, B, T)


def _perf_setup(O, A, domain, n_env=6000, seed=0):
    import torch
    from mopo_amd.bnn import construct_model
    from mopo_amd.rollout import init_sac_params
    rs = np.random.RandomState(3)
    env = rs.normal(size=(n_env, O)).astype(np.float32)
    if domain == 'hopper':
        env[:, 0], env[:, 1] = rs.uniform(0.75, 1.5, n_env), rs.uniform(-0.15, 0.15, n_env)
    if domain == 'ant':
        env[:, 0] = rs.uniform(0.3, 0.9, n_env)
    model = construct_model(obs_dim=O, act_dim=A, hidden_dim=200, num_networks=7, num_elites=5,
                            separate_mean_var=True, seed=seed, dtype='fp32')
    return model, torch.from_numpy(env).cuda(), torch.from_numpy(init_sac_params(O, A)).cuda()


@pytest.mark.parametrize('domain,O,A,B,T', [('halfcheetah', 17, 6, 1000, 5), ('ant', 27, 8, 300, 4)])
def test_perf_mode_retraces_the_training_rollout(domain, O, A, B, T):
    """At the same (seed, epoch) evaluate(policy_deterministic=False) visits the trajectories run() writes to
    its pool: per episode, the penalized return equals the sum of the pooled rewards (pool rows i B + b for
    halfcheetah; ant's survivors followed through the compaction), lengths and terminals bit-exact.  The pool
    holds f32 rewards: |d| <= sum_t 2^-24 |r_t|, plus the f64 sum's own rounding."""
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    model, env, pi = _perf_setup(O, A, domain)
    kind, el = static_fns[domain].term_kind, [0, 1, 2, 3, 4]
    pool = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=B * T)
    ro = ModelRollout(model, B, T)
    steps = ro.run(env, pi, pool, B, T, kind, 1.0, el, seed=7, epoch=2).cpu().numpy()
    got = _host(ro.evaluate(env, pi, B, T, kind, 1.0, el, policy_deterministic=False, seed=7, epoch=2))
    rew = pool.fields['rewards'][:pool.size].cpu().numpy()
    term = pool.fields['terminals'][:pool.size].cpu().numpy()
    ret, scale, length, done = episode_sums(rew, term, steps, B)
    np.testing.assert_array_equal(got['steps'], steps)
    np.testing.assert_array_equal(got['lengths'], length)
    np.testing.assert_array_equal(got['terminated'], done)
    bound = (2.0 ** -24 + 1e-12) * (scale - length)            # scale - length = sum_t |r_t|
    err = np.abs(got['penalized_returns'] - ret)
    print('max |d| = %.3g, max |d| / bound = %.3g' % (err.max(), (err / bound).max()))
    assert (err <= bound).all()
    if domain == 'halfcheetah':
        assert steps.tolist() == [B] * T
        np.testing.assert_array_equal(ret, rew.reshape(T, B).astype(np.float64).sum(0))
    else:
        assert 0 < done.sum() and steps[-1] < B                 # ant: rows end, the batch compacts


def test_perf_mode_hopper_lengths_repeat_and_long_episodes():
    """Hopper (compaction): the lengths add up to run()'s steps; two identical calls agree bit for bit, stats
    included; T = 40 runs on a handle created with max_horizon = 5, past the live-count read-back at step 32."""
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    O, A, B, T = 11, 3, 1000, 5
    model, env, pi = _perf_setup(O, A, 'hopper')
    kind, el = static_fns['hopper'].term_kind, [0, 1, 2, 3, 4]
    pool = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=B * T)
    ro = ModelRollout(model, B, T)
    steps = ro.run(env, pi, pool, B, T, kind, 1.0, el, seed=9, epoch=1).cpu().numpy()
    a = _host(ro.evaluate(env, pi, B, T, kind, 1.0, el, policy_deterministic=False, seed=9, epoch=1))
    b = _host(ro.evaluate(env, pi, B, T, kind, 1.0, el, policy_deterministic=False, seed=9, epoch=1))
    assert int(a['lengths'].sum()) == int(steps.sum()) == pool.size
    np.testing.assert_array_equal(a['steps'], steps)
    assert a['terminated'].sum() > 0 and a['lengths'].min() < a['lengths'].max()
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    long = _host(ro.evaluate(env, pi, B, 40, kind, 1.0, el, seed=9, epoch=1))      # tanh(mu), the default
    assert long['lengths'].max() <= 40 and long['lengths'].min() >= 1
    assert int(long['lengths'].sum()) == int(long['steps'].sum()) and long['steps'][0] == B
    assert (long['terminated'][long['lengths'] < 40] == 1).all() and (long['lengths'][long['terminated'] == 0] == 40).all()
    assert np.isfinite(long['returns']).all() and np.isfinite(long['stats']).all()


def test_results_do_not_depend_on_the_live_count_readback(monkeypatch):
    """The loop reads the live count back every MOPO_EVAL_POLL steps (default 32) to stop early.  Walker2d,
    B = 777, T = 6: read back after every step (episodes still alive: the loop goes on; none left: it stops),
    every second step, and never -- all outputs bit-identical to the default's."""
    import torch
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    c = _case('walker2d', 7, 200, 777, 1, seed=11)
    ro = ModelRollout(make_model(c['mats'], 7, 200), 777, 1)
    env, pi = torch.from_numpy(c['env_obs']).cuda(), torch.from_numpy(c['flat']).cuda()

    def run():
        return _host(ro.evaluate(env, pi, 777, 6, static_fns['walker2d'].term_kind, 1.0, c['elites'], seed=21, epoch=3))
    ref = run()
    assert ref['steps'][1] > 0 and ref['lengths'].min() < ref['lengths'].max()
    for n in ('1', '2', '0'):
        monkeypatch.setenv('MOPO_EVAL_POLL', n)
        got = run()
        for k in ref:
            np.testing.assert_array_equal(got[k], ref[k], err_msg='MOPO_EVAL_POLL=%s %s' % (n, k))


def _check_stats(out):
    from mopo_amd.evaluation import model_evaluation_metrics, model_evaluation_metrics_numpy
    import torch
    exp = model_evaluation_metrics_numpy(out['returns'], out['lengths'], out['penalized_returns'], out['penalty_sums'],
                                         out['terminated'])
    got = model_evaluation_metrics(torch.from_numpy(out['stats']))
    for k, v in exp.items():
        print('%-26s device %.17g numpy %.17g' % (k, got[k], v))
        assert abs(got[k] - v) <= 1e-12 * abs(v), k
    assert out['stats'][11] == len(out['returns']) and not out['stats'][12:].any()


def test_device_stats_equal_numpy():
    """stats against numpy on the returned per-episode arrays at rel 1e-12: a walker batch whose episodes end
    at different steps, a batch of 1, and a batch in which every episode ends at step 1 (walker height 50)."""
    import torch
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    E, H, B, T = 7, 64, 300, 4
    kind = static_fns['walker2d'].term_kind
    for height, n in ((None, B), (None, 1), (50.0, B)):
        c = _case('walker2d', E, H, B, T, seed=5, height=height)
        model = make_model(c['mats'], E, H)
        ro = ModelRollout(model, B, 1)
        out = _host(ro.evaluate(torch.from_numpy(c['env_obs']).cuda(), torch.from_numpy(c['flat']).cuda(), n, T, kind,
                                1.0, c['elites'], seed=3))
        _check_stats(out)
        if height is not None:
            assert (out['lengths'] == 1).all() and out['terminated'].all()
            assert out['steps'].tolist() == [B, 0, 0, 0]
            assert out['stats'][4:8].tolist() == [1.0, 1.0, 1.0, 0.0] and out['stats'][10] == 1.0
        elif n == B:
            assert out['lengths'].min() < out['lengths'].max()


def _mopo(eval_episodes):
    from mopo_amd.mopo import MOPO
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.static import static_fns
    rs = np.random.RandomState(2)
    n = 3000
    obs = rs.normal(size=(n, 17)).astype(np.float32)
    obs[:, 0], obs[:, 1] = rs.uniform(0.9, 1.9, n), rs.uniform(-0.9, 0.9, n)
    pool = SimpleReplayPool(obs_dim=17, act_dim=6, max_size=n)
    pool.add_samples({'observations': obs, 'actions': rs.uniform(-1, 1, (n, 6)), 'rewards': rs.normal(size=(n, 1)),
                      'terminals': np.zeros((n, 1), bool), 'next_observations': obs + 0.1})
    np.random.seed(123)
    algo = MOPO(pool, static_fns['walker2d'], 17, 6, rollout_batch_size=500, rollout_length=2, epoch_length=20,
                model_train_freq=20, separate_mean_var=True, penalty_coeff=1.0, penalty_learned_var=True,
                real_ratio=0.05, target_entropy=-3, seed=5, model_eval_episodes=eval_episodes, model_eval_length=20)
    algo._model.set_elites([0, 1, 2, 3, 4])
    algo._model_train_metrics = {}                     # the model is given (no BNN.train in this epoch)
    d = list(algo.train(1))[0]
    import torch
    torch.cuda.synchronize()
    mp = algo._model_pool
    state = {'sac': algo._sac.get_params()[0].cpu().numpy(), 'ptr': (mp._pointer, mp.size),
             'pool': {k: v[:mp.size].cpu().numpy() for k, v in mp.fields.items()}, 'np': np.random.get_state()}
    return d, state


def test_mopo_epoch_with_model_evaluation_changes_nothing_else():
    """One epoch with model_eval_episodes=64, model_eval_length=20 and one without: SAC parameters, model pool
    and numpy's global stream bit-identical; the model_eval/* keys present and finite only in the first."""
    from mopo_amd.evaluation import MODEL_EVAL_KEYS
    d1, s1 = _mopo(64)
    d0, s0 = _mopo(0)
    np.testing.assert_array_equal(s1['sac'], s0['sac'])
    assert s1['ptr'] == s0['ptr'] and s1['ptr'][1] > 0
    for k in s0['pool']:
        np.testing.assert_array_equal(s1['pool'][k], s0['pool'][k], err_msg=k)
    assert s1['np'][0] == s0['np'][0] and s1['np'][2:] == s0['np'][2:]
    np.testing.assert_array_equal(s1['np'][1], s0['np'][1])
    assert not [k for k in d0 if k.startswith('model_eval/') or k == 'times/model_eval']
    for k in MODEL_EVAL_KEYS:
        assert np.isfinite(d1['model_eval/' + k]), k
    assert d1['times/model_eval'] > 0 and 1 <= d1['model_eval/episode-length-avg'] <= 20
    assert not [k for k in d1 if k.startswith('perf/')]          # no D4RL score from the model
    assert [k for k in d1 if not k.startswith('model_eval/') and k != 'times/model_eval'] == list(d0)


def test_refusals():
    import torch
    from mopo_amd import _lib as L
    from mopo_amd.rollout import ModelRollout
    c = _case('halfcheetah', 32, 32, 64, 3, seed=13, coeff=2.0, learned_var=False, det=False)
    ro = ModelRollout(make_model(c['mats'], 32, 32), 64, 3)
    env, pi = torch.from_numpy(c['env_obs']).cuda(), torch.from_numpy(c['flat']).cuda()
    with pytest.raises(L.MopoError, match='4095'):
        ro.evaluate(env, pi, 64, 4096, 0, 1.0, c['elites'])
    with pytest.raises(L.MopoError, match='4095'):
        ro.evaluate(env, pi, 64, 0, 0, 1.0, c['elites'])
    with pytest.raises(L.MopoError, match='max_batch'):
        ro.evaluate(env, pi, 65, 3, 0, 1.0, c['elites'])
    with pytest.raises(L.MopoError, match='rollout_random'):
        ro.evaluate(env, pi, 64, 3, 0, 1.0, c['elites'], policy_deterministic=True, rollout_random=True)
    with pytest.raises(L.MopoError, match='term_kind'):
        ro.evaluate(env, pi, 64, 3, 9, 1.0, c['elites'])
    out = ro.evaluate(env, pi, 64, 3, 0, 1.0, c['elites'], policy_deterministic=False, rollout_random=True)
    assert (out['lengths'] == 3).all().item()                     # the handle still works after a refusal
