"""GPU: open-loop model validation (ModelRollout.validate, csrc/rollout_val.hip) against a host loop of the oracle
FakeEnv.step fed the dataset's actions, plus ``segment_lengths_numpy`` for the continuation rule.

Tolerances (none taken from the code under test):
* lengths, end reasons, steps, start rows, the NaN / 0xFF tails: bit-exact.
* errors, obs_errors: |d| <= 5e-5 ||1 + |ref|||_2, ref the oracle's (reward, next_obs) vector of that step -- the
  project's per-element 5e-5 (1 + |ref|) carried through the triangle inequality of the norm.
* penalties: rel 1e-5 at step 0 (the one-step tolerance), 5e-5 (1 + |ref|) at later steps (the multi-step
  tolerance test_gpu_rollout.py holds reward - 2 penalty to).
* term_pred: exact wherever the oracle's deciding quantity is more than 1e-3 from its threshold; the mask may
  drop at most 2 % of the compared entries."""
import numpy as np
import pytest

from oracle import bnn as obnn
from oracle import fake_env as ofe
from oracle import rng as orng

pytestmark = pytest.mark.gpu

SHAPES = {'halfcheetah': (17, 6, 200), 'walker2d': (17, 6, 64), 'hopper': (11, 3, 64), 'ant': (27, 8, 200)}
E, ELITES, K, N_ROWS = 7, [4, 1, 0, 6, 2], 5, 600
_POOLS, _ORACLES, _MODELS = {}, {}, {}


@pytest.fixture(scope='module', autouse=True)
def _drop_models():
    """The shared device models go with the module, not with the interpreter."""
    yield
    _MODELS.clear()


def _dataset(domain):
    """600 rows of episodes of length 1..40, next_obs[j] == obs[j + 1] inside an episode; every third episode
    ends with terminals = 1, the others by a discontinuity (the next episode starts somewhere else).  The
    oracle model's weights ride along.  Built once per domain, never modified."""
    if domain in _POOLS:
        return _POOLS[domain]
    O, A, H = SHAPES[domain]
    rs = np.random.RandomState(sum(map(ord, domain)))
    obs, nobs, term, ends = [], [], [], []
    n, ep = 0, 0
    while n < N_ROWS:
        L = min(int(rs.randint(1, 41)), N_ROWS - n)
        o = rs.normal(size=O)
        if domain == 'walker2d':
            o[0], o[1] = rs.uniform(1.0, 1.8), rs.uniform(-0.8, 0.8)
        if domain == 'hopper':
            o[0], o[1] = rs.uniform(0.8, 1.5), rs.uniform(-0.15, 0.15)
        if domain == 'ant':
            o[0] = rs.uniform(0.3, 0.9)
        chain = (o + np.cumsum(np.concatenate([np.zeros((1, O)), rs.normal(size=(L, O)) * 0.02]), 0)).astype(np.float32)
        obs.append(chain[:-1])
        nobs.append(chain[1:])
        t = np.zeros(L, np.uint8)
        t[-1] = ep % 3 == 0
        term.append(t)
        n, ep = n + L, ep + 1
        ends.append(n - 1)
    d = {'observations': np.concatenate(obs), 'next_observations': np.concatenate(nobs),
         'terminals': np.concatenate(term), 'actions': rs.uniform(-1, 1, (N_ROWS, A)).astype(np.float32),
         'rewards': rs.normal(size=(N_ROWS, 1)).astype(np.float32), 'ends': np.array(ends)}
    assert d['observations'].shape == (N_ROWS, O) and ep >= 9
    inputs = np.concatenate([d['observations'], d['actions']], 1)
    d['mats'] = obnn.to_mat_list(obnn.init_params(E, O, A, hidden=H, seed=7, inputs=inputs))
    _POOLS[domain] = d
    return d


def _starts(d, B, seed=1):
    """Injected start rows: the first four are placed (the pool's last row, two rows before a terminal, two
    rows before an unflagged boundary, an episode's first row), the rest uniform."""
    rs = np.random.RandomState(seed)
    ends, term = d['ends'], d['terminals']
    long = ends[:-1][np.diff(np.concatenate([[-1], ends]))[:-1] >= 3]      # last rows of episodes of >= 3 rows
    t_end = [e for e in long if term[e]][0]
    d_end = [e for e in long if not term[e]][0]
    placed = [N_ROWS - 1, t_end - 1, d_end - 1, int(ends[0]) + 1]
    return np.array((placed + rs.randint(0, N_ROWS, max(B - 4, 0)).tolist())[:B], np.int64)


def _near(domain, nobs):
    """Rows whose deciding quantity of the domain's termination rule lies within 1e-3 of a threshold."""
    if domain == 'walker2d':
        return (np.abs(nobs[:, :1] - np.array([0.8, 2.0])).min(1) < 1e-3) | (np.abs(np.abs(nobs[:, 1]) - 1.0) < 1e-3)
    if domain == 'hopper':
        return (np.abs(nobs[:, 0] - 0.7) < 1e-3) | (np.abs(np.abs(nobs[:, 1]) - 0.2) < 1e-3) | \
            (np.abs(nobs[:, 1:] - 100.0).min(1) < 1e-3)
    if domain == 'ant':
        return np.abs(nobs[:, :1] - np.array([0.2, 1.0])).min(1) < 1e-3
    return np.zeros(len(nobs), bool)


def _oracle(d, domain, starts, K, learned_var, det, draws):
    """The host loop: oracle FakeEnv.step on (model state, dataset action) per step, the live segments in their
    original order (the device's order-preserving compaction).  ``draws(k, ids)`` -> (noise of the selected
    member [n, D], member per row [n]).  Returns the per-(step, segment) tables and the injected streams."""
    from mopo_amd.evaluation import segment_lengths_numpy
    p = obnn.from_mat_list(d['mats'])
    B, O = len(starts), d['observations'].shape[1]
    D = O + 1
    lengths, ends = segment_lengths_numpy(d['observations'], d['next_observations'], d['terminals'], N_ROWS, starts, K)
    out = {k: np.full((K, B), np.nan) for k in ('errors', 'obs_errors', 'reward_errors', 'penalties', 'tol')}
    out.update(term_pred=np.full((K, B), 255, np.uint8), term_data=np.full((K, B), 255, np.uint8),
               near=np.zeros((K, B), bool), lengths=lengths, end_reasons=ends, steps=np.zeros(K, np.int64),
               eps_obs=np.zeros((K, B, D)), inds=np.zeros((K, B), np.int32))
    ids = np.arange(B)[lengths > 0]
    obs = d['observations'][starts[ids]].astype(np.float64)
    for k in range(K):
        n = len(ids)
        out['steps'][k] = n
        if n == 0:
            break
        j = starts[ids] + k
        noise_sel, inds = draws(k, ids)
        noise = np.zeros((E, n, D))
        noise[inds, np.arange(n)] = noise_sel
        nobs, _, term, info = ofe.step(p, ELITES, obs, d['actions'][j], ofe.TERMINATION[domain], penalty_coeff=1.0,
                                       penalty_learned_var=learned_var, deterministic=det, noise=noise,
                                       model_inds=inds)
        rew = np.asarray(info['unpenalized_rewards'], np.float64).ravel()
        nobs = np.asarray(nobs, np.float64)
        eo = np.linalg.norm(nobs - d['next_observations'][j].astype(np.float64), axis=1)
        er = rew - d['rewards'][j, 0].astype(np.float64)
        ref = np.concatenate([rew[:, None], nobs], 1)
        out['errors'][k, ids], out['obs_errors'][k, ids], out['reward_errors'][k, ids] = np.hypot(eo, er), eo, er
        out['penalties'][k, ids] = np.asarray(info['penalty'], np.float64).ravel()
        out['tol'][k, ids] = 5e-5 * np.linalg.norm(1 + np.abs(ref), axis=1)
        out['term_pred'][k, ids], out['term_data'][k, ids] = term[:, 0], d['terminals'][j]
        out['near'][k, ids] = _near(domain, nobs)
        out['eps_obs'][k, :n], out['inds'][k, :n] = noise_sel, inds
        go = lengths[ids] > k + 1
        ids, obs = ids[go], nobs[go]
    return out


def _parity_oracle(domain, B, learned_var, det):
    key = (domain, B, learned_var, det)
    if key not in _ORACLES:
        d = _dataset(domain)
        rs = np.random.RandomState(B)
        D = d['observations'].shape[1] + 1
        _ORACLES[key] = _oracle(d, domain, _starts(d, B), K, learned_var, det,
                                lambda k, ids: (rs.normal(size=(len(ids), D)), rs.choice(ELITES, size=len(ids))))
    return _ORACLES[key]


def _model(domain, dtype):
    from mopo_amd.bnn import BNN
    if (domain, dtype) not in _MODELS:
        O, A, H = SHAPES[domain]
        m = BNN({'name': 't', 'num_networks': E, 'num_elites': 5, 'separate_mean_var': True, 'obs_dim': O,
                 'act_dim': A, 'hidden_dim': H, 'dtype': dtype})
        _MODELS[(domain, dtype)] = m.set_params(_dataset(domain)['mats'])
    return _MODELS[(domain, dtype)]


def _device_pool(d, size=None, max_size=N_ROWS):
    from mopo_amd.replay_pool import SimpleReplayPool
    O, A = d['observations'].shape[1], d['actions'].shape[1]
    pool = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=max_size)
    n = N_ROWS if size is None else size
    if n:
        pool.add_samples({k: d[k][:n] for k in ('observations', 'actions', 'rewards', 'terminals',
                                                'next_observations')})
    return pool


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _term_kind(domain):
    from mopo_amd.static import static_fns
    return static_fns[domain].term_kind


def _compare(got, ref, label=''):
    """The device tables against the oracle's at the module docstring's tolerances."""
    for k in ('lengths', 'end_reasons', 'steps', 'term_data'):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    live = np.arange(ref['errors'].shape[0])[:, None] < ref['lengths'][None, :]
    for k in ('errors', 'obs_errors', 'reward_errors', 'penalties'):
        assert np.isnan(got[k][~live]).all() and np.isfinite(got[k][live]).all(), k
    assert (got['term_pred'][~live] == 255).all() and (got['term_pred'][live] <= 1).all()
    if not live.any():
        return
    for k in ('errors', 'obs_errors'):
        r = (np.abs(got[k] - ref[k]) / ref['tol'])[live]
        print('%s %s: max |d| / (5e-5 ||1 + |ref|||) = %.3g' % (label, k, r.max()))
        assert r.max() <= 1.0, k
    pg, pr = got['penalties'].astype(np.float64), ref['penalties']
    r0 = (np.abs(pg[0] - pr[0]) / np.abs(pr[0]))[live[0]]
    print('%s penalty step 0: max rel %.3g' % (label, r0.max()))
    assert r0.max() <= 1e-5
    if live[1:].any():
        r1 = (np.abs(pg[1:] - pr[1:]) / (1 + np.abs(pr[1:])))[live[1:]]
        print('%s penalty steps >= 1: max |d| / (1 + |ref|) = %.3g' % (label, r1.max()))
        assert r1.max() <= 5e-5
    ok = live & ~ref['near']
    assert (live & ref['near']).sum() <= 0.02 * live.sum()
    np.testing.assert_array_equal(got['term_pred'][ok], ref['term_pred'][ok])


def _validate(domain, dtype, B, ref, learned_var, det, ro=None, pool=None, **kw):
    import torch
    from mopo_amd.rollout import ModelRollout
    ro = ro or ModelRollout(_model(domain, dtype), 257, 1)
    pool = pool or _device_pool(_dataset(domain))
    out = ro.validate(pool, B, K, _term_kind(domain), ELITES, start_idx=ref['starts'] if 'starts' in ref else None,
                      eps_obs=None if det else ref['eps_obs'], model_inds=None if det else ref['inds'],
                      penalty_learned_var=learned_var, deterministic=det, **kw)
    torch.cuda.synchronize()
    return _host(out)


def test_the_pool_exercises_every_end_reason():
    """On the oracle's values alone: every end reason occurs and at least a quarter of the segments reach step
    K - 1, for each batch the parity tests run (B = 1 is a single placed row)."""
    from mopo_amd.evaluation import segment_lengths_numpy
    for domain in SHAPES:
        d = _dataset(domain)
        inside = d['ends'][:-1]
        np.testing.assert_array_equal(d['next_observations'][:-1][np.setdiff1d(np.arange(N_ROWS - 1), inside)],
                                      d['observations'][1:][np.setdiff1d(np.arange(N_ROWS - 1), inside)])
        assert (d['next_observations'][inside] != d['observations'][inside + 1]).any(1).all()
        for B in (65, 257):
            length, end = segment_lengths_numpy(d['observations'], d['next_observations'], d['terminals'], N_ROWS,
                                                _starts(d, B), K)
            assert set(end.tolist()) == {0, 1, 2, 3}, (domain, B)
            assert (length == K).sum() >= B / 4 and length.min() >= 1


PARITY = [(dom, dt, True, True) for dom in SHAPES for dt in ('fp32', 'bf16x6')] + \
         [('halfcheetah', 'f16x3', True, True)] + \
         [('walker2d', 'fp32', lv, det) for lv, det in ((True, False), (False, True), (False, False))] + \
         [('ant', 'bf16x6', True, False)]


@pytest.mark.parametrize('domain,dtype,learned_var,det', PARITY)
def test_parity_with_the_oracle(domain, dtype, learned_var, det):
    """K = 5, B in {1, 65, 257}, every stream injected."""
    from mopo_amd.rollout import ModelRollout
    d = _dataset(domain)
    ro, pool = ModelRollout(_model(domain, dtype), 257, 1), _device_pool(d)
    for B in (1, 65, 257):
        ref = dict(_parity_oracle(domain, B, learned_var, det), starts=_starts(d, B))
        got = _validate(domain, dtype, B, ref, learned_var, det, ro=ro, pool=pool)
        np.testing.assert_array_equal(got['start_rows'], ref['starts'])
        _compare(got, ref, '%s %s B=%d' % (domain, dtype, B))


def _check_stats(got, learned_var, corr=True):
    from mopo_amd.evaluation import open_loop_metrics_numpy
    exp = open_loop_metrics_numpy(got['errors'], got['obs_errors'], got['reward_errors'], got['penalties'],
                                  got['term_pred'], got['term_data'], got['lengths'], penalty_learned_var=learned_var)
    s = got['stats']
    assert s.shape == exp.shape and not s[:, 11:].any()
    np.testing.assert_array_equal(s[:, 0], exp[:, 0])
    np.testing.assert_array_equal(s[:-1, 0], got['steps'])
    # sums and means at rel 1e-10.  A standard deviation is a sum of squared deviations x - mean, each carrying
    # the mean's rounding error, which is relative to |mean| and not to the deviation (65 equal values have
    # std 0 exactly or 1e-16 |mean|, by the order of the sum): its scale is std + |mean|.
    scale = {2: np.abs(exp[:, 2]) + np.abs(exp[:, 1]), 7: np.abs(exp[:, 7]) + np.abs(exp[:, 6])}
    for c in (1, 2, 3, 4, 5, 6, 7, 9, 10):
        sc = scale.get(c, np.abs(exp[:, c]))
        print('slot %d: max |d| / scale %.3g' % (c, np.max(np.abs(s[:, c] - exp[:, c]) / np.maximum(sc, 1e-300))))
        assert (np.abs(s[:, c] - exp[:, c]) <= 1e-10 * sc).all(), c
    if corr:   # not for a batch of equal values: its variances are 0 or rounding noise by the order of the sums
        print('correlation: max abs %.3g' % np.abs(s[:, 8] - exp[:, 8]).max())
        assert np.abs(s[:, 8] - exp[:, 8]).max() <= 1e-9
    assert (np.abs(s[:, 8]) <= 1 + 1e-12).all()


@pytest.mark.parametrize('learned_var', [True, False])
def test_device_stats_equal_numpy_and_repeat(learned_var, monkeypatch):
    """stats against open_loop_metrics_numpy of the device's own tables (f64 sums of at most 1285 terms: rel
    1e-10, the correlation abs 1e-9); two runs and runs with the live count read back never / after every step
    are bit-identical."""
    domain, B = 'walker2d', 257
    ref = dict(_parity_oracle(domain, B, learned_var, False), starts=_starts(_dataset(domain), B))
    a = _validate(domain, 'fp32', B, ref, learned_var, False)
    _check_stats(a, learned_var)
    assert a['stats'][K, 0] == a['lengths'].sum() and 0 < a['stats'][K, 8] ** 2 < 1
    b = _validate(domain, 'fp32', B, ref, learned_var, False)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for n in ('0', '1'):
        monkeypatch.setenv('MOPO_EVAL_POLL', n)
        c = _validate(domain, 'fp32', B, ref, learned_var, False)
        for k in a:
            np.testing.assert_array_equal(a[k], c[k], err_msg='MOPO_EVAL_POLL=%s %s' % (n, k))
    # one segment, and a batch whose segments all end after their first step
    one = _validate(domain, 'fp32', 1, dict(ref, starts=ref['starts'][:1]), learned_var, True)
    _check_stats(one, learned_var)
    assert (one['stats'][:, 8] == 0).all()
    last = dict(ref, starts=np.full(65, N_ROWS - 1, np.int64))
    got = _validate(domain, 'fp32', 65, last, learned_var, True)
    _check_stats(got, learned_var, corr=False)
    assert got['steps'].tolist() == [65, 0, 0, 0, 0] and (got['end_reasons'] == 3).all()
    assert not got['stats'][1:K].any() and (got['stats'][0] == got['stats'][K]).all()


def test_perf_mode():
    """Philox streams: the same seed gives the same bits, another seed differs; the start rows are
    oracle.rng.start_rows'; 32 sampled segments recomputed end to end from oracle.rng's member choice and
    observation noise, at the parity tolerances."""
    from mopo_amd.rollout import ModelRollout
    domain, B, seed, epoch, off = 'walker2d', 257, 0x1234567, 3, 1000
    d = _dataset(domain)
    ro, pool = ModelRollout(_model(domain, 'fp32'), 257, 1), _device_pool(d)
    kw = dict(ro=ro, pool=pool, epoch=epoch, uid_offset=off)
    a = _validate(domain, 'fp32', B, {}, True, True, seed=seed, **kw)          # deterministic: start rows only
    uid = off + np.arange(B)
    starts = orng.start_rows(uid, seed, epoch * 4096, N_ROWS)
    np.testing.assert_array_equal(a['start_rows'], starts)
    assert len(set(starts.tolist())) > B // 2
    ref = {'eps_obs': None, 'inds': None}
    s1 = _validate(domain, 'fp32', B, ref, True, False, seed=seed, **kw)
    s2 = _validate(domain, 'fp32', B, ref, True, False, seed=seed, **kw)
    s3 = _validate(domain, 'fp32', B, ref, True, False, seed=seed + 1, **kw)
    for k in s1:
        np.testing.assert_array_equal(s1[k], s2[k], err_msg=k)
    assert (s1['start_rows'] != s3['start_rows']).any() and (s1['errors'][0] != s3['errors'][0]).any()
    np.testing.assert_array_equal(s1['start_rows'], starts)
    pick = np.random.RandomState(0).choice(B, 32, replace=False)
    D = d['observations'].shape[1] + 1

    def draws(k, ids):
        u, step = off + pick[ids], epoch * 4096 + 1 + k
        return orng.obs_noise(u, seed, step, D).astype(np.float64), orng.model_choice(u, seed, step, ELITES)
    ref = _oracle(d, domain, starts[pick], K, True, False, draws)
    sub = {k: (v[:, pick] if v.ndim == 2 else v[pick]) for k, v in s1.items() if k not in ('steps', 'stats')}
    sub['steps'] = ref['steps']                                           # of the whole batch on the device
    _compare(sub, ref, 'perf')
    assert s1['steps'].tolist() == [(s1['lengths'] > k).sum() for k in range(K)]


def test_self_consistent_pool_has_zero_error():
    """A pool whose next_observations / rewards are the oracle model's own deterministic predictions, rounded
    to f32: deterministic validation gives errors within the parity tolerance of 0 at every step."""
    domain, n_ep, L = 'halfcheetah', 40, 6
    d = _dataset(domain)
    O, A, _ = SHAPES[domain]
    p = obnn.from_mat_list(d['mats'])
    rs = np.random.RandomState(5)
    obs = np.zeros((n_ep, L + 1, O), np.float32)
    act = rs.uniform(-1, 1, (n_ep, L, A)).astype(np.float32)
    rew = np.zeros((n_ep, L), np.float32)
    obs[:, 0] = d['observations'][rs.randint(0, N_ROWS, n_ep)]
    for t in range(L):
        nobs, _, _, info = ofe.step(p, ELITES, obs[:, t].astype(np.float64), act[:, t], ofe.TERMINATION[domain],
                                    penalty_coeff=1.0, penalty_learned_var=True, deterministic=True)
        obs[:, t + 1], rew[:, t] = nobs, np.asarray(info['unpenalized_rewards']).ravel()
    term = np.zeros((n_ep, L), np.uint8)
    term[:, -1] = 1
    data = {'observations': obs[:, :-1].reshape(-1, O), 'next_observations': obs[:, 1:].reshape(-1, O),
            'actions': act.reshape(-1, A), 'rewards': rew.reshape(-1, 1), 'terminals': term.reshape(-1)}
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout
    pool = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=n_ep * L)
    pool.add_samples(data)
    ro = ModelRollout(_model(domain, 'fp32'), n_ep, 1)
    got = _host(ro.validate(pool, n_ep, L, _term_kind(domain), ELITES, start_idx=np.arange(n_ep) * L))
    assert (got['lengths'] == L).all() and (got['end_reasons'] == 0).all()
    ref = np.concatenate([rew[:, :, None], obs[:, 1:]], 2).astype(np.float64)          # [n_ep, L, D]
    tol = 5e-5 * np.linalg.norm(1 + np.abs(ref), axis=2).T                                # [L, n_ep]
    print('max err / tol: %.3g' % (got['errors'] / tol).max())
    assert (got['errors'] <= tol).all() and (got['obs_errors'] <= tol).all()


@pytest.mark.parametrize('learned_var', [True, False])
def test_one_step_equals_the_public_fakeenv_step(learned_var):
    """K = 1 against the public device FakeEnv.step(deterministic=True) on the same rows at 5e-5 (1 + |ref|)."""
    from mopo_amd.fake_env import FakeEnv
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    domain, B = 'hopper', 257
    d = _dataset(domain)
    model = _model(domain, 'fp32')
    starts = _starts(d, B)
    got = _host(ModelRollout(model, B, 1).validate(_device_pool(d), B, 1, _term_kind(domain), ELITES, start_idx=starts,
                                                   penalty_learned_var=learned_var))
    env = FakeEnv(model, static_fns[domain], penalty_coeff=1.0, penalty_learned_var=learned_var)
    nobs, _, term, info = env.step(d['observations'][starts], d['actions'][starts], deterministic=True)
    rew = info['unpenalized_rewards'].ravel()
    eo = np.linalg.norm(nobs - d['next_observations'][starts].astype(np.float64), axis=1)
    er = rew - d['rewards'][starts, 0].astype(np.float64)
    tol = 5e-5 * np.linalg.norm(1 + np.abs(np.concatenate([rew[:, None], nobs], 1)), axis=1)
    assert (got['lengths'] == 1).all() and (got['end_reasons'] == 0).all()
    assert (np.abs(got['errors'][0] - np.hypot(eo, er)) <= tol).all()
    assert (np.abs(got['obs_errors'][0] - eo) <= tol).all()
    pen = info['penalty'].ravel().astype(np.float64)
    assert (np.abs(got['penalties'][0] - pen) <= 5e-5 * (1 + np.abs(pen))).all()
    ok = ~_near(domain, nobs)
    np.testing.assert_array_equal(got['term_pred'][0][ok], term.ravel()[ok])


def test_pool_is_untouched_and_its_size_is_read_on_the_device():
    """Every pool field and the pool state are bit-identical before and after; rows past the pool's size are
    never a segment's (a pool of 600 rows holding 300: the segments end at row 299 with reason 3); an empty
    pool ends every segment at once with length 0 and reason 3; B = 0 returns."""
    import torch
    from mopo_amd.evaluation import segment_lengths_numpy
    from mopo_amd.rollout import ModelRollout
    domain = 'walker2d'
    d = _dataset(domain)
    ro = ModelRollout(_model(domain, 'fp32'), 257, 1)
    pool = _device_pool(d, size=300)
    before = {k: v.clone() for k, v in pool.fields.items()}
    state = pool._state.clone()
    starts = np.concatenate([[299, 298, 300, 599, -1], np.random.RandomState(3).randint(0, 300, 60)])
    got = _host(ro.validate(pool, 65, K, _term_kind(domain), ELITES, start_idx=starts, deterministic=False, seed=5))
    torch.cuda.synchronize()
    for k, v in pool.fields.items():
        assert torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)), k
    assert torch.equal(pool._state, state)
    length, end = segment_lengths_numpy(d['observations'], d['next_observations'], d['terminals'], 300, starts, K)
    np.testing.assert_array_equal(got['lengths'], length)
    np.testing.assert_array_equal(got['end_reasons'], end)
    assert got['lengths'][[0, 2, 3, 4]].tolist() == [1, 0, 0, 0] and (got['end_reasons'][[0, 2, 3, 4]] == 3).all()
    assert got['start_rows'][:5].tolist() == [299, 298, -1, -1, -1]
    assert got['steps'][0] == 62 and np.isnan(got['errors'][:, 2:5]).all()
    empty = _device_pool(d, size=0)
    for kw in ({}, {'start_idx': np.arange(65)}):
        e = _host(ro.validate(empty, 65, K, _term_kind(domain), ELITES, seed=1, **kw))
        assert not e['lengths'].any() and (e['end_reasons'] == 3).all() and not e['steps'].any()
        assert not e['stats'].any() and np.isnan(e['errors']).all() and (e['term_pred'] == 255).all()
    z = ro.validate(pool, 0, K, _term_kind(domain), ELITES)
    assert z['lengths'].numel() == 0 and not z['stats'].any().item()


def _mopo(segments):
    from collections import OrderedDict
    from mopo_amd.mopo import MOPO
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.static import static_fns
    rs = np.random.RandomState(2)
    n = 3000
    obs = rs.normal(size=(n + 1, 17)).astype(np.float32)
    obs[1:] = obs[:1] + np.cumsum(rs.normal(size=(n, 17)) * 0.05, 0).astype(np.float32)
    term = np.zeros((n, 1), bool)
    term[199::200] = True
    pool = SimpleReplayPool(obs_dim=17, act_dim=6, max_size=n)
    pool.add_samples({'observations': obs[:-1], 'actions': rs.uniform(-1, 1, (n, 6)), 'rewards': rs.normal(size=(n, 1)),
                      'terminals': term, 'next_observations': obs[1:]})
    np.random.seed(123)
    algo = MOPO(pool, static_fns['halfcheetah'], 17, 6, hidden_dim=64, rollout_batch_size=500, rollout_length=2,
                epoch_length=20, model_train_freq=20, separate_mean_var=True, penalty_coeff=1.0,
                penalty_learned_var=True, real_ratio=0.05, target_entropy=-3, seed=5, model_val_segments=segments,
                model_val_horizon=3)

    def given_model(**kw):                    # the model is given: no BNN.train in this epoch
        algo._model.set_elites([0, 1, 2, 3, 4])
        return OrderedDict(val_loss=0.5)
    algo._train_model = given_model
    d = list(algo.train(1))[0]
    import torch
    torch.cuda.synchronize()
    mp = algo._model_pool
    state = {'sac': algo._sac.get_params()[0].cpu().numpy(), 'ptr': (mp._pointer, mp.size),
             'pool': {k: v[:mp.size].cpu().numpy() for k, v in mp.fields.items()}, 'np': np.random.get_state(),
             'env': {k: v.cpu().numpy() for k, v in pool.fields.items()}}
    return d, state


def test_mopo_epoch_with_validation_changes_nothing_else():
    """One epoch with model_val_segments=64, model_val_horizon=3 and one without: SAC parameters, both pools and
    numpy's global stream bit-identical; the model/open_loop/* keys present and finite only in the first."""
    from mopo_amd.evaluation import open_loop_metrics
    d1, s1 = _mopo(64)
    d0, s0 = _mopo(0)
    np.testing.assert_array_equal(s1['sac'], s0['sac'])
    assert s1['ptr'] == s0['ptr'] and s1['ptr'][1] > 0
    for k in s0['pool']:
        np.testing.assert_array_equal(s1['pool'][k], s0['pool'][k], err_msg=k)
        np.testing.assert_array_equal(s1['env'][k], s0['env'][k], err_msg=k)
    assert s1['np'][0] == s0['np'][0] and s1['np'][2:] == s0['np'][2:]
    np.testing.assert_array_equal(s1['np'][1], s0['np'][1])
    assert not [k for k in d0 if 'open_loop' in k]
    keys = ['model/' + k for k in open_loop_metrics(np.zeros((4, 16)))]
    assert [k for k in d1 if 'open_loop' in k] == keys
    for k in keys:
        assert np.isfinite(d1[k]), k
    assert d1['model/open_loop/alive-h1'] == 64 and d1['model/open_loop/error'] > 0
    assert [k for k in d1 if 'open_loop' not in k] == list(d0)


def test_refusals():
    import ctypes as C
    import torch
    from mopo_amd import _lib as L
    from mopo_amd.rollout import ModelRollout
    domain = 'walker2d'
    d = _dataset(domain)
    ro, pool = ModelRollout(_model(domain, 'fp32'), 64, 1), _device_pool(d)
    kind = _term_kind(domain)

    def works():
        out = ro.validate(pool, 64, 2, kind, ELITES, start_idx=np.zeros(64, np.int64))
        assert (out['lengths'] == 2).all().item()                 # the handle still works after a refusal
    with pytest.raises(L.MopoError, match='4095'):
        ro.validate(pool, 64, 4096, kind, ELITES)
    works()
    with pytest.raises(L.MopoError, match='4095'):
        ro.validate(pool, 64, 0, kind, ELITES)
    works()
    with pytest.raises(L.MopoError, match='max_batch'):
        ro.validate(pool, 65, 3, kind, ELITES)
    works()
    with pytest.raises(L.MopoError, match='term_kind'):
        ro.validate(pool, 64, 3, 9, ELITES)
    works()
    with pytest.raises(L.MopoError, match='elites required'):
        ro.validate(pool, 64, 3, kind, [], deterministic=False)
    works()
    ro.validate(pool, 64, 3, kind, [])                            # deterministic: no elites needed
    desc = pool.desc()
    for f in ('d_obs', 'd_act', 'd_rew', 'd_term', 'd_next_obs', 'd_state'):
        bad = L.PoolDesc(**{n: getattr(desc, n) for n, _ in L.PoolDesc._fields_})
        setattr(bad, f, None)
        with pytest.raises(L.MopoError, match='NULL pool field'):
            ro.validate(bad, 64, 3, kind, ELITES)
        works()
    args, va = L.RolloutArgs(B=1, horizon=1, deterministic=1), L.ValArgs()
    for a, p, v in ((None, desc, va), (args, None, va), (args, desc, None)):
        assert L.lib().mopo_rollout_validate(ro._h, a, p, v, None) == -1
        assert 'NULL argument' in L.lib().mopo_last_error().decode()
    assert L.lib().mopo_rollout_validate(None, args, desc, va, None) == -1
    works()
    # outputs left NULL live in the handle: the call runs and fills the ones that were given
    stats = torch.zeros((3, 16), dtype=torch.float64, device='cuda')
    idx = torch.zeros(64, dtype=torch.int64, device='cuda')
    a2 = L.RolloutArgs(B=64, horizon=2, term_kind=kind, deterministic=1, penalty_learned_var=1, d_start_idx=L.ptr(idx))
    L.check(L.lib().mopo_rollout_validate(ro._h, a2, desc, L.ValArgs(d_stats=L.ptr(stats)), L.stream_ptr()))
    ref = ro.validate(pool, 64, 2, kind, ELITES, start_idx=np.zeros(64, np.int64))
    assert torch.equal(stats, ref['stats'])
