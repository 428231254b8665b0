"""GPU parity at ant's dimensions and the other wide shapes (obs_dim + act_dim in 33..64, or obs_dim in 24..31):
ensemble forward, FakeEnv.step, the fused rollout and BNN.train, in fp32, bf16x6 and f16x3.

Tolerances are those of the narrow-shape tests they mirror:
  * BNN.predict vs the reference graph (tests/golden/wide_fwd_*.npz): mean / log-var 2e-5 (1 + |ref|), var rel 5e-5
    (test_gpu_ref.py test_bnn_predict_vs_reference_graph)
  * BNN.predict vs the f64 oracle: 2e-5 (1 + |ref|) (test_gpu_rollout.py test_bnn_predict_vs_oracle)
  * FakeEnv.step vs tests/golden/wide_fakeenv_*.npz: test_fakeenv_step_vs_reference_golden's assertions
  * fused rollout: counts, pool pointer / size and terminals bit-exact, floats 5e-5 (1 + |ref|)
  * BNN.train epochs: rtol 2e-5, atol 2e-5 max(1, max |ref|) (test_gpu_train.py test_epoch_matches_oracle_steps)
  * 16-bit predict at most 1.5x the fp32 kernel's time (test_ensemble_dtypes_no_pathological_slowdown)
"""
import glob
import os

import numpy as np
import pytest

from oracle import bnn as obnn
from oracle import fake_env as ofe
from oracle import sac as osac
from test_gpu_rollout import _rollout_case, close, make_model
from test_oracle_ref import load_case
from test_wide_oracle import env_params, fwd_params

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
FWD = sorted(glob.glob(os.path.join(GOLD, 'wide_fwd_*.npz')))
ENV = sorted(glob.glob(os.path.join(GOLD, 'wide_fakeenv_*.npz')))
DTYPES = ('fp32', 'bf16x6', 'f16x3')
O, A = 27, 8


def _config(E, H, o, a, dtype, smv=True):
    return {'name': 'wide', 'num_networks': E, 'num_elites': min(5, E), 'separate_mean_var': smv, 'obs_dim': o,
            'act_dim': a, 'hidden_dim': H, 'dtype': dtype}


# ---- 1. BNN.predict vs the reference graph --------------------------------------------------------------------
# E = 32, H = 400 is the fp32-only wide width (the 16-bit dtypes are refused there: test_wide_refusals)
FWD_CASES = [(p, d) for p in FWD for d in DTYPES if d == 'fp32' or 'H400' not in os.path.basename(p)]


def test_wide_forward_case_list():
    assert len(FWD) == 3 and len(FWD_CASES) == 7


@pytest.mark.parametrize('path,dtype', FWD_CASES, ids=['%s-%s' % (os.path.basename(p)[9:-4], d) for p, d in FWD_CASES])
def test_wide_predict_vs_reference_graph(path, dtype):
    from mopo_amd.bnn import BNN
    z = load_case(path)
    E, H, smv = int(z['E']), int(z['H']), bool(z['smv'])
    m = BNN(_config(E, H, O, A, dtype, smv)).set_params(obnn.to_mat_list(fwd_params(z)))
    mean, var = m.predict(z['x'], factored=True)
    for name, got, ref in (('mean', mean, z['mean_f32']), ('log-var', np.log(var), z['logvar_f32'])):
        err = np.abs(np.float64(got) - ref) / (1 + np.abs(ref))
        print('%s %s %s: max scaled err %.3g' % (os.path.basename(path), dtype, name, err.max()))
        assert err.max() <= 2e-5, name
    rv = np.max(np.abs(var - z['var_f32']) / z['var_f32'])
    print('var rel err %.3g' % rv)
    assert rv < 5e-5


# ---- 2. BNN.predict vs the f64 oracle at the shapes where the wide code can go wrong --------------------------
# (25, 8): one feature in the third input block; (27, 8): ant; (31, 8): a full 32-wide head; (24, 8): 32 inputs
# with 4 head blocks; (31, 33): all 64 inputs
SHAPES = [(25, 8), (27, 8), (31, 8), (24, 8), (31, 33)]
BATCHES = (1, 65, 257)   # one row, one row past a 64-row workgroup, a partial last tile
_ORACLE = {}


def _oracle_case(o, a, H, E=7):
    """Weights, inputs and the f64 oracle's outputs of a shape, computed once and shared by the dtypes."""
    key = (o, a, H)
    if key not in _ORACLE:
        rs = np.random.RandomState(1000 * o + 10 * a + H)
        mats = obnn.to_mat_list(obnn.init_params(E, o, a, hidden=H, seed=3, inputs=rs.normal(size=(300, o + a)) * 3))
        x = rs.normal(size=(max(BATCHES), o + a)) * 2
        rm, rv = obnn.forward(obnn.from_mat_list(mats), x.astype(np.float32), dtype=np.float64)
        rm64, rv64 = obnn.forward(obnn.from_mat_list(mats), x, dtype=np.float64)
        for arr in (x, rm, rv, rm64, rv64):
            arr.setflags(write=False)
        _ORACLE[key] = (mats, x, rm, rv, rm64, rv64)
    return _ORACLE[key]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('H', [200, 64, 32])
@pytest.mark.parametrize('o,a', SHAPES)
def test_wide_predict_vs_oracle(o, a, H, dtype):
    mats, x, rm, rv, _, _ = _oracle_case(o, a, H)
    model = make_model(mats, 7, H, O=o, A=a, dtype=dtype)
    for B in BATCHES:
        mean, var = model.predict(x[:B].astype(np.float32), factored=True)
        assert mean.shape == (7, B, o + 1)
        close(mean, rm[:, :B], 2e-5)
        close(var, rv[:, :B], 2e-5)


@pytest.mark.parametrize('dtype', DTYPES)
def test_wide_predict_f64_inputs_vs_oracle(dtype):
    mats, x, _, _, rm64, rv64 = _oracle_case(27, 8, 200)
    mean, var = make_model(mats, 7, 200, O=27, A=8, dtype=dtype).predict(np.array(x[:65]), factored=True)
    close(mean, rm64[:, :65], 2e-5)
    close(var, rv64[:, :65], 2e-5)


# ---- 3. FakeEnv.step vs the reference's FakeEnv.step with mopo/static/ant.py ------------------------------------
_ENV_MATS = {}


@pytest.mark.parametrize('path', ENV, ids=[os.path.basename(c) for c in ENV])
def test_wide_fakeenv_step_vs_reference_golden(path):
    from mopo_amd.fake_env import FakeEnv
    from mopo_amd.static import static_fns
    c = dict(np.load(path))
    E, H, B = int(c['E']), int(c['H']), int(c['B'])
    if 'mats' not in _ENV_MATS:
        _ENV_MATS['mats'] = obnn.to_mat_list(env_params(c))
    model = make_model(_ENV_MATS['mats'], E, H, O=O, A=A)
    model.set_elites(list(c['elites']))
    env = FakeEnv(model, static_fns[str(c['domain'])], penalty_coeff=float(c['penalty_coeff']),
                  penalty_learned_var=bool(c['learned_var']))
    det = bool(c['deterministic'])
    np.random.seed(int(c['seed']))
    nobs, rew, term, info = env.step(c['obs'], c['act'], deterministic=det)
    np.random.seed(int(c['seed']))
    if not det:   # numpy's global stream consumed exactly like the reference (normal then choice)
        np.random.normal(size=(E, B, O + 1))
        np.testing.assert_array_equal(np.random.choice(list(c['elites']), size=B), c['model_inds'])
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
    # terminals bit-exact except where the f32-vs-f64 height is within 1e-4 of one of ant.py's bounds
    bad = term[:, 0] != c['term'][:, 0]
    if bad.any():
        assert (np.abs(c['next_obs'][bad, 0][:, None] - np.array([0.2, 1.0])).min(1) < 1e-4).all()


# ---- 4. fused rollout parity ------------------------------------------------------------------------------------
# the seeds were chosen on the CPU so that the ORACLE's case meets the conditions asserted below
ROLLOUTS = [('ant', 7, 200, 777, 5, 11), ('antangle', 7, 64, 300, 4, 11)]
ROLLOUT_CASES = [c + (d,) for c in ROLLOUTS for d in DTYPES] + [('ant', 7, 200, 5000, 3, 18, 'bf16x6')]   # split path
ROLLOUT_CASES += [('ant', 7, 32, 300, 4, 11, d) for d in ('bf16x6', 'f16x3')]   # the H = 32 wide ring forms
_CASES = {}


def _case(domain, E, H, B, horizon, seed):
    key = (domain, E, H, B, horizon, seed)
    if key not in _CASES:
        _CASES[key] = _rollout_case(domain, E, H, B, horizon, seed=seed, O=O, A=A)
    return _CASES[key]


@pytest.mark.parametrize('domain,E,H,B,horizon,seed,dtype', ROLLOUT_CASES,
                         ids=['%s-H%d-B%d-%s' % (c[0], c[2], c[3], c[6]) for c in ROLLOUT_CASES])
def test_wide_fused_rollout_parity(domain, E, H, B, horizon, seed, dtype):
    import torch
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    c = _case(domain, E, H, B, horizon, seed)
    op = c['pool']
    ref = op.return_all_samples()
    # the oracle's own case: no row excluded, a termination at every step, survivors into the last step
    height = ref['next_observations'][:, 0].astype(np.float64)
    assert (np.abs(height[:, None] - np.array([0.2, 1.0])).min(1) >= 1e-4).all()
    assert len(c['steps']) == horizon
    base = 0
    for n in c['steps']:
        assert ref['terminals'][base:base + n].any()
        base += n
    model = make_model(c['mats'], E, H, O=O, A=A, dtype=dtype)
    dev = torch.device('cuda')
    pool = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=B * horizon + 7)
    ro = ModelRollout(model, B, horizon)
    steps = ro.run(torch.from_numpy(c['env_obs']).to(dev), torch.from_numpy(c['flat']).to(dev), pool, B, horizon,
                   static_fns[domain].term_kind, c['coeff'], c['elites'], start_idx=c['start'], eps_act=c['eps_act'],
                   eps_obs=c['eps_obs'], model_inds=c['inds'])
    exp = np.zeros(horizon, np.int64)
    exp[:len(c['steps'])] = c['steps']
    np.testing.assert_array_equal(steps.cpu().numpy(), exp)
    assert pool.size == op.size and pool._pointer == op._pointer
    got = pool.return_all_samples(as_numpy=True)
    np.testing.assert_array_equal(got['terminals'], ref['terminals'])
    for k in ('observations', 'actions', 'next_observations', 'rewards'):
        close(got[k], ref[k], 5e-5)


def test_hopper_sized_f16x3_h64_rollout_parity():
    """The one narrow instantiation whose code generation moved with the ring kernel's input k-group parameter
    (11 + 3 inputs, H = 64, f16x3, rollout mode: 59 -> 60 VGPRs) against the oracle, at the parity tolerances."""
    import torch
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout
    o, a, E, H, B, horizon = 11, 3, 7, 64, 300, 3
    c = _rollout_case('halfcheetah', E, H, B, horizon, seed=11, O=o, A=a)
    model = make_model(c['mats'], E, H, O=o, A=a, dtype='f16x3')
    pool = SimpleReplayPool(obs_dim=o, act_dim=a, max_size=B * horizon + 7)
    steps = ModelRollout(model, B, horizon).run(
        torch.from_numpy(c['env_obs']).cuda(), torch.from_numpy(c['flat']).cuda(), pool, B, horizon, 0, c['coeff'],
        c['elites'], start_idx=c['start'], eps_act=c['eps_act'], eps_obs=c['eps_obs'], model_inds=c['inds'])
    assert steps.cpu().tolist() == c['steps'] == [B] * horizon
    got, ref = pool.return_all_samples(as_numpy=True), c['pool'].return_all_samples()
    for k in ('observations', 'actions', 'next_observations', 'rewards'):
        close(got[k], ref[k], 5e-5)


# ---- 5. perf-mode (Philox) rollout: sampled rows recomputed by the oracle ---------------------------------------
def test_wide_perf_mode_rows_vs_oracle():
    """O = 27, A = 8, E = 7, H = 200, B = 4096 (the split rollout), h = 3, bf16x6, ant's rule with compaction
    between steps: 64 sampled rows recomputed end to end from the restated Philox streams (oracle/rng.py), as
    test_full_size_perf_mode_rows_vs_oracle does for 17 + 6."""
    import torch
    from oracle import rng as orng
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout, init_sac_params, split_params
    from mopo_amd.static import static_fns
    E, H, B, h, env_n, coeff, tol = 7, 200, 4096, 3, 20000, 1.0, 5e-5
    seed, epoch = 0x1234567890ab, 3
    rs = np.random.RandomState(21)
    env_obs = rs.normal(size=(env_n, O)).astype(np.float32)
    env_obs[:, 0] = rs.uniform(0.25, 0.95, env_n)
    mats = obnn.to_mat_list(obnn.init_params(E, O, A, hidden=H, seed=22,
                                             inputs=np.concatenate([env_obs[:2000], rs.uniform(-1, 1, (2000, A))], 1)))
    p = obnn.from_mat_list(mats)
    flat = init_sac_params(O, A, 256, seed=23)
    P = [q.astype(np.float64) for q in split_params(flat, O, A)[:8]]
    elites = [4, 1, 0, 6, 2]
    model = make_model(mats, E, H, O=O, A=A, dtype='bf16x6')
    pool = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=B * h)
    ro = ModelRollout(model, B, h)
    steps = ro.run(torch.from_numpy(env_obs).cuda(), torch.from_numpy(flat).cuda(), pool, B, h,
                   static_fns['ant'].term_kind, coeff, elites, seed=seed, epoch=epoch).cpu().numpy()
    assert steps[0] == B and pool.size == steps.sum()
    term_dev = pool.fields['terminals'][:pool.size, 0].cpu().numpy()
    rows = np.sort(rs.choice(B, 64, replace=False))
    idx = rows.copy()
    obs = env_obs[orng.start_rows(rows, seed, epoch * 4096, env_n)].astype(np.float64)
    base, checked = 0, 0
    for i in range(h):
        if len(rows) == 0:
            break
        st = epoch * 4096 + 1 + i
        ea = orng.act_noise(rows, seed, st, A).astype(np.float64)
        act, _ = osac.actor_act(P, obs.astype(np.float32).astype(np.float64), ea)
        act = act.astype(np.float32)
        sel = orng.model_choice(rows, seed, st, elites)
        noise = np.broadcast_to(orng.obs_noise(rows, seed, st, O + 1).astype(np.float64), (E, len(rows), O + 1))
        nobs, rew, term, _ = ofe.step(p, elites, obs, act, ofe.TERMINATION['ant'], penalty_coeff=coeff,
                                      penalty_learned_var=True, noise=noise, model_inds=sel)
        pos = torch.from_numpy(base + idx).cuda()
        got = {k: v[pos].cpu().numpy() for k, v in pool.fields.items()}
        if i == 0:
            np.testing.assert_array_equal(got['observations'], obs.astype(np.float32))
        close(got['observations'], obs, tol)
        close(got['actions'], act, tol)
        close(got['next_observations'], nobs, tol)
        close(got['rewards'], rew, tol)
        np.testing.assert_array_equal(got['terminals'], term)
        checked += len(rows)
        live = ~term[:, 0]
        keep = ~term_dev[base:base + steps[i]]
        rank = np.cumsum(keep) - keep
        base += steps[i]
        rows, idx, obs = rows[live], rank[idx[live]], nobs[live]
    assert checked >= 64 + 16


# ---- 6. BNN.train ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', [200, 64])
def test_wide_train_epochs_match_oracle_steps(H):
    """O = 27, A = 8, E = 7, batch 256, 600 rows (a partial last minibatch), two epochs, against
    oracle/bnn_train.py.  bnn_train.hip's use_rows() admits 3 input blocks with 4 head blocks at these two
    widths, so the steps run train_rows_kernel<3, 13, 4> (H = 200) / <3, 4, 4> (H = 64) with the staged
    gather (16 (35 + 28) = 1008 of its 1024 items); without those instantiations step_rows fails."""
    from oracle import bnn_train as ot
    from test_gpu_train import data, model, run_epoch, setup_trainer, to_oracle
    shape, n_rows, batch, epochs = (7, O, A, H), 600, 256, 2
    m = model(shape=shape)
    X, Y = data(n_rows, shape=shape)
    t, start = setup_trainer(m, X, batch)
    np.testing.assert_allclose(start[0], X.mean(0, keepdims=True), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(start[1], X.std(0, keepdims=True), rtol=1e-5, atol=1e-6)
    rs = np.random.RandomState(7)
    st = ot.TrainState(to_oracle(start))
    nb = int(np.ceil(n_rows / batch))
    for _ in range(epochs):
        idxs = rs.randint(n_rows, size=[shape[0], n_rows])
        run_epoch(m, t, X, Y, idxs, batch)
        for b in range(nb):
            bi = idxs[:, b * batch:(b + 1) * batch]
            st.step(X[bi].astype(np.float64), Y[bi].astype(np.float64))
    got = m._train_params(t)
    ref = [st.vals[i] for i in range(len(ot.optvars(st.params())))]
    names = ['W0', 'b0', 'W1', 'b1', 'W2', 'b2', 'W3', 'b3', 'Wm', 'bm', 'Wv', 'bv', 'maxlv', 'minlv']
    for k, (g, r) in enumerate(zip(got[2:], ref)):
        r = r.reshape(g.shape)
        np.testing.assert_allclose(g, r, rtol=2e-5, atol=2e-5 * max(1.0, np.abs(r).max()), err_msg=names[k])


# ---- 7. code-generation cliff guard ---------------------------------------------------------------------------
def test_wide_dtypes_no_pathological_slowdown():
    """bf16x6 and f16x3 predict of 50,000 ant-sized rows take at most 1.5x the fp32 kernel's time."""
    import torch
    E, H, B = 7, 200, 50000
    rs = np.random.RandomState(11)
    mats = obnn.to_mat_list(obnn.init_params(E, O, A, hidden=H, seed=3, inputs=rs.normal(size=(300, O + A))))
    x = torch.from_numpy(rs.normal(size=(B, O + A)).astype(np.float32)).cuda()
    ms = {}
    for dt in DTYPES:
        m = make_model(mats, E, H, O=O, A=A, dtype=dt)
        for _ in range(3):
            m.predict(x)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(10):
            m.predict(x)
        t1.record()
        torch.cuda.synchronize()
        ms[dt] = t0.elapsed_time(t1) / 10
    print('ant-sized predict, ms per 50k rows: %s' % ms)
    for dt, v in ms.items():
        assert v <= 1.5 * ms['fp32'], ms


# ---- 8. refusals ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('o,a,H,dtype,match', [
    (27, 8, 200, 'bf16', 'bf16x6 / f16x3'), (27, 8, 200, 'bf16x3', 'bf16x6 / f16x3'),
    (27, 8, 400, 'f16x3', 'fp32'), (27, 8, 400, 'bf16x6', 'fp32|bf16x6'),
    (32, 33, 200, 'fp32', '<= 64'), (30, 35, 200, 'f16x3', '<= 64'), (32, 8, 200, 'fp32', 'obs_dim <= 31')])
def test_wide_refusals(o, a, H, dtype, match):
    """Unsupported wide combinations are refused where the shape is known (construction), with a message that
    names the limit or the dtypes that do work."""
    from mopo_amd.bnn import BNN
    with pytest.raises(RuntimeError, match=match):
        BNN(_config(7, H, o, a, dtype))
