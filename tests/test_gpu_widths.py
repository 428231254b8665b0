"""GPU parity at the hidden widths the 8- and 16-block ensemble forms and the widened rollout actor add: H = 128
and 256, logical widths rounded up to them (100 -> 8 blocks, 220 -> 16), and policy widths other than 32 / 256.

Tolerances are the project's own, those of the tests these mirror:
  * BNN.predict vs the reference graph (tests/golden/widths_fwd_*.npz) and vs the f64 oracle: mean / log-var
    2e-5 (1 + |ref|) (test_gpu_ref.py, test_gpu_rollout.py test_bnn_predict_vs_oracle)
  * FakeEnv.step vs oracle.fake_env: next_obs / rewards 5e-5 (1 + |ref|), model indices bit-exact, terminals
    bit-exact (halfcheetah: never done; walker2d away from its bounds)
  * the actor vs oracle.sac.actor_act: 2e-5 (1 + |ref|) (test_actor_forward_vs_oracle)
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
from test_widths import _fixture_params

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
FWD = sorted(glob.glob(os.path.join(GOLD, 'widths_fwd_*.npz')))
DTYPES = ('fp32', 'bf16x6', 'f16x3')
BATCHES = (1, 65, 257)   # one row, one row past a 64-row workgroup, a partial last tile across the XCD dealing


# ---- 1. BNN.predict ---------------------------------------------------------------------------------------------
FWD_CASES = [(p, d) for p in FWD for d in DTYPES]


@pytest.mark.parametrize('path,dtype', FWD_CASES, ids=['%s-%s' % (os.path.basename(p)[11:-4], d) for p, d in FWD_CASES])
def test_widths_predict_vs_reference_graph(path, dtype):
    """H = 128 fails without the 8-block forms ("unsupported hidden size"): the test that shows the feature."""
    from mopo_amd.bnn import BNN
    assert len(FWD) == 4
    z = load_case(path)
    E, H, O, A, smv = int(z['E']), int(z['H']), int(z['O']), int(z['A']), bool(z['smv'])
    m = BNN({'name': 'w', 'num_networks': E, 'num_elites': 5, 'separate_mean_var': smv, 'obs_dim': O, 'act_dim': A,
             'hidden_dim': H, 'dtype': dtype}).set_params(obnn.to_mat_list(_fixture_params(z)))
    assert m.hidden_dim == H and 'hidden=%d' % H in repr(m)          # the logical width at the API
    assert [a.shape for a in m.get_params()] == [a.shape for a in obnn.to_mat_list(_fixture_params(z))]
    mean, var = m.predict(z['x'], factored=True)
    for name, got, ref in (('mean', mean, z['mean_f32']), ('log-var', np.log(var), z['logvar_f32'])):
        err = np.abs(np.float64(got) - ref) / (1 + np.abs(ref))
        print('%s %s %s: max scaled err %.3g' % (os.path.basename(path), dtype, name, err.max()))
        assert err.max() <= 2e-5, name


_ORACLE = {}


def _oracle_case(o, a, H, E=3):
    """Weights, inputs and the f64 oracle's outputs of a shape, computed once and shared by the dtypes."""
    key = (o, a, H)
    if key not in _ORACLE:
        rs = np.random.RandomState(1000 * o + 10 * a + H)
        mats = obnn.to_mat_list(obnn.init_params(E, o, a, hidden=H, seed=3, inputs=rs.normal(size=(300, o + a)) * 3))
        x = rs.normal(size=(max(BATCHES), o + a)) * 2
        rm, rlv = obnn.forward(obnn.from_mat_list(mats), x.astype(np.float32), dtype=np.float64, ret_log_var=True)
        rm64, rlv64 = obnn.forward(obnn.from_mat_list(mats), x, dtype=np.float64, ret_log_var=True)
        for arr in (x, rm, rlv, rm64, rlv64):
            arr.setflags(write=False)
        _ORACLE[key] = (mats, x, rm, rlv, rm64, rlv64)
    return _ORACLE[key]


# narrow shapes at every new width and dtype; the wide shape where it has a form: fp32 at both, 16-bit at 8 blocks
PREDICT = [(o, a, H, d) for (o, a) in ((17, 6), (11, 3)) for H in (128, 256, 100, 220) for d in DTYPES]
PREDICT += [(27, 8, H, 'fp32') for H in (128, 256, 100, 220)] + [(27, 8, H, d) for H in (128, 100) for d in DTYPES[1:]]


@pytest.mark.parametrize('o,a,H,dtype', PREDICT, ids=['%d+%d-H%d-%s' % c for c in PREDICT])
def test_widths_predict_vs_oracle(o, a, H, dtype):
    mats, x, rm, rlv, rm64, rlv64 = _oracle_case(o, a, H)
    model = make_model(mats, 3, H, O=o, A=a, dtype=dtype)
    for B in BATCHES:
        mean, var = model.predict(x[:B].astype(np.float32), factored=True)
        assert mean.shape == (3, B, o + 1)
        close(mean, rm[:, :B], 2e-5)
        close(np.log(var), rlv[:, :B], 2e-5)
    mean, var = model.predict(np.array(x[:65]), factored=True)       # f64 inputs once
    close(mean, rm64[:, :65], 2e-5)
    close(np.log(var), rlv64[:, :65], 2e-5)


# ---- 2. FakeEnv.step ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('det', [False, True])
@pytest.mark.parametrize('learned_var', [True, False])
@pytest.mark.parametrize('H,dtype', [(128, 'fp32'), (128, 'bf16x6'), (256, 'bf16x6'), (256, 'f16x3')])
def test_widths_fakeenv_step_vs_oracle(H, dtype, learned_var, det):
    from mopo_amd.fake_env import FakeEnv
    from mopo_amd.static import static_fns
    E, O, A, B = 7, 17, 6, 257
    rs = np.random.RandomState(H + 7)
    mats = obnn.to_mat_list(obnn.init_params(E, O, A, hidden=H, seed=1, inputs=rs.normal(size=(200, O + A))))
    elites = [4, 1, 0, 6, 2]
    model = make_model(mats, E, H, dtype=dtype)
    model.set_elites(elites)
    env = FakeEnv(model, static_fns['walker2d'], penalty_coeff=1.0, penalty_learned_var=learned_var)
    obs = rs.normal(size=(B, O)).astype(np.float32)
    obs[:, 0] = rs.uniform(1.1, 1.7, B)        # walker2d's height / angle well inside their bounds: terminals are
    obs[:, 1] = rs.uniform(-0.5, 0.5, B)       # decided by the model's step, not by f32 rounding at a bound
    act = rs.uniform(-1, 1, size=(B, A)).astype(np.float32)
    np.random.seed(5)
    nobs, rew, term, info = env.step(obs, act, deterministic=det)
    used = np.random.get_state()[1:3]
    np.random.seed(5)
    rn, rr, rt, ri = ofe.step(obnn.from_mat_list(mats), elites, obs, act, ofe.term_walker2d, penalty_coeff=1.0,
                              penalty_learned_var=learned_var, deterministic=det)
    close(nobs, rn, 5e-5)
    close(rew, rr, 5e-5)
    bad = term[:, 0] != rt[:, 0]      # bit-exact except within 1e-4 of one of walker2d.py's four bounds
    if bad.any():
        d = np.minimum(np.abs(rn[bad, 0][:, None] - np.array([0.8, 2.0])).min(1), np.abs(np.abs(rn[bad, 1]) - 1.0))
        assert (d < 1e-4).all()
    # the member choice: numpy's global stream consumed exactly as the oracle (and the reference) consumes it
    assert used[1] == np.random.get_state()[2] and np.array_equal(used[0], np.random.get_state()[1])


# ---- 3. the actor ---------------------------------------------------------------------------------------------------
ACTOR = [(H, dt) for H in (16, 48, 64, 96, 128, 160, 208, 240) for dt in (0, 3, 4)]


@pytest.mark.parametrize('H,dtype', ACTOR, ids=['H%d-dt%d' % c for c in ACTOR])
def test_widths_actor_forward_vs_oracle(H, dtype):
    import torch
    from mopo_amd import _lib as L
    from mopo_amd.rollout import init_sac_params, split_params
    dev = torch.device('cuda')
    for O, A in ((17, 6), (11, 3), (27, 8)):
        flat = init_sac_params(O, A, H, seed=4)
        rs = np.random.RandomState(H + O)
        flat = flat + (rs.normal(size=flat.shape) * 0.01).astype(np.float32)   # non-zero biases
        P = [p.astype(np.float64) for p in split_params(flat, O, A, H)[:8]]
        obs_all = rs.normal(size=(1000, O))
        eps_all = rs.normal(size=(1000, A)).astype(np.float32)
        tp = torch.from_numpy(flat).to(dev)
        for B in (1, 65, 1000):
            obs, eps = obs_all[:B], eps_all[:B]
            to, te = torch.from_numpy(obs.copy()).to(dev), torch.from_numpy(eps.copy()).to(dev)
            act = torch.empty((B, A), device=dev)
            mu = torch.empty((B, A), device=dev)
            L.check(L.lib().mopo_actor_forward_dtype(L.ptr(tp), O, A, H, L.ptr(to), 1, B, L.ptr(te), 0, 0, L.ptr(act),
                                                     L.ptr(mu), dtype, L.stream_ptr()))
            ra, rmu = osac.actor_act(P, obs.astype(np.float32).astype(np.float64), eps.astype(np.float64))
            close(act.cpu().numpy(), ra, 2e-5)
            close(mu.cpu().numpy(), rmu, 2e-5)


@pytest.mark.parametrize('hs', [(48, 200), (128, 64)])
@pytest.mark.parametrize('dtype', [0, 3, 4])
def test_widths_actor_nonsquare_through_pad_index(hs, dtype):
    """A [H1, H2] policy in the device layout SAC keeps it in (rollout.sac_pad_index: the square device_hidden
    network, zero padded), run at that width, against the oracle actor on the [H1, H2] parameters."""
    import torch
    from mopo_amd import _lib as L
    from mopo_amd.rollout import device_hidden, init_sac_params, sac_pad_index, split_params
    O, A, B = 17, 6, 257
    hd = device_hidden(hs)
    flat = init_sac_params(O, A, hs, seed=9)
    rs = np.random.RandomState(hs[0])
    flat = flat + (rs.normal(size=flat.shape) * 0.01).astype(np.float32)
    big = np.zeros(int(L.lib().mopo_sac_param_count(O, A, hd)), np.float32)
    big[sac_pad_index(O, A, hs)] = flat
    P = [p.astype(np.float64) for p in split_params(flat, O, A, hs)[:8]]
    obs = rs.normal(size=(B, O))
    eps = rs.normal(size=(B, A)).astype(np.float32)
    tp, to, te = (torch.from_numpy(x).cuda() for x in (big, obs, eps))
    act = torch.empty((B, A), device='cuda')
    mu = torch.empty((B, A), device='cuda')
    L.check(L.lib().mopo_actor_forward_dtype(L.ptr(tp), O, A, hd, L.ptr(to), 1, B, L.ptr(te), 0, 0, L.ptr(act),
                                             L.ptr(mu), dtype, L.stream_ptr()))
    ra, rmu = osac.actor_act(P, obs.astype(np.float32).astype(np.float64), eps.astype(np.float64))
    close(act.cpu().numpy(), ra, 2e-5)
    close(mu.cpu().numpy(), rmu, 2e-5)


# ---- 4. fused rollout parity ----------------------------------------------------------------------------------------
def _embed_policy(flat, O, A, h, H):
    """A width-h policy / Q parameter vector as the zero-embedded width-H one (each tensor's corner)."""
    from mopo_amd.rollout import sac_param_shapes, split_params
    out = []
    for t, big in zip(split_params(flat, O, A, h), sac_param_shapes(O, A, H)):
        z = np.zeros(big, np.float32)
        z[tuple(slice(0, n) for n in t.shape)] = t
        out.append(z.ravel())
    return np.concatenate(out)


_CASES = {}


def _case(monkeypatch, domain, H, hp, B, horizon, seed):
    """oracle/rollout.py's case with a width-hp policy: _rollout_case builds a 256-wide policy, so it is handed the
    zero embedding of the width-hp one (the same function, exactly); the device runs the width-hp parameters."""
    key = (domain, H, hp, B, horizon, seed)
    if key not in _CASES:
        import mopo_amd.rollout as mr
        init = mr.init_sac_params
        small = {}

        def embedded(O, A, Hfull=256, seed=2):
            assert Hfull == 256
            flat = init(O, A, hp, seed=seed)
            flat = flat + (np.random.RandomState(seed).normal(size=flat.shape) * 0.01).astype(np.float32)
            small['flat'] = flat
            return _embed_policy(flat, O, A, hp, 256)

        monkeypatch.setattr(mr, 'init_sac_params', embedded)
        c = _rollout_case(domain, 7, H, B, horizon, seed=seed)
        monkeypatch.setattr(mr, 'init_sac_params', init)
        c['flat_small'] = small['flat']
        _CASES[key] = c
    return _CASES[key]


ROLLOUTS = [('halfcheetah', 128, 128, 300, 3, 11), ('walker2d', 128, 128, 300, 3, 11),
            ('halfcheetah', 256, 64, 300, 3, 12), ('walker2d', 256, 64, 300, 3, 12)]
ROLLOUT_CASES = [c + (d,) for c in ROLLOUTS for d in DTYPES]


def _run_parity(c, domain, H, hp, B, horizon, dtype):
    import torch
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout, default_actor_dtype
    from mopo_amd.static import static_fns
    op = c['pool']
    ref = op.return_all_samples()
    model = make_model(c['mats'], 7, H, dtype=dtype)
    pool = SimpleReplayPool(obs_dim=17, act_dim=6, max_size=B * horizon + 7)
    ro = ModelRollout(model, B, horizon)
    steps = ro.run(torch.from_numpy(c['env_obs']).cuda(), torch.from_numpy(c['flat_small']).cuda(), pool, B, horizon,
                   static_fns[domain].term_kind, c['coeff'], c['elites'], start_idx=c['start'], eps_act=c['eps_act'],
                   eps_obs=c['eps_obs'], model_inds=c['inds'], pi_hidden=hp, actor_dtype=default_actor_dtype(dtype))
    exp = np.zeros(horizon, np.int64)
    exp[:len(c['steps'])] = c['steps']
    np.testing.assert_array_equal(steps.cpu().numpy(), exp)
    assert pool.size == op.size and pool._pointer == op._pointer
    got = pool.return_all_samples(as_numpy=True)
    np.testing.assert_array_equal(got['terminals'], ref['terminals'])
    for k in ('observations', 'actions', 'next_observations', 'rewards'):
        close(got[k], ref[k], 5e-5)


@pytest.mark.parametrize('domain,H,hp,B,horizon,seed,dtype', ROLLOUT_CASES,
                         ids=['%s-H%d-pi%d-%s' % (c[0], c[1], c[2], c[6]) for c in ROLLOUT_CASES])
def test_widths_fused_rollout_parity(monkeypatch, domain, H, hp, B, horizon, seed, dtype):
    c = _case(monkeypatch, domain, H, hp, B, horizon, seed)
    if domain == 'walker2d':
        assert c['steps'][-1] < B            # compaction between the steps
    _run_parity(c, domain, H, hp, B, horizon, dtype)


def test_widths_fused_rollout_parity_split_path(monkeypatch):
    """B = 4096, halfcheetah: the smallest batch the rollout splits into two row parts on two streams (no
    compaction, B / 2048 >= 2), at H = 128 with a 128-wide policy in the product dtype -- the actor then runs
    beside the other part's ensemble launch."""
    c = _case(monkeypatch, 'halfcheetah', 128, 128, 4096, 3, 18)
    _run_parity(c, 'halfcheetah', 128, 128, 4096, 3, 'bf16x6')


def test_widths_perf_mode_rows_vs_oracle():
    """Perf mode (Philox streams, no injection), halfcheetah, E = 7, H = 256 with a [64, 64] policy, B = 4096 (the
    split rollout), h = 3, bf16x6: 64 sampled rows recomputed end to end from the restated streams
    (oracle/rng.py), as test_wide_perf_mode_rows_vs_oracle does at 27 + 8."""
    import torch
    from oracle import rng as orng
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout, init_sac_params, split_params
    E, O, A, H, hp, B, h, env_n, coeff, tol = 7, 17, 6, 256, 64, 4096, 3, 20000, 1.0, 5e-5
    seed, epoch = 0x1234567890ab, 3
    rs = np.random.RandomState(21)
    env_obs = rs.normal(size=(env_n, O)).astype(np.float32)
    mats = obnn.to_mat_list(obnn.init_params(E, O, A, hidden=H, seed=22,
                                             inputs=np.concatenate([env_obs[:2000], rs.uniform(-1, 1, (2000, A))], 1)))
    p = obnn.from_mat_list(mats)
    flat = init_sac_params(O, A, hp, seed=23)
    flat = flat + (rs.normal(size=flat.shape) * 0.01).astype(np.float32)
    P = [q.astype(np.float64) for q in split_params(flat, O, A, hp)[:8]]
    elites = [4, 1, 0, 6, 2]
    model = make_model(mats, E, H, dtype='bf16x6')
    pool = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=B * h)
    steps = ModelRollout(model, B, h).run(torch.from_numpy(env_obs).cuda(), torch.from_numpy(flat).cuda(), pool, B, h,
                                          0, coeff, elites, seed=seed, epoch=epoch, pi_hidden=hp,
                                          actor_dtype='bf16x6').cpu().numpy()
    assert steps.tolist() == [B] * h and pool.size == B * h
    rows = np.sort(rs.choice(B, 64, replace=False))
    obs = env_obs[orng.start_rows(rows, seed, epoch * 4096, env_n)].astype(np.float64)
    for i in range(h):
        st = epoch * 4096 + 1 + i
        ea = orng.act_noise(rows, seed, st, A).astype(np.float64)
        act, _ = osac.actor_act(P, obs.astype(np.float32).astype(np.float64), ea)
        act = act.astype(np.float32)
        sel = orng.model_choice(rows, seed, st, elites)
        noise = np.broadcast_to(orng.obs_noise(rows, seed, st, O + 1).astype(np.float64), (E, len(rows), O + 1))
        nobs, rew, term, _ = ofe.step(p, elites, obs, act, ofe.TERMINATION['halfcheetah'], penalty_coeff=coeff,
                                      penalty_learned_var=True, noise=noise, model_inds=sel)
        pos = torch.from_numpy(i * B + rows).cuda()
        got = {k: v[pos].cpu().numpy() for k, v in pool.fields.items()}
        if i == 0:
            np.testing.assert_array_equal(got['observations'], obs.astype(np.float32))
        close(got['observations'], obs, tol)
        close(got['actions'], act, tol)
        close(got['next_observations'], nobs, tol)
        close(got['rewards'], rew, tol)
        np.testing.assert_array_equal(got['terminals'], term)
        obs = nobs


# ---- 5. BNN.train -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,batch', [(128, 256), (100, 250)])
def test_widths_train_epochs_match_oracle_steps(H, batch, tmp_path):
    """E = 7, 17 + 6, 600 rows (a partial last minibatch), two epochs against oracle/bnn_train.py.  H = 128 runs
    the fused row kernels train_rows_kernel<2, 8, 3>; H = 100 has no row-block instantiation and takes the generic
    path.  Then the trained logical parameters go through BNN.set_params (the packer's zero embedding), predict
    and save / load."""
    from oracle import bnn_train as ot
    from mopo_amd.bnn import BNN
    from test_gpu_train import data, model, run_epoch, setup_trainer, to_oracle
    shape, n_rows, epochs = (7, 17, 6, H), 600, 2
    m = model(shape=shape)
    X, Y = data(n_rows, shape=shape)
    t, start = setup_trainer(m, X, batch)
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
        assert g.shape[-1] in (H, 18) or g.shape[1] in (H, 23)             # the logical shapes
        np.testing.assert_allclose(g, r, rtol=2e-5, atol=2e-5 * max(1.0, np.abs(r).max()), err_msg=names[k])
    # the trained logical parameters: repacked for inference, predicted with, saved and loaded
    m.set_params(got)
    m.name, m.model_dir = 'BNN', str(tmp_path)
    m.save(str(tmp_path), 0)
    os.rename(str(tmp_path / 'BNN_0.mat'), str(tmp_path / 'BNN.mat'))
    os.rename(str(tmp_path / 'BNN_0.nns'), str(tmp_path / 'BNN.nns'))
    back = BNN({'name': 'BNN', 'model_dir': str(tmp_path), 'load_model': True, 'num_elites': 2,
                'separate_mean_var': True})
    assert back.hidden_dim == H
    for a, b in zip(back.get_params(), got):
        np.testing.assert_array_equal(a, b)
    x = X[:65]
    m0, v0 = m.predict(x)
    m1, v1 = back.predict(x)
    np.testing.assert_array_equal(m0, m1)
    rm, rv = obnn.forward(obnn.from_mat_list(got), x, dtype=np.float64)
    close(m0, rm, 2e-5)
    close(v0, rv, 2e-5)


# ---- 6. MOPO ------------------------------------------------------------------------------------------------------------
def test_widths_mopo_epoch_and_model_eval():
    """hidden_dim = 128 with hidden_sizes [128, 128]: one short epoch through MOPO.train with model_eval episodes;
    the first rollout step's actions against the oracle actor (test_mopo_nonsquare_policy_hidden_sizes' form)."""
    from oracle import rng as orng
    from mopo_amd.mopo import MOPO
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import split_params
    from mopo_amd.static import static_fns
    rs = np.random.RandomState(5)
    n = 2000
    obs = rs.normal(size=(n, 17)).astype(np.float32)
    pool = SimpleReplayPool(obs_dim=17, act_dim=6, max_size=n)
    pool.add_samples({'observations': obs, 'actions': rs.uniform(-1, 1, (n, 6)), 'rewards': rs.normal(size=(n, 1)),
                      'terminals': np.zeros((n, 1), bool), 'next_observations': obs + 0.1})
    algo = MOPO(pool, static_fns['halfcheetah'], 17, 6, rollout_batch_size=500, rollout_length=2, epoch_length=40,
                model_train_freq=40, separate_mean_var=True, real_ratio=0.05, target_entropy=-3, max_model_t=3,
                hidden_dim=128, network_kwargs={'hidden_sizes': [128, 128]}, ensemble_dtype='fp32', actor_dtype='fp32',
                model_eval_episodes=64, model_eval_length=5)
    assert algo._sac.hidden_sizes == (128, 128) and algo._pi_hidden == 128 and algo._model.hidden_dim == 128
    P = split_params(algo._sac.get_params()[0].cpu().numpy().astype(np.float64), 17, 6, (128, 128))
    d = list(algo.train(1))
    assert all(np.isfinite(v) for v in d[-1].values())
    assert any(k.startswith('model_eval') for k in d[-1])
    mp = algo._model_pool
    o0 = mp.fields['observations'][:500].cpu().numpy().astype(np.float64)
    a0 = mp.fields['actions'][:500].cpu().numpy().astype(np.float64)
    eps = orng.act_noise(np.arange(500), algo._seed, 1, 6).astype(np.float64)
    ref, _ = osac.actor_act(P[:8], o0, eps)
    np.testing.assert_allclose(a0, ref, atol=2e-5)


# ---- 7. code-generation cliff guard ---------------------------------------------------------------------------------
@pytest.mark.parametrize('H', [128, 256])
def test_widths_dtypes_no_pathological_slowdown(H):
    """A rolled part loop in a 16-bit kernel costs ~70x (scratch-indexed operands); the project's guard for that
    failure: each 16-bit dtype's 50k-row predict takes at most 1.5x fp32's at the same width."""
    import torch
    E, O, A, B = 7, 17, 6, 50000
    rs = np.random.RandomState(3)
    mats = obnn.to_mat_list(obnn.init_params(E, O, A, hidden=H, seed=3, inputs=rs.normal(size=(300, O + A))))
    x = torch.from_numpy(rs.normal(size=(B, O + A)).astype(np.float32)).cuda()
    ms = {}
    for dt in DTYPES:
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
    print('H = %d predict, ms per 50k rows: %s' % (H, ms))
    for dt, v in ms.items():
        assert v <= 1.5 * ms['fp32'], ms


# ---- 8. refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('o,a,H,dtype,match', [
    (17, 6, 128, 'bf16', 'fp32, bf16x6 and f16x3'), (17, 6, 256, 'bf16x3', 'fp32, bf16x6 and f16x3'),
    (17, 6, 300, 'fp32', 'up to 256'), (17, 6, 300, 'f16x3', 'up to 256'), (17, 6, 420, 'fp32', 'fp32 and f16x3'),
    (27, 8, 256, 'bf16x6', 'fp32'), (27, 8, 256, 'f16x3', 'fp32'), (27, 8, 128, 'bf16', 'bf16x6 / f16x3')])
def test_widths_refusals(o, a, H, dtype, match):
    """What still has no kernel is refused where the shape is known (construction), naming what does run."""
    from mopo_amd.bnn import BNN
    with pytest.raises(RuntimeError, match=match):
        BNN({'name': 'r', 'num_networks': 7, 'num_elites': 5, 'separate_mean_var': True, 'obs_dim': o, 'act_dim': a,
             'hidden_dim': H, 'dtype': dtype})
