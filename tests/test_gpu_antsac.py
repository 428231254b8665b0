"""GPU: the SAC step with critic inputs past one 32-wide layer-1 group (obs_dim <= 31, act_dim <= 8, so
obs_dim + act_dim up to 39; ant is 27 + 8), against the fp64 oracle and the reference-graph fixture.

The forward row blocks of sac_rows.h run layer 1 as 4-deep MFMA k-steps over the inputs and the bias column;
handles with obs_dim + act_dim >= 32 launch the wide forms (10 k-steps instead of 8).  The shapes below sit where
that can go wrong: the bias alone in a 9th k-step (W = 32), the action crossing the group boundary, the bias
starting the 10th step (W = 36), the bias in the last slot (W = 39), and W = 31 as the control that still runs
the narrow kernels.

Tolerances are those of the tests each case mirrors (test_gpu_sac.py's docstring, test_gpu_ref.py,
test_gpu_mopo.py::test_mopo_epoch_vs_oracle_epoch): fp32 device vs fp64 oracle, identical rows and noise:
  * logged losses / means / alpha / grad norms: rel 2e-4;  gradients: |d| <= 1e-4 max|g| of the tensor + 1e-7
  * params after one step: 1e-6 (+ 2 lr_t where the gradient is ~0);  20 steps: losses within 1e-3 relative
  * a MOPO epoch: pool 5e-5 (1 + |ref|), terminals and sizes bit-exact, SAC state p50 <= 1e-6 / p99 <= 1e-4 /
    max <= 1e-3 after 50 steps, last losses 1e-3
"""
import os

import numpy as np
import pytest

from oracle import replay_pool as opool
from oracle import sac as osac

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')
ANT = os.path.join(GOLD, 'antsac_O27_A8_H64.npz')
O, A, H = 27, 8, 256


def flat(ts):
    return np.concatenate([np.asarray(t).ravel() for t in ts])


def make_pools(rs, o, a, sizes=(500, 3000), oracle=True):
    """An env pool and a model pool of random transitions on the device (and their oracle twins)."""
    import torch
    from mopo_amd.replay_pool import SimpleReplayPool
    out = []
    for n in sizes:
        s = {'observations': rs.normal(size=(n, o)).astype(np.float32),
             'actions': rs.uniform(-1, 1, (n, a)).astype(np.float32),
             'next_observations': rs.normal(size=(n, o)).astype(np.float32),
             'rewards': rs.normal(size=(n, 1)).astype(np.float32),
             'terminals': rs.uniform(size=(n, 1)) < 0.1}
        p = SimpleReplayPool(obs_dim=o, act_dim=a, max_size=n + 10)
        p.add_samples(s)
        op = None
        if oracle:
            op = opool.Pool(o, a, n + 10)
            op.add_samples(s)
        out.append((p, op))
    torch.cuda.synchronize()
    return out


def host_batch(env_op, mod_op, idx, n_env):
    b1 = env_op.batch_by_indices(idx[:n_env])
    b2 = mod_op.batch_by_indices(idx[n_env:])
    return {k: np.concatenate([b1[k], b2[k]]).astype(np.float64) for k in b1}   # mopo.py:815-816


def one_step(o, a, h, n, seed):
    """One injected step on the device and in the oracle from the same parameters (non-zero biases), rows and
    noise.  Returns (sac, oracle state after the step, oracle logs, oracle pre-step gradients)."""
    from mopo_amd.sac import SAC
    rs = np.random.RandomState(seed)
    (env_p, env_op), (mod_p, mod_op) = make_pools(rs, o, a, sizes=(300, 900))
    params = [p + rs.normal(size=p.shape) * 0.02 for p in osac.init_params(o, a, h, seed=seed + 1)]
    sac = SAC(o, a, list(h) if isinstance(h, tuple) else h, batch_size=n, real_ratio=0.05, target_entropy=-3,
              params=flat(params).astype(np.float32), log_alpha=0.1)
    ne = sac.n_env
    idx = np.concatenate([rs.randint(0, 300, ne), rs.randint(0, 900, n - ne)])
    e1 = rs.normal(size=(n, a)).astype(np.float32)
    e2 = rs.normal(size=(n, a)).astype(np.float32)
    st = osac.SACState([p.astype(np.float32).astype(np.float64) for p in params], log_alpha=np.float32(0.1))
    g = {}
    logs_ref = osac.sac_step(st, host_batch(env_op, mod_op, idx, ne), e1.astype(np.float64), e2.astype(np.float64),
                             grads_out=g, target_entropy=-3.0)
    sac._do_training(0, env_p, mod_p, idx=idx, eps_s=e1, eps_n=e2)
    return sac, st, logs_ref, g


def check_grads(sac, g, what=''):
    dev = sac.get_grads()[0].cpu().numpy()
    off = 0
    for i, gr in enumerate(g['pi'] + g['q1'] + g['q2']):
        m = gr.size
        scale = np.abs(gr).max() + 1e-12
        err = np.abs(dev[off:off + m] - gr.ravel()).max()
        print('%s grad tensor %d: err %.3g scale %.3g' % (what, i, err, scale))
        assert err <= 1e-4 * scale + 1e-7, '%s grad tensor %d: err %.3g scale %.3g' % (what, i, err, scale)
        off += m
    assert off == dev.size


# ---- 1. one step at ant's shape ---------------------------------------------------------------------------------
def test_antsac_one_step_parity():
    """27 + 8, H = 256, batch 256 against the f64 oracle: logs, every gradient tensor, Adam's first step, the
    Polyak target and log_alpha, as test_gpu_sac.py::test_sac_one_step_parity does at 17 + 6."""
    sac, st, logs_ref, g = one_step(O, A, H, 256, seed=0)
    assert sac.n_env == 12
    lg = sac.logs()
    for k in ['Q/q1_loss', 'sac_Q/q2_loss', 'sac_Q/q1', 'sac_Q/q2', 'sac_pi/alpha', 'sac_pi/pi_entropy',
              'sac_pi/logp_pi', 'sac_pi/pi_global_norm', 'sac_Q/q_global_norm']:
        np.testing.assert_allclose(lg[k], logs_ref[k], rtol=2e-4, atol=1e-6, err_msg=k)
    np.testing.assert_allclose(lg['policy_loss'], logs_ref['pi_loss'], rtol=2e-4, atol=1e-6)
    check_grads(sac, g, 'ant')
    ga = sac.get_grads()[1]
    np.testing.assert_allclose(float(ga.item()), g['alpha'], rtol=1e-4, atol=1e-6)
    lr_t = 3e-4 * np.sqrt(1 - 0.999) / (1 - 0.9)          # Adam's first step is ~lr_t sign(g)
    p_new, la_new = sac.get_params()
    p_new = p_new.cpu().numpy()
    p_ref = flat(st.params)
    gr = flat(g['pi'] + g['q1'] + g['q2'])
    d = np.abs(p_new - p_ref)
    tiny = np.abs(gr) < 1e-3 * np.abs(gr).max()
    assert d[~tiny].max() <= 1e-6 + 1e-6 * np.abs(p_ref[~tiny]).max()
    assert d[tiny].max() <= 1e-6 + 2 * lr_t
    np.testing.assert_allclose(float(la_new.item()), float(st.log_alpha), atol=1e-6)
    np.testing.assert_allclose(sac.get_target().cpu().numpy(), flat(st.target), atol=2e-6 + 5e-3 * 2 * lr_t)


# ---- 2. the shapes where the wide layer 1 can go wrong ----------------------------------------------------------
@pytest.mark.parametrize('o,a,h,n', [(24, 8, 64, 100), (31, 1, 64, 48), (28, 8, 256, 40), (31, 8, 32, 40),
                                     (27, 8, (256, 128), 256), (28, 3, 64, 100)])
def test_antsac_one_step_gradients_edge_shapes(o, a, h, n):
    """W = 32 (a 9th k-step holding the bias alone), W = 32 with one action column past the group boundary,
    W = 36 (the bias starts the 10th step; batch not a multiple of 16), W = 39 (the bias in the last slot), ant
    with non-square hidden sizes, and W = 31 (still the narrow kernels): every gradient tensor of one step."""
    sac, _, _, g = one_step(o, a, h, n, seed=7)
    check_grads(sac, g, '(%d, %d, %s, %d)' % (o, a, h, n))


# ---- 3. twenty steps --------------------------------------------------------------------------------------------
def test_antsac_twenty_steps_track_oracle():
    from mopo_amd.sac import SAC
    rs = np.random.RandomState(1)
    (env_p, env_op), (mod_p, mod_op) = make_pools(rs, O, A)
    params = osac.init_params(O, A, H, seed=6)
    sac = SAC(O, A, H, batch_size=256, real_ratio=0.05, target_entropy=-3, params=flat(params).astype(np.float32))
    st = osac.SACState([p.astype(np.float64) for p in params])
    for it in range(20):
        idx = np.concatenate([rs.randint(0, env_p.size, 12), rs.randint(0, mod_p.size, 244)])
        e1, e2 = rs.normal(size=(256, A)).astype(np.float32), rs.normal(size=(256, A)).astype(np.float32)
        ref = osac.sac_step(st, host_batch(env_op, mod_op, idx, 12), e1.astype(np.float64), e2.astype(np.float64))
        sac._do_training(it, env_p, mod_p, idx=idx, eps_s=e1, eps_n=e2)
        lg = sac.logs()
        for k in ['Q/q1_loss', 'sac_Q/q2_loss', 'sac_pi/alpha', 'sac_pi/logp_pi']:
            np.testing.assert_allclose(lg[k], ref[k], rtol=1e-3, atol=1e-5, err_msg='%s @ step %d' % (k, it))


# ---- 4. the fused launches against the separate launches --------------------------------------------------------
@pytest.mark.parametrize('o,a,h,n', [(27, 8, 256, 256), (24, 8, 64, 100)])
def test_antsac_fused_launches_bit_identical_to_separate_launches(o, a, h, n, monkeypatch):
    """The wide forms of all three fusion levels compute the same arithmetic: 300 graph-replayed steps end
    bit-identical for MOPO_SAC_FUSE = 0, 1, 2, with finite logs (no hand-off wait gave up)."""
    import torch
    from mopo_amd.sac import SAC
    rs = np.random.RandomState(21)
    (env_p, _), (mod_p, _) = make_pools(rs, o, a, sizes=(400, 2000), oracle=False)
    fl = flat(osac.init_params(o, a, h, seed=3)).astype(np.float32)
    out = {}
    for fuse in ('0', '1', '2'):
        monkeypatch.setenv('MOPO_SAC_FUSE', fuse)
        sac = SAC(o, a, h, batch_size=n, real_ratio=0.05, target_entropy=-3, params=fl)
        sac._do_training(0, env_p, mod_p, n_steps=300, seed=19)
        torch.cuda.synchronize()
        lg = sac.logs()
        assert all(np.isfinite(v) for v in lg.values()), (fuse, lg)
        out[fuse] = {k: v.cpu().numpy() for k, v in sac.state_dict().items()}
    assert np.abs(out['0']['params'] - np.append(fl, 0.0)).max() > 0
    for f in ('1', '2'):
        for k in out['0']:
            np.testing.assert_array_equal(out[f][k], out['0'][k], err_msg='MOPO_SAC_FUSE=%s %s' % (f, k))


# ---- 5. graph replay --------------------------------------------------------------------------------------------
def test_antsac_graph_replay_matches_eager():
    import torch
    from mopo_amd.rollout import init_sac_params
    from mopo_amd.sac import SAC
    rs = np.random.RandomState(2)
    (env_p, _), (mod_p, _) = make_pools(rs, O, A, oracle=False)
    init = init_sac_params(O, A, H, seed=9)
    a = SAC(O, A, H, params=init, use_graph=True, target_entropy=-3)
    b = SAC(O, A, H, params=init, use_graph=False, target_entropy=-3)
    a._do_training(0, env_p, mod_p, n_steps=50, seed=123)
    b._do_training(0, env_p, mod_p, n_steps=50, seed=123)
    torch.cuda.synchronize()
    pa, pb = a.get_params()[0], b.get_params()[0]
    assert torch.equal(pa, pb)
    assert torch.isfinite(pa).all()
    assert all(np.isfinite(v) for v in a.logs().values())


# ---- 6. the reference's own graph at ant's shape ----------------------------------------------------------------
def test_antsac_steps_vs_reference_graph():
    """The assertions of test_gpu_ref.py::test_sac_steps_vs_reference_graph on the case at ant's shape (the f32
    execution of MOPO._build / _do_training / _update_target, tests/golden/make_antsac_vectors.py)."""
    import test_gpu_ref
    test_gpu_ref.test_sac_steps_vs_reference_graph(ANT)


# ---- 7. a whole MOPO epoch on ant -------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['fp32', 'bf16x6', 'f16x3'])
def test_antsac_mopo_epoch_vs_oracle_epoch(dtype):
    """test_gpu_mopo.py::test_mopo_epoch_vs_oracle_epoch at 27 + 8 with ant's termination rule (a row ends unless
    next_obs is finite and 0.2 <= next_obs[:, 0] <= 1.0), K = 50: MOPO(...) constructs, rolls out into the model
    pool with compaction between the horizon steps, trains SAC for the epoch and reports logs, all through the
    public classes; the oracle recomputes the epoch end to end from the restated streams (oracle/rng.py, keyed
    by the rollout row's id, so the survivors of each step keep their streams).
    The inputs are made so that the rollout survives: the env observations' column 0 is drawn inside the band,
    and the given model's log-variance ceiling (max_logvar, 0.5 at initialisation: an observation noise of
    ~0.8, which alone ends 60 % of the rows per step) is set to -4 as after training (noise ~0.13).  Conditions
    on that input, checked on the oracle alone: its model pool holds at least half of B x h rows (4646 of 5000:
    compaction at every step), and no next observation lies within 2e-4 of a band edge -- twice the pool
    tolerance 5e-5 (1 + |ref|) there, so the bit-exact terminals and sizes do not hinge on a rounding (the input
    seed was chosen for that: 5.3e-4)."""
    import torch
    from oracle import bnn as obnn
    from oracle import fake_env as ofe
    from oracle import rng as orng
    from mopo_amd.mopo import MOPO
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.static import static_fns
    E, Hm, K = 7, 200, 50
    B, h, seed = 1000, 5, 0x5eed
    rs = np.random.RandomState(36)
    n_env = 3000
    obs = rs.normal(size=(n_env, O)).astype(np.float32)
    obs[:, 0] = rs.uniform(0.45, 0.75, n_env)
    env = {'observations': obs,
           'actions': rs.uniform(-1, 1, (n_env, A)).astype(np.float32),
           'rewards': rs.normal(size=(n_env, 1)).astype(np.float32),
           'terminals': rs.uniform(size=(n_env, 1)) < 0.05}
    env['next_observations'] = (env['observations'] + 0.1 * rs.normal(size=(n_env, O))).astype(np.float32)
    pool = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=n_env)
    pool.add_samples(env)
    algo = MOPO(pool, static_fns['ant'], O, A, rollout_batch_size=B, rollout_length=h, epoch_length=K,
                model_train_freq=250, real_ratio=0.05, target_entropy=-3, ensemble_dtype=dtype, actor_dtype=None,
                num_networks=E, num_elites=5, hidden_dim=Hm, separate_mean_var=True, penalty_coeff=1.0,
                penalty_learned_var=True, seed=seed)
    mats = obnn.to_mat_list(obnn.init_params(E, O, A, hidden=Hm, seed=32,
                                             inputs=np.concatenate([env['observations'], env['actions']], 1)))
    mats[14] = np.full_like(mats[14], -4.0)             # max_logvar
    elites = [3, 0, 6, 1, 4]
    algo._model.set_params(mats)
    algo._model.set_elites(elites)
    algo._model_train_metrics = {}                     # the model is given (no BNN.train in this epoch)
    p0, la0 = algo._sac.get_params()
    flat0 = p0.cpu().numpy().astype(np.float64)
    diags = list(algo.train(1))
    torch.cuda.synchronize()
    assert len(diags) == 1 and np.isfinite(diags[0]['Q_loss']) and np.isfinite(diags[0]['training/policy_loss'])
    # ---- the oracle epoch: rollout (epoch 0: start rows at step 0, horizon step i at 1 + i), rows compacted
    bnn = obnn.from_mat_list(mats)
    P0, off = [], 0
    for s in osac.param_shapes(O, A, 256):
        P0.append(flat0[off:off + int(np.prod(s))].reshape(s))
        off += int(np.prod(s))
    envp = opool.Pool(O, A, n_env)
    envp.add_samples(env)
    modp = opool.Pool(O, A, algo._model_pool._max_size)
    uid = np.arange(B)
    cur = envp.batch_by_indices(orng.start_rows(uid, seed, 0, n_env))['observations']
    margin = np.inf
    for i in range(h):
        ea = orng.act_noise(uid, seed, 1 + i, A).astype(np.float64)
        act, _ = osac.actor_act(P0[:8], cur.astype(np.float32).astype(np.float64), ea)
        act = act.astype(np.float32)
        noise = np.broadcast_to(orng.obs_noise(uid, seed, 1 + i, O + 1).astype(np.float64), (E, len(uid), O + 1))
        nobs, rew, term, _ = ofe.step(bnn, elites, cur, act, ofe.TERMINATION['ant'], penalty_coeff=1.0,
                                      penalty_learned_var=True, noise=noise,
                                      model_inds=orng.model_choice(uid, seed, 1 + i, elites))
        modp.add_samples({'observations': cur, 'actions': act, 'next_observations': nobs, 'rewards': rew,
                          'terminals': term})
        assert np.isfinite(nobs).all()
        margin = min(margin, np.abs(nobs[:, 0] - 0.2).min(), np.abs(nobs[:, 0] - 1.0).min())
        live = ~term[:, 0]
        if not live.any():
            break
        uid, cur = uid[live], nobs[live]
    print('ant epoch %s: oracle model pool %d of %d rows, band margin %.3g' % (dtype, modp.size, B * h, margin))
    assert modp.size >= B * h // 2 and margin >= 2e-4, (modp.size, margin)
    mp = algo._model_pool
    assert mp.size == modp.size
    got = {k: v[:mp.size].cpu().numpy() for k, v in mp.fields.items()}
    for k in ('observations', 'actions', 'next_observations', 'rewards'):
        err = np.abs(got[k].astype(np.float64) - modp.fields[k][:mp.size]) / (1 + np.abs(modp.fields[k][:mp.size]))
        assert err.max() <= 5e-5, (k, err.max())
    np.testing.assert_array_equal(got['terminals'], modp.fields['terminals'][:mp.size])
    # ---- the oracle epoch: K SAC steps on batches of the oracle's pools (step counter k, seed + 7919 * 0)
    st = osac.SACState(P0, log_alpha=float(la0.item()))
    n, n_env_b = 256, int(256 * 0.05)
    for k in range(K):
        idx = orng.sac_batch_indices(n, n_env_b, envp.size, modp.size, seed, k)
        e_b, m_b = envp.batch_by_indices(idx[:n_env_b]), modp.batch_by_indices(idx[n_env_b:])
        batch = {f: np.concatenate([e_b[f], m_b[f]]).astype(np.float64) for f in e_b}
        lg = osac.sac_step(st, batch, orng.sac_noise(n, A, seed, k, 0).astype(np.float64),
                           orng.sac_noise(n, A, seed, k, 1).astype(np.float64), target_entropy=-3.0)
    ref = {'params': np.append(flat(st.params), st.log_alpha), 'target': flat(st.target),
           'adam_m': np.concatenate([flat(st.opt_pi.m), flat(st.opt_q1.m), flat(st.opt_q2.m), flat(st.opt_a.m)]),
           'adam_v': np.concatenate([flat(st.opt_pi.v), flat(st.opt_q1.v), flat(st.opt_q2.v), flat(st.opt_a.v)])}
    dev = {k: v.cpu().numpy().astype(np.float64) for k, v in algo._sac.state_dict().items()}
    q = {}
    for k in ref:
        assert dev[k].shape == ref[k].shape, k
        e = np.abs(dev[k] - ref[k]) / (1 + np.abs(ref[k]))
        q[k] = [float(np.quantile(e, x)) for x in (0.5, 0.99, 1.0)]
    print('ant epoch %s vs oracle epoch, scaled error p50 / p99 / max:' % dtype, q)
    assert all(v[0] <= 1e-6 and v[1] <= 1e-4 and v[2] <= 1e-3 for v in q.values()), q
    dl = algo._sac.logs()
    for dk, rk in (('Q/q1_loss', 'Q/q1_loss'), ('sac_Q/q2_loss', 'sac_Q/q2_loss'), ('policy_loss', 'pi_loss')):
        assert abs(dl[dk] - lg[rk]) <= 1e-3 * (1 + abs(lg[rk])), (dk, dl[dk], lg[rk])


# ---- 8. refusals ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('o,a,match', [(32, 8, 'obs_dim <= 31'), (27, 9, 'act_dim <= 8')])
def test_antsac_refusals(o, a, match):
    """Past the limits the handle is refused at construction, with a message that names the limit."""
    from mopo_amd.sac import SAC
    with pytest.raises(RuntimeError, match=match):
        SAC(o, a, 256, batch_size=256)


# ---- 9. code-generation cliff guard -----------------------------------------------------------------------------
def test_antsac_no_pathological_slowdown():
    """200 graph-replayed steps at 27 + 8 take at most 1.5x the time of 200 at 17 + 6 (both H = 256, batch 256,
    same process): the wide forms carry 10 more operand registers per lane and two more layer-1 k-steps, not a
    spill or an occupancy cliff."""
    import torch
    from mopo_amd.rollout import init_sac_params
    from mopo_amd.sac import SAC
    us = {}
    for o, a in ((17, 6), (27, 8)):
        rs = np.random.RandomState(5)
        (env_p, _), (mod_p, _) = make_pools(rs, o, a, oracle=False)
        sac = SAC(o, a, 256, batch_size=256, params=init_sac_params(o, a, 256, seed=4), target_entropy=-3)
        sac._do_training(0, env_p, mod_p, n_steps=200, seed=3)          # captures the graphs
        torch.cuda.synchronize()
        best = np.inf
        for rep in range(3):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            sac._do_training(200 * (rep + 1), env_p, mod_p, n_steps=200, seed=3)
            t1.record()
            torch.cuda.synchronize()
            best = min(best, t0.elapsed_time(t1) * 1e3 / 200)
        assert all(np.isfinite(v) for v in sac.logs().values())
        us[(o, a)] = best
    print('SAC us/step (200 graph-replayed steps, best of 3): 17+6 %.2f, 27+8 %.2f, ratio %.3f'
          % (us[(17, 6)], us[(27, 8)], us[(27, 8)] / us[(17, 6)]))
    assert us[(27, 8)] <= 1.5 * us[(17, 6)], us
