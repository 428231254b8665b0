"""Every arm of the 16-bit ensemble dispatch (csrc/bnn.hip launch_bf16 .. launch_f16s) that no other GPU test
visibly reaches, in both launch modes: BNN.predict (FWD_PREDICT) and one FakeEnv.step (FWD_ROLLOUT: the selected
member's mean / std and the learned-variance penalty) against oracle/bnn.py and oracle/fake_env.py.

What each shape runs (NB2 = hidden blocks of 16 rounded up to even, NBU = the blocks in use):
  * bf16 (P = 1) and bf16x3 (P = 2), bnn_fwd_bf16_kernel: H = 16 (NB2 2, NBU 1), 32 (2, 2), 48 (4, 3), 64 (4, 4),
    200 (14, 13), 400 and 416 (26, 26 -- 400's 25th block is not skipped);
  * bf16x6 (P = 3) at H = 16 and 48: the same kernel with NBU = NB2 - 1 (whole block counts run the ring);
  * f16x3 at H = 400: bnn_fwd_f16h_kernel (column halves), at H = 416: bnn_fwd_f16s_kernel over 26 whole blocks;
  * 11 + 3 inputs (one input k-group, 8 outputs: the 2-block head) on bf16x3 at H = 200 and bf16 at H = 64.
E = 2 and B = 37: two full 16-row tiles and a 5-row one in one partial workgroup, the second member behind them.

Tolerances are tests/test_gpu_ref.py's TOL per dtype, on |d| / (1 + |ref|), for the mean, the log-variance and the
step's next observations, rewards, penalty and picked member's mean and std.
"""
import numpy as np
import pytest

from oracle import bnn as obnn
from oracle import fake_env as ofe
from test_gpu_ref import TOL

pytestmark = pytest.mark.gpu
E, B, ELITES = 2, 37, [1, 0]

CASES = [(17, 6, H, d) for d in ('bf16', 'bf16x3') for H in (16, 48, 32, 64, 200, 400, 416)]
CASES += [(17, 6, 16, 'bf16x6'), (17, 6, 48, 'bf16x6'), (17, 6, 400, 'f16x3'), (17, 6, 416, 'f16x3')]
CASES += [(11, 3, 200, 'bf16x3'), (11, 3, 64, 'bf16')]

_REF = {}


def _reference(O, A, H):
    """Parameters, inputs and the oracle's outputs of a shape: computed once, shared by the dtypes, read-only."""
    key = (O, A, H)
    if key not in _REF:
        rs = np.random.RandomState(100 * O + H)
        mats = obnn.to_mat_list(obnn.init_params(E, O, A, hidden=H, seed=3, inputs=rs.normal(size=(300, O + A)) * 3))
        obs = rs.normal(size=(B, O)).astype(np.float32)
        act = rs.uniform(-1, 1, size=(B, A)).astype(np.float32)
        x = np.concatenate((obs, act), axis=1)
        mean, logvar = obnn.forward(obnn.from_mat_list(mats), x, dtype=np.float64, ret_log_var=True)
        np.random.seed(5)
        nobs, rew, term, info = ofe.step(obnn.from_mat_list(mats), ELITES, obs, act, ofe.term_halfcheetah,
                                         penalty_coeff=1.0, penalty_learned_var=True)
        ref = dict(mats=mats, obs=obs, act=act, x=x, mean=mean, logvar=logvar, nobs=np.asarray(nobs),
                   rew=np.asarray(rew), penalty=np.asarray(info['penalty']), sel_mean=np.asarray(info['mean']),
                   sel_std=np.asarray(info['std']))
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    return float((np.abs(got - ref) / (1 + np.abs(ref))).max())


@pytest.mark.parametrize('O,A,H,dtype', CASES, ids=['%d+%d-H%d-%s' % c for c in CASES])
def test_dispatch_predict_and_step_vs_oracle(O, A, H, dtype):
    from mopo_amd.bnn import BNN
    from mopo_amd.fake_env import FakeEnv
    from mopo_amd.static import static_fns
    r = _reference(O, A, H)
    model = BNN({'name': 'd', 'num_networks': E, 'num_elites': E, 'separate_mean_var': True, 'obs_dim': O,
                 'act_dim': A, 'hidden_dim': H, 'dtype': dtype}).set_params(r['mats'])
    model.set_elites(ELITES)
    tol = TOL[dtype]
    mean, var = model.predict(np.array(r['x']), factored=True)
    assert mean.shape == (E, B, O + 1)
    errs = {'mean': _err(mean, r['mean']), 'log-var': _err(np.log(var), r['logvar'])}
    env = FakeEnv(model, static_fns['halfcheetah'], penalty_coeff=1.0, penalty_learned_var=True)
    np.random.seed(5)
    nobs, rew, term, info = env.step(np.array(r['obs']), np.array(r['act']))
    assert not np.asarray(term).any()
    errs.update({'next_obs': _err(nobs, r['nobs']), 'reward': _err(rew, r['rew']),
                 'penalty': _err(info['penalty'], r['penalty']),
                 # the picked member's mean and std (the same members, from the same numpy stream)
                 'sel-mean': _err(info['mean'], r['sel_mean']), 'sel-std': _err(info['std'], r['sel_std'])})
    print('%d+%d H=%d %s (tol %.0e): %s' % (O, A, H, dtype, tol, '  '.join('%s %.3g' % kv for kv in errs.items())))
    for name, e in errs.items():
        assert e <= tol, '%s: max scaled err %.3g > %.3g' % (name, e, tol)
