"""The bf16x6 ring kernel's packed remainder k-group (bnn_kernels.h bnn_fwd_ring_kernel<KP>, mlp_tile.h kpack_slot).

At H = 197..200 the last 32-deep k-group of every hidden-width input holds 2 real values per lane; the kernel runs
it as one slice of one packed fragment per output block (two MFMAs, the second half full) instead of three slices
and six half-zero 16-deep MFMAs.  H = 193..196 and 201..208 keep the unpacked path and weight layout, so the tests run both
sides of the dispatch boundary, the narrow (3- and 2-block) and the wide (4-block) head, and the remainder alone.

Tolerances are those of tests/test_gpu_ring_waits.py and tests/test_gpu_ref.py: |d| <= 2e-5 (1 + |ref|) on mean,
variance and log-variance, 5e-5 relative on the variance.  The isolated-remainder cases are held to the criterion
tests/test_gpu_rollout.py has for the split dtypes: no worse than twice the fp32 kernel's own error, floor 2e-6.
"""
import functools

import numpy as np
import pytest

from oracle import bnn as obnn

pytestmark = pytest.mark.gpu
E, B = 3, 133   # 133 rows: 9 tiles of 16 -> a partial workgroup (4 tiles), a partial wave, a partial tile (5 rows)
TOL, VAR_REL = 2e-5, 5e-5
PACKED_H = [197, 198, 199, 200]      # 197, 198: padding inside the lane's two registers
UNPACKED_H = [193, 196, 201, 208]    # both sides of the dispatch boundary
REM = slice(192, 200)                # the remainder k-group's features at H = 200
REM_SCALE = 32.0                     # rows 192..199 alone feed a layer: scaled up so every layer's output is O(1)


def scaled_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    return float(np.max(np.abs(a - b) / (1 + np.abs(b))))


def make_model(mats, H, O, A, dtype):
    from mopo_amd.bnn import BNN
    return BNN({'name': 'kpack', 'num_networks': E, 'num_elites': E, 'separate_mean_var': True, 'obs_dim': O,
                'act_dim': A, 'hidden_dim': H, 'dtype': dtype}).set_params(list(mats))


@functools.lru_cache(maxsize=None)
def case(H, O, A):
    """Weights, inputs and the f64 oracle's outputs of one shape (computed once, shared, read-only)."""
    rs = np.random.RandomState(1000 * H + O)
    mats = obnn.to_mat_list(obnn.init_params(E, O, A, hidden=H, seed=3, inputs=rs.normal(size=(300, O + A)) * 3))
    x = (rs.normal(size=(B, O + A)) * 2).astype(np.float32)
    rm, rv = obnn.forward(obnn.from_mat_list(mats), x, dtype=np.float64)
    for a in mats + [x, rm, rv]:
        a.setflags(write=False)
    return tuple(mats), x, rm, rv


def check_predict(H, O, A):
    mats, x, rm, rv = case(H, O, A)
    mean, var = make_model(mats, H, O, A, 'bf16x6').predict(x, factored=True)
    errs = (scaled_err(mean, rm), scaled_err(var, rv), scaled_err(np.log(var), np.log(rv)),
            float(np.max(np.abs(var - rv) / rv)))
    print('H=%d O=%d A=%d: mean %.3g var %.3g log-var %.3g var rel %.3g' % ((H, O, A) + errs))
    assert errs[0] <= TOL and errs[1] <= TOL and errs[2] <= TOL and errs[3] < VAR_REL, errs


@pytest.mark.parametrize('O,A', [(17, 6), (11, 3)])
@pytest.mark.parametrize('H', PACKED_H + UNPACKED_H)
def test_predict_vs_f64_oracle(H, O, A):
    check_predict(H, O, A)


@pytest.mark.parametrize('H', [200, 197])
def test_wide_predict_vs_f64_oracle(H):
    """27 + 8 inputs: two input k-groups of 32 and the 4-block head (a 4-fragment remainder slice)."""
    check_predict(H, 27, 8)


# ---- the remainder in isolation -----------------------------------------------------------------------------
HID = (4, 6, 8, 10, 12)   # to_mat_list: the K = H weight matrices (hidden layers 1..3, mean head, log-var head)


@functools.lru_cache(maxsize=None)
def isolated_case(keep_remainder):
    """H = 200 with rows 0..191 (keep_remainder) or rows 192..199 of every K = H weight matrix zeroed."""
    H, O, A = 200, 17, 6
    mats = [np.array(a) for a in case(H, O, A)[0]]
    for i in HID:
        assert mats[i].shape[1] == H
        if keep_remainder:
            mats[i][:, :192, :] = 0
            mats[i][:, REM, :] *= REM_SCALE
        else:
            mats[i][:, REM, :] = 0
    x = case(H, O, A)[1]
    rm, rv = obnn.forward(obnn.from_mat_list(mats), x, dtype=np.float64)
    for a in mats + [rm, rv]:
        a.setflags(write=False)
    return tuple(mats), x, rm, rv


def head_input(mats, x):
    """The last hidden layer's activations [E, B, H] in f64 (oracle.bnn.forward's steps)."""
    p = obnn.from_mat_list(list(mats))
    h = (x.astype(np.float64) - p['mu']) / p['sigma']
    h = obnn.swish(np.einsum('ij,ajk->aik', h, p['W'][0].astype(np.float64)) + p['b'][0])
    for l in range(1, 4):
        h = obnn.swish(np.matmul(h, p['W'][l].astype(np.float64)) + p['b'][l])
    return h, p


@pytest.mark.parametrize('keep_remainder', [True, False], ids=['rows_0_191_zeroed', 'rows_192_199_zeroed'])
def test_remainder_in_isolation(keep_remainder):
    mats, x, rm, rv = isolated_case(keep_remainder)
    mean, var = make_model(mats, 200, 17, 6, 'bf16x6').predict(x, factored=True)
    m32, v32 = make_model(mats, 200, 17, 6, 'fp32').predict(x, factored=True)
    em, ev, em32, ev32 = scaled_err(mean, rm), scaled_err(var, rv), scaled_err(m32, rm), scaled_err(v32, rv)
    print('mean %.3g (fp32 %.3g) var %.3g (fp32 %.3g)' % (em, em32, ev, ev32))
    assert em <= max(2 * em32, 2e-6), (em, em32)
    assert ev <= max(2 * ev32, 2e-6), (ev, ev32)


def test_fused_rollout_h198():
    """300 rows, 3 steps, halfcheetah with sampling on, against the oracle rollout (the tolerances of the H = 200
    bf16x6 cases of tests/test_gpu_rollout.py test_fused_rollout_parity)."""
    import torch
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    from test_gpu_rollout import _rollout_case, close
    from test_gpu_rollout import make_model as rollout_model
    domain, E7, H, n, horizon = 'halfcheetah', 7, 198, 300, 3
    c = _rollout_case(domain, E7, H, n, horizon, seed=11)
    model = rollout_model(c['mats'], E7, H, dtype='bf16x6')
    dev = torch.device('cuda')
    pool = SimpleReplayPool(obs_dim=17, act_dim=6, max_size=n * horizon + 7)
    ro = ModelRollout(model, n, horizon)
    steps = ro.run(torch.from_numpy(c['env_obs']).to(dev), torch.from_numpy(c['flat']).to(dev), pool, n, horizon,
                   static_fns[domain].term_kind, c['coeff'], c['elites'], start_idx=c['start'], eps_act=c['eps_act'],
                   eps_obs=c['eps_obs'], model_inds=c['inds'])
    exp = np.zeros(horizon, np.int64)
    exp[:len(c['steps'])] = c['steps']
    np.testing.assert_array_equal(steps.cpu().numpy(), exp)
    op = c['pool']
    assert pool.size == op.size and pool._pointer == op._pointer
    got, ref = pool.return_all_samples(as_numpy=True), op.return_all_samples()
    np.testing.assert_array_equal(got['terminals'], ref['terminals'])
    for k in ('observations', 'actions', 'next_observations', 'rewards'):
        close(got[k], ref[k], 5e-5)
