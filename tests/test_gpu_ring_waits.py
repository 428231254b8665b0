"""The LDS-ring ensemble kernel (bnn_kernels.h bnn_fwd_ring_kernel) reads its weight fragments from LDS ahead of the
MFMAs that consume them, under counted ``s_waitcnt lgkmcnt(N)`` while slice copies are in flight.  A fragment
consumed ahead of its wait is wrong in a few tiles of a few launches, so besides parity against the f64 oracle
at every ring shape (H = 32, 64, 200: 2, 4 and 14 hidden blocks, the last with the half-K final k-group; both
head widths) these tests hold the kernel to run-to-run bit identity.

Tolerances are the ones tests/test_gpu_ref.py and tests/test_gpu_rollout.py hold bf16x6 and f16x3 to:
|d| <= 2e-5 (1 + |ref|) on mean, variance and log-variance, and 5e-5 relative on the variance.
"""
import functools

import numpy as np
import pytest

from oracle import bnn as obnn

pytestmark = pytest.mark.gpu
E, B = 3, 133   # 133 rows: 9 tiles of 16 -> a partial workgroup (4 tiles), a partial wave, a partial tile (5 rows)
TOL, VAR_REL = 2e-5, 5e-5
# every (hidden blocks, head blocks) pair the library instantiates the ring kernel for: the 2-block head (O, A =
# 11, 3) exists at H = 64 and 200 only (bnn.hip launch_bf16)
RING_SHAPES = [(32, 17, 6), (64, 17, 6), (64, 11, 3), (200, 17, 6), (200, 11, 3)]


def scaled_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    return float(np.max(np.abs(a - b) / (1 + np.abs(b))))


@functools.lru_cache(maxsize=None)
def case(H, O, A):
    """Weights, inputs and the f64 oracle's outputs of one shape (computed once, shared, read-only)."""
    rs = np.random.RandomState(1000 * H + O)
    mats = obnn.to_mat_list(obnn.init_params(E, O, A, hidden=H, seed=3, inputs=rs.normal(size=(300, O + A)) * 3))
    x = (rs.normal(size=(B, O + A)) * 2).astype(np.float32)
    rm, rv = obnn.forward(obnn.from_mat_list(mats), x, dtype=np.float64)
    for a in mats + [x, rm, rv]:
        a.setflags(write=False)
    return mats, x, rm, rv


def make_model(mats, H, O, A, dtype, n=E):
    from mopo_amd.bnn import BNN
    return BNN({'name': 'ring', 'num_networks': n, 'num_elites': min(5, n), 'separate_mean_var': True, 'obs_dim': O,
                'act_dim': A, 'hidden_dim': H, 'dtype': dtype}).set_params(mats)


@pytest.mark.parametrize('dtype', ['bf16x6', 'f16x3'])
@pytest.mark.parametrize('H,O,A', RING_SHAPES)
def test_ring_predict_vs_f64_oracle(H, O, A, dtype):
    mats, x, rm, rv = case(H, O, A)
    mean, var = make_model(mats, H, O, A, dtype).predict(x, factored=True)
    errs = (scaled_err(mean, rm), scaled_err(var, rv), scaled_err(np.log(var), np.log(rv)),
            float(np.max(np.abs(var - rv) / rv)))
    print('H=%d O=%d A=%d %s: mean %.3g var %.3g log-var %.3g var rel %.3g' % ((H, O, A, dtype) + errs))
    assert errs[0] <= TOL and errs[1] <= TOL and errs[2] <= TOL and errs[3] < VAR_REL, errs


@pytest.mark.parametrize('dtype', ['bf16x6', 'f16x3'])
@pytest.mark.parametrize('H,rows', [(32, B), (64, B), (200, B), (200, 4099)])
def test_ring_predict_is_bit_identical_run_to_run(H, rows, dtype):
    """Ten predict calls on the same inputs give equal bits (4099 rows: 65 workgroups per member in flight)."""
    mats, x, _, _ = case(H, 17, 6)
    if rows != B:
        x = (np.random.RandomState(rows).normal(size=(rows, 23)) * 2).astype(np.float32)
    model = make_model(mats, H, 17, 6, dtype)
    m0, v0 = model.predict(x, factored=True)
    for _ in range(9):
        m, v = model.predict(x, factored=True)
        np.testing.assert_array_equal(m.view(np.uint32), m0.view(np.uint32))
        np.testing.assert_array_equal(v.view(np.uint32), v0.view(np.uint32))


@pytest.mark.parametrize('dtype', ['bf16x6', 'f16x3'])
def test_ring_rollout_is_bit_identical_run_to_run(dtype):
    """Two rollouts with one seed (B = 2112, h = 2) leave equal pool rows."""
    import torch
    from mopo_amd.bnn import construct_model
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout, init_sac_params
    dev = torch.device('cuda')
    model = construct_model(obs_dim=17, act_dim=6, hidden_dim=200, num_networks=7, num_elites=5,
                            separate_mean_var=True, seed=0, dtype=dtype)
    n, h = 2112, 2
    env = torch.from_numpy(np.random.RandomState(4).normal(size=(5000, 17)).astype(np.float32)).to(dev)
    pi = torch.from_numpy(init_sac_params(17, 6)).to(dev)
    ro = ModelRollout(model, n, h)
    rows = []
    for _ in range(2):
        pool = SimpleReplayPool(obs_dim=17, act_dim=6, max_size=n * h)
        steps = ro.run(env, pi, pool, n, h, 0, 1.0, [0, 1, 2, 3, 4], seed=11, epoch=0)
        assert pool.size == int(steps.sum())
        rows.append({k: v[:pool.size].cpu().numpy().copy() for k, v in pool.fields.items()})
    assert rows[0]['next_observations'].shape[0] > 0 and np.isfinite(rows[0]['next_observations']).all()
    for k in rows[0]:
        a, b = rows[0][k], rows[1][k]
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=k)
