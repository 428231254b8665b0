"""The two forms of the training rollout's FakeEnv post kernel give the same bits.

``rollout_post_flat_kernel`` (one thread per (row, dim), the default for sampled steps with the max-aleatoric
penalty) and ``rollout_post_kernel`` (one 32-lane group per row, ``MOPO_POST_FLAT=0``) share the sample and the
observation noise of ``csrc/rollout_post.h`` and differ in how rows map to lanes, in where the pool position is
computed and in their epilogues.  Each case runs the same rollout once per form, in one process, each on a fresh
``ModelRollout`` and pool, and requires every pool field over the whole pool, ``steps``, the pool pointer and the
pool size to be equal bit for bit.  Every case: max-aleatoric penalty, not deterministic, coefficient 1 (the
only mode the flat form runs), E = 7, H = 64 (the post kernels do not depend on H).
"""
import numpy as np
import pytest

from test_gpu_rollout import _rollout_case, make_model

pytestmark = pytest.mark.gpu

DIMS = {'halfcheetah': (17, 6), 'walker2d': (17, 6), 'hopper': (11, 3), 'ant': (27, 8)}
E, H = 7, 64
# (domain, B, horizon, mode, pool max_size or None for B * horizon + 7, staged).  parity: the injected streams of
# _rollout_case; perf: the device's own Philox draws
CASES = [
    # the split path: parts of 2112 and 2021 rows, so a partial last 16-row block and a partial last 8-row block
    ('halfcheetah', 4133, 3, 'parity', None, False),
    ('halfcheetah', 4133, 3, 'perf', None, False),
    # compaction: keep / blockcnt written by both forms
    ('walker2d', 777, 4, 'parity', None, False),
    ('walker2d', 777, 4, 'perf', None, False),
    # D = 12: the flat block is 192 threads and a wave holds parts of six rows
    ('hopper', 300, 3, 'perf', None, False),
    # D = 28, the wide model
    ('ant', 300, 3, 'perf', None, False),
    # a pool smaller than B * horizon: the positions wrap (the flat form takes the modulo once per row)
    ('halfcheetah', 1000, 3, 'perf', 2500, False),
    # the staged layout: stage_base instead of the pool state
    ('halfcheetah', 1000, 3, 'perf', None, True),
]
_INPUTS = {}


def _inputs(domain, B, horizon):
    """Env rows, model, policy and injected streams of one (domain, B, horizon), computed once."""
    key = (domain, B, horizon)
    if key not in _INPUTS:
        o, a = DIMS[domain]
        _INPUTS[key] = _rollout_case(domain, E, H, B, horizon, seed=11, O=o, A=a)
    return _INPUTS[key]


def _run(monkeypatch, flat, domain, B, horizon, mode, max_size, staged):
    import torch
    from mopo_amd.replay_pool import SimpleReplayPool
    from mopo_amd.rollout import ModelRollout
    from mopo_amd.static import static_fns
    monkeypatch.setenv('MOPO_POST_FLAT', flat)
    c = _inputs(domain, B, horizon)
    o, a = DIMS[domain]
    model = make_model(c['mats'], E, H, O=o, A=a)
    pool = SimpleReplayPool(obs_dim=o, act_dim=a, max_size=max_size or B * horizon + 7)
    streams = dict(start_idx=c['start'], eps_act=c['eps_act'], eps_obs=c['eps_obs'], model_inds=c['inds']) \
        if mode == 'parity' else dict(seed=0x1234567890ab, epoch=3)
    steps = ModelRollout(model, B, horizon).run(
        torch.from_numpy(c['env_obs']).cuda(), torch.from_numpy(c['flat']).cuda(), pool, B, horizon,
        static_fns[domain].term_kind, 1.0, c['elites'], staged=staged, **streams)
    out = {k: v.cpu().numpy() for k, v in pool.fields.items()}
    out.update(steps=steps.cpu().numpy(), pointer=np.int64(pool._pointer), size=np.int64(pool.size))
    return out


@pytest.mark.parametrize('domain,B,horizon,mode,max_size,staged', CASES,
                         ids=['%s-B%d-%s%s%s' % (c[0], c[1], c[3], '-wrap' if c[4] else '', '-staged' if c[5] else '')
                              for c in CASES])
def test_flat_and_group_post_kernels_give_the_same_bits(monkeypatch, domain, B, horizon, mode, max_size, staged):
    flat = _run(monkeypatch, '1', domain, B, horizon, mode, max_size, staged)
    group = _run(monkeypatch, '0', domain, B, horizon, mode, max_size, staged)
    assert set(flat) == {'observations', 'actions', 'rewards', 'terminals', 'next_observations', 'steps', 'pointer',
                         'size'}
    for k in flat:
        np.testing.assert_array_equal(flat[k], group[k], err_msg=k)
    steps = flat['steps']
    assert steps[0] == B and np.isfinite(flat['next_observations']).all()
    if domain == 'walker2d':   # rows end and the rest are compacted: both forms wrote keep / blockcnt
        assert 0 < steps[-1] < steps[0] and (np.diff(steps) <= 0).all()
    if domain == 'halfcheetah':
        assert steps.tolist() == [B] * horizon
        n = len(flat['rewards'])
        if not staged:   # the wrapping case: 3000 rows into 2500 positions
            assert flat['size'] == min(B * horizon, n) and flat['pointer'] == B * horizon % n
