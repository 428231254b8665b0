"""CPU: the host side of the open-loop model validation -- the continuation rule, the statistics table by hand,
the metric keys, the CLI flags down to the MOPO kwargs, the C-ABI declaration.  The device side is
tests/test_gpu_model_val.py."""
import inspect
import json
from collections import OrderedDict

import numpy as np
import pytest


def _pool40():
    """40 rows: episode A rows 0..9 ends by terminal; B rows 10..21 ends by a discontinuity without a flag
    (a timeout); C is the single row 22 (terminal); D rows 23..39 runs into the end of the pool."""
    obs = np.arange(40, dtype=np.float32)[:, None] * np.ones((1, 3), np.float32)
    nobs = obs + 1                                        # next_obs[j] == obs[j + 1] inside an episode
    term = np.zeros(40, np.uint8)
    term[9] = 1
    nobs[21] += 0.5                                       # B's last row: obs[22] is not next_obs[21]
    term[22] = 1
    return obs, nobs, term


def test_segment_lengths_on_a_hand_built_pool():
    from mopo_amd.evaluation import END_REASONS, segment_lengths_numpy
    obs, nobs, term = _pool40()
    assert END_REASONS == ('horizon', 'terminal', 'discontinuity', 'end-of-pool')
    # (start, K) -> (length, reason)
    cases = [((0, 5), (5, 0)),        # K shorter than the episode
             ((0, 10), (10, 0)),      # K exactly the episode: the horizon comes first
             ((0, 15), (10, 1)),      # K longer: the terminal flag ends it
             ((7, 5), (3, 1)),
             ((10, 30), (12, 2)),     # the unflagged discontinuity
             ((20, 2), (2, 0)), ((20, 3), (2, 2)),
             ((22, 4), (1, 1)),       # the one-row episode
             ((22, 1), (1, 0)),
             ((23, 40), (17, 3)),     # runs into the end of the pool
             ((39, 3), (1, 3)),       # starts at the last row
             ((39, 1), (1, 0)),
             ((40, 3), (0, 3)), ((-1, 3), (0, 3))]   # a start outside the pool takes no step
    for (start, K), exp in cases:
        length, end = segment_lengths_numpy(obs, nobs, term, 40, [start], K)
        assert (int(length[0]), int(end[0])) == exp, (start, K)
    # vectorised over the starts, and size < len(obs) cuts the pool
    length, end = segment_lengths_numpy(obs, nobs, term, 30, [0, 10, 23, 29, 30], 12)
    assert length.tolist() == [10, 12, 7, 1, 0] and end.tolist() == [1, 0, 3, 3, 3]
    assert length.dtype == np.int32 and end.dtype == np.uint8


def test_discontinuity_compares_bit_patterns():
    """NaN == NaN bit for bit continues; +0.0 against -0.0 is a discontinuity (the kernel compares words)."""
    from mopo_amd.evaluation import segment_lengths_numpy
    obs = np.zeros((4, 2), np.float32)
    nobs = np.zeros((4, 2), np.float32)
    obs[1, 0] = nobs[0, 0] = np.nan
    nobs[1, 1] = -0.0
    length, end = segment_lengths_numpy(obs, nobs, np.zeros(4), 4, [0], 4)
    assert (int(length[0]), int(end[0])) == (2, 2)


def test_metrics_table_by_hand():
    """K = 3 steps x B = 4 segments with lengths (3, 1, 2, 0): step 0 has n = 3, step 1 n = 2 with a constant
    penalty (zero variance), step 2 n = 1; both of those have correlation 0."""
    from mopo_amd.evaluation import open_loop_metrics_numpy
    nan = np.nan
    lengths = [3, 1, 2, 0]
    eo = np.array([[3.0, 6.0, 0.0, nan], [5.0, nan, 8.0, nan], [1.0, nan, nan, nan]])
    er = np.array([[4.0, -8.0, 2.0, nan], [-12.0, nan, 6.0, nan], [0.0, nan, nan, nan]])
    e = np.sqrt(eo ** 2 + er ** 2)                       # 5 10 2 / 13 10 / 1
    u = np.array([[6.0, 9.0, 3.0, nan], [4.0, nan, 4.0, nan], [1.0, nan, nan, nan]], np.float32)
    tp = np.array([[0, 1, 0, 255], [1, 255, 0, 255], [0, 255, 255, 255]], np.uint8)
    td = np.array([[0, 1, 0, 255], [0, 255, 0, 255], [1, 255, 255, 255]], np.uint8)
    t = open_loop_metrics_numpy(e, eo, er, u, tp, td, lengths, penalty_learned_var=True)
    assert t.shape == (4, 16) and not t[:, 11:].any()
    # step 0: err 5, 10, 2; u 6, 9, 3
    m, mu = 17 / 3, 6.0
    var_e = ((5 - m) ** 2 + (10 - m) ** 2 + (2 - m) ** 2) / 3
    cov = ((6 - mu) * (5 - m) + (9 - mu) * (10 - m) + (3 - mu) * (2 - m)) / 3
    exp0 = [3, m, np.sqrt(var_e), 10, 3.0, 14 / 3, 6.0, np.sqrt(6.0), cov / np.sqrt(var_e * 6.0), 2 / 3, 0.0]
    np.testing.assert_allclose(t[0, :11], exp0, rtol=1e-14, atol=0)
    # step 1: err 13, 10; u 4, 4 -> zero variance of u: correlation 0
    np.testing.assert_allclose(t[1, :11], [2, 11.5, 1.5, 13, 6.5, 9.0, 4.0, 0.0, 0.0, 0.0, 0.5], rtol=1e-14, atol=0)
    # step 2: n = 1 -> correlation 0
    np.testing.assert_allclose(t[2, :11], [1, 1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0], rtol=1e-14, atol=0)
    # pooled: the six live entries
    ev, uv = np.array([5, 10, 2, 13, 10, 1.0]), np.array([6, 9, 3, 4, 4, 1.0])
    corr = np.mean((ev - ev.mean()) * (uv - uv.mean())) / (ev.std() * uv.std())
    expp = [6, ev.mean(), ev.std(), 13, 23 / 6, 32 / 6, uv.mean(), uv.std(), corr, 3 / 6, 2 / 6]
    np.testing.assert_allclose(t[3, :11], expp, rtol=1e-14, atol=0)
    # the mean-distance penalty is held against err_obs: coverage and correlation change, the means do not
    t2 = open_loop_metrics_numpy(e, eo, er, u, tp, td, lengths, penalty_learned_var=False)
    np.testing.assert_array_equal(t2[:, :8], t[:, :8])
    assert t2[0, 9] == 1.0 and t2[1, 9] == 0.0 and t2[3, 9] == 4 / 6
    ov = np.array([3, 6, 0, 5, 8, 1.0])
    np.testing.assert_allclose(t2[3, 8], np.mean((ov - ov.mean()) * (uv - uv.mean())) / (ov.std() * uv.std()),
                               rtol=1e-14)
    # no segment at all: every row zero
    z = open_loop_metrics_numpy(e[:, 3:], eo[:, 3:], er[:, 3:], u[:, 3:], tp[:, 3:], td[:, 3:], [0])
    assert z.shape == (4, 16) and not z.any()


def test_metric_key_names():
    from mopo_amd.evaluation import OPEN_LOOP_SLOTS, open_loop_metrics
    K = 3
    stats = np.arange((K + 1) * 16, dtype=np.float64).reshape(K + 1, 16) + 0.25
    d = open_loop_metrics(stats)
    assert isinstance(d, OrderedDict)
    per = ['error', 'obs-error', 'penalty', 'covered', 'alive']
    exp = ['open_loop/%s-h%d' % (n, k) for k in range(1, K + 1) for n in per]
    exp += ['open_loop/' + n for n in ('error', 'penalty', 'penalty-error-corr', 'covered', 'termination-mismatch')]
    assert list(d) == exp
    col = {n: i for i, n in enumerate(OPEN_LOOP_SLOTS)}
    for k in range(1, K + 1):
        assert d['open_loop/error-h%d' % k] == stats[k - 1, col['error']]
        assert d['open_loop/obs-error-h%d' % k] == stats[k - 1, col['obs-error']]
        assert d['open_loop/penalty-h%d' % k] == stats[k - 1, col['penalty']]
        assert d['open_loop/covered-h%d' % k] == stats[k - 1, col['covered']]
        assert d['open_loop/alive-h%d' % k] == stats[k - 1, col['n']]
    for n in ('error', 'penalty', 'penalty-error-corr', 'covered', 'termination-mismatch'):
        assert d['open_loop/' + n] == stats[K, col[n]]


def test_mopo_defaults_to_no_validation():
    from mopo_amd.mopo import MOPO
    sig = inspect.signature(MOPO.__init__).parameters
    assert sig['model_val_segments'].default == 0 and sig['model_val_horizon'].default is None
    assert MOPO.MODEL_VAL_SEED_XOR != MOPO.MODEL_EVAL_SEED_XOR and MOPO.MODEL_VAL_SEED_XOR >> 62 == 1
    for seed in (0, 88, 2 ** 31, 2 ** 61 - 1):
        k = seed ^ MOPO.MODEL_VAL_SEED_XOR
        assert k >= 2 ** 62 > seed + 7919 * 10 ** 6 and k != seed ^ MOPO.MODEL_EVAL_SEED_XOR


def test_cli_flags_reach_the_spec_and_default_off(capsys):
    from mopo_amd.__main__ import main
    cfg = '--config=examples.config.d4rl.halfcheetah_mixed'
    assert main(['run_example_dry', 'examples.development', cfg, '--model-val-segments=64',
                 '--model-val-horizon=20']) == 0
    out = capsys.readouterr().out
    kw = json.loads(out[:out.rindex('}') + 1])['algorithm_params']['kwargs']
    assert (kw['model_val_segments'], kw['model_val_horizon']) == (64, 20)
    assert main(['run_example_dry', 'examples.development', cfg]) == 0
    out = capsys.readouterr().out
    kw = json.loads(out[:out.rindex('}') + 1])['algorithm_params']['kwargs']
    assert 'model_val_segments' not in kw and 'model_val_horizon' not in kw


def test_run_local_forwards_the_flags(monkeypatch):
    from mopo_amd import __main__ as cli
    from mopo_amd import run
    seen = []
    monkeypatch.setattr(run, 'main', lambda argv: seen.append(list(argv)))
    base = ['run_local', 'examples.development', '--config=examples.config.d4rl.halfcheetah_mixed', '--data=x.npz']
    assert cli.main(base + ['--model-val-segments=32', '--model-val-horizon=5']) == 0
    assert cli.main(base) == 0
    a, b = seen
    assert a[a.index('--model-val-segments') + 1] == '32' and a[a.index('--model-val-horizon') + 1] == '5'
    assert not [x for x in b if x.startswith('--model-val')]


@pytest.mark.parametrize('flags,exp', [(['--model-val-segments', '16', '--model-val-horizon', '30'],
                                        {'model_val_segments': 16, 'model_val_horizon': 30}),
                                       (['--model-val-segments', '0'], {'model_val_segments': 0}), ([], {})])
def test_run_flags_reach_the_mopo_kwargs(monkeypatch, flags, exp):
    import mopo_amd.loader
    import mopo_amd.mopo
    import mopo_amd.replay_pool
    from mopo_amd import run
    seen = {}

    class Algo:
        def train(self, n):
            return iter(())

    def from_config(params, pool, static_fns, **kw):
        seen.update(kw)
        return Algo()

    monkeypatch.setattr(mopo_amd.mopo, 'from_config', from_config)
    monkeypatch.setattr(mopo_amd.loader, 'restore_pool', lambda pool, path: None)
    monkeypatch.setattr(mopo_amd.replay_pool, 'SimpleReplayPool', lambda **kw: object())
    run.main(['--config', 'examples.config.d4rl.halfcheetah_mixed', '--data', 'x.npz'] + flags)
    assert {k: v for k, v in seen.items() if k.startswith('model_val')} == exp


def test_validate_is_declared_and_bound():
    import os
    from mopo_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, 'include', 'mopo_hip.h')).read()
    assert 'int mopo_rollout_validate(' in src and '} mopo_val_args;' in src
    assert 'mopo_rollout_validate' in _lib.SIGNATURES
    assert hasattr(_lib.lib(), 'mopo_rollout_validate')
    # the ctypes struct follows the header's field order
    names = [n for n, _ in _lib.ValArgs._fields_]
    first = src.index('double* d_err;')
    pos = [src.index(' ' + n + ';', first - 1) for n in names]
    assert pos == sorted(pos) and pos[0] == first + len('double*')
