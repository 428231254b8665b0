"""CPU: the host side of model-based policy evaluation -- the metric dict against evaluate_rollouts, the
CLI flags down to the MOPO kwargs, the C-ABI declaration.  The device side is tests/test_gpu_model_eval.py."""
import inspect
import json
from collections import OrderedDict

import numpy as np
import pytest


def _paths(rs, n):
    out = []
    for _ in range(n):
        T = int(rs.randint(1, 40))
        out.append({'rewards': rs.normal(size=(T, 1)) * 3 + 1, 'penalty': rs.uniform(0, 2, T),
                    'terminated': bool(rs.randint(2))})
    return out


@pytest.mark.parametrize('n', [1, 7, 300])
def test_numpy_metrics_equal_evaluate_rollouts(n):
    from mopo_amd.evaluation import MODEL_EVAL_KEYS, evaluate_rollouts, model_evaluation_metrics_numpy
    paths = _paths(np.random.RandomState(n), n)
    ref = evaluate_rollouts(paths)
    ret = [float(np.sum(p['rewards'])) for p in paths]
    length = [len(p['rewards']) for p in paths]
    pen = [float(np.sum(p['penalty'])) for p in paths]
    pret = [r - 0.5 * q for r, q in zip(ret, pen)]
    term = [p['terminated'] for p in paths]
    got = model_evaluation_metrics_numpy(ret, length, pret, pen, term)
    assert isinstance(got, OrderedDict) and tuple(got) == MODEL_EVAL_KEYS
    assert list(got)[:8] == list(ref)                        # evaluate_rollouts' keys, in its order
    for k, v in ref.items():
        assert got[k] == float(v), k
    assert got['penalized-return-average'] == float(np.mean(pret))
    assert got['penalty-average'] == float(np.sum(pen) / np.sum(length))
    assert got['terminated-fraction'] == float(np.mean(term))
    assert not any(k.startswith('perf/') or 'Normalized' in k for k in got)   # no D4RL score from the model


def test_device_stats_map_to_the_same_keys():
    from mopo_amd.evaluation import MODEL_EVAL_KEYS, model_evaluation_metrics
    stats = np.arange(16, dtype=np.float64) + 0.5
    d = model_evaluation_metrics(stats)
    assert tuple(d) == MODEL_EVAL_KEYS and len(d) == 11
    assert [d[k] for k in MODEL_EVAL_KEYS] == list(stats[:11])


def test_mopo_defaults_to_no_model_evaluation():
    from mopo_amd.mopo import MOPO
    sig = inspect.signature(MOPO.__init__).parameters
    assert sig['model_eval_episodes'].default == 0 and sig['model_eval_length'].default is None
    # the evaluation's Philox key differs from the rollouts' (seed) and the SAC steps' (seed + 7919 epoch)
    for seed in (0, 88, 2 ** 31, 2 ** 61 - 1):
        k = seed ^ MOPO.MODEL_EVAL_SEED_XOR
        assert k >= 2 ** 62 > seed + 7919 * 10 ** 6


def test_cli_flags_reach_the_spec_and_default_off(capsys):
    from mopo_amd.__main__ import main
    cfg = '--config=examples.config.d4rl.halfcheetah_mixed'
    assert main(['run_example_dry', 'examples.development', cfg, '--model-eval-episodes=64',
                 '--model-eval-length=200']) == 0
    out = capsys.readouterr().out
    kw = json.loads(out[:out.rindex('}') + 1])['algorithm_params']['kwargs']
    assert (kw['model_eval_episodes'], kw['model_eval_length']) == (64, 200)
    assert main(['run_example_dry', 'examples.development', cfg]) == 0
    out = capsys.readouterr().out
    kw = json.loads(out[:out.rindex('}') + 1])['algorithm_params']['kwargs']
    assert 'model_eval_episodes' not in kw and 'model_eval_length' not in kw


def test_run_local_forwards_the_flags(monkeypatch):
    from mopo_amd import __main__ as cli
    from mopo_amd import run
    seen = []
    monkeypatch.setattr(run, 'main', lambda argv: seen.append(list(argv)))
    base = ['run_local', 'examples.development', '--config=examples.config.d4rl.halfcheetah_mixed', '--data=x.npz']
    assert cli.main(base + ['--model-eval-episodes=32', '--model-eval-length=50']) == 0
    assert cli.main(base) == 0
    a, b = seen
    assert a[a.index('--model-eval-episodes') + 1] == '32' and a[a.index('--model-eval-length') + 1] == '50'
    assert not [x for x in b if x.startswith('--model-eval')]


@pytest.mark.parametrize('flags,exp', [(['--model-eval-episodes', '16', '--model-eval-length', '30'],
                                        {'model_eval_episodes': 16, 'model_eval_length': 30}),
                                       (['--model-eval-episodes', '0'], {'model_eval_episodes': 0}), ([], {})])
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
    assert {k: v for k, v in seen.items() if k.startswith('model_eval')} == exp


def test_evaluate_is_declared_and_bound():
    import os
    from mopo_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, 'include', 'mopo_hip.h')).read()
    assert 'int mopo_rollout_evaluate(' in src and '} mopo_eval_args;' in src
    assert 'mopo_rollout_evaluate' in _lib.SIGNATURES
    assert hasattr(_lib.lib(), 'mopo_rollout_evaluate')
    # the ctypes struct follows the header's field order
    names = [n for n, _ in _lib.EvalArgs._fields_]
    pos = [src.index(' ' + n + ';', src.index('int policy_deterministic')) if n != 'policy_deterministic'
           else src.index('int policy_deterministic') for n in names]
    assert pos == sorted(pos)
