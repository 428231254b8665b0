"""CPU: the hard-truncation cases of tests/halt_cases.py meet the conditions tests/test_gpu_halt.py relies on, and
the host side of the feature: the quantile rule, the C layout of the appended fields, the Python / CLI validation.

The threshold of a case is a condition, not a tolerance (halt_cases.py): the table's entry is the midpoint of the
widest gap of the case's sorted u between the 50th and 90th percentile; no u of the f64 or of the f32 oracle lies
within 10 x the kind's device tolerance of it (kinds 0, 1: rel 1e-5; kinds 2, 3: 2 sqrt(D) 2e-5 (1 + max |ref|));
at least 10 % of the rows halt and at least 10 % reach the last step; and no row's termination rule is decided
within RULE_MARGIN of a bound.  The GPU tests then compare halted sets and terminals exactly, no row excluded.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import halt_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('key', hc.all_keys(), ids=lambda k: '-'.join(str(x) for x in k))
def test_case_meets_the_threshold_conditions(key):
    u, u32, m = hc.case_values(key)
    thr = hc.THRESHOLDS[key]
    assert thr == hc.gap_threshold(u)                      # the committed table is the rule's answer
    s = np.sort(u)                                         # between the 50th and 90th percentile's order statistics
    assert s[int(0.5 * (len(s) - 1))] < thr < s[int(np.ceil(0.9 * (len(s) - 1)))]
    r64, r32 = (np.abs(u - thr) / m).min(), (np.abs(u32 - thr) / m).min()
    halt, last = hc.case_shares(key)
    print('%s: threshold %.6g, min |u - thr| / margin: f64 %.3g f32 %.3g; halted %.3f, reach the last step %.3f'
          % (key, thr, r64, r32, halt, last))
    assert r64 > 1 and r32 > 1
    assert np.array_equal(u > thr, u32 > thr)              # both oracles halt the same rows
    assert halt >= 0.1 and last >= 0.1


@pytest.mark.parametrize('name', sorted(hc.ROLLOUT_CASES))
def test_rollout_case_rules_are_decided_clear_of_their_bounds(name):
    """Terminals are compared exactly on the GPU: every rule verdict has RULE_MARGIN to spare, the walker2d and
    ant cases really end rows by the rule (rule and halt together), some rows by both on one step."""
    for kind in hc.ROLLOUT_KINDS:
        c = hc.rollout_case(name, kind)
        d = np.concatenate([v['rule_distance'] for v in c['visits']])
        rule = np.concatenate([v['rule'] for v in c['visits']])
        halted = np.concatenate([v['halted'] for v in c['visits']])
        assert d.min() > hc.RULE_MARGIN
        assert len(c['steps']) == c['horizon'] and sum(c['halted_n']) == halted.sum()
        if c['domain'] != 'halfcheetah':
            assert (rule & ~halted).sum() >= 10 and (rule & halted).sum() >= 1
        else:
            assert not rule.any()
        # halted rows carry exactly the halt reward and a terminal in the oracle pool, the others neither
        ref = c['ref']
        np.testing.assert_array_equal(ref['rewards'][:, 0] == hc.HALT_REWARD, halted)
        np.testing.assert_array_equal(ref['terminals'][:, 0], rule | halted)


@pytest.mark.parametrize('shape', sorted(hc.STEP_SHAPES))
def test_step_case_rules_are_decided_clear_of_their_bounds(shape):
    c = hc.step_case(*shape)
    for det in (False, True):
        r = hc.step_reference(shape[0], shape[1], 1, max(hc.STEP_B), det, 1.0)
        assert hc.rule_distance(c['domain'], r['next_obs']).min() > hc.RULE_MARGIN
        if not det:    # sampled steps end rows by the rule, and halt rows the rule lets live
            assert r['rule'].any() and (r['halted'] & ~r['rule'][:, 0]).any()
    # the smaller batches are prefixes: the one-row batch halts under some kind and survives under another
    firsts = [bool(hc.step_u(shape[0], shape[1], k)[0] > hc.THRESHOLDS[('step',) + shape + (k,)]) for k in hc.KINDS]
    print(shape, 'row 0 halts per kind:', firsts)


def test_apply_halt_is_the_rule():
    rew = np.array([[1.0], [2.0], [3.0], [4.0]])
    term = np.array([[False], [True], [False], [False]])
    u = np.array([0.5, 2.0, np.nan, 1.0])
    r, t, h = hc.apply_halt(rew, term, u, 1.0, -7.0)
    assert h.tolist() == [False, True, True, False]          # u > threshold or NaN; u == threshold stays
    assert r[:, 0].tolist() == [1.0, -7.0, -7.0, 4.0] and t[:, 0].tolist() == [False, True, True, False]
    assert rew[1, 0] == 2.0 and not term[2, 0]               # inputs untouched


# ---- the quantile rule ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 10, 257, 1000])
def test_quantile_rule_against_numpy_sort(n):
    import torch
    from mopo_amd.evaluation import halt_threshold_from_quantile
    rs = np.random.RandomState(n)
    u = rs.gamma(2.0, size=n).astype(np.float32)
    u[rs.randint(0, n, n // 5)] = u[0]                       # ties
    s = np.sort(u)
    for q in (1e-9, 0.1, 0.5, 0.9, 0.99, 1.0, 1.0 / n, max(n - 1.0, 0.5) / n):
        want = s[int(np.ceil(q * n)) - 1]
        assert halt_threshold_from_quantile(u, q) == want
        assert halt_threshold_from_quantile(torch.from_numpy(u), q) == want
        assert halt_threshold_from_quantile(torch.from_numpy(u[::-1].copy()), q) == want
    for bad in (0.0, -0.1, 1.0001, float('nan')):
        with pytest.raises(ValueError):
            halt_threshold_from_quantile(u, bad)
    with pytest.raises(ValueError):
        halt_threshold_from_quantile(u[:0], 0.5)


# ---- the C layout --------------------------------------------------------------------------------------------------
C_PROBE = r'''
#include <stddef.h>
#include <stdio.h>
#include "mopo_hip.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("mopo_fakeenv_args %zu\n", sizeof(mopo_fakeenv_args));
  printf("mopo_rollout_args %zu\n", sizeof(mopo_rollout_args));
  printf("mopo_eval_args %zu\n", sizeof(mopo_eval_args));
  F(mopo_fakeenv_args, d_ens_var); F(mopo_fakeenv_args, halt); F(mopo_fakeenv_args, halt_threshold);
  F(mopo_fakeenv_args, halt_reward);
  F(mopo_rollout_args, actor_dtype); F(mopo_rollout_args, halt); F(mopo_rollout_args, halt_threshold);
  F(mopo_rollout_args, halt_reward); F(mopo_rollout_args, d_halted);
  F(mopo_eval_args, d_stats); F(mopo_eval_args, d_halted);
  return 0;
}
'''


def test_struct_layout_matches_the_header(tmp_path):
    """The ctypes mirrors against a C program compiled with include/mopo_hip.h: sizes, the offsets of the appended
    fields, and that they come last (behind the last field the structs had before)."""
    from mopo_amd import _lib as L
    cc = next((c for c in ('cc', 'gcc', 'clang', '/opt/rocm/llvm/bin/clang') if shutil.which(c)), None)
    assert cc, 'no C compiler found'
    src, exe = tmp_path / 'probe.c', tmp_path / 'probe'
    src.write_text(C_PROBE)
    subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(line.rsplit(' ', 1) for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                              text=True).stdout.splitlines())
    mirrors = {'mopo_fakeenv_args': L.FakeEnvArgs, 'mopo_rollout_args': L.RolloutArgs, 'mopo_eval_args': L.EvalArgs}
    for name, val in got.items():
        if '.' in name:
            st, f = name.split('.')
            assert getattr(mirrors[st], f).offset == int(val), name
        else:
            assert C.sizeof(mirrors[name]) == int(val), name
    assert [f for f, _ in L.FakeEnvArgs._fields_][-4:] == ['d_ens_var', 'halt', 'halt_threshold', 'halt_reward']
    assert [f for f, _ in L.RolloutArgs._fields_][-5:] == ['actor_dtype', 'halt', 'halt_threshold', 'halt_reward',
                                                          'd_halted']
    assert [f for f, _ in L.EvalArgs._fields_][-2:] == ['d_stats', 'd_halted']
    z = L.RolloutArgs(B=1)
    assert z.halt == 0 and z.halt_threshold == 0.0 and z.halt_reward == 0.0 and not z.d_halted


def test_entry_point_is_declared_and_bound():
    from mopo_amd import _lib as L
    assert hasattr(L.lib(), 'mopo_rollout_penalty_profile') and 'mopo_rollout_penalty_profile' in L.SIGNATURES
    assert 'mopo_rollout_penalty_profile' in open(os.path.join(ROOT, 'include', 'mopo_hip.h')).read()


# ---- Python and CLI validation ---------------------------------------------------------------------------------------
def test_halt_fields_validation():
    from mopo_amd.fake_env import halt_fields
    assert halt_fields() == (0, 0.0, 0.0) and halt_fields(None, -100.0) == (0, 0.0, 0.0)
    assert halt_fields(2.5, -100) == (1, 2.5, -100.0)
    assert halt_fields(float('inf'), 0.0) == (1, float('inf'), 0.0)
    for thr, rew in ((1.0, None), (float('nan'), -1.0), (1.0, float('inf')), (1.0, float('nan'))):
        with pytest.raises(ValueError):
            halt_fields(thr, rew)


def test_config_validation():
    from mopo_amd.config import check_halt_kwargs
    assert check_halt_kwargs({}) == {}
    ok = {'halt_quantile': 0.9, 'halt_reward': -100.0}
    assert check_halt_kwargs(dict(ok)) == ok
    check_halt_kwargs({'halt_threshold': 1.5, 'halt_reward': -1})
    for bad in ({'halt_threshold': 1.0, 'halt_quantile': 0.9, 'halt_reward': -1.0}, {'halt_threshold': 1.0},
                {'halt_quantile': 0.9}, {'halt_quantile': 0.0, 'halt_reward': -1.0},
                {'halt_quantile': 1.5, 'halt_reward': -1.0}, {'halt_threshold': float('nan'), 'halt_reward': -1.0},
                {'halt_threshold': 1.0, 'halt_reward': float('-inf')}):
        with pytest.raises(ValueError):
            check_halt_kwargs(bad)


def test_cli_flags_reach_the_variant_spec():
    from mopo_amd.__main__ import get_parser, variant_spec
    args = get_parser().parse_args(['--config', 'halfcheetah_medium', '--halt-quantile', '0.95', '--halt-reward', '-50'])
    kw = variant_spec(args)['algorithm_params']['kwargs']
    assert kw['halt_quantile'] == 0.95 and kw['halt_reward'] == -50.0 and 'halt_threshold' not in kw
    both = get_parser().parse_args(['--config', 'halfcheetah_medium', '--halt-quantile', '0.95', '--halt-threshold',
                                    '2', '--halt-reward', '-50'])
    with pytest.raises(ValueError):
        variant_spec(both)
    alone = get_parser().parse_args(['--config', 'halfcheetah_medium', '--halt-threshold', '2'])
    with pytest.raises(ValueError):
        variant_spec(alone)
    off = variant_spec(get_parser().parse_args(['--config', 'halfcheetah_medium']))['algorithm_params']['kwargs']
    assert not any(k.startswith('halt_') for k in off)


def test_run_cli_has_the_flags():
    import mopo_amd.run as run
    with pytest.raises(SystemExit) as e:
        run.main(['--help'])
    assert e.value.code == 0
    src = open(run.__file__).read()
    for flag in ('--halt-threshold', '--halt-quantile', '--halt-reward'):
        assert flag in src
