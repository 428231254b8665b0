"""CPU: the oracle and the slot maps at ant's dimensions (27 observations + 8 actions: 35 inputs, 28 outputs).

  * the oracle against the wide reference fixtures (tests/golden/make_wide.py: the reference's own
    ``_compile_outputs`` and ``FakeEnv.step`` with ``mopo/static/ant.py``), at the tolerances of
    test_oracle_ref.py (forward in f64: 1e-10 relative) and test_oracle.py (FakeEnv post-processing bit-exact
    where the fixture stores the reference forward's mean / var);
  * ``slot_feat`` / ``head_col`` (csrc/mlp_tile.h), the two maps every packer and kernel shares, compiled as they
    stand with the host C++ compiler: every input feature and every head column appears exactly once.
"""
import ctypes
import glob
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import bnn as obnn
from oracle import fake_env as ofe
from test_oracle_ref import load_case, rel, scaled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
FWD = sorted(glob.glob(os.path.join(GOLD, 'wide_fwd_*.npz')))
ENV = sorted(glob.glob(os.path.join(GOLD, 'wide_fakeenv_*.npz')))
O, A = 27, 8


def wide_params(E, H, smv, seed, want_sha):
    """Weights of a wide case: regenerated from the seed as make_wide.py does, checked by sha256."""
    rs = np.random.RandomState(seed + 100)
    fit = rs.normal(size=(400, O + A)) * 1.5 + 0.2
    p = obnn.init_params(E, O, A, hidden=H, seed=seed, smv=smv, inputs=fit)
    h = hashlib.sha256()
    for a in obnn.to_mat_list(p):
        h.update(np.ascontiguousarray(a, np.float32).tobytes())
    assert h.hexdigest() == str(want_sha), 'regenerated weights differ from the reference case'
    return p


def fwd_params(z):
    return wide_params(int(z['E']), int(z['H']), bool(z['smv']), int(z['seed']), z['weights_sha'])


def env_params(c):
    return wide_params(int(c['E']), int(c['H']), True, int(c['wseed']), c['weights_sha'])


def test_wide_fixture_count():
    assert len(FWD) == 3 and len(ENV) == 20
    cases = [dict(np.load(p)) for p in ENV]
    assert {int(c['B']) for c in cases} == {1, 7, 64, 257}
    for key in ('learned_var', 'deterministic'):
        assert {int(c[key]) for c in cases} == {0, 1}
    assert {c['obs'].dtype for c in cases} == {np.dtype(np.float32), np.dtype(np.float64)}
    term = np.concatenate([c['term'][:, 0] for c in cases])
    assert term.any() and not term.all()          # both outcomes of ant.py's rule


@pytest.mark.parametrize('path', FWD, ids=[os.path.basename(p) for p in FWD])
def test_wide_forward_oracle_vs_reference_graph(path):
    z = load_case(path)
    assert (int(z['O']), int(z['A'])) == (O, A)
    assert not z['x'][0].any() and np.all(np.abs(z['x'][1]) == 40.0)   # the zero row, the saturating row
    p = fwd_params(z)
    m64, v64 = obnn.forward(p, z['x'], dtype=np.float64)
    assert rel(m64, z['mean_f64']) < 1e-10 or scaled(m64, z['mean_f64']) < 1e-13
    assert rel(v64, z['var_f64']) < 1e-10
    _, lv64 = obnn.forward(p, z['x'], dtype=np.float64, ret_log_var=True)
    assert scaled(lv64, z['logvar_f64']) < 1e-13
    assert scaled(m64, z['mean_f32']) < 2e-6
    assert rel(v64, z['var_f32']) < 2e-6


@pytest.mark.parametrize('path', ENV, ids=[os.path.basename(c) for c in ENV])
def test_wide_fakeenv_oracle_vs_reference(path):
    c = dict(np.load(path))
    params = env_params(c)
    det = bool(c['deterministic'])
    term_fn = ofe.TERMINATION[str(c['domain'])]
    kw = dict(penalty_coeff=float(c['penalty_coeff']), penalty_learned_var=bool(c['learned_var']), deterministic=det)
    if 'ref_mean' in c:
        np.random.seed(int(c['seed']))
        nobs, rew, term, info = ofe.step(params, list(c['elites']), c['obs'], c['act'], term_fn,
                                         predicted=(c['ref_mean'], c['ref_var']), **kw)
        if not det:
            np.testing.assert_array_equal(info['model_inds'], c['model_inds'])
        for got, key in ((nobs, 'next_obs'), (rew, 'rew'), (term, 'term'), (info['penalty'], 'penalty'),
                         (info['mean'], 'info_mean'), (info['std'], 'info_std'), (info['log_prob'], 'log_prob'),
                         (info['dev'], 'dev')):
            np.testing.assert_array_equal(got, c[key], err_msg=key)
        m, v = obnn.forward(params, np.concatenate((c['obs'], c['act']), axis=-1))
        assert np.max(np.abs(m - c['ref_mean']) / (1 + np.abs(c['ref_mean']))) < 2e-6
        assert np.max(np.abs(v - c['ref_var']) / np.abs(c['ref_var'])) < 2e-6
    np.random.seed(int(c['seed']))
    nobs, rew, term, info = ofe.step(params, list(c['elites']), c['obs'], c['act'], term_fn, **kw)
    if not det:
        np.testing.assert_array_equal(info['model_inds'], c['model_inds'])
    for got, key in ((nobs, 'next_obs'), (rew, 'rew'), (info['mean'], 'info_mean'), (info['std'], 'info_std')):
        assert np.max(np.abs(got - c[key]) / (1 + np.abs(c[key]))) < 5e-6, key
    if info['penalty'] is not None:
        assert np.max(np.abs(info['penalty'] - c['penalty']) / np.abs(c['penalty'])) < 5e-6
    bad = term[:, 0] != c['term'][:, 0]     # only where f32 rounding moves the height across a bound
    if bad.any():
        assert (np.abs(c['next_obs'][bad, 0][:, None] - np.array([0.2, 1.0])).min(1) < 1e-4).all()


# ---- slot_feat / head_col as csrc/mlp_tile.h states them -------------------------------------------------------
@pytest.fixture(scope='module')
def slot_maps(tmp_path_factory):
    src = open(os.path.join(ROOT, 'mopo_amd', 'csrc', 'mlp_tile.h')).read()
    fns = []
    for name in ('slot_feat', 'head_col'):
        m = re.search(r'__host__ __device__ __forceinline__ (int %s\(int slot, int \w+\) \{.*?\n\})' % name, src, re.S)
        assert m, name
        fns.append('extern "C" ' + m.group(1))
    cxx = next((c for c in (shutil.which('c++'), shutil.which('g++'), shutil.which('clang++'),
                            '/opt/rocm/lib/llvm/bin/clang++') if c and os.path.exists(c)), None)
    assert cxx, 'no host C++ compiler to build the slot maps with'
    d = tmp_path_factory.mktemp('slotmaps')
    cpp, so = str(d / 'maps.cpp'), str(d / 'maps.so')
    open(cpp, 'w').write('\n'.join(fns) + '\n')
    subprocess.check_call([cxx, '-O1', '-shared', '-fPIC', '-o', so, cpp])
    lib = ctypes.CDLL(so)
    for f in (lib.slot_feat, lib.head_col):
        f.argtypes, f.restype = [ctypes.c_int, ctypes.c_int], ctypes.c_int
    return lib


@pytest.mark.parametrize('IN', [33, 35, 48, 64, 23, 14])
def test_slot_feat_covers_every_feature_once(slot_maps, IN):
    """Over the 64 slots of a wide input row (4 k-groups of 16, or 2 of 32) every feature of IN appears exactly
    once and every other slot is padding (-1); a tail block of rem features uses registers t < ceil(rem / 4)."""
    got = [slot_maps.slot_feat(s, IN) for s in range(64)]
    assert sorted(k for k in got if k >= 0) == list(range(IN))
    assert all(k == -1 for k in got if k < 0)
    blk, rem = divmod(IN, 16)
    for s, k in enumerate(got):
        if s < 16 * blk:
            assert k == s
        elif k >= 0:
            assert s // 16 == blk and (s & 3) < (rem + 3) // 4


@pytest.mark.parametrize('D', [25, 28, 32, 18, 12])
def test_head_col_covers_every_column_once(slot_maps, D):
    """Over the 64 slots of a 4-block head every column of the fused [mean | log-var] head (2 D of them) appears
    exactly once; registers j < Q hold log-var columns, Q <= j < 2 Q mean columns (Q = ceil(D / 4))."""
    got = [slot_maps.head_col(s, D) for s in range(64)]
    assert sorted(c for c in got if c >= 0) == list(range(2 * D))
    Q = (D + 3) // 4
    for s, c in enumerate(got):
        j = 4 * (s >> 4) + (s & 3)
        if c >= 0:
            assert (c >= D) == (j < Q) and j < 2 * Q
