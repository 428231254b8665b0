"""GPU parity: every form of the ensemble training step (csrc/bnn_train.hip, train_rows.h, gemm_group.h) against
the fp64 oracle (oracle/bnn_train.py), at the cases of tests/train_cases.py.

test_gpu_train.py runs five of step_rows' ten train_rows_kernel<G0, GH, GD> instantiations, at hidden widths
that fill their last 16-block (or half of it), E = 3 / 7, and one shape of the generic path.  Here:
  a  every row form, over both minibatch geometries (train_cases.GEOMETRY: every launch path of an epoch);
  b  a partial last hidden block (H % 16 = 4, 12; 13 full blocks), with predict on the trained parameters;
  c  member counts 1, 8, 9, 16 (the second workgroup tier, tile lists that overflow across XCDs), the shuffle
     between two epochs at E = 16, the num_networks refusal;
  d  the generic grouped-GEMM step: widths without a row form, odd D, H % 4 != 0, K > 256, more than 8 members
     (a backward launch's two problems per member then exceed one grouped launch: step_impl once refused them);
  e  single-row minibatches;
  f  a and b again with MOPO_TRAIN_ROWS=0 (every shape on the generic path), without and with a
     retired knob that the library no longer reads;
  g  mopo_bnn_train_logs against the oracle's loss;  h  mopo_bnn_train_eval_mse;  i  snapshot / restore.
Each parity case first asks mopo_bnn_train_step_form which path its shape takes in this process, so a case
written for a row form cannot pass on the generic path unnoticed, and prints that form with its worst d / tol.

Tolerance of every parity case: the project's for several Adam steps (test_epoch_matches_oracle_steps), rtol
2e-5, atol 2e-5 max(1, max|ref|) per variable; tests/test_train_cases.py shows fp32 arithmetic alone stays
within 0.03 of it at every case.  Loss and mse values: rel 1e-5 (test_eval_mse_matches_oracle).
"""
import ctypes as C
import os

import numpy as np
import pytest

import train_cases as tc
from oracle import bnn as obnn
from oracle import bnn_train as ot

pytestmark = pytest.mark.gpu

# MOPO_TRAIN_ROWS is read once per process by the library; with 0 every shape takes the generic path (group f)
ROWS_ON = int(os.environ.get('MOPO_TRAIN_ROWS', '1') or 0) != 0


def cases(*groups):
    sel = [c for c in tc.CASES if c.group in groups]
    return pytest.mark.parametrize('case', sel, ids=tc.case_id)


def step_form(o, a, H, named):
    """Assert the path (o, a, H) steps on in this process is the one the case names; its printable name."""
    from mopo_amd import _lib as L
    blocks = (C.c_int * 3)(-1, -1, -1)
    r = L.lib().mopo_bnn_train_step_form(o, a, H, blocks)
    assert r == L.lib().mopo_bnn_train_step_form(o, a, H, None)           # blocks3 may be NULL
    want = named if ROWS_ON else None
    if want is None:
        assert r == 0 and tuple(blocks) == (-1, -1, -1), (r, tuple(blocks))
        return tc.form_name(None)
    assert r == 1 and tuple(blocks) == tuple(want), (r, tuple(blocks), want)
    return tc.form_name(tuple(blocks))


def make_model(E, o, a, H, mats):
    from mopo_amd.bnn import BNN
    return BNN({'name': 'forms', 'num_networks': E, 'num_elites': min(2, E), 'separate_mean_var': True,
                'obs_dim': o, 'act_dim': a, 'hidden_dim': H}).set_params(mats)


def trainer(m, mats, X, batch, max_eval=64):
    """test_gpu_train.setup_trainer, plus: the device's scaler is numpy's (mats[0:2] were fitted on X)."""
    from test_gpu_train import setup_trainer
    t, start = setup_trainer(m, X, batch, max_eval)
    np.testing.assert_allclose(start[0], mats[0], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(start[1], mats[1], rtol=1e-5, atol=1e-6)
    for s, m0 in zip(start[2:], mats[2:]):
        np.testing.assert_array_equal(s, m0)
    return t, start


def epoch(t, x, y, ix, batch):
    import torch
    from mopo_amd import _lib as L
    L.check(L.lib().mopo_bnn_train_epoch(t, L.ptr(x), L.ptr(y), L.ptr(ix), ix.shape[1], batch, None))
    torch.cuda.synchronize()


def close(got, ref, tol):
    assert np.max(np.abs(got - ref) / (1 + np.abs(ref))) <= tol


def run_parity(case):
    """Steps the case's epochs on the device and in the oracle; (model, trained .mat arrays, X)."""
    import torch
    from mopo_amd import _lib as L
    form = step_form(case.o, case.a, case.H, case.form)
    mats, X, Y, idxs = tc.case_inputs(case)
    batch = tc.GEOMETRY[case.geometry][1]
    m = make_model(case.E, case.o, case.a, case.H, mats)
    t, start = trainer(m, mats, X, batch)
    x, y = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    ix = None
    for idx, keys in tc.case_epochs(case):
        if keys is None:
            ix = torch.from_numpy(idx.astype(np.int32)).cuda()
        else:   # BNN.train's shuffle_rows between epochs: the device reorders the indices it trained on
            k = torch.from_numpy(keys).cuda()
            L.check(L.lib().mopo_bnn_train_shuffle(t, L.ptr(ix), L.ptr(k), idx.shape[1], None))
            torch.cuda.synchronize()
            np.testing.assert_array_equal(ix.cpu().numpy(), idx)             # np.argsort order, bit-exact
        epoch(t, x, y, ix, batch)
    got = m._train_params(t)
    ref = tc.oracle_steps(start, X, Y, idxs, batch)
    ratios = [tc.tol_ratio(g, r) for g, r in zip(got[2:], ref)]
    k = int(np.argmax(ratios))
    print('\n%-28s E=%-2d form %-9s worst d/tol %.3f (%s)' % (tc.case_id(case), case.E, form, ratios[k], tc.NAMES[k]))
    np.testing.assert_array_equal(got[0], start[0])                           # the scaler is no optimised variable
    np.testing.assert_array_equal(got[1], start[1])
    for name, g, r, s in zip(tc.NAMES, got[2:], ref, mats[2:]):
        assert g.shape == s.shape, name                                       # the logical shapes
        r = r.reshape(g.shape)
        np.testing.assert_allclose(g, r, rtol=tc.RTOL, atol=tc.ATOL * max(1.0, np.abs(r).max()), err_msg=name)
    return m, got, X


@cases('a')
def test_row_forms_match_oracle(case):
    run_parity(case)


@cases('b')
def test_partial_hidden_block_matches_oracle(case):
    """H % 16 != 0 inside a form's block range: the LDS activation columns H .. 16 GH must be zero, the weight
    rows k >= K must fall past the buffer range, the plain-offset loads' columns c >= N must only reach outputs
    the epilogue zeroes.  Then the trained logical arrays are repacked for inference and predicted with."""
    m, got, X = run_parity(case)
    m.set_params(got)
    x = X[:65]
    mean, var = m.predict(x)
    rm, rv = obnn.forward(obnn.from_mat_list(got), x, dtype=np.float64)
    close(mean, rm, 2e-5)
    close(var, rv, 2e-5)


@cases('c')
def test_member_counts_match_oracle(case):
    run_parity(case)


@cases('d')
def test_generic_path_matches_oracle(case):
    run_parity(case)


@cases('e')
def test_single_row_minibatches_match_oracle(case):
    run_parity(case)


@pytest.mark.parametrize('E', [0, 17])
def test_num_networks_outside_1_16_is_refused(E):
    from mopo_amd import _lib as L
    t = C.c_void_p()
    rc = L.lib().mopo_bnn_train_create(C.byref(t), E, 11, 3, 32, 24, 64, 1e-3)
    assert rc != 0 and not t.value
    assert 'num_networks' in L.lib().mopo_last_error().decode()


# ---- f. the knobs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('knobs', ['MOPO_TRAIN_ROWS=0', 'MOPO_TRAIN_ROWS=0,MOPO_TRAIN_WGRAD_TILE=16'])
def test_generic_path_knobs_match_oracle(knobs):
    """MOPO_TRAIN_ROWS=0 sends every shape of groups a and b down the generic path (twelve grouped-GEMM launches).
    MOPO_TRAIN_WGRAD_TILE was read by a three-launch row path that no build could reach and that has been removed;
    nothing reads it now, so setting it must change nothing.  MOPO_TRAIN_ROWS is read once per process, so each
    setting runs the two groups in a fresh process, where the step-form assertion expects the generic path."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **dict(kv.split('=') for kv in knobs.split(',')))
    r = subprocess.run([sys.executable, '-m', 'pytest', '-p', 'no:cacheprovider', '-q', '-x', '-s', '-m', 'gpu',
                        os.path.abspath(__file__), '-k', 'row_forms_match or partial_hidden_block'],
                       cwd=root, env=env, capture_output=True, text=True, timeout=300)
    print('\n[%s]\n%s' % (knobs, '\n'.join(l for l in r.stdout.splitlines() if 'worst d/tol' in l)))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    last = r.stdout.splitlines()[-1]
    n = len([c for c in tc.CASES if c.group in 'ab'])
    assert ' %d passed' % n in ' ' + last and 'skipped' not in last, r.stdout[-500:]
    assert r.stdout.count('form generic') == n                              # every one of them on the generic path


# ---- g. the loss log ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('E,o,a,H,named', tc.LOSS_CASES, ids=['E%d-%d+%d-H%d' % c[:4] for c in tc.LOSS_CASES])
def test_loss_log_matches_oracle(E, o, a, H, named):
    """mopo_bnn_train_logs after one eager minibatch (17 rows of a batch-24 trainer: a full row block and one
    row): the step's loss on the pre-step parameters, without the decays and the 0.01 bound terms."""
    import torch
    from mopo_amd import _lib as L
    from test_gpu_train import to_oracle
    form = step_form(o, a, H, named)
    mats, X, Y, idx = tc.loss_inputs(E, o, a, H)
    m = make_model(E, o, a, H, mats)
    t, start = trainer(m, mats, X, 24)
    epoch(t, torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), torch.from_numpy(idx.astype(np.int32)).cuda(), 24)
    out = np.full(1, np.nan, np.float32)
    L.check(L.lib().mopo_bnn_train_logs(t, L.ptr(out), 1))
    ref = tc.data_loss(to_oracle(start), X[idx], Y[idx])
    print('\nloss log E=%d %d+%d H=%d form %s: %.7g vs %.7g, rel %.2e' % (E, o, a, H, form, out[0], ref,
                                                                         abs(out[0] - ref) / abs(ref)))
    np.testing.assert_allclose(out[0], ref, rtol=1e-5)


# ---- h. eval_mse --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(7, 17, 6, 200), (3, 10, 3, 50)], ids=['E7-17+6-H200', 'E3-10+3-H50'])
def test_eval_mse_sizes_and_member_rows(shape):
    """n = 1, 31 (the small-tile branch), 32, 50 on the first n rows, n = 50 on each member's own rows, and the
    refusals of n = 0 and n > max(max_batch, max_eval)."""
    import torch
    from mopo_amd import _lib as L
    from test_gpu_train import to_oracle
    E, o, a, H = shape
    X, Y = tc.make_data(200, o, a, seed=4)
    mats = tc.make_mats(E, o, a, H, X)
    m = make_model(E, o, a, H, mats)
    t, start = trainer(m, mats, X, 24, max_eval=64)
    p = to_oracle(start)
    x, y = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    out = torch.empty(E, dtype=torch.float32, device='cuda')
    mse = L.lib().mopo_bnn_train_eval_mse
    for n in (1, 31, 32, 50):
        out.fill_(float('nan'))
        L.check(mse(t, L.ptr(x), L.ptr(y), None, n, L.ptr(out), None))
        ref = ot.mse_losses(p, np.tile(X[None, :n], [E, 1, 1]), np.tile(Y[None, :n], [E, 1, 1]))
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-5, err_msg='n = %d' % n)
    rs = np.random.RandomState(9)
    rows = np.stack([rs.choice(200, 50, replace=False) for _ in range(E)]).astype(np.int32)
    assert len({tuple(r) for r in rows}) == E
    out.fill_(float('nan'))
    L.check(mse(t, L.ptr(x), L.ptr(y), L.ptr(torch.from_numpy(rows).cuda()), 50, L.ptr(out), None))
    np.testing.assert_allclose(out.cpu().numpy(), ot.mse_losses(p, X[rows], Y[rows]), rtol=1e-5, err_msg='member rows')
    for n in (0, 65):
        assert mse(t, L.ptr(x), L.ptr(y), None, n, L.ptr(out), None) != 0
        assert 'mopo_bnn_train_eval_mse: n must be in' in L.lib().mopo_last_error().decode()
    torch.cuda.synchronize()


# ---- i. snapshot / restore ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('E', [5, 16])
def test_snapshot_restore_is_bit_exact(E):
    """_save_state / _set_state (bnn.py:264-285): the snapshotted members return to the values they had when
    snapshotted, every other member and the shared log-var bounds keep what the epoch trained."""
    import torch
    from mopo_amd import _lib as L
    lib = L.lib()
    o, a, H = 11, 3, 32
    rows, batch = tc.GEOMETRY['short']
    X, Y = tc.make_data(rows, o, a)
    mats = tc.make_mats(E, o, a, H, X)
    m = make_model(E, o, a, H, mats)
    t, start = trainer(m, mats, X, batch)
    ids = [E - 1, 1, E - 1, E // 2, 1]                      # duplicates: each member is copied once
    saved = sorted(set(ids) | {0})
    L.check(lib.mopo_bnn_train_snapshot_members(t, (C.c_int * len(ids))(*ids), len(ids), None))
    L.check(lib.mopo_bnn_train_snapshot(t, 0, None))
    for bad in (E, -1):
        assert lib.mopo_bnn_train_snapshot(t, bad, None) != 0
        assert 'mopo_bnn_train_snapshot: bad member' in lib.mopo_last_error().decode()
    idx = np.random.RandomState(7).randint(rows, size=[E, rows]).astype(np.int32)
    epoch(t, torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), torch.from_numpy(idx).cuda(), batch)
    trained = m._train_params(t)
    L.check(lib.mopo_bnn_train_restore(t, None))
    torch.cuda.synchronize()
    back = m._train_params(t)
    others = [e for e in range(E) if e not in saved]
    assert len(saved) == 4 and others
    for k in range(2, 14):                                   # the per-member variables
        np.testing.assert_array_equal(back[k][saved], start[k][saved])
        np.testing.assert_array_equal(back[k][others], trained[k][others])
        for e in range(E):                                   # and the epoch did move every member
            assert not np.array_equal(trained[k][e], start[k][e])
    for k in (0, 1, 14, 15):                                 # scaler and the shared bounds: not snapshotted
        np.testing.assert_array_equal(back[k], trained[k])
    L.check(lib.mopo_bnn_train_restore(t, None))             # nothing is pending: a second restore is a no-op
    torch.cuda.synchronize()
    for b2, b1 in zip(m._train_params(t), back):
        np.testing.assert_array_equal(b2, b1)
