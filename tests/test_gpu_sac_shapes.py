"""GPU parity: the SAC update (csrc/sac.hip) over the shapes mopo_sac_create accepts, against the fp64 oracle.

The cases, their groups and the tolerances are tests/sac_cases.py's (the tolerances are those of
tests/test_gpu_sac.py; none is new); tests/test_sac_cases.py shows on the CPU that fp32 rounding alone stays
within a tenth of every bound at every case, so a miss here is the kernels'.  Each test prints its worst
ratio to tolerance (1.0 is the bound) before it asserts.

A hand-off wait that gave up surfaces as SAC.logs() raising 'timed out': a finding about the fused launch,
to be read from the code, not a flake to run again.
"""
import numpy as np
import pytest

import sac_cases as sc

pytestmark = pytest.mark.gpu


def device_pools(ci):
    import torch
    from mopo_amd.replay_pool import SimpleReplayPool
    c = ci['case']
    out = []
    for s in (ci['env'], ci['mod']):
        p = SimpleReplayPool(obs_dim=c.o, act_dim=c.a, max_size=len(s['rewards']))
        p.add_samples(s)
        out.append(p)
    torch.cuda.synchronize()
    return out


def make_sac(ci, **kw):
    from mopo_amd.sac import SAC
    c = ci['case']
    hidden = c.hidden if np.isscalar(c.hidden) else list(c.hidden)
    sac = SAC(c.o, c.a, hidden, batch_size=c.n, real_ratio=sc.real_ratio(c), target_entropy=sc.TARGET_ENTROPY,
              params=sc.flat(ci['params']), log_alpha=float(ci['log_alpha']), action_prior=c.prior, **kw)
    assert sac.n_env == c.n_env and sac.hidden == sc.device_width(c.hidden)
    assert sac.n_params == sc.flat(ci['params']).size
    return sac


def device_state(sac):
    return {k: v.cpu().numpy() for k, v in sac.state_dict().items()}


def device_logs(sac):
    """The step's logs under the oracle's keys; raises if a hand-off wait gave up; all finite."""
    lg = sac.logs()
    assert all(np.isfinite(v) for v in lg.values()), lg
    return {rk: lg[dk] for dk, rk in sc.LOG_PAIRS}


def assert_padding_zero(sac):
    """A [H1, H2] network runs zero-padded to the square device width: everything outside each tensor's
    [H1, H2] corner stays exactly 0 in every raw device buffer (params, target, Adam m, v, gradients)."""
    pad = np.ones(sac._n_dev, bool)
    pad[sac._pad] = False
    assert pad.any()
    for w, extra in ((0, 1), (1, 0), (2, 1), (3, 1), (4, 1)):
        raw = sac._copy(w, sac._n_dev + extra).cpu().numpy()[:sac._n_dev]
        assert np.all(raw[pad] == 0), (w, np.abs(raw[pad]).max())


def report(case, ratios, extra=''):
    name, w = sc.worst(ratios)
    print('RATIO %s %-36s worst d/tol %.4f (%s)%s' % (case.group, sc.case_id(case), w, name, extra))
    bad = {k: round(v, 3) for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (sc.case_id(case), bad)


def assert_clipped_columns_stand_still(case, ci, ls_raw, got, grads=None):
    """The head columns whose raw log-std is clipped on every row of every step: no gradient reaches their
    pi.Wl column and pi.bl entry (clip_by_value's mask), exactly -- the gradient and both Adam slots are 0 and
    the parameters keep their bits, as in the oracle."""
    cols = sc.clipped_columns(ls_raw)
    want = np.flatnonzero(sc.head_classes(case) != 0)
    np.testing.assert_array_equal(cols, want)
    if not len(cols):
        return
    at = sc.head_column_index(case, cols)
    assert len(at) == len(cols) * (sc.osac._hs(case.hidden)[1] + 1)
    for name, v in (('gradient', grads), ('adam_m', got['adam_m']), ('adam_v', got['adam_v'])):
        if v is not None:
            assert np.all(np.asarray(v)[at] == 0), (name, np.abs(np.asarray(v)[at]).max())
    before = sc.flat(ci['params'])
    assert before.dtype == got['params'].dtype == np.float32
    np.testing.assert_array_equal(got['params'][at].view(np.uint32), before[at].view(np.uint32))
    moved = np.ones(before.size, bool)
    moved[at] = False
    assert (got['params'][:-1][moved] != before[moved]).mean() > 0.5          # ... while most of the rest moved


@pytest.mark.parametrize('case', [c for c in sc.by_group('A', 'B', 'G') if not c.steps], ids=sc.case_id)
def test_one_injected_step_vs_oracle(case):
    """Groups A, B, G: one step on injected rows and noise; logs, every gradient and the alpha gradient, the
    parameters, Adam slots and targets after the step.  G: the heads are saturated (sac_cases.py), and what
    the gradient mask must leave untouched is untouched exactly."""
    ci, ref = sc.reference_step(case)
    env_p, mod_p = device_pools(ci)
    sac = make_sac(ci)
    sac._do_training(0, env_p, mod_p, idx=ci['idx'], eps_s=ci['eps_s'], eps_n=ci['eps_n'])
    got = dict(logs=device_logs(sac), **device_state(sac))
    g, ga = sac.get_grads()
    got['grads'], got['g_alpha'] = [g.cpu().numpy()], float(ga.item())
    report(case, sc.step_ratios(got, ref))
    if not np.isscalar(case.hidden):
        assert_padding_zero(sac)
    if case.head:
        assert_clipped_columns_stand_still(case, ci, ref['ls_raw'][0], got, got['grads'][0])


@pytest.mark.parametrize('case', [c for c in sc.by_group('C', 'D', 'G') if c.steps], ids=sc.case_id)
def test_perf_mode_steps_vs_oracle(case):
    """Groups C, D, G: perf-mode steps under graph replay (device Philox rows and noise) against the oracle on
    the restated streams.  The handle does not expose the rows it sampled; a wrong row shows in every
    compared quantity, and a read of the unused NaN pool (n_env = 0, n_env = n) in all of them at once."""
    ref = sc.reference_steps(case)
    ci = sc.case_inputs(case)
    env_p, mod_p = device_pools(ci)
    sac = make_sac(ci)
    sac._do_training(0, env_p, mod_p, n_steps=case.steps, seed=sc.PERF_SEED)
    got = dict(logs=device_logs(sac), **device_state(sac))
    assert all(np.isfinite(v).all() for v in got.values() if isinstance(v, np.ndarray))
    report(case, sc.multi_ratios(got, ref), ' K=%d' % case.steps)
    if not np.isscalar(case.hidden):
        assert_padding_zero(sac)
    if case.head:
        assert_clipped_columns_stand_still(case, ci, ref['ls_raw'][:, 0], got)


@pytest.mark.parametrize('case', sc.by_group('E'), ids=sc.case_id)
def test_fused_launch_forms_bit_identical(case, monkeypatch):
    """Group E: MOPO_SAC_FUSE 0 (F1, F2, B1 separate), 1 (F2 + B1 one launch) and 2 (all three) compute the same
    arithmetic: 100 graph-replayed steps end bit-identical, with finite logs (a consumer that gave up waiting,
    or one that did not wait because its counter was never reset, would show here)."""
    import torch
    ci = sc.case_inputs(case)
    env_p, mod_p = device_pools(ci)
    out = {}
    for fuse in ('0', '1', '2'):
        monkeypatch.setenv('MOPO_SAC_FUSE', fuse)
        sac = make_sac(ci)
        sac._do_training(0, env_p, mod_p, n_steps=100, seed=19)
        torch.cuda.synchronize()
        device_logs(sac)
        out[fuse] = device_state(sac)
    for f in ('1', '2'):
        for k in out['0']:
            np.testing.assert_array_equal(out[f][k], out['0'][k], err_msg='MOPO_SAC_FUSE=%s %s' % (f, k))


@pytest.mark.parametrize('case', sc.by_group('E'), ids=sc.case_id)
def test_graph_replay_bit_identical_to_eager(case):
    """Group E: 11 steps = the 8-step, the 2-step and the 1-step graph, against eager launches."""
    ci = sc.case_inputs(case)
    env_p, mod_p = device_pools(ci)
    out = []
    for use_graph in (True, False):
        sac = make_sac(ci, use_graph=use_graph)
        sac._do_training(0, env_p, mod_p, n_steps=11, seed=19)
        device_logs(sac)
        out.append(device_state(sac))
    for k in out[0]:
        np.testing.assert_array_equal(out[0][k], out[1][k], err_msg=k)
    assert np.abs(out[0]['params'][:-1] - sc.flat(ci['params'])).max() > sc.LR_T


@pytest.mark.parametrize('kw,message', sc.REFUSALS, ids=[','.join('%s=%s' % kv for kv in kw.items()) for kw, _ in sc.REFUSALS])
def test_refusals(kw, message):
    """Group F: what mopo_sac_create does not take is refused at construction, by name."""
    from mopo_amd.sac import SAC
    with pytest.raises(RuntimeError, match=message):
        SAC(11, 3, **kw)
