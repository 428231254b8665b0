"""CPU: SAC at ant's shape (27 observations + 8 actions: the critics read 35 inputs, past one 32-wide layer-1
group).  The f64 oracle is pinned to the reference's own graph at this shape (tests/golden/antsac_O27_A8_H64.npz,
made by tests/golden/make_antsac_vectors.py the way the ref_sac_* cases are), the config knows the domain's
dimensions, and the parameter layout / non-square embedding helpers hold at 27 + 8."""
import os

import numpy as np
import pytest

import test_oracle_ref as tor
from oracle import sac as osac

ANT = os.path.join(tor.GOLD, 'antsac_O27_A8_H64.npz')
O, A = 27, 8


def test_antsac_fixture_shape():
    z = tor.load_case(ANT)
    assert (int(z['O']), int(z['A']), int(z['H']), int(z['n']), int(z['steps'])) == (O, A, 64, 64, 2)
    assert z['init8'].shape == (O + A, 64)          # q1's first layer: 35 input rows
    assert os.path.getsize(ANT) < 1 << 20
    with np.load(ANT, allow_pickle=False) as raw:   # arrays only
        assert len(raw.files) == len(z)


def test_sac_oracle_vs_reference_graph_at_ant_shape():
    """The assertions of test_oracle_ref.py::test_sac_oracle_vs_reference_graph, on the case at ant's shape."""
    tor.test_sac_oracle_vs_reference_graph(ANT)


def test_actor_oracle_vs_reference_graph_at_ant_shape():
    z = tor.load_case(ANT)
    P = osac.split([z['init%d' % i].astype(np.float64) for i in range(20)])[0]
    a, mu = osac.actor_act(P, z['b0_observations'].astype(np.float64), z['b0_noise0'][0].astype(np.float64))
    np.testing.assert_allclose(a, z['actor_pi_f64'], rtol=0, atol=1e-12)
    np.testing.assert_allclose(mu, z['actor_mu_f64'], rtol=0, atol=1e-12)
    assert np.max(np.abs(a - z['actor_pi_f32'])) < 1e-6


def test_config_dims_of_ant():
    from mopo_amd.config import DIMS
    from mopo_amd.static import static_fns
    assert DIMS['ant'] == (27, 8) and DIMS['antangle'] == (27, 8)
    assert 'ant' in static_fns and 'antangle' in static_fns


def test_user_config_module_with_ant_domain(tmp_path, monkeypatch):
    """A user's own config module with ``domain: 'ant'`` resolves as the D4RL ones do: ``get_params`` merges it
    and ``DIMS`` gives the dimensions ``run.py`` / ``mopo.from_config`` build the pool and MOPO from."""
    from mopo_amd.config import DIMS, get_params
    pkg = tmp_path / 'usercfg'
    pkg.mkdir()
    (pkg / '__init__.py').write_text('')
    (pkg / 'ant_mixed.py').write_text(
        "params = {'type': 'MOPO', 'universe': 'gym', 'domain': 'ant', 'task': 'medium-replay-v0',\n"
        "          'exp_name': 'ant_medium_replay', 'kwargs': {'rollout_length': 5, 'penalty_coeff': 1.0}}\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    p = get_params('usercfg.ant_mixed')
    assert DIMS[p['domain']] == (27, 8)
    assert p['kwargs']['rollout_length'] == 5 and p['kwargs']['network_kwargs']['hidden_sizes'] == [256, 256]


def _count(shapes):
    return sum(int(np.prod(s)) for s in shapes)


@pytest.mark.parametrize('hs', [[256, 256], [256, 128]])
def test_param_shapes_and_pad_index_at_ant_shape(hs):
    from mopo_amd.rollout import device_hidden, sac_pad_index, sac_param_shapes
    shapes = sac_param_shapes(O, A, hs)
    assert [tuple(s) for s in shapes] == [tuple(s) for s in osac.param_shapes(O, A, hs)]
    assert _count(shapes) == _count(osac.param_shapes(O, A, hs))
    assert shapes[8] == (O + A, hs[0]) and shapes[14] == (O + A, hs[0])
    hd, idx = device_hidden(hs), sac_pad_index(O, A, hs)
    assert hd == 256
    if hs[0] == hs[1]:
        assert idx is None
        return
    # the non-square embedding is a permutation into the padded square network: each tensor's corner
    dshapes = sac_param_shapes(O, A, hd)
    assert idx.size == _count(shapes) and len(np.unique(idx)) == idx.size
    assert idx.min() >= 0 and idx.max() < _count(dshapes)
    dev = np.zeros(_count(dshapes))
    logical = np.arange(1, idx.size + 1, dtype=np.float64)
    dev[idx] = logical
    off_l = off_d = 0
    for ls, ds in zip(shapes, dshapes):
        dt = dev[off_d:off_d + int(np.prod(ds))].reshape(ds)
        lt = logical[off_l:off_l + int(np.prod(ls))].reshape(ls)
        np.testing.assert_array_equal(dt[tuple(slice(0, n) for n in ls)], lt)
        assert dt.sum() == lt.sum()          # nothing outside the corner
        off_l += int(np.prod(ls))
        off_d += int(np.prod(ds))


def test_init_params_at_ant_shape_without_the_library_count():
    """init_sac_params on a non-square net (no C-ABI count to compare with) fills exactly the shapes' total."""
    from mopo_amd.rollout import init_sac_params, sac_param_shapes
    flat = init_sac_params(O, A, [256, 128], seed=3)
    assert flat.dtype == np.float32 and flat.size == _count(sac_param_shapes(O, A, [256, 128]))
