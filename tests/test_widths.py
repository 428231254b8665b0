"""CPU: the hidden-width rules of the ensemble and the rollout actor, and the zero embedding behind them.

  * ``mopo_bnn_device_hidden`` / ``mopo_actor_device_hidden`` (host-only C functions: the library states the
    rule, nothing here restates it): monotone, >= the request, the identity on every width that ran before the
    8- and 16-block forms existed, -1 past the limits;
  * ``embed_hidden`` / ``extract_hidden`` (the embedding the device packer applies, stated on the .mat layout)
    round-trip and pad only with zeros, and ``slot_feat`` (csrc/mlp_tile.h, what the packer really walks) lays a
    logical width into a wider form with every unit once and -1 (zero) in every other slot;
  * exactness in the oracle: the forward on zero-embedded parameters equals the forward on the logical ones bit
    for bit (in a fixed summation order; f64 through BLAS to its reassociation), and one training step leaves
    every padded entry exactly 0 and the rest equal;
  * the oracle against the reference's own ``_compile_outputs`` at H = 128, 256, 100 (17 + 6) and 128 (27 + 8)
    (tests/golden/make_widths.py), at test_oracle_ref.py's 1e-10 relative.
"""
import glob
import hashlib
import os

import numpy as np
import pytest

from mopo_amd import _lib
from mopo_amd.bnn import _hidden_axes, embed_hidden, extract_hidden
from oracle import bnn as obnn
from oracle import bnn_train as obt
from test_oracle_ref import load_case, rel, scaled
from test_wide_oracle import slot_maps  # noqa: F401  (fixture: slot_feat compiled as mlp_tile.h states it)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FWD = sorted(glob.glob(os.path.join(GOLD, 'widths_fwd_*.npz')))
FP32, BF16, BF16X3, BF16X6, F16X3 = range(5)


# ---- 1. width rules ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [FP32, BF16X6, F16X3])
@pytest.mark.parametrize('wide', [0, 1])
def test_bnn_device_hidden_rule(dtype, wide):
    f = _lib.lib().mopo_bnn_device_hidden
    top = 256 if not wide or dtype == FP32 else 208
    got = [f(h, dtype, wide) for h in range(1, top + 1)]
    assert all(g >= h for h, g in zip(range(1, top + 1), got))               # >= the request (so never -1)
    assert all(a <= b for a, b in zip(got, got[1:]))                          # monotone
    for h in [32, 64] + list(range(193, 209)):                                # what ran before: itself
        assert f(h, dtype, wide) == h
    assert f(100, dtype, wide) == 128 and f(128, dtype, wide) == 128 and f(70, dtype, wide) == 128
    if top == 256:
        assert f(220, dtype, wide) == 256 and f(256, dtype, wide) == 256 and f(209, dtype, wide) == 256
    else:
        assert f(209, dtype, wide) == -1 and f(256, dtype, wide) == -1       # wide 16-bit stops at 208
    # past the limits: 257..384 and above 400 (416: the 16-bit kernels' 26 whole blocks)
    assert all(f(h, dtype, wide) == -1 for h in (257, 300, 384, 417, 1000, 0, -5))
    want400 = 400 if (dtype == FP32 or (dtype == F16X3 and not wide)) else -1
    assert f(400, dtype, wide) == want400 and f(385, dtype, wide) == (385 if want400 > 0 else -1)


def test_bnn_device_hidden_plain_bf16_keeps_its_widths():
    """bf16 and bf16x3 get no new form: the widths they ran stay, everything else is refused (-1)."""
    f = _lib.lib().mopo_bnn_device_hidden
    for dtype in (BF16, BF16X3):
        for h in (16, 32, 48, 64, 200, 208, 400):
            assert f(h, dtype, 0) == h
        for h in (65, 100, 128, 192, 209, 256, 300):
            assert f(h, dtype, 0) == -1
        assert all(f(h, dtype, 1) == -1 for h in (32, 64, 128, 200))        # never on a wide model
    assert f(64, 5, 0) == -1 and f(64, -1, 0) == -1                           # not a dtype


def test_actor_device_hidden_rule():
    g = _lib.lib().mopo_actor_device_hidden
    for dtype in (FP32, BF16X6, F16X3):
        got = [g(h, dtype) for h in range(1, 257)]
        assert all(k >= h for h, k in zip(range(1, 257), got))
        assert all(a <= b for a, b in zip(got, got[1:]))
        assert g(32, dtype) == 32 and g(256, dtype) == 256
        assert all(k % 32 == 0 for k in got)                                  # 32-deep k-groups
        for h in range(16, 257, 16):                                          # every width mopo_sac_create takes
            assert 0 <= g(h, dtype) - h < 32
        assert g(257, dtype) == -1 and g(0, dtype) == -1 and g(512, dtype) == -1
    assert g(64, BF16) == -1 and g(64, BF16X3) == -1                          # no such actor form


# ---- 2. the embedding ----------------------------------------------------------------------------------------
def _mats(E, O, A, H, smv, seed):
    rs = np.random.RandomState(seed)
    p = obnn.init_params(E, O, A, hidden=H, seed=seed, smv=smv, inputs=rs.normal(size=(200, O + A)) * 1.5 + 0.2)
    return p, obnn.to_mat_list(p)


@pytest.mark.parametrize('H,Hd,smv', [(100, 128, True), (220, 256, False), (70, 128, False), (128, 128, True)])
def test_embedding_round_trips_and_pads_with_zeros(H, Hd, smv):
    _, mats = _mats(3, 17, 6, H, smv, 5)
    big = embed_hidden(mats, Hd)
    back = extract_hidden(big, H)
    assert len(big) == len(mats) == (16 if smv else 14)
    for a, b in zip(mats, back):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    hidden = dict()
    for i, ax in _hidden_axes(len(mats)):
        hidden.setdefault(i, []).append(ax)
    for i, (a, b) in enumerate(zip(mats, big)):
        want = tuple(Hd if ax in hidden.get(i, []) else n for ax, n in enumerate(a.shape))
        assert b.shape == want
        mask = np.ones(b.shape, bool)
        mask[tuple(slice(0, n) for n in a.shape)] = False
        assert not b[mask].any()                                              # only zeros were added
        assert int(mask.sum()) == b.size - a.size
    with pytest.raises(ValueError):
        embed_hidden(mats, H - 1)


@pytest.mark.parametrize('H,blocks', [(100, 8), (70, 8), (113, 8), (220, 16), (241, 16), (150, 13), (40, 4), (5, 2)])
def test_slot_feat_embeds_a_logical_width_in_a_wider_form(slot_maps, H, blocks):  # noqa: F811
    """What the device packer walks: over the form's 16 * blocks slots every logical unit appears exactly once and
    every other slot is -1, which the packers turn into zero weights and biases."""
    got = [slot_maps.slot_feat(s, H) for s in range(16 * blocks)]
    assert sorted(k for k in got if k >= 0) == list(range(H))
    assert all(k == -1 for k in got if k < 0)
    assert all(k == -1 for k in got[16 * ((H + 15) // 16):])                  # whole spare blocks: padding only


# ---- 3. exactness in the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize('H,Hd,smv', [(100, 128, True), (100, 128, False), (220, 256, True), (220, 256, False)])
def test_oracle_forward_on_embedded_params_is_bit_equal(H, Hd, smv):
    E, O, A = 3, 17, 6
    p, mats = _mats(E, O, A, H, smv, 11)
    q = obnn.from_mat_list(embed_hidden(mats, Hd), smv=smv)
    rs = np.random.RandomState(1)
    x = rs.normal(size=(33, O + A)) * 1.5 + 0.2
    x[0] = 0.0
    x[1] = 40.0
    # Bit equality needs a fixed summation order.  numpy's f64 matmul goes through BLAS, whose blocking (and so
    # the order in which the SAME nonzero terms are added) depends on the matrix sizes: at 100 -> 128 it moved
    # results by up to 3e-13 relative on this host, at 220 -> 256 by nothing.  The same oracle code in
    # np.longdouble runs numpy's own k-sequential loops (no BLAS): there the padded terms are the only
    # difference, they are exact zeros, and the outputs must be equal bit for bit -- at more than f64 precision.
    m0, lv0 = obnn.forward(p, x, dtype=np.longdouble, ret_log_var=True)
    m1, lv1 = obnn.forward(q, x, dtype=np.longdouble, ret_log_var=True)
    assert m0.dtype == np.longdouble and np.finfo(np.longdouble).eps <= np.finfo(np.float64).eps
    assert np.array_equal(m0, m1) and np.array_equal(lv0, lv1)
    # f64 through BLAS: equal up to its reassociation of at most 256 terms per dot product over 5 layers,
    # 5 * 256 * 2^-53 ~ 1.4e-13 of the sum of the terms' magnitudes (a few units here)
    f0, flv0 = obnn.forward(p, x, dtype=np.float64, ret_log_var=True)
    f1, flv1 = obnn.forward(q, x, dtype=np.float64, ret_log_var=True)
    assert scaled(f1, f0) < 1e-12 and scaled(flv1, flv0) < 1e-12
    assert scaled(f0, m0.astype(np.float64)) < 1e-12


@pytest.mark.parametrize('H,Hd,smv', [(100, 128, True), (220, 256, False)])
def test_oracle_training_step_keeps_padding_zero(H, Hd, smv):
    """One Adam step (loss, decays, update) on embedded parameters: every padded entry stays exactly 0 -- the
    outgoing gradient is 0 * delta, the incoming delta is zero because the next layer's rows are zero -- and the
    logical entries get the logical network's update."""
    E, O, A, B = 2, 11, 3, 24
    p, mats = _mats(E, O, A, H, smv, 13)
    q = obnn.from_mat_list(embed_hidden(mats, Hd), smv=smv)
    rs = np.random.RandomState(2)
    X = rs.normal(size=(E, B, O + A)) * 1.5 + 0.2
    Y = rs.normal(size=(E, B, O + 1))
    # np.longdouble: numpy's own k-sequential loops, the fixed summation order bit equality needs (see the forward
    # test above); np.float64: through BLAS, the logical entries equal to its reassociation, the padding still 0
    for dt, exact in ((np.longdouble, True), (np.float64, False)):
        sp, sq = obt.TrainState(p, dtype=dt), obt.TrainState(q, dtype=dt)
        lp, lq = sp.step(X, Y, dt), sq.step(X, Y, dt)
        assert lp == lq if exact else abs(lp - lq) <= 1e-12 * (1 + abs(lp))
        vp, vq = sp.vals, sq.vals                                              # the optvars after the step
        assert len(vp) == len(vq)
        padded = 0
        for a0, a, b in zip(obt.optvars(p), vp, vq):
            core = b[tuple(slice(0, n) for n in a.shape)]
            assert np.array_equal(core, a) if exact else scaled(core, np.asarray(a, np.float64)) < 1e-12
            if a.shape[0] == E:
                assert not np.array_equal(np.asarray(a, np.float64), a0)       # the step moved the logical entries
            mask = np.ones(b.shape, bool)
            mask[tuple(slice(0, n) for n in a.shape)] = False
            assert not b[mask].any()                                           # exactly 0, in either arithmetic
            padded += int(mask.sum())
        assert padded > 0


# ---- 4. the oracle against the reference at the new widths ------------------------------------------------------
def _fixture_params(z):
    E, H, O, A, smv, seed = (int(z[k]) for k in ('E', 'H', 'O', 'A', 'smv', 'seed'))
    rs = np.random.RandomState(seed + 100)
    fit = rs.normal(size=(400, O + A)) * 1.5 + 0.2
    p = obnn.init_params(E, O, A, hidden=H, seed=seed, smv=bool(smv), inputs=fit)
    h = hashlib.sha256()
    for a in obnn.to_mat_list(p):
        h.update(np.ascontiguousarray(a, np.float32).tobytes())
    assert h.hexdigest() == str(z['weights_sha']), 'regenerated weights differ from the reference case'
    return p


def test_widths_fixture_set():
    got = sorted((int(z['H']), int(z['O']), int(z['A']), int(z['B'])) for z in map(load_case, FWD))
    assert got == [(100, 17, 6, 64), (128, 17, 6, 64), (128, 27, 8, 64), (256, 17, 6, 64)]
    for path in FWD:
        assert os.path.getsize(path) < 1 << 20


@pytest.mark.parametrize('path', FWD, ids=[os.path.basename(p) for p in FWD])
def test_widths_forward_oracle_vs_reference_graph(path):
    z = load_case(path)
    assert not z['x'][0].any() and np.all(np.abs(z['x'][1]) == 40.0) and np.all(z['x'][2] == -z['x'][1])
    p = _fixture_params(z)
    m64, v64 = obnn.forward(p, z['x'], dtype=np.float64)
    _, lv64 = obnn.forward(p, z['x'], dtype=np.float64, ret_log_var=True)
    assert rel(m64, z['mean_f64']) < 1e-10 or scaled(m64, z['mean_f64']) < 1e-13
    assert rel(v64, z['var_f64']) < 1e-10
    assert rel(lv64, z['logvar_f64']) < 1e-10 or scaled(lv64, z['logvar_f64']) < 1e-13
    # the reference's own f32 execution sits at f32 rounding of the f64 one
    assert scaled(z['mean_f32'], z['mean_f64']) < 2e-5 and scaled(z['logvar_f32'], z['logvar_f64']) < 2e-5
