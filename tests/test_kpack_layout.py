"""CPU: the packed remainder k-group of the bf16x6 ring kernel (mlp_tile.h kpack_slot) restated in numpy.

At H = 197..200 a lane holds 2 real values k = 0, 1 in the last 32-deep k-group of a hidden-width input.  The six
products x_p w_q, p + q < 3, of both values are 12 element slots: slots 0..7 are the 8 elements of one 32-deep
MFMA, slots 8..11 the low 4 elements of a second one (its upper 4 meet zeros), both against one weight fragment of
four dwords {w0, w1, w2, w0} (a dword = the part's bf16 pair of k = 0, 1); the second MFMA meets dwords 0, 1.
The sum over the 12 slots must equal the six-product sum of the split restated in tests/test_split.py.
"""
import numpy as np

from test_gpu_kpack import REM, head_input, isolated_case
from test_split import split3

# per operand dword (0..3: the first MFMA, 4..5: the second one's low half): activation part, weight part
XP = (0, 0, 0, 1, 2, 1)
WP = (0, 1, 2, 0, 0, 1)
SLOTS = [(i & 1, XP[i >> 1], WP[i >> 1]) for i in range(12)]    # (k, x part, w part) of element slot i


def test_every_kept_pair_once_per_k():
    kept = sorted((p, q) for p in range(3) for q in range(3) if p + q < 3)
    for k in (0, 1):
        assert sorted((xp, wp) for kk, xp, wp in SLOTS if kk == k) == kept
    # dword d holds k = 0 in its low half, k = 1 in its high half, of one (x part, w part) pair
    for d in range(6):
        assert SLOTS[2 * d][0] == 0 and SLOTS[2 * d + 1][0] == 1 and SLOTS[2 * d][1:] == SLOTS[2 * d + 1][1:]


def test_one_fragment_feeds_both_mfmas():
    """The weight fragment is {w0, w1, w2, w0}; the second MFMA's live weight dwords are its dwords 0, 1."""
    assert WP[:4] == (0, 1, 2, 0)
    assert WP[4:] == WP[:2]
    # and the activation operands: {x0, x0, x0, x1} and {x2, x1}
    assert XP[:4] == (0, 0, 0, 1) and XP[4:] == (2, 1)


def test_slot_sum_equals_six_products():
    rs = np.random.RandomState(7)
    n = 50000
    x = (rs.normal(size=(n, 2)) * np.exp2(rs.randint(-20, 20, (n, 2)))).astype(np.float32)
    w = (rs.normal(size=(n, 2)) * np.exp2(rs.randint(-20, 20, (n, 2)))).astype(np.float32)
    xp = [a.astype(np.float64) for a in split3(x)[:3]]
    wp = [a.astype(np.float64) for a in split3(w)[:3]]
    # the fragment and the two activation operands, element by element (slot i = dword i // 2, half i % 2)
    frag = np.stack([wp[WP[i >> 1]][:, i & 1] for i in range(8)], 1)
    b_full = np.stack([xp[XP[i >> 1]][:, i & 1] for i in range(8)], 1)
    b_half = np.stack([xp[XP[4 + (i >> 1)]][:, i & 1] for i in range(4)], 1)
    packed = (frag * b_full).sum(1) + (frag[:, :4] * b_half).sum(1)
    six = sum(xp[p][:, k] * wp[q][:, k] for k in (0, 1) for p in range(3) for q in range(3) if p + q < 3)
    # the same 12 exact products (each 8 x 8 significand bits); in f64 the two sums differ by f64 rounding only
    assert np.all(np.abs(packed - six) <= 2.0 ** -48 * np.abs(x.astype(np.float64) * w).sum(1))
    # against the unsplit product: the dropped x1 w2 + x2 w1 + x2 w2 (tests/test_split.py's bound)
    exact = (x.astype(np.float64) * w.astype(np.float64)).sum(1)
    assert np.all(np.abs(packed - exact) <= (2.0 ** -23 + 2.0 ** -32) * np.abs(x.astype(np.float64) * w).sum(1))


def test_isolated_remainder_case_can_fail():
    """CPU part of the isolated-remainder case: its outputs are not ~0, and one second-order product (x1 w1)
    missing from the head's remainder alone would exceed twice the criterion's 2e-6 floor."""
    mats, x, rm, rv = isolated_case(True)
    assert np.median(np.abs(rm)) > 0.1 and np.ptp(np.log(rv)) > 0.1
    h, p = head_input(mats, x)
    x1 = split3(h[:, :, REM].astype(np.float32))[1].astype(np.float64)
    w1 = split3(p['W'][4][:, REM, :])[1].astype(np.float64)
    dropped = np.matmul(x1, w1)
    err = float(np.max(np.abs(dropped) / (1 + np.abs(rm))))
    print('x1 w1 of the head remainder: %.3g' % err)
    assert err > 4e-6
