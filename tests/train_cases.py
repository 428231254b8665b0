"""The ensemble training step's parity cases, shared by tests/test_train_cases.py (CPU: every case is well
conditioned, fp32 against fp64 oracle) and tests/test_gpu_train_forms.py (GPU: csrc/bnn_train.hip against the
fp64 oracle).  A plain module: no fixtures, no GPU, nothing but numpy and the oracle.

A case names the path its shape must take (``form``: the <G0, GH, GD> of train_rows_kernel, or None for the
generic grouped-GEMM step) so that a test can ask mopo_bnn_train_step_form whether it did.

Minibatch geometries, the smallest that still reach every launch path of mopo_bnn_train_epoch:
  short   batch 24 (1.5 row blocks) over 79 rows: 3 full minibatches (the 2-step graph, then the 1-step graph
          with copy_back), the staged gather, and an eager partial minibatch of 7 rows (one partial row block);
  long    batch 40 over 473 rows: 11 full minibatches (the 8-step graph, then 2, then 1) and a partial
          minibatch of 33 rows (two full row blocks plus one row);
  single  batch 1 over 5 rows: single-row minibatches, all of them full.
"""
import collections

import numpy as np

from oracle import bnn as obnn
from oracle import bnn_train as ot

GEOMETRY = {'short': (79, 24), 'long': (473, 40), 'single': (5, 1)}   # name -> (rows, batch)
NAMES = ['W0', 'b0', 'W1', 'b1', 'W2', 'b2', 'W3', 'b3', 'Wm', 'bm', 'Wv', 'bv', 'maxlv', 'minlv']
# the project's tolerance for several Adam steps, fp32 device against the fp64 oracle
# (test_gpu_train.test_epoch_matches_oracle_steps): rtol, and atol = ATOL * max(1, max|ref|) per variable
RTOL, ATOL = 2e-5, 2e-5

# group: the issue's section (a row forms, b partial last hidden block, c member counts, d generic path,
# e single-row minibatches); shuffle: epoch k + 1 runs on epoch k's indices reordered by np.argsort of fresh
# uniform keys (BNN.train's shuffle_rows) instead of fresh bootstrap indices; seed: the data seed
Case = collections.namedtuple('Case', 'group E o a H geometry form epochs shuffle seed')


def _c(group, E, o, a, H, geometry, form, epochs=1, shuffle=False, seed=1):
    return Case(group, E, o, a, H, geometry, form, epochs, shuffle, seed)


CASES = [
    # a. every row form the five older shapes leave out, and both geometries
    _c('a', 3, 11, 3, 200, 'short', (1, 13, 2)),
    _c('a', 3, 17, 6, 32, 'short', (2, 2, 3)),
    _c('a', 3, 17, 6, 256, 'short', (2, 16, 3)),
    _c('a', 3, 11, 3, 256, 'short', (1, 16, 2)),
    _c('a', 3, 11, 3, 128, 'short', (1, 8, 2)),
    _c('a', 3, 27, 8, 200, 'short', (3, 13, 4)),
    _c('a', 7, 17, 6, 256, 'long', (2, 16, 3)),
    _c('a', 7, 11, 3, 200, 'long', (1, 13, 2)),
    _c('a', 3, 27, 8, 64, 'long', (3, 4, 4)),
    # b. a partial last hidden block of 4, 8 or 12 units (and 13 full blocks: H = 208)
    _c('b', 3, 17, 6, 196, 'short', (2, 13, 3)),
    _c('b', 3, 17, 6, 204, 'short', (2, 13, 3)),
    _c('b', 3, 17, 6, 208, 'short', (2, 13, 3)),
    _c('b', 3, 17, 6, 116, 'short', (2, 8, 3)),
    _c('b', 3, 17, 6, 244, 'short', (2, 16, 3)),
    _c('b', 3, 11, 3, 20, 'short', (1, 2, 2)),
    _c('b', 3, 11, 3, 28, 'short', (1, 2, 2)),
    _c('b', 3, 27, 8, 52, 'short', (3, 4, 4)),
    _c('b', 3, 27, 8, 196, 'short', (3, 13, 4)),
    # c. member counts: one workgroup tier (1, 8), a second tier with ids past E (9), the limit (16)
    _c('c', 1, 11, 3, 32, 'short', (1, 2, 2)),
    _c('c', 8, 11, 3, 32, 'short', (1, 2, 2)),
    _c('c', 9, 11, 3, 32, 'short', (1, 2, 2)),
    _c('c', 16, 11, 3, 32, 'short', (1, 2, 2), epochs=2, shuffle=True),
    _c('c', 9, 17, 6, 200, 'long', (2, 13, 3)),
    # d. the generic path: no row form at this width, odd D, H % 4 != 0, tiny, K > 256
    _c('d', 3, 11, 3, 64, 'short', None),
    _c('d', 3, 10, 3, 32, 'short', None),
    _c('d', 3, 10, 3, 50, 'short', None),
    _c('d', 3, 11, 3, 30, 'short', None),
    _c('d', 2, 3, 1, 8, 'short', None),
    _c('d', 2, 17, 6, 400, 'short', None),
    # ... and with more than 8 members: a backward launch holds two problems per member, a grouped-GEMM launch
    # at most 16 (gemm_group.h MAXP), so step_impl deals them over several launches (16 + 2, 16 + 16)
    _c('d', 9, 10, 3, 32, 'short', None),
    _c('d', 16, 11, 3, 64, 'short', None),
    # e. single-row minibatches
    _c('e', 3, 11, 3, 32, 'single', (1, 2, 2), epochs=2),
]


def case_id(c):
    return '%s-E%d-%d+%d-H%d-%s' % (c.group, c.E, c.o, c.a, c.H, c.geometry)


def form_name(form):
    return 'generic' if form is None else '<%d,%d,%d>' % tuple(form)


def make_data(n, o, a, seed=1):
    """tests/test_gpu_train.py data(): unit-normal inputs, targets a noisy linear map of the observations."""
    rs = np.random.RandomState(seed)
    X = rs.normal(size=(n, o + a)).astype(np.float32)
    Y = np.concatenate([X[:, :1] * 0.3 + 0.1 * rs.normal(size=(n, 1)), 0.2 * X[:, :o] + 0.05 * rs.normal(size=(n, o))],
                       1).astype(np.float32)
    return X, Y


def make_mats(E, o, a, H, X):
    """The 16 .mat arrays of a fresh ensemble whose scaler is fitted on X, with test_gpu_train.model()'s
    changes: biases 0.1 * normal (so the bias paths carry weight), max log-var 0.5, min log-var -3."""
    mats = obnn.to_mat_list(obnn.init_params(E, o, a, hidden=H, seed=3, inputs=X))
    rs = np.random.RandomState(103)
    for i in range(3, 14, 2):
        mats[i] = (rs.normal(size=mats[i].shape) * 0.1).astype(np.float32)
    mats[14] = np.full_like(mats[14], 0.5)
    mats[15] = np.full_like(mats[15], -3.0)
    return [np.ascontiguousarray(m, np.float32) for m in mats]


def case_epochs(c):
    """[(idxs [E, rows] int, keys or None)] per epoch, from RandomState(7): bootstrap indices, and for a
    shuffle case the float64 keys whose argsort turned the previous epoch's indices into this one's."""
    n = GEOMETRY[c.geometry][0]
    rs = np.random.RandomState(7)
    out = []
    for ep in range(c.epochs):
        if ep and c.shuffle:
            keys = rs.uniform(size=[c.E, n])
            idxs = out[-1][0][np.arange(c.E)[:, None], np.argsort(keys, axis=-1)]
            out.append((idxs, keys))
        else:
            out.append((rs.randint(n, size=[c.E, n]), None))
    return out


def case_inputs(c):
    """(mats, X, Y, idxs_per_epoch) of a case; the minibatches are idxs[:, b * batch:(b + 1) * batch]."""
    n = GEOMETRY[c.geometry][0]
    X, Y = make_data(n, c.o, c.a, c.seed)
    return make_mats(c.E, c.o, c.a, c.H, X), X, Y, [ix for ix, _ in case_epochs(c)]


def oracle_steps(mats, X, Y, idxs_per_epoch, batch, dtype=np.float64):
    """The 14 optimised variables after every minibatch of every epoch, stepped by oracle/bnn_train.py."""
    p = obnn.from_mat_list([np.asarray(m, np.float64) for m in mats], smv=True)
    st = ot.TrainState(p, dtype=dtype)
    for idxs in idxs_per_epoch:
        for b in range(int(np.ceil(idxs.shape[1] / batch))):
            bi = idxs[:, b * batch:(b + 1) * batch]
            st.step(X[bi].astype(dtype), Y[bi].astype(dtype), dtype)
    return st.vals


def tol_ratio(got, ref):
    """Worst |got - ref| / tol over a variable's elements, tol = RTOL |ref| + ATOL max(1, max|ref|)."""
    ref = np.asarray(ref, np.float64).reshape(np.shape(got))
    tol = RTOL * np.abs(ref) + ATOL * max(1.0, np.abs(ref).max())
    return float((np.abs(np.asarray(got, np.float64) - ref) / tol).max())


# ---- the loss log (mopo_bnn_train_logs): a row form with a partial block, a generic shape, two workgroup tiers
LOSS_CASES = [(3, 17, 6, 196, (2, 13, 3)), (3, 10, 3, 32, None), (9, 11, 3, 32, (1, 2, 2))]
LOSS_ROWS = 17   # one eager minibatch of a batch-24 trainer: a full row block and one row


def loss_inputs(E, o, a, H):
    """(mats, X, Y, idx [E, LOSS_ROWS]) of a loss-log case: the short geometry's data, one partial minibatch."""
    n = GEOMETRY['short'][0]
    X, Y = make_data(n, o, a)
    return make_mats(E, o, a, H, X), X, Y, np.random.RandomState(7).randint(n, size=[E, LOSS_ROWS])


def data_loss(p, X, Y, dtype=np.float64):
    """The data term of the train loss (bnn.py:241-249) on parameters p and per-member rows X, Y [E, B, .]:
    sum over members of mean(err^2 exp(-lv)) + mean(lv) -- no decays, no 0.01 log-var bound terms."""
    _, mean, lv = ot.forward3d(p, X, dtype)
    err = mean - Y.astype(dtype)
    return float(np.sum(np.mean(err * err * np.exp(-lv), axis=(1, 2)) + np.mean(lv, axis=(1, 2))))
