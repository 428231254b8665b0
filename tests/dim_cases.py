"""The observation / action block shapes of the ensemble forward and everything behind it, shared by
tests/test_dim_cases.py (CPU) and tests/test_gpu_dims.py (GPU).  A helper: no tests here.

The narrow forward forms are chosen by KG0 = ceil(IN / 16), NBO = ceil(2 D / 16) (D = obs_dim + 1) and
tail_steps(IN); ``SHAPES`` walks every value of each and the boundaries between them.  Which kernel form runs a
(shape, hidden, dtype) is the library's answer (``mopo_bnn_forward_form``, host only); nothing here restates it.

Parameters are ``oracle.bnn.init_params`` with the scaler fitted on spread inputs, plus what makes a misplaced
column, feature or unit visible in the outputs (tests/test_dim_cases.py measures that it does):
  * the members' biases spread (``BIAS_STD``, as tests/penalty_kinds.py),
  * ``max_logvar`` / ``min_logvar`` different in every column and close enough to the raw log-variance that each
    bound shapes the output (at the reference's 0.5 / -10 the lower bound moves nothing),
  * every weight matrix times ``FACTOR``.
"""
import ctypes
import functools

import numpy as np

from oracle import bnn as obnn

# (obs_dim, act_dim) -> what the shape is there for
SHAPES = {
    (3, 1): 'pendulum, D = 4',
    (7, 8): '2 D = 16, one full head block; IN = 15',
    (8, 1): 'smallest NBO = 2, D = 9',
    (11, 3): 'hopper',
    (15, 1): 'IN = 16 and 2 D = 32, both exactly full',
    (12, 6): 'KG0 = 2 with NBO = 2, tail 1',
    (15, 8): 'KG0 = 2 with NBO = 2, D = 16',
    (16, 1): 'IN = 17, smallest NBO = 3',
    (17, 6): 'the control',
    (20, 6): 'IN = 26, tail 3: the non-skipping H = 200 / 400 forms',
    (23, 8): 'IN = 31, 2 D = 48 full: the last narrow shape an actor can drive',
    (23, 9): 'IN = 32 exactly',
    (7, 12): 'KG0 = 2 with NBO = 1',
    (17, 16): 'wide by inputs alone',
}
# predict and FakeEnv.step only: the rollout's actor stops at act_dim 8
NO_ROLLOUT = ((23, 9), (7, 12), (17, 16))
ROLLOUT_SHAPES = tuple(s for s in SHAPES if s not in NO_ROLLOUT)

HIDDEN = (32, 64, 128, 200, 256, 400)            # the six hidden forms
HIDDEN_ALL_SHAPES = (64, 200)                    # every shape runs these two
ALL_HIDDEN_SHAPES = ((3, 1), (8, 1), (11, 3), (12, 6), (20, 6))   # these run all six
DTYPE_IDS = {'fp32': 0, 'bf16': 1, 'bf16x3': 2, 'bf16x6': 3, 'f16x3': 4}
MAIN_DTYPES = ('fp32', 'bf16x6', 'f16x3')
PLAIN_DTYPES = ('bf16', 'bf16x3')                # at PLAIN_SHAPES, on the widths they have
PLAIN_SHAPES = ((8, 1), (12, 6))
# |d| <= TOL (1 + |ref|) on mean and log-variance (tests/test_gpu_ref.py TOL)
TOL = {'fp32': 2e-5, 'bf16x6': 2e-5, 'f16x3': 2e-5, 'bf16x3': 2e-3, 'bf16': 3e-2}

E, ELITES = 2, [1, 0]
BATCHES = (1, 37)                                # 37: two full 16-row tiles and a 5-row one
BIAS_STD = 0.5
FACTOR = 2.5          # on every weight matrix; test_dim_cases.py (c): sensitivity >= 100 tol, f32 rounding <= 0.1 tol
SEEDS = {}            # (O, A, H) -> seed where the default fails test_dim_cases.py (c)

# one saturated-clamp case per head-block class (natural NBO 1, 2, 3 and the wide form's 4), at hidden 64
SATURATED_SHAPES = ((3, 1), (11, 3), (17, 6), (17, 16))
SAT_MARGIN = 15.0     # the raw log-variance lies at least this far outside the bound (softplus_fast's outer
                      # branches begin at 13.94)


def forward_form(O, A, H, dtype):
    """(KG0, hidden blocks, NBO, wide) of the kernel form that runs the shape, or None where none does."""
    from mopo_amd import _lib as L
    b = (ctypes.c_int * 4)()
    d = DTYPE_IDS[dtype] if isinstance(dtype, str) else int(dtype)
    return tuple(b) if L.lib().mopo_bnn_forward_form(int(O), int(A), int(H), d, b) == 1 else None


def shape_hiddens(shape):
    return HIDDEN if shape in ALL_HIDDEN_SHAPES else HIDDEN_ALL_SHAPES


@functools.lru_cache(None)
def predict_cases():
    """Every (O, A, H, dtype) of the table that the form function says a kernel runs."""
    out = []
    for (O, A) in SHAPES:
        for H in shape_hiddens((O, A)):
            for dt in MAIN_DTYPES + (PLAIN_DTYPES if (O, A) in PLAIN_SHAPES else ()):
                if forward_form(O, A, H, dt) is not None:
                    out.append((O, A, H, dt))
    return tuple(out)


def param_sets():
    """The (O, A, H) whose parameters the cases share across dtypes."""
    return tuple((O, A, H) for (O, A) in SHAPES for H in shape_hiddens((O, A)))


def case_id(c):
    return '-'.join(str(v) for v in c)


def _spread(lo, hi, D, rs):
    """D distinct values, evenly spaced over [lo, hi] in a random column order."""
    return rs.permutation(np.linspace(lo, hi, D)).astype(np.float32)[None, :]


@functools.lru_cache(None)
def case(O, A, H, saturated=False):
    """Parameters (oracle dict ``params``, ``mats``) and the 37 input rows ``x`` (f64; the f32 inputs are their
    cast, B = 1 the first row) of one (shape, hidden).  Never modified by a test."""
    seed = SEEDS.get((O, A, H), 7000 + 101 * O + 7 * A + H)
    rs = np.random.RandomState(seed)
    IN, D = O + A, O + 1
    fit = rs.normal(size=(400, IN)) * 1.5 + 0.2
    p = obnn.init_params(E, O, A, hidden=H, seed=seed + 1, inputs=fit, bias_std=BIAS_STD)
    p['W'] = [(w * np.float32(FACTOR)).astype(np.float32) for w in p['W']]
    p['Wv'] = (p['Wv'] * np.float32(FACTOR)).astype(np.float32)
    p['max_logvar'] = _spread(-0.5, 1.5, D, rs)
    p['min_logvar'] = _spread(-3.5, -1.5, D, rs)
    x = rs.normal(size=(max(BATCHES), IN)) * 1.5 + 0.2
    if saturated:
        # shift the log-variance head's bias per column: d % 3 == 0 above max_logvar, 1 below min_logvar, 2 as it was
        _, raw = raw_heads(p, x)
        bv = p['bv'].astype(np.float64).copy()
        for d in range(D):
            if d % 3 == 0:
                bv[:, 0, d] += p['max_logvar'][0, d] + SAT_MARGIN - raw[:, :, d].min(1)
            elif d % 3 == 1:
                bv[:, 0, d] += p['min_logvar'][0, d] - SAT_MARGIN - raw[:, :, d].max(1)
        p['bv'] = bv.astype(np.float32)
    return dict(params=p, mats=obnn.to_mat_list(p), x=x, seed=seed)


# ---- the oracle in stages (f64), for the sensitivity measurements -------------------------------------------
def hidden_acts(p, x):
    """The four hidden activations [E, B, H] of ``oracle.bnn.forward`` in f64, each stage as the oracle writes it."""
    f = np.float64
    h = (np.asarray(x, f) - p['mu'].astype(f)) / p['sigma'].astype(f)
    acts = []
    h = obnn.swish(np.einsum('ij,ajk->aik', h, p['W'][0].astype(f)) + p['b'][0].astype(f))
    acts.append(h)
    for l in range(1, obnn.N_HIDDEN):
        h = obnn.swish(np.matmul(h, p['W'][l].astype(f)) + p['b'][l].astype(f))
        acts.append(h)
    return acts


def heads_from(p, h, layer):
    """(mean, raw log-variance) from the activation ``h`` [E, rows, H] of hidden layer ``layer`` (1..4), f64."""
    f = np.float64
    for l in range(layer, obnn.N_HIDDEN):
        h = obnn.swish(np.matmul(h, p['W'][l].astype(f)) + p['b'][l].astype(f))
    mean = np.matmul(h, p['W'][obnn.N_HIDDEN].astype(f)) + p['b'][obnn.N_HIDDEN].astype(f)
    raw = np.matmul(h, p['Wv'].astype(f)) + p['bv'].astype(f)
    return mean, raw


def raw_heads(p, x):
    return heads_from(p, hidden_acts(p, x)[-1], obnn.N_HIDDEN)


def clamp(raw, maxlv, minlv):
    """bnn.py:669-670 in f64."""
    lv = maxlv - obnn.softplus(maxlv - raw)
    return minlv + obnn.softplus(lv - minlv)


def outputs(p, x):
    """The compared outputs in f64: (mean, log-variance) [E, B, D]."""
    return obnn.forward(p, x, dtype=np.float64, ret_log_var=True)


# ---- rollout cases --------------------------------------------------------------------------------------------
ROLLOUT_B, ROLLOUT_HORIZON, ROLLOUT_E = 100, 3, 7
# (domain, O, A, H) -> seed where the default leaves a row within 2 TERM_MARGIN of a bound or the batch does not
# compact at both steps (found by walking up from the default; test_dim_cases.py (d) holds every case to TERM_MARGIN)
ROLLOUT_SEEDS = {('walker2d', 3, 1, 64): 402, ('walker2d', 3, 1, 200): 535, ('walker2d', 8, 1, 200): 591,
                 ('walker2d', 11, 3, 200): 627, ('walker2d', 15, 1, 64): 531, ('walker2d', 15, 1, 200): 667,
                 ('walker2d', 12, 6, 200): 639, ('walker2d', 15, 8, 64): 540, ('walker2d', 16, 1, 64): 542,
                 ('walker2d', 20, 6, 64): 591, ('walker2d', 20, 6, 200): 727, ('walker2d', 23, 8, 64): 626}
TERM_MARGIN = 1e-3


def rollout_cases():
    """(domain, O, A, H, dtype): every actor-driven shape at hidden 64 and 200 in fp32 and f16x3 under walker2d's
    rule (rows terminate, the batch compacts), halfcheetah once, and the two 16-bit shapes that used to have no
    kernel at hidden 32."""
    out = [('walker2d', O, A, H, dt) for (O, A) in ROLLOUT_SHAPES for H in HIDDEN_ALL_SHAPES for dt in ('fp32', 'f16x3')]
    out.append(('halfcheetah', 12, 6, 64, 'fp32'))
    out += [('walker2d', 11, 3, 32, 'f16x3'), ('walker2d', 8, 1, 32, 'f16x3')]
    return out


def rollout_seed(domain, O, A, H):
    return ROLLOUT_SEEDS.get((domain, O, A, H), 300 + 11 * O + A + H)


_ROLLOUTS = {}


def rollout_case(domain, O, A, H):
    """tests/test_gpu_rollout.py's oracle rollout at this shape, computed once (the dtypes share it)."""
    from test_gpu_rollout import _rollout_case
    key = (domain, O, A, H)
    if key not in _ROLLOUTS:
        _ROLLOUTS[key] = _rollout_case(domain, ROLLOUT_E, H, ROLLOUT_B, ROLLOUT_HORIZON, rollout_seed(*key), O=O, A=A)
    return _ROLLOUTS[key]


def term_distance(domain, next_obs):
    """Per row, the distance of the deciding quantities of the termination rule to its nearest bound."""
    if domain == 'walker2d':
        h, a = next_obs[:, 0], next_obs[:, 1]
        return np.minimum(np.abs(h[:, None] - np.array([0.8, 2.0])).min(1), np.abs(a[:, None] - np.array([-1.0, 1.0])).min(1))
    return np.full(len(next_obs), np.inf)
