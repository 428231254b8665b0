"""The SAC update's shape cases, shared by tests/test_sac_cases.py (CPU: the table holds what it promises and
every case is well conditioned, fp32 oracle against fp64 oracle) and tests/test_gpu_sac_shapes.py (GPU:
csrc/sac.hip against the fp64 oracle).  A plain module: no fixtures, no GPU, nothing but numpy and the oracle.

``mopo_sac_create`` takes any hidden width that is a multiple of 16 up to 256, any batch in [1, 1024],
obs_dim <= 31, act_dim <= 8 and any n_env in [0, batch].  The groups:
  A  every device width once (16 .. 256, and three [H1, H2] networks that run zero-padded), one injected step;
  B  the weight-gradient launch's K passes (sac_wgrad.h stages the batch in chunks of 256 rows: 1 .. 4 passes,
     full and partial last chunks) and row-block counts past 16 and past 32, one injected step;
  C  the pool split: n_env = 0 and n_env = n (the unused pool is one row of NaN), n_env = 1, an even split;
     perf mode (device Philox batches and noise), 3 steps;
  D  perf-mode steps under graph replay against the oracle run on the restated streams (oracle/rng.py),
     among them the shapes with a single B1 block (H <= 64 and batch <= 16), whose prefetch is its own launch;
  E  the launch forms (MOPO_SAC_FUSE 0 / 1 / 2, graph replay against eager steps): bit-identity, no oracle;
  F  refusals (REFUSALS below);
  G  saturated policy heads (``Case.head``, HEAD_MODES): the log-std clip's clamped branches and its gradient
     mask, which no other group reaches (their raw log-std lies in [-1.97, 1.90]).  Injected steps, one
     perf-mode case, and a copy of that in group E.  Where a raw log-std is below the lower bound the
     injected noise is exactly 0: std = e^-20 is below EPS and below half an ulp of mu, so with noise
     u - mu is 0 or +-1 ulp in f32 and zz / (std + EPS) amplifies that by 1e8 in the oracle as in any kernel.

The tolerances are the project's own (tests/test_gpu_sac.py's docstring and its non-square perf-mode test);
the *_ratio functions express a comparison in units of its tolerance, so that 1.0 is the GPU bound and the
CPU conditioning test can ask for CONDITION of it.
"""
import collections
import contextlib
import functools

import numpy as np

from oracle import rng as orng
from oracle import sac as osac

LR, LOG_ALPHA, TARGET_ENTROPY = 3e-4, 0.1, -3.0
LR_T = LR * np.sqrt(1 - 0.999) / (1 - 0.9)     # TF1 Adam's first step size
ENV_ROWS, MODEL_ROWS = 300, 900
PERF_SEED = 77                                 # the device seed of the perf-mode groups (the Philox key)
WG_KC = 256                                    # sac_wgrad.h: batch rows staged per pass of a weight-gradient tile
GRAD_NAMES = ['pi.W1', 'pi.b1', 'pi.W2', 'pi.b2', 'pi.Wm', 'pi.bm', 'pi.Wl', 'pi.bl'] + \
    ['%s.%s' % (q, t) for q in ('q1', 'q2') for t in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3')]
LOG_PAIRS = [(k, k) for k in ('Q/q1_loss', 'sac_Q/q2_loss', 'sac_Q/q1', 'sac_Q/q2', 'sac_pi/alpha', 'sac_pi/pi_entropy',
                              'sac_pi/logp_pi', 'sac_pi/pi_global_norm', 'sac_Q/q_global_norm')] + \
    [('policy_loss', 'pi_loss')]               # (device key, oracle key)
LOSS_PAIRS = [('Q/q1_loss', 'Q/q1_loss'), ('sac_Q/q2_loss', 'sac_Q/q2_loss'), ('policy_loss', 'pi_loss')]

# seed: the data seed (pools, parameters, injected rows and noise); steps: perf-mode steps (0: one injected step)
# head: how the log-std head is saturated ('' : as initialised; HEAD_MODES)
Case = collections.namedtuple('Case', 'group o a hidden n n_env seed prior steps head')

# The log-std head's columns by class: +1 above the upper bound on every row (bl += HEAD_UP), -1 below the lower
# one (bl -= HEAD_DOWN), 0 inside as initialised.  'cross' shifts no whole column: cross_head() makes column
# CROSS_COL lie above the bound on some rows and inside on the others.
HEAD_MODES = {
    'upper': lambda j: 1 + 0 * j,
    'lower': lambda j: -1 + 0 * j,
    'mixed': lambda j: np.where(j % 3 == 0, 1, np.where(j % 3 == 1, -1, 0)),   # dim_cases.SATURATED_SHAPES' scheme
    'even': lambda j: np.where(j % 2 == 0, 1, 0),
    'cross': lambda j: 0 * j,
}
HEAD_UP, HEAD_DOWN = 6.0, 26.0
CROSS_COL = 4                                  # of the six, the column whose raw value separates the clusters best
CLIP_MARGIN = 0.5                              # every raw log-std of a G case lies this far from both bounds
INSIDE = 2.0                                   # 'cross': the rows that stay inside stay above -INSIDE


def _c(group, o, a, hidden, n, n_env=None, seed=0, prior='uniform', steps=0, head=''):
    return Case(group, o, a, hidden, n, int(n * 0.05) if n_env is None else n_env, seed, prior, steps, head)


CASES = [
    # A. every device width once; (o, a, n) mixed so that each edge appears
    _c('A', 1, 1, 16, 1),
    _c('A', 31, 8, 32, 16),            # wide layer-1 form (o + a > 31)
    _c('A', 11, 3, 48, 17),
    _c('A', 17, 6, 64, 15),
    _c('A', 11, 3, 80, 100),
    _c('A', 27, 8, 96, 40),            # wide
    _c('A', 17, 6, 112, 33),
    _c('A', 8, 8, 128, 64),
    _c('A', 17, 6, 144, 257),
    _c('A', 31, 1, 160, 48),           # o + a = 32: the first wide width
    _c('A', 11, 3, 176, 31),
    _c('A', 24, 8, 192, 100),          # wide
    _c('A', 17, 6, 208, 250),
    _c('A', 3, 2, 224, 130),
    _c('A', 31, 8, 240, 1000),         # wide
    _c('A', 17, 6, 256, 1024),
    _c('A', 11, 3, (200, 48), 100),
    _c('A', 11, 3, (16, 256), 100),
    _c('A', 11, 3, (100, 100), 100),   # device width 112: both layers padded
    # B. weight-gradient K passes and row-block counts
    _c('B', 17, 6, 256, 257),
    _c('B', 17, 6, 256, 511),
    _c('B', 17, 6, 256, 512),
    _c('B', 17, 6, 256, 513),
    _c('B', 17, 6, 256, 768),
    _c('B', 17, 6, 256, 769),
    _c('B', 17, 6, 256, 1024, seed=1),
    _c('B', 11, 3, 80, 272),
    _c('B', 11, 3, 80, 528),
    _c('B', 11, 3, 80, 1023),
    _c('B', 27, 8, 256, 513),
    _c('B', 27, 8, 256, 1024),
    _c('B', 3, 1, 16, 1024),
    _c('B', 17, 6, 256, 513, prior='normal'),
    # C. pool split, perf mode, 3 steps
    _c('C', 17, 6, 64, 40, n_env=0, steps=3),
    _c('C', 17, 6, 64, 40, n_env=40, steps=3),
    _c('C', 11, 3, 48, 17, n_env=1, steps=3),
    _c('C', 17, 6, 256, 300, n_env=150, steps=3),
    # D. perf-mode steps under graph replay (10 = the 8-step graph, then the 2-step one)
    _c('D', 17, 6, 256, 1024, steps=10),
    _c('D', 11, 3, 80, 528, steps=10),
    _c('D', 27, 8, 256, 1000, steps=10),
    _c('D', 11, 3, (48, 200), 300, steps=10),
    _c('D', 3, 1, 16, 1, steps=10),    # one B1 block: the prefetch is a launch of its own
    _c('D', 11, 3, 64, 16, steps=10),  # ...
    _c('D', 11, 3, 32, 9, steps=10),   # ...
    # E. launch forms: bit-identity only
    _c('E', 17, 6, 256, 1024),
    _c('E', 27, 8, 240, 1000),
    _c('E', 11, 3, 80, 528),
    _c('E', 17, 6, 64, 40, head='even'),   # G's perf-mode case under the launch forms and graph replay
    # G. saturated heads: one injected step; lower-clipped entries carry zero noise
    _c('G', 3, 1, 16, 17, head='upper'),               # A = 1, one B1 block
    _c('G', 3, 1, 16, 17, head='lower'),
    _c('G', 11, 3, 64, 40, head='mixed'),
    _c('G', 17, 6, 256, 100, head='mixed'),
    _c('G', 17, 6, 256, 100, head='cross'),            # the mask is per element, not per column
    # wide layer 1.  seed 0: fp32 rounds the Polyak average of one unmoved bl entry near -26 by an ulp (1.9e-6),
    # 0.65 of the target tolerance; without the head shifts the same shape and seed sit at 0.009
    _c('G', 27, 8, 96, 40, seed=1, prior='normal', head='mixed'),
    _c('G', 17, 6, 256, 513, head='mixed'),            # three K passes: sac_wgrad.h recomputes the clamp per chunk
    _c('G', 11, 3, (48, 200), 100, head='mixed'),      # zero-padded widths
    _c('G', 17, 6, 64, 40, steps=3, head='even'),      # perf mode: the upper clip and the inside class only
]

# F. refusals: (constructor keywords over SAC(11, 3, ...), a pattern of the message)
REFUSALS = [
    (dict(batch_size=0), r'batch must be in \[1, 1024\]'),
    (dict(batch_size=1025), r'batch must be in \[1, 1024\]'),
    (dict(hidden=257), r'hidden width must be a multiple of 16, <= 256'),
    (dict(real_ratio=1.5), r'n_env must be in \[0, batch\]'),
]


def by_group(*groups):
    return [c for c in CASES if c.group in groups]


def device_width(hidden):
    """The square width the device runs at (mopo_amd.rollout.device_hidden): max(H1, H2) rounded up to 16."""
    return (max(osac._hs(hidden)) + 15) // 16 * 16


def hidden_id(hidden):
    return 'H%d' % hidden if np.isscalar(hidden) else 'H%dx%d' % tuple(hidden)


def case_id(c):
    s = '%s-%d+%d-%s-n%d-e%d' % (c.group, c.o, c.a, hidden_id(c.hidden), c.n, c.n_env)
    return s + ('-normal' if c.prior == 'normal' else '') + ('-' + c.head if c.head else '')


def real_ratio(c):
    """A ratio with int(n * ratio) == n_env (mopo.py:803): 0.0, 0.5 and 1.0 where they say it exactly."""
    if c.n_env == int(c.n * 0.05):
        return 0.05
    for r in (0.0, 0.5, 1.0):
        if int(c.n * r) == c.n_env:
            return r
    r = (c.n_env + 0.5) / c.n
    assert int(c.n * r) == c.n_env
    return r


def flat(ts):
    return np.concatenate([np.asarray(t).ravel() for t in ts])


def make_pool(rs, rows, o, a):
    return {'observations': rs.normal(size=(rows, o)).astype(np.float32),
            'actions': rs.uniform(-1, 1, (rows, a)).astype(np.float32),
            'next_observations': rs.normal(size=(rows, o)).astype(np.float32),
            'rewards': rs.normal(size=(rows, 1)).astype(np.float32),
            'terminals': rs.uniform(size=(rows, 1)) < 0.1}


def nan_pool(o, a):
    """One row of NaN: the pool a step must never read (n_env = 0: the env pool; n_env = n: the model pool)."""
    f = lambda w: np.full((1, w), np.nan, np.float32)
    return {'observations': f(o), 'actions': f(a), 'next_observations': f(o), 'rewards': f(1),
            'terminals': np.ones((1, 1), bool)}


def case_inputs(c):
    """dict: env / mod (pool sample dicts), params (the 20 tensors, fp32, the [H1, H2] layout), log_alpha, and
    the first step's idx [n] (first n_env index the env pool), eps_s, eps_n [n, a].  Injected cases draw those
    from the data seed; perf-mode cases (steps > 0) restate the device's streams at step 0.  All of it fp32."""
    rs = np.random.RandomState(1000 + c.seed)
    env, mod = make_pool(rs, ENV_ROWS, c.o, c.a), make_pool(rs, MODEL_ROWS, c.o, c.a)
    if c.group == 'C' and c.n_env == 0:
        env = nan_pool(c.o, c.a)
    if c.group == 'C' and c.n_env == c.n:
        mod = nan_pool(c.o, c.a)
    params = [(p + rs.normal(size=p.shape) * 0.02).astype(np.float32)      # non-zero biases
              for p in osac.init_params(c.o, c.a, c.hidden, seed=9)]
    if c.head == 'cross':
        cross_head(c, env, mod, params)
    elif c.head:
        cls = head_classes(c)
        params[7] = (params[7] + np.where(cls > 0, HEAD_UP, np.where(cls < 0, -HEAD_DOWN, 0.0))).astype(np.float32)
    ne, nm = len(env['rewards']), len(mod['rewards'])
    if c.steps:
        assert not c.head or (head_classes(c) >= 0).all(), 'the lower clip needs injected (zeroed) noise'
        idx, e1, e2 = perf_streams(c, ne, nm, 0)
    else:
        idx = np.concatenate([rs.randint(0, ne, c.n_env), rs.randint(0, nm, c.n - c.n_env)]).astype(np.int64)
        e1 = rs.normal(size=(c.n, c.a)).astype(np.float32)
        e2 = rs.normal(size=(c.n, c.a)).astype(np.float32)
    ci = dict(case=c, env=env, mod=mod, params=params, log_alpha=np.float32(LOG_ALPHA), idx=idx, eps_s=e1, eps_n=e2)
    if c.head and (head_classes(c) < 0).any():
        # no noise where the fp64 oracle's raw log-std is below the lower bound: u == mu in every precision
        raw = head_raw(params, host_batch(ci, idx, np.float64))
        e1[raw[0] < osac.LOG_STD_MIN] = 0
        e2[raw[1] < osac.LOG_STD_MIN] = 0
    return ci


def head_classes(c):
    """Per column of the log-std head: +1 shifted above the upper bound, -1 below the lower one, 0 left alone."""
    return np.asarray(HEAD_MODES[c.head](np.arange(c.a)))


def head_raw(params, batch):
    """The raw (unclipped) log-std of pi(s) and pi(s') on ``batch`` [2, n, a], in the parameters' precision."""
    P = [np.asarray(p, batch['observations'].dtype) for p in params[:8]]
    z = np.zeros((len(batch['observations']), P[7].size), batch['observations'].dtype)
    return np.stack([osac.pi_forward(P, batch[k], z)[4]['ls_raw'] for k in ('observations', 'next_observations')])


def cross_head(c, env, mod, params):
    """'cross': observations in two clusters (an eighth of their spread around two centres), then column CROSS_COL
    of Wl times a power of two and its bias shifted, so that on every pool row -- pi(s) and pi(s') alike -- the
    column's raw log-std is either above the upper bound or inside, above -INSIDE, at least 0.2 further from the
    bound than CLIP_MARGIN.  Which side a row falls on is its cluster's; every change is exact in f32."""
    rs = np.random.RandomState(5000 + c.seed)
    centres = rs.normal(size=(2, c.o))
    for pool in (env, mod):
        for k in ('observations', 'next_observations'):
            z = rs.randint(0, 2, len(pool[k]))
            pool[k] = (0.125 * pool[k] + centres[z]).astype(np.float32)
    f = np.float64
    both = {k: np.concatenate([env[k], mod[k]]).astype(f) for k in ('observations', 'next_observations')}
    v = head_raw([p.astype(f) for p in params], both)[:, :, CROSS_COL].ravel()
    cut = 0.5 * (v.min() + v.max())
    lo, hi = v[v < cut], v[v >= cut]
    gap, width = hi.min() - lo.max(), lo.max() - lo.min()
    m = CLIP_MARGIN + 0.2
    k = 2.0 ** np.ceil(np.log2(2 * m / gap))
    assert gap > 0 and k * width <= osac.LOG_STD_MAX - m + INSIDE - 0.2, (gap, width, k)
    params[6] = params[6].copy()
    params[6][:, CROSS_COL] *= np.float32(k)
    params[7] = params[7].copy()
    params[7][CROSS_COL] = np.float32(k * params[7][CROSS_COL] + (osac.LOG_STD_MAX - m - k * lo.max()))


def perf_streams(c, env_size, model_size, k, seed=PERF_SEED):
    """(idx, eps_s, eps_n) of perf-mode step k of a fresh handle: the device's Philox streams, restated."""
    return (orng.sac_batch_indices(c.n, c.n_env, env_size, model_size, seed, k),
            orng.sac_noise(c.n, c.a, seed, k, 0), orng.sac_noise(c.n, c.a, seed, k, 1))


def host_batch(ci, idx, dtype):
    """_training_batch (mopo.py:801-821): the env rows then the model rows, per field."""
    ne = ci['case'].n_env
    return {k: np.concatenate([ci['env'][k][idx[:ne]], ci['mod'][k][idx[ne:]]]).astype(dtype) for k in ci['env']}


def _state(ci, dtype):
    return osac.SACState([p.astype(dtype) for p in ci['params']], log_alpha=ci['log_alpha'], lr=LR, dtype=dtype)


def _snapshot(st):
    """params / target / Adam slots the way SAC.state_dict() lays them out (log_alpha and its slots last)."""
    opts = (st.opt_pi, st.opt_q1, st.opt_q2, st.opt_a)
    return {'params': np.append(flat(st.params), st.log_alpha), 'target': flat(st.target),
            'adam_m': np.concatenate([flat(o.m) for o in opts]), 'adam_v': np.concatenate([flat(o.v) for o in opts])}


def _assert_dtype(x, dtype):
    for v in (x.values() if isinstance(x, dict) else x):
        if isinstance(v, (dict, list)):
            _assert_dtype(v, dtype)
        else:
            assert np.asarray(v).dtype == dtype, (np.asarray(v).dtype, dtype)


def _margins(st, batch, e1):
    """(min |Q1(s, pi) - Q2(s, pi)|, max |Q|, min distance of a raw log-std from its clip bounds) of the
    pre-step parameters: how far the step's two discrete decisions are from flipping."""
    P, Q1, Q2 = osac.split(st.params)
    _, a_pi, _, _, cpi = osac.pi_forward(P, batch['observations'], e1)
    q1 = osac.q_forward(Q1, batch['observations'], a_pi)[0]
    q2 = osac.q_forward(Q2, batch['observations'], a_pi)[0]
    r = cpi['ls_raw']
    clip = min(np.abs(r - osac.LOG_STD_MIN).min(), np.abs(r - osac.LOG_STD_MAX).min())
    return float(np.abs(q1 - q2).min()), float(max(np.abs(q1).max(), np.abs(q2).max())), float(clip)


# The clip rule restated broken, for the sensitivity measurement of group G: name -> (keywords of broken_rule,
# the class of entries the break shows on: +1 upper, -1 lower, 0 either)
BREAKS = {
    'no clamp': (dict(lo=-np.inf, hi=np.inf), 0),
    'upper bound 2.5': (dict(hi=2.5), 1), 'upper bound 1.5': (dict(hi=1.5), 1),
    'lower bound -19.5': (dict(lo=-19.5), -1), 'lower bound -20.5': (dict(lo=-20.5), -1),
    'no mask': (dict(mask='none'), 0),
    'mask below only': (dict(mask='lower'), 1), 'mask above only': (dict(mask='upper'), -1),
}


def breaks_of(c):
    """The BREAKS that a case's classes can show ('cross' has upper entries)."""
    cls = set(head_classes(c).tolist()) | ({1} if c.head == 'cross' else set())
    return [k for k, (_, side) in BREAKS.items() if side == 0 or side in cls]


@contextlib.contextmanager
def broken_rule(lo=osac.LOG_STD_MIN, hi=osac.LOG_STD_MAX, mask='both'):
    """oracle/sac.py with other clip bounds (its module constants) for the length of the block; yields the
    ``clip_mask`` keyword of sac_step."""
    keep = osac.LOG_STD_MIN, osac.LOG_STD_MAX
    osac.LOG_STD_MIN, osac.LOG_STD_MAX = lo, hi
    try:
        with np.errstate(over='ignore'):       # an unclamped std of e^8 overflows sigmoid's exp to the right limit
            yield dict(clip_mask=mask)
    finally:
        osac.LOG_STD_MIN, osac.LOG_STD_MAX = keep


def oracle_step(ci, dtype=np.float64, rule=None):
    """One step of oracle/sac.py on the case's first batch, run in ``dtype``: dict with the pre-step ``grads``
    (the 20 tensors), ``g_alpha``, ``logs``, the state after the step (``params`` / ``target`` / ``adam_m`` /
    ``adam_v`` flat, log_alpha last where SAC.state_dict() has it), ``margins`` (_margins) and ``ls_raw``
    (head_raw).  ``rule``: keywords of broken_rule, the step under a broken clip rule."""
    c = ci['case']
    dtype = np.dtype(dtype)
    st = _state(ci, dtype)
    batch = host_batch(ci, ci['idx'], dtype)
    e1, e2 = ci['eps_s'].astype(dtype), ci['eps_n'].astype(dtype)
    margins = _margins(st, batch, e1)
    raw = head_raw(st.params, batch)
    got = {}
    with broken_rule(**(rule or {})) as kw:
        logs = osac.sac_step(st, batch, e1, e2, target_entropy=TARGET_ENTROPY, grads_out=got, action_prior=c.prior, **kw)
    out = dict(grads=got['pi'] + got['q1'] + got['q2'], g_alpha=got['alpha'], logs=logs, **_snapshot(st))
    _assert_dtype(out, dtype)        # an fp32 run that picked up an fp64 constant would flatter the case
    out['margins'] = margins
    out['ls_raw'] = raw
    return out


def oracle_steps(c, K=None, seed=PERF_SEED, dtype=np.float64):
    """K perf-mode steps (default: the case's) of a fresh handle on the restated device streams
    (oracle.rng.sac_batch_indices / sac_noise): the last step's ``logs``, the state after it as in
    oracle_step, and the batch rows of every step (``idx`` [K, n])."""
    dtype = np.dtype(dtype)
    ci = case_inputs(c)
    st = _state(ci, dtype)
    ne, nm = len(ci['env']['rewards']), len(ci['mod']['rewards'])
    rows, raws = [], []
    for k in range(c.steps if K is None else K):
        idx, e1, e2 = perf_streams(c, ne, nm, k, seed)
        batch = host_batch(ci, idx, dtype)
        raws.append(head_raw(st.params, batch))
        logs = osac.sac_step(st, batch, e1.astype(dtype), e2.astype(dtype),
                             target_entropy=TARGET_ENTROPY, action_prior=c.prior)
        rows.append(idx)
    out = dict(logs=logs, **_snapshot(st))
    _assert_dtype(out, dtype)
    out['idx'] = np.stack(rows)
    out['ls_raw'] = np.stack(raws)         # [K, 2, n, a]: each step's raw log-std of pi(s), pi(s'), pre-step
    return out


def clipped_columns(ls_raw):
    """The head columns whose raw log-std of pi(s) is outside the clip bounds on every row of ``ls_raw``
    ([..., n, a]): their Wl column and bl entry get exactly no gradient."""
    r = np.asarray(ls_raw).reshape(-1, np.asarray(ls_raw).shape[-1])
    return np.flatnonzero(((r < osac.LOG_STD_MIN) | (r > osac.LOG_STD_MAX)).all(0))


def head_column_index(c, cols):
    """Where column j of pi.Wl and entry j of pi.bl (j in ``cols``) lie in the flat [H1, H2] parameter layout
    (the same offsets in the gradients and, the four optimizers laid out pi, q1, q2, alpha, the Adam slots)."""
    sizes = [int(np.prod(s)) for s in osac.PI_SHAPES(c.o, c.a, c.hidden)]
    off = sum(sizes[:6])
    h2 = osac._hs(c.hidden)[1]
    wl = [off + np.arange(h2) * c.a + j for j in cols]
    return np.concatenate(wl + [off + sizes[6] + np.asarray(cols, np.int64)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def reference_step(c):
    """(case_inputs, fp64 oracle_step) of a case, computed once and shared; callers leave it unchanged."""
    ci = case_inputs(c)
    return ci, oracle_step(ci)


@functools.lru_cache(maxsize=None)
def reference_steps(c):
    return oracle_steps(c)


# ---- comparisons in units of their GPU tolerance
def log_ratio(got, ref):
    """Logged scalars: rel 2e-4, atol 1e-6."""
    return abs(float(got) - float(ref)) / (2e-4 * abs(float(ref)) + 1e-6)


def grad_ratio(got, ref):
    """One gradient tensor (or Adam slot): |d| <= 1e-4 max|ref| + 1e-7."""
    ref = np.asarray(ref, np.float64)
    d = np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref)
    return float(d.max() / (1e-4 * (np.abs(ref).max() + 1e-12) + 1e-7))


def tensor_ratios(got_flat, refs):
    """grad_ratio per tensor of ``refs`` (a list) over the flat ``got_flat`` in the same order."""
    out, off = [], 0
    for r in refs:
        m = np.asarray(r).size
        out.append(grad_ratio(got_flat[off:off + m], np.asarray(r).ravel()))
        off += m
    assert off == np.asarray(got_flat).size
    return out


def slot_ratios(got_flat, ref_flat, refs):
    """An Adam slot array (20 tensors then alpha's) against the oracle's, tensor by tensor."""
    sizes = [np.asarray(r).size for r in refs] + [1]
    parts = np.split(np.asarray(ref_flat, np.float64), np.cumsum(sizes)[:-1])
    return tensor_ratios(np.asarray(got_flat, np.float64), parts)


def param_ratio(got, ref, gref):
    """Parameters after one step (flat, without log_alpha): 1e-6 + 1e-6 max|p| where the gradient is not
    tiny; 1e-6 + 2 lr_t where it is (Adam's first step is lr_t sign(g): a vanishing gradient may flip)."""
    got, ref, gref = (np.asarray(x, np.float64).ravel() for x in (got, ref, gref))
    d = np.abs(got - ref)
    tiny = np.abs(gref) < 1e-3 * np.abs(gref).max()
    r = 0.0
    if (~tiny).any():
        r = d[~tiny].max() / (1e-6 + 1e-6 * np.abs(ref[~tiny]).max())
    if tiny.any():
        r = max(r, d[tiny].max() / (1e-6 + 2 * LR_T))
    return float(r)


def target_ratio(got, ref):
    d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    return float(d.max() / (2e-6 + 5e-3 * 2 * LR_T))


def loss_ratio(got, ref):
    """Last-step losses of several steps: within 1e-3 (1 + |ref|)."""
    return abs(float(got) - float(ref)) / (1e-3 * (1 + abs(float(ref))))


def steps_ratio(got, ref):
    """State after several steps: scaled error |d| / (1 + |ref|), p99 <= 1e-4 and max <= 1e-2."""
    ref = np.asarray(ref, np.float64)
    err = np.abs(np.asarray(got, np.float64) - ref) / (1 + np.abs(ref))
    return float(max(np.quantile(err, 0.99) / 1e-4, err.max() / 1e-2))


def step_ratios(got, ref):
    """Every one-step comparison of ``got`` (an oracle_step-shaped dict; logs under the oracle's keys) against
    the fp64 ``ref``: {name: ratio}."""
    out = {'log ' + rk: log_ratio(got['logs'][rk], ref['logs'][rk]) for _, rk in LOG_PAIRS}
    for name, r in zip(GRAD_NAMES, tensor_ratios(flat(got['grads']), ref['grads'])):
        out['grad ' + name] = r
    out['grad alpha'] = grad_ratio([got['g_alpha']], [ref['g_alpha']])
    out['params'] = param_ratio(got['params'][:-1], ref['params'][:-1], flat(ref['grads']))
    out['log_alpha'] = abs(float(got['params'][-1]) - float(ref['params'][-1])) / 1e-6
    for k in ('adam_m', 'adam_v'):
        for name, r in zip(GRAD_NAMES + ['alpha'], slot_ratios(got[k], ref[k], ref['grads'])):
            out['%s %s' % (k, name)] = r
    out['target'] = target_ratio(got['target'], ref['target'])
    return out


def multi_ratios(got, ref):
    """Every several-step comparison of ``got`` (logs under the oracle's keys) against the fp64 ``ref``."""
    out = {'loss ' + rk: loss_ratio(got['logs'][rk], ref['logs'][rk]) for _, rk in LOSS_PAIRS}
    for k in ('params', 'target', 'adam_m', 'adam_v'):
        out[k] = steps_ratio(got[k], ref[k])
    return out


def worst(ratios):
    k = max(ratios, key=ratios.get)
    return k, ratios[k]
