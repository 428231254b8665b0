"""Hard truncation (MOReL's HALT): the rule restated on the oracle, and the cases tests/test_halt_cases.py (CPU) and
tests/test_gpu_halt.py (GPU) share.  A helper: no tests here.

The rule (include/mopo_hip.h "Hard truncation"): with the penalty u of the selected kind at the row's (s, a), a row
halts iff not (u <= threshold); a halted row is terminal and its penalized reward is exactly halt_reward; nothing
else of any row changes.  ``apply_halt`` states it on the outputs of ``oracle.fake_env.step``; ``rollout_case``
re-loops ``oracle.rollout.rollout`` with it applied before the pool add.  u is ``penalty_kinds.penalty`` (numpy
f64) on ``oracle.bnn.forward``'s f64 member outputs.

Thresholds are a condition, not a tolerance: a case's threshold is the midpoint of the widest gap between
consecutive sorted u values of the case -- every (step, row) its rows would visit without halting -- between the
50th and the 90th percentile.  tests/test_halt_cases.py holds every case to: no u (f64 oracle or f32 oracle) within
``margin`` = 10 x the kind's device tolerance of the threshold, at least 10 % of the rows halt, at least 10 % reach
the last step.  The device's halted set is then the oracle's, exactly, with no row excluded.  THRESHOLDS is the
checked table; a case that misses the condition gets another seed, fewer rows or larger weights, never a wider
bound.

Every random stream of a rollout case is drawn per ORIGINAL row (its start index) and step, and a step injects the
live rows' entries in compacted order: a row's trajectory does not depend on which other rows halted, so the u
values a threshold is chosen from do not depend on the threshold.
"""
import functools

import numpy as np

import penalty_kinds as pk
from oracle import bnn as obnn
from oracle import fake_env as ofe

E, H = 7, 64
ELITES = [4, 1, 0, 6, 2]
BIAS_STD = pk.BIAS_STD
HALT_REWARD = -100.0
KINDS = (0, 1, 2, 3)


# ---- the rule ------------------------------------------------------------------------------------------------------
def apply_halt(rew, term, u, threshold, halt_reward=HALT_REWARD):
    """(rewards, terminals, halted) of ``oracle.fake_env.step``'s penalized ``rew`` [B, 1] / ``term`` [B, 1] under
    the rule, for the rows' penalties ``u`` [B]."""
    halted = ~(np.asarray(u) <= threshold)
    rew, term = np.array(rew, np.float64), np.array(term, bool)
    rew[halted] = halt_reward
    term[halted] = True
    return rew, term, halted


def member_outputs(p, obs, act, dtype=np.float64):
    return obnn.forward(p, np.concatenate([np.asarray(obs, np.float64), np.asarray(act, np.float64)], 1), dtype=dtype)


def margin(kind, u, mean, var):
    """10 x the device tolerance of a kind's u, per row: kinds 0 and 1 rel 1e-5 (tests/test_gpu_rollout.py's
    penalty tolerance); kinds 2 and 3 ``penalty_kinds.oracle_bound``."""
    return 10 * (1e-5 * np.abs(u) if kind < 2 else pk.oracle_bound(mean, var))


def gap_threshold(u):
    """The midpoint of the widest gap between consecutive sorted values of ``u`` from its 50th to its 90th
    percentile."""
    s = np.sort(np.asarray(u, np.float64).ravel())
    lo, hi = int(0.5 * (len(s) - 1)), int(np.ceil(0.9 * (len(s) - 1)))
    g = np.diff(s[lo:hi + 1])
    k = int(np.argmax(g))
    return float(0.5 * (s[lo + k] + s[lo + k + 1]))


FACTOR = 2.5    # on every weight matrix (tests/dim_cases.py FACTOR): at the initial scale the members' spread is all
                # bias, u barely depends on the row and its sorted values leave no gap


def _params(O, A, seed, inputs, factor=FACTOR):
    """``oracle.bnn.init_params`` with spread biases and weights times ``factor``; the mean and log-variance heads
    of observations 0 and 1 -- what the walker2d, hopper and ant rules read -- scaled down, so that the rules end
    rows at a moderate rate and a real share of them reaches the last step."""
    p = obnn.init_params(E, O, A, hidden=H, seed=seed, inputs=inputs, bias_std=BIAS_STD)
    p['W'] = [(w * np.float32(factor)).astype(np.float32) for w in p['W']]
    p['Wv'] = (p['Wv'] * np.float32(factor)).astype(np.float32)
    p['W'][-1][:, :, 1:3] *= np.float32(0.1)
    p['b'][-1][:, :, 1:3] *= np.float32(0.1)
    p['bv'][:, :, 1:3] -= np.float32(3.0)
    return p


def _start_states(rs, domain, n, O, near=1.0, far=3.0):
    """Start states in two clusters (7 in 10 at ``near`` standard deviations of the scaler's data, the rest at
    ``far``): the far rows' penalties stand clear of the near rows', which leaves the sorted u values a wide gap."""
    obs = rs.normal(size=(n, O)) * np.where(rs.uniform(size=(n, 1)) < 0.7, near, far)
    if domain in ('walker2d', 'hopper'):
        obs[:, 0], obs[:, 1] = rs.uniform(1.2, 1.6, n), rs.uniform(-0.15, 0.15, n)
    if domain == 'ant':
        obs[:, 0] = rs.uniform(0.5, 0.7, n)
    return obs.astype(np.float32)


# ---- 1. FakeEnv.step -----------------------------------------------------------------------------------------------
# (O, A) -> (domain, seed, weight factor); a seed that leaves a rule verdict within RULE_MARGIN of a bound, or a
# threshold condition unmet, is walked up in tens (tests/test_halt_cases.py holds every case to both)
STEP_SHAPES = {(17, 6): ('walker2d', 41, FACTOR), (11, 3): ('hopper', 72, FACTOR), (27, 8): ('ant', 43, FACTOR)}
STEP_B = (1, 37, 257)


@functools.lru_cache(None)
def step_case(O, A):
    """257 rows of one shape (the smaller batches are its first rows): inputs, both random streams, the f64 and
    f32 oracle's member outputs.  Never modified by a test."""
    domain, seed, factor = STEP_SHAPES[(O, A)]
    rs = np.random.RandomState(seed)
    B = max(STEP_B)
    obs = _start_states(rs, domain, B, O)
    act = rs.uniform(-1, 1, size=(B, A)).astype(np.float32)
    p = _params(O, A, seed + 1, np.concatenate([rs.normal(size=(400, O)), rs.uniform(-1, 1, (400, A))], 1), factor)
    noise = rs.normal(size=(E, B, O + 1))
    inds = rs.choice(ELITES, size=B)
    mean, var = member_outputs(p, obs, act)
    mean32, var32 = member_outputs(p, obs, act, np.float32)
    return dict(domain=domain, O=O, A=A, params=p, mats=obnn.to_mat_list(p), obs=obs, act=act, noise=noise,
                inds=inds, mean=mean, var=var, mean32=mean32, var32=var32)


def step_u(O, A, kind):
    c = step_case(O, A)
    return pk.penalty(kind, c['mean'], c['var'])


def step_reference(O, A, kind, B, det, coeff):
    """``oracle.fake_env.step`` on the case's first B rows with the rule applied: dict of next_obs, rew, term,
    halted, unpen, u, info (the oracle's)."""
    c = step_case(O, A)
    kw = dict(deterministic=True) if det else dict(noise=c['noise'][:, :B], model_inds=c['inds'][:B])
    nobs, rew, term, info = ofe.step(c['params'], ELITES, c['obs'][:B].astype(np.float64), c['act'][:B],
                                     ofe.TERMINATION[c['domain']], penalty_coeff=0.0, **kw)
    u = step_u(O, A, kind)[:B]
    rew2, term2, halted = apply_halt(rew - coeff * u[:, None], term, u, THRESHOLDS[('step', O, A, kind)])
    return dict(next_obs=nobs, rew=rew2, term=term2, halted=halted, rule=np.array(term, bool), unpen=rew, u=u,
                info=info)


# ---- 2. the fused rollout, parity mode ------------------------------------------------------------------------------
# name -> (domain, O, A, B, seed, weight factor, near, far); horizon 4, kinds 1 and 2.  The 16400 values of the
# 4100-row case leave no gap of 10 tolerances unless its two clusters of start states lie far apart.
ROLLOUT_CASES = {
    'halfcheetah-300': ('halfcheetah', 17, 6, 300, 51, FACTOR, 1.0, 3.0),
    'walker2d-300': ('walker2d', 17, 6, 300, 52, FACTOR, 1.0, 3.0),
    'ant-300': ('ant', 27, 8, 300, 103, FACTOR, 1.0, 3.0),
    'halfcheetah-4100': ('halfcheetah', 17, 6, 4100, 54, FACTOR, 0.3, 20.0),
}
ROLLOUT_HORIZON = 4
ROLLOUT_KINDS = (1, 2)
ROLLOUT_COEFF = 1.0


@functools.lru_cache(None)
def rollout_setup(name):
    from mopo_amd.rollout import init_sac_params, split_params
    domain, O, A, B, seed, factor, near, far = ROLLOUT_CASES[name]
    rs = np.random.RandomState(seed)
    env_n, h = 3000, ROLLOUT_HORIZON
    env_obs = _start_states(rs, domain, env_n, O, near, far)
    p = _params(O, A, seed + 1, np.concatenate([rs.normal(size=(400, O)), rs.uniform(-1, 1, (400, A))], 1), factor)
    flat = init_sac_params(O, A, 256, seed=seed + 2)
    P = [q.astype(np.float64) for q in split_params(flat, O, A)[:8]]
    start = rs.randint(0, env_n, B)
    # per original row and step: the policy noise, the selected member and its observation noise
    return dict(domain=domain, O=O, A=A, B=B, horizon=h, env_obs=env_obs, params=p, mats=obnn.to_mat_list(p),
                flat=flat, P=P, start=start, eps_act=rs.normal(size=(h, B, A)).astype(np.float32),
                eps_sel=rs.normal(size=(h, B, O + 1)), inds=rs.choice(ELITES, size=(h, B)).astype(np.int32))


def _rollout_loop(name, kind, threshold, horizon=None, coeff=ROLLOUT_COEFF, halt_reward=HALT_REWARD):
    """oracle.rollout.rollout's loop on the case's streams with the rule applied before the pool add
    (``threshold`` None: no halting).  Returns the oracle pool, steps_added, halted per step, the streams in
    compacted order, and per visited (step, row): u (f64 oracle), u32 (f32 oracle), margin, halted."""
    from oracle import replay_pool as opool
    from oracle import sac as osac
    s = rollout_setup(name)
    O, A, B, h = s['O'], s['A'], s['B'], horizon or s['horizon']
    pool = opool.Pool(O, A, B * h + 7)
    ids = np.arange(B)
    obs = s['env_obs'][s['start']]
    eps_act, eps_obs = np.zeros((h, B, A), np.float32), np.zeros((h, B, O + 1))
    inds_all = np.zeros((h, B), np.int32)
    steps, halted_n, visits = [], [], []
    for i in range(h):
        n = len(ids)
        ea, inds, nz = s['eps_act'][i, ids], s['inds'][i, ids], s['eps_sel'][i, ids]
        act, _ = osac.actor_act(s['P'], obs.astype(np.float32).astype(np.float64), ea.astype(np.float64))
        act = act.astype(np.float32)
        noise = np.zeros((E, n, O + 1))
        noise[inds, np.arange(n)] = nz
        nobs, rew, term, _ = ofe.step(s['params'], ELITES, obs, act, ofe.TERMINATION[s['domain']], noise=noise,
                                      model_inds=inds)
        mean, var = member_outputs(s['params'], obs, act)
        u = pk.penalty(kind, mean, var)
        u32 = pk.penalty(kind, *member_outputs(s['params'], obs, act, np.float32))
        rule = np.array(term, bool)
        if threshold is None:
            rew, halted = rew - coeff * u[:, None], np.zeros(n, bool)
        else:
            rew, term, halted = apply_halt(rew - coeff * u[:, None], term, u, threshold, halt_reward)
        eps_act[i, :n], eps_obs[i, :n], inds_all[i, :n] = ea, nz, inds
        steps.append(n)
        halted_n.append(int(halted.sum()))
        visits.append(dict(step=i, ids=ids, u=u, u32=u32, margin=margin(kind, u, mean, var), halted=halted,
                           rule=rule[:, 0], rule_distance=rule_distance(s['domain'], nobs)))
        pool.add_samples({'observations': obs, 'actions': act, 'next_observations': nobs, 'rewards': rew,
                          'terminals': term})
        nt = ~np.asarray(term, bool)[:, 0]
        if nt.sum() == 0:
            break
        obs, ids = nobs[nt], ids[nt]
    return dict(s, pool=pool, ref=pool.return_all_samples(), steps=steps, halted_n=halted_n, visits=visits,
                eps_act_c=eps_act, eps_obs_c=eps_obs, inds_c=inds_all, horizon=h)


@functools.lru_cache(None)
def rollout_unhalted(name, kind):
    return _rollout_loop(name, kind, None)


@functools.lru_cache(None)
def rollout_case(name, kind, horizon=None):
    return _rollout_loop(name, kind, THRESHOLDS[('rollout', name, kind)], horizon=horizon)


def case_values(key):
    """(u, u32, margin) over everything the case's rows visit without halting: what its threshold is chosen from."""
    if key[0] == 'step':
        _, O, A, kind = key
        c = step_case(O, A)
        u = pk.penalty(kind, c['mean'], c['var'])
        return u, pk.penalty(kind, c['mean32'], c['var32']), margin(kind, u, c['mean'], c['var'])
    v = rollout_unhalted(key[1], key[2])['visits']
    return tuple(np.concatenate([x[k] for x in v]) for k in ('u', 'u32', 'margin'))


def case_shares(key):
    """(share of the case's rows that halt, share that reach the last step) at the table's threshold."""
    if key[0] == 'step':
        u = case_values(key)[0]
        halted = ~(u <= THRESHOLDS[key])
        return float(halted.mean()), float((~halted).mean())
    c = rollout_case(key[1], key[2])
    last = c['steps'][c['horizon'] - 1] if len(c['steps']) == c['horizon'] else 0
    return sum(c['halted_n']) / c['B'], last / c['B']


def rule_distance(domain, next_obs):
    """Per row, the distance of what the termination rule reads to its nearest bound (inf: a never-done rule)."""
    x, y = next_obs[:, 0], next_obs[:, 1]
    if domain == 'walker2d':
        return np.minimum(np.abs(x[:, None] - np.array([0.8, 2.0])).min(1), np.abs(np.abs(y) - 1.0))
    if domain == 'hopper':
        return np.minimum(np.abs(x - 0.7), np.abs(np.abs(y) - 0.2))
    if domain == 'ant':
        return np.abs(x[:, None] - np.array([0.2, 1.0])).min(1)
    return np.full(len(next_obs), np.inf)


RULE_MARGIN = 1e-3    # tests/dim_cases.py TERM_MARGIN: 20 x the 5e-5 state tolerance


def all_keys():
    return [('step', O, A, k) for (O, A) in STEP_SHAPES for k in KINDS] + \
           [('rollout', n, k) for n in ROLLOUT_CASES for k in ROLLOUT_KINDS]


# The checked table (tests/test_halt_cases.py recomputes every entry from gap_threshold and holds it to the
# conditions above).
THRESHOLDS = {
    ('step', 17, 6, 0): 3.9972519015431618,
    ('step', 17, 6, 1): 3.4984104900555506,
    ('step', 17, 6, 2): 7.3598358820516134,
    ('step', 17, 6, 3): 4.4527558692279161,
    ('step', 11, 3, 0): 3.1483136842387967,
    ('step', 11, 3, 1): 2.9009802850865851,
    ('step', 11, 3, 2): 5.6261568783572429,
    ('step', 11, 3, 3): 3.7030603985707136,
    ('step', 27, 8, 0): 4.595797309963638,
    ('step', 27, 8, 1): 4.5125199968264251,
    ('step', 27, 8, 2): 11.103066362925754,
    ('step', 27, 8, 3): 5.866586178438304,
    ('rollout', 'halfcheetah-300', 1): 3.462670894674706,
    ('rollout', 'halfcheetah-300', 2): 8.656354303401562,
    ('rollout', 'walker2d-300', 1): 3.6985507770824171,
    ('rollout', 'walker2d-300', 2): 9.0898476535766477,
    ('rollout', 'ant-300', 1): 4.6302298454385831,
    ('rollout', 'ant-300', 2): 12.441150275811491,
    ('rollout', 'halfcheetah-4100', 1): 3.7242537155692981,
    ('rollout', 'halfcheetah-4100', 2): 16.646785154914653,
}
