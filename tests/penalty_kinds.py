"""The penalty kinds in numpy f64, and the cases tests/test_penalty_kinds.py (CPU) and
tests/test_gpu_penalty_kinds.py (GPU) share.  A helper: no tests here.

``penalty(kind, means, variances)`` is the definition table of DESIGN section 2, written out in f64 on
``oracle.bnn.forward`` outputs ([E, B, D]; d = 0 the reward, d = 1.. the observations) BEFORE the residual add:

  0 mean_distance   max_e || mu_e - mean over members ||        over the obs dims   (fake_env.py:98-108)
  1 max_aleatoric   max_e || sigma_e ||                         over all D dims     (fake_env.py:110)
  2 max_pairwise    max_{i<j} || mu_i - mu_j ||                 over the obs dims; 0 when E = 1
  3 ensemble_std    sqrt(sum_d (1/E) sum_e [sigma_e[d]^2 + (mu_e[d] - mubar[d])^2])   over all D dims

The cases are seeded random-init ensembles.  Their seeds are chosen on the CPU (test_penalty_kinds.py) so that the
four kinds differ pairwise by more than 100 x the GPU test's tolerance on at least 90 % of the rows: a GPU test
that passes can then tell the kinds apart.  A case that fails that check gets another seed, never a looser bound.
"""
import functools
import itertools

import numpy as np

from oracle import bnn as obnn

PENALTY_KINDS = ('mean_distance', 'max_aleatoric', 'max_pairwise', 'ensemble_std')


def penalty(kind, means, variances):
    """The penalty [B] of ``kind`` (a name or its id) in f64."""
    k = PENALTY_KINDS.index(kind) if isinstance(kind, str) else int(kind)
    mu, var = np.asarray(means, np.float64), np.asarray(variances, np.float64)
    E = mu.shape[0]
    if k == 0:
        d = mu[:, :, 1:] - mu[:, :, 1:].mean(0)
        return np.sqrt((d * d).sum(2)).max(0)
    if k == 1:
        return np.sqrt(var.sum(2)).max(0)
    if k == 2:
        out = np.zeros(mu.shape[1])
        for i, j in itertools.combinations(range(E), 2):
            d = mu[i, :, 1:] - mu[j, :, 1:]
            out = np.maximum(out, np.sqrt((d * d).sum(1)))
        return out
    if k == 3:
        d = mu - mu.mean(0)
        return np.sqrt((var + d * d).mean(0).sum(1))
    raise ValueError('unknown penalty kind %r' % (kind,))


# ---- tolerances -------------------------------------------------------------------------------------------
KERNEL_RTOL = 1e-5     # the kernel against f64 on the device's own member outputs: the project's penalty tolerance


def oracle_bound(means, variances):
    """|u - u_ref| allowed against the f64 oracle, per row: 2 sqrt(D) 2e-5 (1 + max |ref|) over the row's means
    and stds.  The kinds are at most 2-Lipschitz in the stacked member outputs (a max or a root-mean-square of
    norms of the outputs or of their differences), each output is held to the ensemble tolerance
    2e-5 (1 + |ref|), and a norm over D outputs gathers at most sqrt(D) of that."""
    mu, sd = np.asarray(means, np.float64), np.sqrt(np.asarray(variances, np.float64))
    D = mu.shape[2]
    top = np.maximum(np.abs(mu).max((0, 2)), np.abs(sd).max((0, 2)))
    return 2 * np.sqrt(D) * 2e-5 * (1 + top)


def separation(means, variances, tol):
    """The smallest, over the pairs of kinds, fraction of rows on which the two kinds differ by more than
    100 x tol (``tol``: a per-row array, or 'kernel' for KERNEL_RTOL times the larger of the two)."""
    u = [penalty(k, means, variances) for k in range(4)]
    worst = 1.0
    for a, b in itertools.combinations(range(4), 2):
        t = KERNEL_RTOL * np.maximum(u[a], u[b]) if isinstance(tol, str) else tol
        worst = min(worst, float(np.mean(np.abs(u[a] - u[b]) > 100 * t)))
    return worst


# ---- 1. the kernel's arithmetic alone (mopo_fakeenv_step, caller-owned member outputs) ----------------------
H = 32
# the spread of the members' biases (oracle.bnn.init_params; its default 0.01 gives members that all but agree:
# the two kinds over the means near 0, max_aleatoric within 0.2 % of ensemble_std, no seed separates them)
BIAS_STD = 0.5
KERNEL_E = (1, 2, 7, 32)
KERNEL_OA = ((3, 1), (17, 6), (31, 8), (27, 8))     # D = 4, 18, 32 (a full lane group) and a wide model
KERNEL_B = (1, 65, 257)
KERNEL_SMV = (True, False)
KERNEL_SEEDS = {}                                   # (E, O, A, smv) -> seed, where the default does not separate


def kernel_case(E, O, A, smv):
    """Weights (the .mat list) and 257 input rows of one shape; the smaller batches are its first rows."""
    seed = KERNEL_SEEDS.get((E, O, A, smv), 1000 + 37 * E + O + (0 if smv else 500))
    rs = np.random.RandomState(seed)
    obs = rs.normal(size=(max(KERNEL_B), O)).astype(np.float32)
    act = rs.uniform(-1, 1, size=(max(KERNEL_B), A)).astype(np.float32)
    p = obnn.init_params(E, O, A, hidden=H, seed=seed + 1, smv=smv, inputs=np.concatenate([obs, act], 1),
                         bias_std=BIAS_STD)
    return dict(params=p, mats=obnn.to_mat_list(p), obs=obs, act=act, seed=seed)


# ---- 2. FakeEnv.step against the f64 oracle ------------------------------------------------------------------
STEP_SHAPE = dict(E=7, O=17, A=6, B=257)
STEP_SEED = 23     # 21: max_pairwise and ensemble_std within 100 x the bound of each other on every row


@functools.lru_cache(None)
def step_case():
    E, O, A, B = (STEP_SHAPE[k] for k in 'EOAB')
    rs = np.random.RandomState(STEP_SEED)
    obs = rs.normal(size=(B, O)).astype(np.float32)
    act = rs.uniform(-1, 1, size=(B, A)).astype(np.float32)
    p = obnn.init_params(E, O, A, hidden=H, seed=STEP_SEED + 1, inputs=np.concatenate([obs, act], 1), bias_std=BIAS_STD)
    mu, var = obnn.forward(p, np.concatenate([obs, act], 1), dtype=np.float64)
    noise = rs.normal(size=(E, B, O + 1))
    inds = rs.choice([4, 1, 0, 6, 2], size=B)
    return dict(params=p, mats=obnn.to_mat_list(p), obs=obs, act=act, mean=mu, var=var, noise=noise, inds=inds)


# ---- 3. the fused rollout, parity mode -------------------------------------------------------------------------
# name -> (domain, O, A, B, horizon, seed): one stream; the split path; compaction; a wide model
ROLLOUT_CASES = {
    'halfcheetah-300': ('halfcheetah', 17, 6, 300, 3, 31),
    'halfcheetah-4096': ('halfcheetah', 17, 6, 4096, 2, 32),
    'walker2d-300': ('walker2d', 17, 6, 300, 3, 33),
    'ant-130': ('ant', 27, 8, 130, 2, 34),
}
ROLLOUT_E = 7


@functools.lru_cache(None)
def rollout_case(name, det):
    """The oracle rollout with ``penalty_coeff = 0`` -- every transition but the penalty -- with each random
    stream drawn in the reference's order and recorded for injection (the loop of oracle.rollout, as
    tests/test_gpu_rollout.py runs it), and per pool row the f64 member outputs of the pool's own (obs, act):
    ``mean`` / ``var`` [E, rows, D]."""
    from mopo_amd.rollout import init_sac_params, split_params
    from oracle import fake_env as ofe
    from oracle import replay_pool as opool
    from oracle import sac as osac
    domain, O, A, B, horizon, seed = ROLLOUT_CASES[name]
    E = ROLLOUT_E
    rs = np.random.RandomState(seed)
    env_n = 3000
    env_obs = rs.normal(size=(env_n, O)).astype(np.float32)
    if domain == 'walker2d':
        env_obs[:, 0], env_obs[:, 1] = rs.uniform(1.2, 1.6, env_n), rs.uniform(-0.3, 0.3, env_n)
    if domain == 'ant':
        env_obs[:, 0] = rs.uniform(0.5, 0.7, env_n)
    inputs = np.concatenate([env_obs, rs.uniform(-1, 1, (env_n, A))], 1)
    p = obnn.init_params(E, O, A, hidden=H, seed=seed + 1, inputs=inputs, bias_std=BIAS_STD)
    flat = init_sac_params(O, A, 256, seed=seed + 2)
    P = [q.astype(np.float64) for q in split_params(flat, O, A)[:8]]
    elites = [4, 1, 0, 6, 2]
    model_pool = opool.Pool(O, A, B * horizon + 7)
    np.random.seed(seed)
    start = np.random.randint(0, env_n, B)
    obs = env_obs[start]
    act_rs = np.random.RandomState(seed + 99)    # stands in for TF's policy noise stream
    eps_act = np.zeros((horizon, B, A), np.float32)
    eps_obs = np.zeros((horizon, B, O + 1))
    inds_all = np.zeros((horizon, B), np.int32)
    steps = []
    for i in range(horizon):
        n = len(obs)
        ea = act_rs.normal(size=(n, A)).astype(np.float32)
        act, _ = osac.actor_act(P, obs.astype(np.float32).astype(np.float64), ea.astype(np.float64))
        act = act.astype(np.float32)
        if det:
            nobs, rew, term, _ = ofe.step(p, elites, obs, act, ofe.TERMINATION[domain], deterministic=True)
        else:
            noise = np.random.normal(size=(E, n, O + 1))
            inds = np.random.choice(elites, size=n)
            nobs, rew, term, _ = ofe.step(p, elites, obs, act, ofe.TERMINATION[domain], noise=noise, model_inds=inds)
            eps_obs[i, :n], inds_all[i, :n] = noise[inds, np.arange(n)], inds
        eps_act[i, :n] = ea
        steps.append(n)
        model_pool.add_samples({'observations': obs, 'actions': act, 'next_observations': nobs, 'rewards': rew,
                                'terminals': term})
        if term.all():
            break
        obs = nobs[~term[:, 0]]
    ref = model_pool.return_all_samples()
    mean, var = obnn.forward(p, np.concatenate([ref['observations'], ref['actions']], 1), dtype=np.float64)
    return dict(domain=domain, O=O, A=A, B=B, horizon=horizon, env_obs=env_obs, mats=obnn.to_mat_list(p), flat=flat,
                elites=elites, start=start, eps_act=eps_act, eps_obs=eps_obs, inds=inds_all, steps=steps,
                pool=model_pool, ref=ref, mean=mean, var=var)
