"""Evaluation rollouts in a real environment and the normalized return (host loop around the device policy).

Reference: ``RLAlgorithm._evaluation_paths`` / ``_evaluate_rollouts`` (softlearning/algorithms/
rl_algorithm.py:258-304), ``rollout`` / ``rollouts`` (softlearning/samplers/utils.py:36-92), MOPO's
deterministic evaluation policy and ``perf/*`` keys (mopo/algorithms/mopo.py:577-629), the D4RL env
name and reference scores (mopo.py:115-123, d4rl.infos).  The environment is any object with the gym
API (``reset() -> obs``, ``step(action) -> (obs, reward, done, info)``): MuJoCo is not in this image,
so the caller supplies it.  Actions come from the device actor (``mopo_actor_forward_dtype``): the
deterministic branch of get_action_meta, tanh(mu) (mopo.py:481-482).
"""
from collections import OrderedDict

import numpy as np

from . import _lib as L

# d4rl/infos.py REF_MIN_SCORE / REF_MAX_SCORE of the MuJoCo v0 tasks the configs name (random-policy and
# expert returns per domain; d4rl is not installed here, so the published constants are restated)
_DOMAIN_REF = {'halfcheetah': (-280.178953, 12135.0), 'hopper': (-20.272305, 3234.3),
               'walker2d': (1.629008, 4592.3)}
_DATASETS = ('random', 'medium', 'expert', 'medium-replay', 'medium-expert')
REF_MIN_SCORE = {'%s-%s-v0' % (d, s): v[0] for d, v in _DOMAIN_REF.items() for s in _DATASETS}
REF_MAX_SCORE = {'%s-%s-v0' % (d, s): v[1] for d, v in _DOMAIN_REF.items() for s in _DATASETS}


def env_name_of(model_name):
    """mopo.py:115-118: '<task>_smv_1_0' -> '<task>-v0'."""
    return (model_name[:-8] if '_smv' in model_name else model_name[:-4]) + '-v0'


def ref_scores(model_name):
    """(min_ret, max_ret) of mopo.py:119-123 (0, 0 when the task is not a D4RL one)."""
    n = env_name_of(model_name or '')
    return (REF_MIN_SCORE[n], REF_MAX_SCORE[n]) if n in REF_MIN_SCORE else (0.0, 0.0)


class DevicePolicy:
    """The current policy on the device: ``actions(obs[B, O]) -> [B, A]`` (deterministic: tanh(mu))."""

    def __init__(self, pi_params, obs_dim, act_dim, hidden=256, deterministic=True, dtype=0):
        self.P, self.O, self.A, self.H = pi_params, obs_dim, act_dim, hidden
        self.deterministic, self.dtype = deterministic, dtype
        self._step = 0

    def actions(self, obs):
        import torch
        o = torch.as_tensor(np.ascontiguousarray(obs, np.float32)).cuda()
        if o.dim() == 1:
            o = o[None]
        B = int(o.shape[0])
        act = torch.empty((B, self.A), dtype=torch.float32, device=o.device)
        mu = torch.empty_like(act)
        ptr = self.P if isinstance(self.P, int) else L.ptr(self.P)
        self._step += 1
        L.check(L.lib().mopo_actor_forward_dtype(ptr, self.O, self.A, self.H, L.ptr(o), 0, B, None, 2024,
                                                 self._step, L.ptr(act), L.ptr(mu), self.dtype, L.stream_ptr()))
        return (mu if self.deterministic else act).cpu().numpy()


def rollout(env, policy, path_length, break_on_terminal=True):
    """One episode (samplers/utils.py:36-80): observations, actions, rewards, terminals, next_observations."""
    obs = env.reset()
    path = {k: [] for k in ('observations', 'actions', 'rewards', 'terminals', 'next_observations')}
    infos = []
    for t in range(path_length):
        a = policy.actions(np.asarray(obs)[None])[0]
        nobs, r, done, info = env.step(a)
        for k, v in zip(path, (obs, a, [r], [done], nobs)):
            path[k].append(np.asarray(v))
        infos.append(info)
        obs = nobs
        if done and break_on_terminal:
            break
    out = {k: np.stack(v) for k, v in path.items()}
    out['infos'] = infos
    return out


def evaluation_paths(env, policy, n_episodes, path_length):
    """_evaluation_paths (rl_algorithm.py:258-279): ``n_episodes`` rollouts, none if n_episodes < 1."""
    return [rollout(env, policy, path_length) for _ in range(n_episodes)] if n_episodes >= 1 else []


def evaluate_rollouts(paths, env=None):
    """_evaluate_rollouts (rl_algorithm.py:281-304)."""
    total = [float(np.sum(p['rewards'])) for p in paths]
    lengths = [len(p['rewards']) for p in paths]
    d = OrderedDict((('return-average', np.mean(total)), ('return-min', np.min(total)),
                     ('return-max', np.max(total)), ('return-std', np.std(total)),
                     ('episode-length-avg', np.mean(lengths)), ('episode-length-min', np.min(lengths)),
                     ('episode-length-max', np.max(lengths)), ('episode-length-std', np.std(lengths))))
    if env is not None and hasattr(env, 'get_path_infos'):
        for k, v in env.get_path_infos(paths).items():
            d['env_infos/{}'.format(k)] = v
    return d


def perf_metrics(evaluation, min_ret, max_ret):
    """mopo.py:623-629: perf/AverageReturn, perf/AverageLength, perf/NormalizedReturn (D4RL tasks)."""
    out = OrderedDict([('perf/AverageReturn', evaluation['return-average']),
                       ('perf/AverageLength', evaluation['episode-length-avg'])])
    if min_ret != max_ret:
        out['perf/NormalizedReturn'] = (out['perf/AverageReturn'] - min_ret) / (max_ret - min_ret)
    return out


# ---- evaluation inside the learned model (ModelRollout.evaluate, csrc/rollout_eval.hip) -------------------
# The episodes run in FakeEnv, not in the task: the returns are returns UNDER THE MODEL, biased wherever the
# model is wrong (the policy is trained to exploit exactly those places as far as the penalty lets it).  They
# are no D4RL score, so no perf/NormalizedReturn is derived from them.
def halt_threshold_from_quantile(u, q):
    """The hard-truncation threshold at quantile ``q`` of the penalties ``u`` (``ModelRollout.penalty_profile``;
    a tensor or an array): the order statistic ``sorted(u)[ceil(q * N) - 1]``, a value of ``u`` itself (no
    interpolation), so exactly ``N - ceil(q * N)`` dataset rows lie above it when the values are distinct.
    ``0 < q <= 1``; deterministic (``torch.sort``).  Returns a Python float."""
    import math
    import torch
    if not 0.0 < float(q) <= 1.0:
        raise ValueError('halt quantile must satisfy 0 < q <= 1 (got %r)' % (q,))
    t = torch.as_tensor(u).reshape(-1)
    n = int(t.numel())
    if n == 0:
        raise ValueError('halt quantile of an empty penalty profile')
    return float(torch.sort(t)[0][int(math.ceil(float(q) * n)) - 1])


MODEL_EVAL_KEYS = ('return-average', 'return-min', 'return-max', 'return-std', 'episode-length-avg',
                   'episode-length-min', 'episode-length-max', 'episode-length-std', 'penalized-return-average',
                   'penalty-average', 'terminated-fraction')


def model_evaluation_metrics(stats):
    """The device statistics ``ModelRollout.evaluate(...)['stats']`` (f64[16]; the first eleven in
    ``MODEL_EVAL_KEYS`` order) as evaluate_rollouts' OrderedDict plus ``penalized-return-average`` (mean
    of the penalized returns, fake_env.py:115), ``penalty-average`` (mean penalty per step taken) and
    ``terminated-fraction`` (episodes ended by the termination rule before the length cap).  The penalty is
    the selected kind's (``fake_env.PENALTY_KINDS``; ``penalty_kind`` of ``ModelRollout.evaluate`` / ``MOPO``)."""
    s = stats.detach().cpu().numpy() if hasattr(stats, 'detach') else np.asarray(stats)
    return OrderedDict((k, float(s[i])) for i, k in enumerate(MODEL_EVAL_KEYS))


def model_evaluation_metrics_numpy(returns, lengths, penalized_returns, penalty_sums, terminated):
    """The same dict from per-episode host arrays (what the device reduction must equal)."""
    r, n = np.asarray(returns, np.float64), np.asarray(lengths, np.float64)
    vals = (np.mean(r), np.min(r), np.max(r), np.std(r), np.mean(n), np.min(n), np.max(n), np.std(n),
            np.mean(np.asarray(penalized_returns, np.float64)), np.sum(np.asarray(penalty_sums, np.float64)) / np.sum(n),
            np.mean(np.asarray(terminated, np.float64)))
    return OrderedDict((k, float(v)) for k, v in zip(MODEL_EVAL_KEYS, vals))


# ---- open-loop validation of the learned model on dataset trajectories (ModelRollout.validate,
# csrc/rollout_val.hip) ----------------------------------------------------------------------------------
# The dataset's own actions replayed through the model from dataset states, the model fed its predictions:
# error(k) is the compounding-error curve, and the penalty recorded beside it shows whether u(s, a) tracks
# (and bounds) the true error, the assumption MOPO's guarantee rests on.
OPEN_LOOP_SLOTS = ('n', 'error', 'error-std', 'error-max', 'obs-error', 'reward-error', 'penalty', 'penalty-std',
                   'penalty-error-corr', 'covered', 'termination-mismatch')
END_REASONS = ('horizon', 'terminal', 'discontinuity', 'end-of-pool')


def open_loop_metrics(stats):
    """The device statistics ``ModelRollout.validate(...)['stats']`` (f64[K + 1, 16], columns in
    ``OPEN_LOOP_SLOTS`` order; row k - 1 over the segments alive at step k, row K pooled over all steps) as an
    OrderedDict: per step k = 1..K ``open_loop/error-h{k}`` (mean L2 error of the predicted (reward, next state)
    after k model steps), ``obs-error-h{k}``, ``penalty-h{k}``, ``covered-h{k}`` (fraction with penalty >= error)
    and ``alive-h{k}`` (segments that reached the step); pooled ``open_loop/error``, ``penalty``,
    ``penalty-error-corr`` (Pearson), ``covered`` and ``termination-mismatch`` (the termination rule on the
    predicted state against the data's flag).  ``penalty*`` / ``covered*`` report the selected penalty kind
    (``fake_env.PENALTY_KINDS``; ``penalty_kind`` of ``ModelRollout.validate`` / ``MOPO``): compared with the
    error over all outputs for max_aleatoric and ensemble_std, over the obs dims for mean_distance and
    max_pairwise."""
    s = stats.detach().cpu().numpy() if hasattr(stats, 'detach') else np.asarray(stats)
    K = s.shape[0] - 1
    out = OrderedDict()
    for k in range(1, K + 1):
        for name, col in (('error', 1), ('obs-error', 4), ('penalty', 6), ('covered', 9), ('alive', 0)):
            out['open_loop/%s-h%d' % (name, k)] = float(s[k - 1, col])
    for name, col in (('error', 1), ('penalty', 6), ('penalty-error-corr', 8), ('covered', 9),
                      ('termination-mismatch', 10)):
        out['open_loop/' + name] = float(s[K, col])
    return out


def open_loop_metrics_numpy(errors, obs_errors, reward_errors, penalties, term_pred, term_data, lengths,
                            penalty_learned_var=True, penalty_kind=None):
    """The same [K + 1, 16] table from the per-segment host arrays ([K, B]; ``lengths`` [B]): what the device
    reduction must equal.  Entry (k, b) counts when k < lengths[b]; the penalty is compared with ``errors`` for
    the learned-variance penalty (a norm over all outputs) and with ``obs_errors`` for the mean-distance one (a
    norm over the obs dims); ``penalty_kind`` names any of ``fake_env.PENALTY_KINDS`` instead (ensemble_std with
    ``errors``, max_pairwise with ``obs_errors``).  The correlation is 0 for fewer than two entries or a zero variance; a row
    without entries is all zero."""
    e, eo = np.asarray(errors, np.float64), np.asarray(obs_errors, np.float64)
    er, u = np.asarray(reward_errors, np.float64), np.asarray(penalties, np.float64)
    tp, td = np.asarray(term_pred), np.asarray(term_data)
    K, B = e.shape
    live = np.arange(K)[:, None] < np.asarray(lengths).reshape(1, B)
    if penalty_kind is not None:
        from .fake_env import penalty_kind_id
        penalty_learned_var = penalty_kind_id(penalty_kind) in (1, 3)   # the kinds over all D outputs
    es = e if penalty_learned_var else eo
    table = np.zeros((K + 1, 16))
    for k in range(K + 1):
        m = live[k] if k < K else live          # row K: k-major, then b -- the boolean mask's own order
        sel = (lambda x: x[k][m]) if k < K else (lambda x: x[m])
        n = int(m.sum())
        if n == 0:
            continue
        ek, uk, sk = sel(e), sel(u), sel(es)
        du, ds = uk - uk.mean(), sk - sk.mean()
        vu, vs = float(np.sum(du * du)), float(np.sum(ds * ds))
        corr = 0.0 if n < 2 or vu == 0.0 or vs == 0.0 else float(np.sum(du * ds)) / np.sqrt(vu * vs)
        table[k, :11] = (n, ek.mean(), ek.std(), ek.max(), sel(eo).mean(), np.abs(sel(er)).mean(), uk.mean(),
                         uk.std(), corr, np.mean(uk >= sk), np.mean(sel(tp) != sel(td)))
    return table


def segment_lengths_numpy(obs, next_obs, terminals, size, start, K):
    """The continuation rule of the open-loop validation on the host: for each start row, ``(lengths,
    end_reasons)`` of a segment of at most K steps over pool rows [0, size).  After step k (row j = start + k):
    reason 0 (``END_REASONS``) when k + 1 == K, else 1 when ``terminals[j]``, else 3 when j + 1 >= size, else 2
    when ``obs[j + 1]`` differs from ``next_obs[j]`` in any 32-bit pattern (a timeout boundary of a D4RL
    qlearning_dataset, or a wrapped pool's seam; NaN cannot fool it), else the segment goes on.  A start outside
    [0, size) takes no step: length 0, reason 3."""
    o = np.ascontiguousarray(obs, np.float32).view(np.uint32)
    no = np.ascontiguousarray(next_obs, np.float32).view(np.uint32)
    t = np.asarray(terminals).reshape(-1) != 0
    start = np.asarray(start, np.int64).reshape(-1)
    lengths, ends = np.zeros(start.size, np.int32), np.zeros(start.size, np.uint8)
    for b, r in enumerate(start):
        if r < 0 or r >= size:
            ends[b] = 3
            continue
        for k in range(K):
            j = int(r) + k
            lengths[b] = k + 1
            if k + 1 == K:
                ends[b] = 0
            elif t[j]:
                ends[b] = 1
            elif j + 1 >= size:
                ends[b] = 3
            elif np.any(o[j + 1] != no[j]):
                ends[b] = 2
            else:
                continue
            break
    return lengths, ends
