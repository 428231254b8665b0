"""Fused model rollout: ``MOPO._rollout_model`` (mopo/algorithms/mopo.py:723-765) on one GPU.

``ModelRollout.run`` launches the whole horizon (actor -> ensemble -> FakeEnv post -> compaction
-> pool append, csrc/rollout.hip) on the current stream with no host synchronisation; the
transitions land in a device ``SimpleReplayPool`` in the reference's order.  Two RNG modes:

* ``perf`` (default): Philox on the device (start rows, policy noise, member choice, obs noise).
* ``parity``: every stream injected -- start rows, TF policy noise ``eps_act`` and the numpy
  FakeEnv draws (the selected member's noise and the member index per row), so the result can be
  compared to the reference for identical inputs.
"""
import ctypes as C
import os

import numpy as np

from . import _lib as L


def hidden_pair(H):
    """The two hidden widths of the policy / Q MLPs (mopo.py:275-280, 311-325: ``hidden_sizes``): an int
    H means [H, H]."""
    if isinstance(H, (int, np.integer)):
        return int(H), int(H)
    hs = [int(x) for x in H]
    if len(hs) != 2 or min(hs) < 1:
        raise NotImplementedError('policy / Q hidden_sizes must be two widths [H1, H2] (got %r)' % (H,))
    return hs[0], hs[1]


def device_hidden(H):
    """The square width the device kernels run a [H1, H2] network at: max(H1, H2) rounded up to 16.
    A narrower layer is embedded with zero weights and biases, which is exact for the relu MLPs: a
    padded unit is relu(0) = 0 forward, its relu mask is off backward, so its weights' gradients, Adam
    moments and updates stay exactly 0 (and the Polyak average of zeros is 0)."""
    h1, h2 = hidden_pair(H)
    return (max(h1, h2) + 15) // 16 * 16


def sac_param_shapes(O, A, H=256):
    """Creation order of get_vars('main') (mopo.py:32-33, 298-324): pi, q1, q2 in TF [in,out] layout;
    ``H`` an int or [H1, H2]."""
    h1, h2 = hidden_pair(H)
    pi = [(O, h1), (h1,), (h1, h2), (h2,), (h2, A), (A,), (h2, A), (A,)]
    q = [(O + A, h1), (h1,), (h1, h2), (h2,), (h2, 1), (1,)]
    return pi + q + q


def init_sac_params(O, A, H=256, seed=2):
    """tf.layers.dense defaults: glorot_uniform kernels, zero biases; returns a flat float32 array in
    the [H1, H2] network's own layout."""
    rng = np.random.RandomState(seed)
    parts = []
    for shp in sac_param_shapes(O, A, H):
        if len(shp) == 2:
            lim = np.sqrt(6.0 / (shp[0] + shp[1]))
            parts.append(rng.uniform(-lim, lim, size=shp).astype(np.float32).ravel())
        else:
            parts.append(np.zeros(shp, np.float32))
    flat = np.concatenate(parts)
    if hidden_pair(H)[0] == hidden_pair(H)[1]:
        assert flat.size == L.lib().mopo_sac_param_count(O, A, hidden_pair(H)[0])
    return flat


def sac_pad_index(O, A, H):
    """Positions of a [H1, H2] network's flat parameters inside the flat layout of the square
    device_hidden(H) network (each tensor's [:rows, :cols] corner); None when H is already square."""
    h1, h2 = hidden_pair(H)
    hd = device_hidden(H)
    if h1 == h2 == hd:
        return None
    idx, off = [], 0
    for ls, ds in zip(sac_param_shapes(O, A, (h1, h2)), sac_param_shapes(O, A, hd)):
        if len(ls) == 2:
            idx.append((off + np.arange(ls[0])[:, None] * ds[1] + np.arange(ls[1])[None, :]).ravel())
        else:
            idx.append(off + np.arange(ls[0]))
        off += int(np.prod(ds))
    return np.concatenate(idx).astype(np.int64)


def split_params(flat, O, A, H=256):
    out, off = [], 0
    for shp in sac_param_shapes(O, A, H):
        n = int(np.prod(shp))
        out.append(flat[off:off + n].reshape(shp))
        off += n
    return out


_ACTOR_DTYPES = {'fp32': 0, 'bf16x6': 3, 'f16x3': 4}


def default_actor_dtype(ensemble_dtype):
    """The rollout policy's arithmetic for an ensemble dtype: the exact-operand forms beside the exact-operand
    ensembles -- f32 MFMA beside fp32, the exact bf16x6 split beside bf16x6 -- so the whole rollout computes on
    the reference's f32 operands; else the f16x3 actor (~22-bit operands on the f16 MFMA, held to the fp32
    actor tolerances) beside the reduced-operand ensembles (f16x3, bf16x3, bf16)."""
    return ensemble_dtype if ensemble_dtype in ('fp32', 'bf16x6') else 'f16x3'


class ModelRollout:
    """Owns the rollout workspace for up to ``max_batch`` rows x ``max_horizon`` steps."""

    def __init__(self, model, max_batch, max_horizon=32):
        self.model = model
        self.max_batch, self.max_horizon = int(max_batch), int(max_horizon)
        h = C.c_void_p()
        L.check(L.lib().mopo_rollout_create(C.byref(h), model.handle, self.max_batch, self.max_horizon))
        self._h = h

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and h.value:
            L.lib().mopo_rollout_destroy(h)
            self._h = None

    def run(self, env_obs, pi_params, pool, batch_size, horizon, term_kind, penalty_coeff, elites,
            seed=0, epoch=0, pi_hidden=256, start_idx=None, eps_act=None, eps_obs=None, model_inds=None,
            staged=False, uid_offset=0, stream=None, step_desc=None, step_hook=None, penalty_learned_var=True,
            deterministic=False, rollout_random=False, act_uniform=None, actor_dtype=None, penalty_kind=None,
            halt_threshold=None, halt_reward=None):
        """Returns the device int64[horizon] tensor of rows added per step (steps_added).
        ``halt_threshold`` / ``halt_reward``: hard truncation (``fake_env.halt_fields``; None: off) -- a row whose
        penalty is not <= the threshold enters the pool terminal with the reward ``halt_reward`` and is dropped by
        the compaction, which then runs for the never-done domains too; the rows halted per step are left in
        ``self.last_halted`` (device int64[horizon]; None when off).
        ``step_desc(i)`` / ``step_hook(i, steps)``: per-step staging (see mopo_rollout_run_staged_steps).
        ``penalty_learned_var`` / ``deterministic``: FakeEnv's modes (fake_env.py:69-110; every D4RL
        config uses the learned-var penalty, not deterministic); ``rollout_random``: uniform actions
        (mopo.py:736-738), ``act_uniform`` [horizon, B, A] injects them in parity mode.
        ``actor_dtype``: 'fp32', 'bf16x6' or 'f16x3' policy forward (default: default_actor_dtype).
        ``penalty_kind``: one of ``fake_env.PENALTY_KINDS`` (None: by ``penalty_learned_var``); 'max_pairwise'
        and 'ensemble_std' run csrc/penalty.hip behind every ensemble launch when ``penalty_coeff`` != 0."""
        import torch
        dev = env_obs.device
        B = int(batch_size)
        # every steps[i], i < horizon, is stored by the rollout's advance kernels when B > 0 (no fill launch);
        # the elites' device copy is kept while they stay the same (no H2D copy per rollout)
        legacy = os.environ.get('MOPO_ROLLOUT_FILL') == '1'                       # A/B knob: the old launches
        alloc = torch.empty if (B > 0 and int(horizon) > 0 and not legacy) else torch.zeros
        steps = alloc(max(horizon, 1), dtype=torch.int64, device=dev)
        keep = [steps]
        args = self._args(keep, env_obs, pi_params, B, horizon, term_kind, penalty_coeff, elites, seed, epoch,
                          pi_hidden, start_idx, eps_act, eps_obs, model_inds, uid_offset, steps, penalty_learned_var,
                          deterministic, rollout_random, act_uniform, actor_dtype, legacy, penalty_kind=penalty_kind,
                          halt=(halt_threshold, halt_reward))
        self.last_halted = None
        if args.halt:
            self.last_halted = torch.zeros(max(horizon, 1), dtype=torch.int64, device=dev)[:horizon]
            keep.append(self.last_halted)
            args.d_halted = L.ptr(self.last_halted)
        if step_hook is not None:
            # one call per horizon step into the staging block step_hook(i) names; step_hook(i, steps)
            # is then called after step i is enqueued (multi-GPU: gather step i while i + 1 computes)
            for i in range(int(horizon)):
                L.check(L.lib().mopo_rollout_run_staged_steps(self._h, args, step_desc(i), i, i + 1,
                                                              L.stream_ptr(stream)))
                step_hook(i, steps)
            self._keepalive = keep
            return steps[:horizon]
        desc = pool.desc() if not isinstance(pool, L.PoolDesc) else pool
        fn = L.lib().mopo_rollout_run_staged if staged else L.lib().mopo_rollout_run
        L.check(fn(self._h, args, desc, L.stream_ptr(stream)))
        self._keepalive = keep
        return steps[:horizon]

    def _args(self, keep, env_obs, pi_params, B, horizon, term_kind, penalty_coeff, elites, seed, epoch, pi_hidden,
              start_idx, eps_act, eps_obs, model_inds, uid_offset, steps, penalty_learned_var, deterministic,
              rollout_random, act_uniform, actor_dtype, fresh_elites=False, penalty_kind=None, halt=(None, None)):
        """The C ABI's mopo_rollout_args; every tensor it points to is appended to ``keep``."""
        import torch
        from .fake_env import halt_fields, penalty_kind_id
        halt = halt_fields(*halt)
        # a named kind wins over run()'s default penalty_learned_var=True (only FakeEnv refuses a contradiction)
        kind = penalty_kind_id(penalty_kind, None if penalty_kind is not None else penalty_learned_var)
        dev = env_obs.device
        ekey = (tuple(int(e) for e in np.asarray(elites).ravel()), str(dev))
        if getattr(self, '_elites', (None, None))[0] != ekey or fresh_elites:
            self._elites = (ekey, torch.as_tensor(np.asarray(elites, np.int32)).to(dev))
        el = self._elites[1]
        keep.append(el)

        def dptr(x, dt):
            if x is None:
                return None
            t = torch.as_tensor(x).to(dev, dt).contiguous()
            keep.append(t)
            return L.ptr(t)

        return L.RolloutArgs(
            d_env_obs=L.ptr(env_obs), env_size=int(env_obs.shape[0]), d_start_idx=dptr(start_idx, torch.int64),
            d_pi_params=pi_params if isinstance(pi_params, int) else L.ptr(pi_params), pi_hidden=int(pi_hidden), d_elites=L.ptr(el), n_elites=int(el.numel()),
            B=B, horizon=int(horizon), penalty_coeff=float(penalty_coeff), term_kind=int(term_kind),
            seed=int(seed) & (2 ** 64 - 1), epoch=int(epoch), uid_offset=int(uid_offset),
            d_eps_act=dptr(eps_act, torch.float32), d_eps_obs=dptr(eps_obs, torch.float64),
            d_model_inds=dptr(model_inds, torch.int32), d_steps=L.ptr(steps),
            penalty_learned_var=kind, deterministic=int(bool(deterministic)),
            rollout_random=int(bool(rollout_random)), d_act_uniform=dptr(act_uniform, torch.float32),
            actor_dtype=_ACTOR_DTYPES[actor_dtype or default_actor_dtype(self.model.dtype)],
            halt=halt[0], halt_threshold=halt[1], halt_reward=halt[2])

    def penalty_profile(self, pool, kind, n_rows=None, stream=None):
        """``u(observations[j], actions[j])`` of penalty ``kind`` (a name of ``fake_env.PENALTY_KINDS`` or its id)
        for the first ``n_rows`` rows of ``pool`` (a ``SimpleReplayPool``, default: its ``size`` rows; or a
        ``PoolDesc`` with ``n_rows`` given): a device f32[n_rows] tensor, computed in chunks of ``max_batch`` on
        the current stream (csrc/penalty_profile.hip) -- the distribution a ``halt_threshold`` is calibrated on
        (``evaluation.halt_threshold_from_quantile``).  Nothing is drawn; the pool is only read."""
        import torch
        from .fake_env import penalty_kind_id
        desc = pool.desc() if not isinstance(pool, L.PoolDesc) else pool
        dev = pool._state.device if hasattr(pool, '_state') else torch.device('cuda')
        n = int(pool.size if n_rows is None else n_rows)
        u = torch.empty(max(n, 0), dtype=torch.float32, device=dev)
        L.check(L.lib().mopo_rollout_penalty_profile(self._h, desc, n, penalty_kind_id(kind), L.ptr(u),
                                                     L.stream_ptr(stream)))
        return u

    def evaluate(self, env_obs, pi_params, n_episodes, max_length, term_kind, penalty_coeff, elites,
                 policy_deterministic=True, seed=0, epoch=0, pi_hidden=256, start_idx=None, eps_act=None,
                 eps_obs=None, model_inds=None, uid_offset=0, stream=None, penalty_learned_var=True,
                 deterministic=False, rollout_random=False, act_uniform=None, actor_dtype=None, penalty_kind=None,
                 halt_threshold=None, halt_reward=None):
        """Model-based policy evaluation (csrc/rollout_eval.hip): ``n_episodes`` episodes of at most
        ``max_length`` <= 4095 steps of the policy inside the learned model, from env-pool start states, on the
        current stream; nothing enters a pool and numpy's global stream is not drawn from.
        ``policy_deterministic``: tanh(mu) actions (the evaluation policy, mopo.py:481-482), else sampled --
        then the episodes are the trajectories ``run`` visits for the same arguments.  The other arguments
        are ``run``'s; the penalty sums and penalized returns are of the selected ``penalty_kind``.  Returns device tensors: ``returns`` (unpenalized), ``penalized_returns``,
        ``penalty_sums`` (f64[n]), ``lengths`` (i32[n]), ``terminated`` (u8[n]; ended by the termination rule), ``halted`` (u8[n]; ended by ``halt_threshold`` /
        ``halt_reward``, ``run``'s hard truncation -- zeros when off), ``steps`` (int64[max_length] live
        episodes per step) and ``stats`` (f64[16], see ``evaluation.model_evaluation_metrics``).  These are
        returns under the model: biased wherever the model is wrong."""
        import torch
        dev = env_obs.device
        n, T = int(n_episodes), int(max_length)
        out = {'returns': torch.zeros(n, dtype=torch.float64, device=dev),
               'penalized_returns': torch.zeros(n, dtype=torch.float64, device=dev),
               'penalty_sums': torch.zeros(n, dtype=torch.float64, device=dev),
               'lengths': torch.zeros(n, dtype=torch.int32, device=dev),
               'terminated': torch.zeros(n, dtype=torch.uint8, device=dev),
               'halted': torch.zeros(n, dtype=torch.uint8, device=dev),
               'steps': torch.zeros(max(T, 1), dtype=torch.int64, device=dev),
               'stats': torch.zeros(16, dtype=torch.float64, device=dev)}
        keep = list(out.values())
        args = self._args(keep, env_obs, pi_params, n, T, term_kind, penalty_coeff, elites, seed, epoch, pi_hidden,
                          start_idx, eps_act, eps_obs, model_inds, uid_offset, out['steps'], penalty_learned_var,
                          deterministic, rollout_random, act_uniform, actor_dtype, penalty_kind=penalty_kind,
                          halt=(halt_threshold, halt_reward))
        ev = L.EvalArgs(policy_deterministic=int(bool(policy_deterministic)), d_return=L.ptr(out['returns']),
                        d_pen_return=L.ptr(out['penalized_returns']), d_pen_sum=L.ptr(out['penalty_sums']),
                        d_length=L.ptr(out['lengths']), d_terminated=L.ptr(out['terminated']),
                        d_stats=L.ptr(out['stats']), d_halted=L.ptr(out['halted']))
        L.check(L.lib().mopo_rollout_evaluate(self._h, args, ev, L.stream_ptr(stream)))
        self._keepalive = keep
        return out

    def validate(self, pool, n_segments, horizon, term_kind, elites, seed=0, epoch=0, start_idx=None, eps_obs=None,
                 model_inds=None, uid_offset=0, stream=None, penalty_learned_var=True, deterministic=True,
                 penalty_kind=None):
        """Open-loop model validation (csrc/rollout_val.hip): ``n_segments`` segments of at most ``horizon`` <=
        4095 steps, each from a row of ``pool`` (a ``SimpleReplayPool`` or a ``PoolDesc``), replaying the
        DATASET's actions through the model on the model's own predicted states and comparing every step with
        the row's ``next_observations`` / ``rewards``.  A segment stops with the data: at a terminal flag (end
        reason 1), where ``observations[j + 1]`` is not bit for bit ``next_observations[j]`` (2: an episode
        boundary without a flag), at the pool's last valid row (3), or after ``horizon`` steps (0).  The policy
        is never run, the pool is only read and numpy's global stream is not drawn from.  ``deterministic``
        (the default here): the mean over all members, no sampling.  Returns device tensors: ``errors``,
        ``obs_errors``, ``reward_errors`` (f64[horizon, n]; NaN past a segment's length), ``penalties``
        (f32[horizon, n]), ``term_pred`` / ``term_data`` (u8[horizon, n]; 0xFF past the length), ``lengths``
        (i32[n]), ``end_reasons`` (u8[n]), ``start_rows`` (int64[n]), ``steps`` (int64[horizon] live segments per step) and ``stats``
        (f64[horizon + 1, 16], see ``evaluation.open_loop_metrics``).  ``penalty_kind`` (one of
        ``fake_env.PENALTY_KINDS``, None: by ``penalty_learned_var``) selects the penalty of ``penalties`` and of
        the statistics; call once per kind on the same segments to compare them.  A pool holding the model's own training
        rows gives an in-distribution, optimistic curve; pass unseen trajectories for a held-out one."""
        import torch
        desc = pool.desc() if not isinstance(pool, L.PoolDesc) else pool
        dev = pool._state.device if hasattr(pool, '_state') else torch.device('cuda')
        n, K = int(n_segments), int(horizon)
        kk = max(K, 1)
        f64 = dict(dtype=torch.float64, device=dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        out = {'errors': torch.full((kk, n), float('nan'), **f64),
               'obs_errors': torch.full((kk, n), float('nan'), **f64),
               'reward_errors': torch.full((kk, n), float('nan'), **f64),
               'penalties': torch.full((kk, n), float('nan'), dtype=torch.float32, device=dev),
               'term_pred': torch.full((kk, n), 255, **u8),
               'term_data': torch.full((kk, n), 255, **u8),
               'lengths': torch.zeros(n, dtype=torch.int32, device=dev),
               'end_reasons': torch.zeros(n, **u8),
               'start_rows': torch.full((n,), -1, dtype=torch.int64, device=dev),
               'steps': torch.zeros(kk, dtype=torch.int64, device=dev),
               'stats': torch.zeros((kk + 1, 16), **f64)}
        keep = list(out.values())
        # the policy / env-obs / penalty_coeff fields are ignored by the entry point: any device tensor names the
        # device for _args, and its pointers to it are dropped again below
        args = self._args(keep, out['stats'], 0, n, K, term_kind, 0.0, elites, seed, epoch, 0, start_idx, None,
                          eps_obs, model_inds, uid_offset, out['steps'], penalty_learned_var, deterministic, False,
                          None, 'fp32', penalty_kind=penalty_kind)
        args.d_env_obs, args.env_size, args.d_steps = None, 0, None
        va = L.ValArgs(d_err=L.ptr(out['errors']), d_err_obs=L.ptr(out['obs_errors']),
                       d_err_rew=L.ptr(out['reward_errors']), d_pen=L.ptr(out['penalties']),
                       d_term_pred=L.ptr(out['term_pred']), d_term_data=L.ptr(out['term_data']),
                       d_length=L.ptr(out['lengths']), d_end=L.ptr(out['end_reasons']),
                       d_start=L.ptr(out['start_rows']), d_steps=L.ptr(out['steps']),
                       d_stats=L.ptr(out['stats']))
        L.check(L.lib().mopo_rollout_validate(self._h, args, desc, va, L.stream_ptr(stream)))
        self._keepalive = keep
        return out
