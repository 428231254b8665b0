"""simple_run-style driver (simple_run/main.py:146-225) for the MI355X path.

    python -m mopo_amd.run --config examples.config.d4rl.halfcheetah_mixed \
        --data halfcheetah-medium-replay-v0.npz --model-dir models/ --epochs 10

``--data``: local qlearning_dataset arrays (d4rl downloads are unavailable offline).
``--model-dir``: directory holding '<model_name>.mat' (bnn.py:276-281); without it the ensemble
is trained from its initial weights to early stopping first (mopo.py:526-531).
``--ensemble-dtype`` / ``--actor-dtype``: the forward arithmetic (mopo_amd.bnn.DTYPES).
``--model-eval-episodes`` / ``--model-eval-length``: evaluate the policy inside the learned model after every
epoch (``model_eval/*``: the return under the model, not a D4RL score); off by default.
``--model-val-segments`` / ``--model-val-horizon``: replay dataset trajectories open-loop through the trained
model (``model/open_loop/*``: the compounding error and the penalty's calibration); off by default.
``--penalty-kind``: the reward penalty (mopo_amd.fake_env.PENALTY_KINDS); default: the config's choice.
``--halt-threshold`` or ``--halt-quantile``, with ``--halt-reward``: hard truncation of the model rollouts where
the penalty exceeds the threshold (given, or that quantile of the penalty over the dataset); off by default.
"""
import argparse
import json

from .bnn import DEFAULT_ENSEMBLE_DTYPE, DTYPES
from .fake_env import PENALTY_KINDS


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--config', required=True)
    p.add_argument('--data', required=True)
    p.add_argument('--model-dir', default=None)
    p.add_argument('--epochs', type=int, default=None)
    p.add_argument('--seed', type=int, default=88)                 # simple_run/base.py run_params
    p.add_argument('--ensemble-dtype', default=None, choices=DTYPES,
                   help='ensemble forward arithmetic (default: the config kwarg ensemble_dtype, else %s)'
                        % DEFAULT_ENSEMBLE_DTYPE)
    p.add_argument('--actor-dtype', default=None, choices=('fp32', 'bf16x6', 'f16x3'),
                   help='rollout policy forward (default: the ensemble dtype for fp32 and bf16x6, else f16x3)')
    p.add_argument('--model-eval-episodes', type=int, default=None,
                   help='episodes of the policy inside the learned model after every epoch (model_eval/* keys; '
                        'default: the config kwarg model_eval_episodes, else 0 = none)')
    p.add_argument('--model-eval-length', type=int, default=None,
                   help='step cap of those episodes, <= 4095 (default: max_path_length)')
    p.add_argument('--model-val-segments', type=int, default=None,
                   help='dataset segments replayed open-loop through the trained model (model/open_loop/* keys; '
                        'default: the config kwarg model_val_segments, else 0 = none)')
    p.add_argument('--model-val-horizon', type=int, default=None,
                   help='step cap of those segments, <= 4095 (default: rollout_length)')
    p.add_argument('--penalty-kind', default=None, choices=PENALTY_KINDS,
                   help='the reward penalty u of r - penalty_coeff * u (default: the config kwarg penalty_kind, else '
                        'by its penalty_learned_var: max_aleatoric / mean_distance)')
    p.add_argument('--halt-threshold', type=float, default=None,
                   help='hard truncation: a model transition whose penalty exceeds this is terminal with --halt-reward')
    p.add_argument('--halt-quantile', type=float, default=None,
                   help='... the threshold as this quantile (0 < q <= 1) of the penalty over the dataset instead')
    p.add_argument('--halt-reward', type=float, default=None, help='the reward of a halted transition, e.g. -100')
    a = p.parse_args(argv)
    from .config import DIMS, get_params
    from .loader import restore_pool
    from .mopo import from_config
    from .replay_pool import SimpleReplayPool
    from .static import static_fns
    params = get_params(a.config)
    obs_dim, act_dim = DIMS[params['domain']]
    pool = SimpleReplayPool(obs_dim=obs_dim, act_dim=act_dim, max_size=int(1e6))   # simple_run/base.py:267-272
    restore_pool(pool, a.data)
    over = {k: v for k, v in (('ensemble_dtype', a.ensemble_dtype), ('actor_dtype', a.actor_dtype),
                              ('penalty_kind', a.penalty_kind)) if v}
    over.update((k, v) for k, v in (('model_eval_episodes', a.model_eval_episodes),
                                    ('model_eval_length', a.model_eval_length),
                                    ('model_val_segments', a.model_val_segments),
                                    ('model_val_horizon', a.model_val_horizon),
                                    ('halt_threshold', a.halt_threshold), ('halt_quantile', a.halt_quantile),
                                    ('halt_reward', a.halt_reward)) if v is not None)
    algo = from_config(params, pool, static_fns[params['domain']], model_load_dir=a.model_dir, seed=a.seed, **over)
    for diag in algo.train(a.epochs):
        print(json.dumps({k: float(v) for k, v in diag.items()}), flush=True)


if __name__ == '__main__':
    main()
