"""Fused model evaluation against the host loop DevicePolicy.actions + FakeEnv.step: halfcheetah, E = 7, H = 200,
1024 episodes x 1000 steps, bf16x6; three timed runs of each after a warm-up, in this process (DESIGN 4 quotes
the best).  Also the training rollout's per-kernel times at the same 1024 rows (the ensemble launch alone).
Raw JSON lines to $MOPO_OUT/model_eval_speed.txt (default bench_out/):  python scripts/model_eval_speed.py"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mopo_amd import _lib as L
from mopo_amd.bnn import construct_model
from mopo_amd.evaluation import DevicePolicy
from mopo_amd.fake_env import FakeEnv
from mopo_amd.replay_pool import SimpleReplayPool
from mopo_amd.rollout import ModelRollout, init_sac_params
from mopo_amd.static import static_fns

B, T, O, A = 1024, 1000, 17, 6
lines = []


def emit(**kw):
    lines.append(json.dumps(kw))
    print(lines[-1], flush=True)


rs = np.random.RandomState(0)
env_np = rs.normal(size=(20000, O)).astype(np.float32)
env = torch.from_numpy(env_np).cuda()
pi = torch.from_numpy(init_sac_params(O, A)).cuda()
model = construct_model(obs_dim=O, act_dim=A, hidden_dim=200, num_networks=7, num_elites=5, separate_mean_var=True,
                        seed=0, dtype='bf16x6')
model.set_elites([0, 1, 2, 3, 4])
ro = ModelRollout(model, B, 5)

# fused
for rep in range(4):   # the first is the warm-up (allocations, clocks)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = ro.evaluate(env, pi, B, T, 0, 1.0, [0, 1, 2, 3, 4], seed=1, epoch=rep)
    stats = out['stats'].cpu().numpy()
    dt = time.perf_counter() - t0
    emit(what='fused evaluate', rep=rep, warmup=rep == 0, seconds=dt, us_per_step=dt / T * 1e6,
         return_average=float(stats[0]), length_avg=float(stats[4]))

# the ensemble kernel alone at these 1024 rows (live per-kernel timing of a 5-step training rollout)
pool = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=B * 5)
for rep in range(3):
    L.check(L.lib().mopo_rollout_profile(ro._h, 1))
    ro.run(env, pi, pool, B, 5, 0, 1.0, [0, 1, 2, 3, 4], seed=1, epoch=rep)
    ms = (C.c_double * 6)()
    n = (C.c_int64 * 6)()
    L.check(L.lib().mopo_rollout_profile_read(ro._h, ms, n, 6))
    L.check(L.lib().mopo_rollout_profile(ro._h, 0))
    emit(what='training rollout kernels, 1024 rows', rep=rep,
         us_per_launch={k: (ms[i] / n[i] * 1e3 if n[i] else None)
                        for i, k in enumerate(('start', 'actor', 'ensemble', 'post', 'compact', 'advance'))})

# host loop: what the parent offers
fe = FakeEnv(model, static_fns['halfcheetah'], penalty_coeff=1.0, penalty_learned_var=True)
policy = DevicePolicy(pi, O, A, 256, deterministic=True, dtype=3)
for rep in range(4):
    np.random.seed(rep)
    obs = env_np[np.random.randint(0, len(env_np), B)]
    ret = np.zeros(B)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(T):
        act = policy.actions(obs)
        obs, rew, term, info = fe.step(obs, act)
        ret += np.asarray(info['unpenalized_rewards']).ravel()
    dt = time.perf_counter() - t0
    emit(what='host loop DevicePolicy.actions + FakeEnv.step', rep=rep, warmup=rep == 0, seconds=dt,
         us_per_step=dt / T * 1e6, return_average=float(ret.mean()))

out = os.environ.get('MOPO_OUT', 'bench_out')
os.makedirs(out, exist_ok=True)
open(os.path.join(out, 'model_eval_speed.txt'), 'w').write('\n'.join(lines) + '\n')
