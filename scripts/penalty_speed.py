"""The cost of the penalty kinds on the training rollout: the C2 workload (halfcheetah, E = 7, H = 200, 50k rows,
horizon 5, bf16x6), penalty_coeff = 1, each of the four kinds in this process.  Whole-rollout transitions/s over
ROUNDS rounds that alternate the kinds (each timed window REPS rollouts, ending in a device synchronise), after a
warm-up of every kind; then, in a run of its own with the live per-kernel timing on (one stream, no split), the
ensemble launch's and the penalty kernel's time per launch.  The comparison is each new kind against
max_aleatoric on the same tree (DESIGN 4 quotes the medians).
Raw JSON lines to $MOPO_OUT/penalty_speed.txt (default bench_out/):  python scripts/penalty_speed.py"""
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
from mopo_amd.fake_env import PENALTY_KINDS
from mopo_amd.replay_pool import SimpleReplayPool
from mopo_amd.rollout import ModelRollout, init_sac_params

B, T, O, A = 50000, 5, 17, 6
ROUNDS, REPS = 5, 100
KC = ('start', 'actor', 'ensemble', 'post', 'compact', 'advance', 'penalty')
lines = []


def emit(**kw):
    lines.append(json.dumps(kw))
    print(lines[-1], flush=True)


rs = np.random.RandomState(0)
env = torch.from_numpy(rs.normal(size=(100000, O)).astype(np.float32)).cuda()
pi = torch.from_numpy(init_sac_params(O, A)).cuda()
model = construct_model(obs_dim=O, act_dim=A, hidden_dim=200, num_networks=7, num_elites=5, separate_mean_var=True,
                        seed=0, dtype='bf16x6')
model.set_elites([0, 1, 2, 3, 4])
ro = ModelRollout(model, B, T)
pool = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=B * T)


def rollout(kind, epoch):
    return ro.run(env, pi, pool, B, T, 0, 1.0, [0, 1, 2, 3, 4], seed=1, epoch=epoch, penalty_kind=kind)


for kind in PENALTY_KINDS:   # warm-up: allocations (mean_all / std_all on first use), code objects, clocks
    for rep in range(3):
        rollout(kind, rep)
torch.cuda.synchronize()

rates = {k: [] for k in PENALTY_KINDS}
for rnd in range(ROUNDS):
    for kind in PENALTY_KINDS:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for rep in range(REPS):
            rollout(kind, rnd * REPS + rep)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rates[kind].append(B * T * REPS / dt)
        emit(what='rollout', kind=kind, round=rnd, seconds=dt, transitions_per_s=rates[kind][-1])
base = float(np.median(rates['max_aleatoric']))
for kind in PENALTY_KINDS:
    r = rates[kind]
    emit(what='rollout summary', kind=kind, median=float(np.median(r)), min=min(r), max=max(r),
         median_vs_max_aleatoric=float(np.median(r)) / base)

# per-kernel times (profiling runs one stream and records events around every launch: not the rates above)
for kind in PENALTY_KINDS:
    for rep in range(3):
        L.check(L.lib().mopo_rollout_profile(ro._h, 1))
        rollout(kind, rep)
        ms = (C.c_double * len(KC))()
        n = (C.c_int64 * len(KC))()
        L.check(L.lib().mopo_rollout_profile_read(ro._h, ms, n, len(KC)))
        L.check(L.lib().mopo_rollout_profile(ro._h, 0))
        emit(what='kernels, one stream', kind=kind, rep=rep, launches={k: int(n[i]) for i, k in enumerate(KC)},
             us_per_launch={k: (ms[i] / n[i] * 1e3 if n[i] else None) for i, k in enumerate(KC)})

out = os.environ.get('MOPO_OUT', 'bench_out')
os.makedirs(out, exist_ok=True)
open(os.path.join(out, 'penalty_speed.txt'), 'w').write('\n'.join(lines) + '\n')
