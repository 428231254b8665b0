"""Fused open-loop validation against the host loop that does the same work with the public FakeEnv.step plus torch
gathers: halfcheetah shape, E = 7, H = 200, bf16x6, 4096 segments x 20 steps, deterministic, learned-variance
penalty.  hipEvents around each, best of 3 after a warm-up (DESIGN 4 quotes both).  The pool is one long chain
with a terminal every 1000 rows, so nearly every segment runs all 20 steps in both forms.
Raw JSON lines to $MOPO_OUT/open_loop_speed.txt (default bench_out/):  python scripts/open_loop_speed.py"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mopo_amd.bnn import construct_model
from mopo_amd.fake_env import FakeEnv
from mopo_amd.replay_pool import SimpleReplayPool
from mopo_amd.rollout import ModelRollout
from mopo_amd.static import static_fns

B, K, O, A, N = 4096, 20, 17, 6, 100000
lines = []


def emit(**kw):
    lines.append(json.dumps(kw))
    print(lines[-1], flush=True)


rs = np.random.RandomState(0)
chain = (rs.normal(size=(1, O)) + np.cumsum(rs.normal(size=(N + 1, O)) * 0.02, 0)).astype(np.float32)
term = np.zeros((N, 1), bool)
term[999::1000] = True
pool = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=N)
pool.add_samples({'observations': chain[:-1], 'actions': rs.uniform(-1, 1, (N, A)), 'rewards': rs.normal(size=(N, 1)),
                  'terminals': term, 'next_observations': chain[1:]})
model = construct_model(obs_dim=O, act_dim=A, hidden_dim=200, num_networks=7, num_elites=5, separate_mean_var=True,
                        seed=0, dtype='bf16x6')
model.set_elites([0, 1, 2, 3, 4])
ro = ModelRollout(model, B, 1)
start = torch.from_numpy(rs.randint(0, N, B)).cuda()
ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fn):
    torch.cuda.synchronize()
    ev0.record()
    out = fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1), out


def fused():
    return ro.validate(pool, B, K, 0, [0, 1, 2, 3, 4], start_idx=start)


fe = FakeEnv(model, static_fns['halfcheetah'], penalty_coeff=1.0, penalty_learned_var=True)
F = pool.fields


def host_loop():
    """The same segments with the public pieces: per step one gather of the live rows' actions / targets, one
    FakeEnv.step on device tensors, the errors and the continuation rule in torch."""
    ids = torch.arange(B, device='cuda')
    obs = F['observations'][start].double()
    err = torch.full((K, B), float('nan'), dtype=torch.float64, device='cuda')
    pen = torch.full((K, B), float('nan'), dtype=torch.float32, device='cuda')
    for k in range(K):
        j = start[ids] + k
        nobs, _, _, info = fe.step(obs, F['actions'][j], deterministic=True)
        eo = (nobs - F['next_observations'][j].double()).norm(dim=1)
        er = info['unpenalized_rewards'][:, 0] - F['rewards'][j, 0].double()
        err[k, ids], pen[k, ids] = torch.hypot(eo, er), info['penalty'][:, 0]
        nxt = (j + 1).clamp(max=N - 1)
        go = (j + 1 < N) & ~F['terminals'][j, 0] & \
            (F['observations'][nxt].view(torch.int32) == F['next_observations'][j].view(torch.int32)).all(1)
        ids, obs = ids[go], nobs[go]
        if ids.numel() == 0:
            break
    return err, pen


for name, fn in (('fused validate', fused), ('host loop FakeEnv.step + torch gathers', host_loop)):
    best = None
    for rep in range(4):   # the first is the warm-up (allocations, clocks)
        ms, out = timed(fn)
        emit(what=name, rep=rep, warmup=rep == 0, ms=ms, us_per_step=ms / K * 1e3)
        best = ms if rep and (best is None or ms < best) else best
    emit(what=name, best_ms=best)
    if name.startswith('fused'):
        f_err = out['errors']
    else:
        d = (out[0] - f_err).abs()
        emit(what='agreement', max_abs_error_difference=float(d[~d.isnan()].max()), live=int((~out[0].isnan()).sum()),
             live_fused=int((~f_err.isnan()).sum()))

out = os.environ.get('MOPO_OUT', 'bench_out')
os.makedirs(out, exist_ok=True)
open(os.path.join(out, 'open_loop_speed.txt'), 'w').write('\n'.join(lines) + '\n')
