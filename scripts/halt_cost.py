"""What hard truncation costs (DESIGN 4 quotes both figures):

  1. the headline workload C2 (bench.py's own model, pool, policy and rollout call: halfcheetah-mixed, E = 7,
     H = 200, 50000 rows x 5 steps, the product-default dtype) with the max_aleatoric penalty halted at the dataset's
     0.99 quantile, against the same rollouts without halting -- which leave the split two-stream path for the
     compacting one;
  2. ModelRollout.penalty_profile over a 1e6-row pool against the host loop that computes the same u with the public
     FakeEnv.step (deterministic) in chunks of the same size.

hipEvents / wall clock around each, best of 3 after a warm-up.  Raw JSON lines to $MOPO_OUT/halt_cost.txt (default
bench_out/):  python scripts/halt_cost.py"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from mopo_amd.evaluation import halt_threshold_from_quantile  # noqa: E402
from mopo_amd.fake_env import FakeEnv  # noqa: E402
from mopo_amd.replay_pool import SimpleReplayPool  # noqa: E402
from mopo_amd.rollout import ModelRollout  # noqa: E402
from mopo_amd.static import static_fns  # noqa: E402

lines = []


def emit(**kw):
    lines.append(json.dumps(kw))
    print(lines[-1], flush=True)


sys.argv = [sys.argv[0]]
args = bench.parse()
dev = torch.device('cuda:0')
model, pool, ro, pi, env, _ = bench.build(args, dev, 0, world=1)
spec = bench.CONFIGS[args.config]
tk, pen = static_fns[spec['domain']].term_kind, spec['penalty']
O, A = bench.O, bench.A

# ---- 1. C2, halting at the dataset's 0.99 quantile of max_aleatoric -----------------------------------------------
env_obs, env_act = bench.make_env(spec)
data = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=len(env_obs))
data.add_samples({'observations': env_obs, 'actions': env_act, 'rewards': np.zeros((len(env_obs), 1)),
                  'terminals': np.zeros((len(env_obs), 1), bool), 'next_observations': env_obs})
u = ro.penalty_profile(data, 'max_aleatoric')
thr = halt_threshold_from_quantile(u, 0.99)
emit(what='C2 threshold', quantile=0.99, threshold=thr, dataset_rows=int(u.numel()),
     dataset_share_above=float((u > thr).float().mean()))


def rollouts(n, first, **kw):
    total = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outs = [ro.run(env, pi, pool, args.batch, args.horizon, tk, pen, [0, 1, 2, 3, 4], seed=88, epoch=first + i,
                   actor_dtype=args.actor_dtype, **kw) for i in range(n)]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    total = int(sum(int(x.sum().item()) for x in outs))
    return total, dt


for name, kw in (('C2 no halting', {}), ('C2 halt at q = 0.99', dict(halt_threshold=thr, halt_reward=-100.0)),
                 ('C2 halt armed, threshold +inf (compacting path, nothing halts)',
                  dict(halt_threshold=float('inf'), halt_reward=-100.0))):
    rollouts(args.warmup, 0, **kw)
    best = None
    for rep in range(3):
        total, dt = rollouts(args.steps, args.warmup + rep * args.steps, **kw)
        emit(what=name, rep=rep, transitions=total, ms_per_rollout=dt / args.steps * 1e3,
             transitions_per_s=total / dt, launch_rows_per_s=args.batch * args.horizon * args.steps / dt)
        best = dt if best is None or dt < best else best
    halted = None if ro.last_halted is None else ro.last_halted.cpu().tolist()
    emit(what=name, best_ms_per_rollout=best / args.steps * 1e3, last_halted_per_step=halted)

# ---- 2. the penalty over a 1e6-row pool --------------------------------------------------------------------------
N, CH = 1000000, args.batch
rs = np.random.RandomState(3)
big = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=N)
big.add_samples({'observations': rs.normal(size=(N, O)).astype(np.float32), 'actions': rs.uniform(-1, 1, (N, A)),
                 'rewards': np.zeros((N, 1)), 'terminals': np.zeros((N, 1), bool),
                 'next_observations': np.zeros((N, O), np.float32)})
F = big.fields
fe = FakeEnv(model, static_fns['halfcheetah'], penalty_coeff=1.0, penalty_kind='max_aleatoric')
ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fn):
    torch.cuda.synchronize()
    ev0.record()
    out = fn()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1), out


def host_loop(kind):
    fe_k = FakeEnv(model, static_fns['halfcheetah'], penalty_coeff=1.0, penalty_kind=kind)
    return torch.cat([fe_k.step(F['observations'][j:j + CH], F['actions'][j:j + CH], deterministic=True)[3]['penalty'][:, 0]
                      for j in range(0, N, CH)])


for kind in ('max_aleatoric', 'max_pairwise'):
    res = {}
    for name, fn in (('penalty_profile', lambda: ro.penalty_profile(big, kind)),
                     ('host loop of FakeEnv.step chunks', lambda: host_loop(kind))):
        best = None
        for rep in range(4):   # the first is the warm-up
            ms, out = timed(fn)
            emit(what=name, kind=kind, rows=N, chunk=CH, rep=rep, warmup=rep == 0, ms=ms)
            best = ms if rep and (best is None or ms < best) else best
        emit(what=name, kind=kind, best_ms=best, rows_per_s=N / best * 1e3)
        res[name] = out
    a, b = res['penalty_profile'], res['host loop of FakeEnv.step chunks']
    emit(what='agreement', kind=kind, max_rel_difference=float(((a - b).abs() / b).max()))

out = os.environ.get('MOPO_OUT', 'bench_out')
os.makedirs(out, exist_ok=True)
open(os.path.join(out, 'halt_cost.txt'), 'w').write('\n'.join(lines) + '\n')
