"""Speed of the ensemble forward and the rollout actor across hidden widths: ms per 50k-row launch at
H in {64, 128, 200, 256} per dtype, each width's rate against the shipped H = 200 kernel of the same dtype scaled
by the algorithmic FLOP per row (oracle.bnn.flops_per_row; the actor: 2 (O H + H H + 2 H A)), and the whole
rollout's transitions/s at the C2 sizes (halfcheetah, E = 7, 50000 rows, horizon 5) with H = 128 and 256.

Kernel intervals are taken between two HIP events created with hipEventDisableSystemFence (no system-scope
release in front of the timestamp) around REPS back-to-back launches on the current stream.
Raw JSON lines to $MOPO_OUT/width_speed.txt (default bench_out/):  python scripts/width_speed.py
``WIDTH_SPEED_TAG`` labels the lines of a variant build (the H = 256 bf16x6 A/B: DESIGN section 2)."""
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
from mopo_amd.replay_pool import SimpleReplayPool
from mopo_amd.rollout import ModelRollout, default_actor_dtype, init_sac_params
from oracle.bnn import flops_per_row

E, O, A, B, REPS = 7, 17, 6, 50000, 20
DTYPES = ('fp32', 'bf16x6', 'f16x3')
TAG = os.environ.get('WIDTH_SPEED_TAG', 'shipped')
ONLY = os.environ.get('WIDTH_SPEED_ONLY')   # e.g. "256:bf16x6": just that ensemble cell (variant builds)
lines = []

hip = C.CDLL('libamdhip64.so')
EVENT_DISABLE_SYSTEM_FENCE = 0x20000000


def emit(**kw):
    lines.append(json.dumps(dict(kw, tag=TAG)))
    print(lines[-1], flush=True)


def hip_ok(rc):
    if rc != 0:
        raise RuntimeError('HIP call failed: %d' % rc)


class Interval:
    def __init__(self):
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for ev in (self.a, self.b):
            hip_ok(hip.hipEventCreateWithFlags(C.byref(ev), C.c_uint(EVENT_DISABLE_SYSTEM_FENCE)))

    def ms(self, fn, reps):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        hip_ok(hip.hipEventRecord(self.a, stream))
        for _ in range(reps):
            fn()
        hip_ok(hip.hipEventRecord(self.b, stream))
        hip_ok(hip.hipEventSynchronize(self.b))
        out = C.c_float()
        hip_ok(hip.hipEventElapsedTime(C.byref(out), self.a, self.b))
        return out.value / reps


iv = Interval()
rs = np.random.RandomState(0)
x = torch.from_numpy(rs.normal(size=(B, O + A)).astype(np.float32)).cuda()
cells = [(H, dt) for H in (64, 128, 200, 256) for dt in DTYPES]
if ONLY:
    cells = [(int(ONLY.split(':')[0]), ONLY.split(':')[1])]

# ---- ensemble: BNN.predict's launch ----------------------------------------------------------------------------
ens = {}
for H, dt in cells:
    m = construct_model(obs_dim=O, act_dim=A, hidden_dim=H, num_networks=E, num_elites=5, separate_mean_var=True,
                        seed=0, dtype=dt)
    mean = torch.empty((E, B, O + 1), device='cuda')
    var = torch.empty_like(mean)
    fn = lambda: L.check(L.lib().mopo_bnn_predict(m.handle, L.ptr(x), 0, B, L.ptr(mean), L.ptr(var), L.stream_ptr(None)))
    iv.ms(fn, 5)
    best = min(iv.ms(fn, REPS) for _ in range(3))
    ens[(H, dt)] = best
    emit(what='ensemble predict', H=H, dtype=dt, ms_per_50k=best, gflop=flops_per_row(E, O + A, H, O + 1) * B / 1e9,
         tflops=flops_per_row(E, O + A, H, O + 1) * B / best / 1e9)
for (H, dt), ms in ens.items():
    if (200, dt) in ens and H != 200:
        want = ens[(200, dt)] * flops_per_row(E, O + A, H, O + 1) / flops_per_row(E, O + A, 200, O + 1)
        emit(what='ensemble vs H = 200 scaled by FLOP', H=H, dtype=dt, ms=ms, ms_at_h200_rate=want, ratio=want / ms)

if not ONLY:
    # ---- actor ------------------------------------------------------------------------------------------------------
    obs = torch.from_numpy(rs.normal(size=(B, O))).cuda()
    act = torch.empty((B, A), device='cuda')
    mu = torch.empty_like(act)
    ac = {}
    for H in (64, 128, 208, 256):
        pi = torch.from_numpy(init_sac_params(O, A, H)).cuda()
        for dt, code in (('fp32', 0), ('bf16x6', 3), ('f16x3', 4)):
            fn = lambda: L.check(L.lib().mopo_actor_forward_dtype(L.ptr(pi), O, A, H, L.ptr(obs), 1, B, None, 1, 0,
                                                                  L.ptr(act), L.ptr(mu), code, L.stream_ptr(None)))
            iv.ms(fn, 5)
            ac[(H, dt)] = min(iv.ms(fn, REPS) for _ in range(3))
            emit(what='actor forward (pack + kernel)', H=H, dtype=dt, ms_per_50k=ac[(H, dt)])
    for (H, dt), ms in ac.items():
        if H != 256:
            fl = lambda h: 2.0 * (O * h + h * h + 2 * h * A)
            want = ac[(256, dt)] * fl(H) / fl(256)
            emit(what='actor vs H = 256 scaled by FLOP', H=H, dtype=dt, ms=ms, ms_at_h256_rate=want, ratio=want / ms)

    # ---- the whole rollout at the C2 sizes ----------------------------------------------------------------------
    env = torch.from_numpy(rs.normal(size=(100000, O)).astype(np.float32)).cuda()
    for H, hp in ((200, 256), (128, 128), (256, 256), (256, 64)):
        for dt in ('bf16x6', 'f16x3', 'fp32'):
            m = construct_model(obs_dim=O, act_dim=A, hidden_dim=H, num_networks=E, num_elites=5,
                                separate_mean_var=True, seed=0, dtype=dt)
            m.set_elites([0, 1, 2, 3, 4])
            pi = torch.from_numpy(init_sac_params(O, A, hp)).cuda()
            pool = SimpleReplayPool(obs_dim=O, act_dim=A, max_size=B * 5)
            ro = ModelRollout(m, B, 5)
            run = lambda k: ro.run(env, pi, pool, B, 5, 0, 1.0, [0, 1, 2, 3, 4], seed=1, epoch=k, pi_hidden=hp,
                                   actor_dtype=default_actor_dtype(dt))
            for k in range(3):
                run(k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(10):
                run(3 + k)
            torch.cuda.synchronize()
            dtm = (time.perf_counter() - t0) / 10
            emit(what='rollout 50000 x 5', H=H, pi_hidden=hp, dtype=dt, ms=dtm * 1e3, transitions_per_s=B * 5 / dtm)

out = os.path.join(os.environ.get('MOPO_OUT', 'bench_out'), 'width_speed.txt')
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, 'a') as f:
    f.write('\n'.join(lines) + '\n')
