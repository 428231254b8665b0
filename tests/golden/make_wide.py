"""Golden vectors at ant's dimensions (27 observations + 8 actions: 35 inputs, 28 outputs), made by EXECUTING
the reference's own code, as make_ref_vectors.py and make_golden.py do for 17 + 6.

Run in the build container only (reads /root/reference; nothing here runs on the GPU box):

    python tests/golden/make_wide.py

Executed from the reference (read-only, loaded by file path through make_ref_vectors.load_reference /
make_golden._load):
  * ensemble forward: ``BNN._compile_outputs`` (bnn.py:631-675) on a stand-in built by ``BNN.add`` /
    ``FC.construct_vars`` (make_ref_vectors.build_bnn), in f32 and in f64
  * ``FakeEnv.step`` (fake_env.py:37-131) with ``mopo/static/ant.py``'s ``termination_fn``
Outputs: tests/golden/wide_fwd_*.npz (continued in parts/ past 900 kB: test_oracle_ref.load_case) and
tests/golden/wide_fakeenv_*.npz -- arrays only.  No weights are stored: they are regenerated from
``oracle.bnn.init_params(seed)`` and pinned by their sha256.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import tfstub  # noqa: E402
from make_golden import REF, _load  # noqa: E402
from make_ref_vectors import build_bnn, load_reference, save_split, sha  # noqa: E402
from oracle import bnn as obnn  # noqa: E402

O, A = 27, 8


def wide_params(E, H, smv, seed):
    """The weights of a wide case (the tests regenerate them the same way and check the sha256)."""
    rs = np.random.RandomState(seed + 100)
    fit = rs.normal(size=(400, O + A)) * 1.5 + 0.2
    return obnn.init_params(E, O, A, hidden=H, seed=seed, smv=smv, inputs=fit), rs


def forward_case(refs, name, E, H, B, smv, seed):
    p, rs = wide_params(E, H, smv, seed)
    x = rs.normal(size=(B, O + A)) * 1.5 + 0.2
    x[0] = 0.0                                        # the all-zero row
    x[1] = 40.0 * np.sign(rs.normal(size=O + A))      # far outside the data: saturated swish / bounds
    x = x.astype(np.float32)
    out = dict(E=E, H=H, B=B, O=O, A=A, smv=int(smv), seed=seed, x=x, weights_sha=sha(obnn.to_mat_list(p)))
    bnn = refs[2]
    for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
        obj = build_bnn(refs, p, E, O, A, H, smv, dt)
        xin = tfstub.w(torch.as_tensor(np.asarray(x, np.float32 if dt == torch.float32 else np.float64)))
        mean, var = bnn.BNN._compile_outputs(obj, xin)
        _, lv = bnn.BNN._compile_outputs(obj, xin, ret_log_var=True)
        out['mean_' + tag] = tfstub.u(mean).detach().numpy()
        out['var_' + tag] = tfstub.u(var).detach().numpy()
        out['logvar_' + tag] = tfstub.u(lv).detach().numpy()
    save_split(os.path.join(HERE, 'wide_fwd_%s.npz' % name), out)   # every committed file stays below 1 MiB


class _Model:
    """Stand-in for the TF BNN: reference ``random_inds`` + the reference graph's forward (f32)."""

    def __init__(self, refs, params, E, H, elites):
        self._refs, self.num_nets, self._model_inds = refs, E, list(elites)
        self.random_inds = types.MethodType(refs[2].BNN.random_inds, self)
        self._obj = build_bnn(refs, params, E, O, A, H, True, torch.float32)
        self.last = None

    def predict(self, inputs, factored=True):
        assert factored
        x = tfstub.w(torch.as_tensor(np.asarray(inputs, np.float32)))       # the f32 placeholder feed
        mean, var = self._refs[2].BNN._compile_outputs(self._obj, x)
        self.last = (mean.detach().numpy().copy(), var.detach().numpy().copy())
        return self.last


def fakeenv_cases(refs, E=7, H=64, seed=16):
    fe = _load('mopo.models.fake_env', os.path.join(REF, 'mopo/models/fake_env.py'))
    ant = _load('ref_static_ant', os.path.join(REF, 'mopo/static/ant.py')).StaticFns
    params, rs = wide_params(E, H, True, seed)
    wsha = sha(obnn.to_mat_list(params))
    elites = list(rs.permutation(E)[:5])
    cid = 0
    for B in (1, 7, 64, 257):
        for learned_var in (True, False):
            for det in (False, True):
                for f64 in (False, True):
                    if (det or f64) and B not in (7, 257):
                        continue
                    obs = (rs.normal(size=(B, O)) * 1.5 + 0.2).astype(np.float32)
                    obs[:, 0] = rs.uniform(0.1, 1.1, size=B)     # both outcomes of ant.py's rule
                    if f64:
                        obs = obs.astype(np.float64) + 1e-3       # later horizon steps feed f64 next_obs
                    act = rs.uniform(-1, 1, size=(B, A)).astype(np.float32)
                    coeff = 1.0 if cid % 2 == 0 else 5.0
                    cseed = 2000 + cid
                    model = _Model(refs, params, E, H, elites)
                    env = fe.FakeEnv(model, ant, penalty_coeff=coeff, penalty_learned_var=learned_var)
                    np.random.seed(cseed)
                    nobs, rew, term, info = env.step(obs, act, deterministic=det)
                    after = np.random.get_state()[2]
                    np.random.seed(cseed)
                    if not det:
                        np.random.normal(size=(E, B, O + 1))
                    inds = np.zeros(B, np.int64) if det else np.random.choice(elites, size=B)
                    assert det or np.random.get_state()[2] == after
                    case = dict(E=E, H=H, B=B, O=O, A=A, domain='ant', learned_var=int(learned_var),
                                deterministic=int(det), penalty_coeff=coeff, seed=cseed, wseed=seed, weights_sha=wsha,
                                elites=np.array(elites, np.int64), obs=obs, act=act,
                                model_inds=np.asarray(inds, np.int64), next_obs=nobs, rew=rew, term=term,
                                info_mean=info['mean'], info_std=info['std'], log_prob=info['log_prob'],
                                dev=info['dev'], unpenalized=info['unpenalized_rewards'], penalty=info['penalty'])
                    if B <= 64:
                        case['ref_mean'], case['ref_var'] = model.last
                    np.savez_compressed(os.path.join(HERE, 'wide_fakeenv_%03d.npz' % cid), **case)
                    cid += 1
    return cid


def main():
    refs = load_reference()
    forward_case(refs, 'E7_H200', 7, 200, 40, True, 51)
    forward_case(refs, 'E7_H64_joint', 7, 64, 40, False, 52)
    forward_case(refs, 'E32_H400', 32, 400, 40, True, 53)    # the fp32-only wide width
    print('wrote 3 forward cases and %d fakeenv cases' % fakeenv_cases(refs))


if __name__ == '__main__':
    main()
