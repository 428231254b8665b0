"""Golden vectors at the hidden widths 128, 256 and 100 (the 8- and 16-block forms of the ensemble forward and a
width that is rounded up to one), made by EXECUTING the reference's own code, as make_wide.py does for 27 + 8.

Run where the reference checkout is (make_golden.REF; no GPU needed, and no test reads the reference):

    python tests/golden/make_widths.py

Executed from the reference (read-only, loaded by file path through make_ref_vectors.load_reference):
``BNN._compile_outputs`` (bnn.py:631-675) on a stand-in built by ``BNN.add`` / ``FC.construct_vars``
(make_ref_vectors.build_bnn), in f32 and in f64.
Outputs: tests/golden/widths_fwd_*.npz -- arrays only.  No weights are stored: they are regenerated from
``oracle.bnn.init_params(seed)`` and pinned by their sha256.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

import tfstub  # noqa: E402
from make_ref_vectors import build_bnn, load_reference, save_split, sha  # noqa: E402
from oracle import bnn as obnn  # noqa: E402


def widths_params(E, O, A, H, smv, seed):
    """The weights of a case (the tests regenerate them the same way and check the sha256)."""
    rs = np.random.RandomState(seed + 100)
    fit = rs.normal(size=(400, O + A)) * 1.5 + 0.2
    return obnn.init_params(E, O, A, hidden=H, seed=seed, smv=smv, inputs=fit), rs


def forward_case(refs, name, E, O, A, H, B, smv, seed):
    p, rs = widths_params(E, O, A, H, smv, seed)
    x = rs.normal(size=(B, O + A)) * 1.5 + 0.2
    x[0] = 0.0                                        # the all-zero row
    x[1] = 40.0 * np.sign(rs.normal(size=O + A))      # far outside the data: saturated swish / bounds
    x[2] = -x[1]
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
    save_split(os.path.join(HERE, 'widths_fwd_%s.npz' % name), out)   # every committed file stays below 1 MiB


def main():
    refs = load_reference()
    forward_case(refs, 'E7_H128', 7, 17, 6, 128, 64, True, 61)
    forward_case(refs, 'E7_H256', 7, 17, 6, 256, 64, True, 62)
    forward_case(refs, 'E7_H100', 7, 17, 6, 100, 64, False, 63)      # rounded up to 8 blocks; the joint head
    forward_case(refs, 'E7_H128_O27_A8', 7, 27, 8, 128, 64, True, 64)
    print('wrote 4 forward cases')


if __name__ == '__main__':
    main()
