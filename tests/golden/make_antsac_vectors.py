"""Golden vectors of the SAC step at ant's shape (27 observations + 8 actions: 35 critic inputs, past the one
32-wide layer-1 group), made like the ``ref_sac_*`` cases: ``make_ref_vectors.sac_case`` executes the
reference's ``MOPO._build`` / ``_do_training`` / ``_update_target`` under tests/golden/tfstub.py, in f32 and f64.

Run where the reference checkout is present (see make_ref_vectors.py):

    python tests/golden/make_antsac_vectors.py

Output: tests/golden/antsac_O27_A8_H64.npz -- arrays only (O = 27, A = 8, H = 64, batch 64, 2 steps, compact
form).  The name deliberately matches none of the globs the older tests count (ref_sac_*, ...).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_ref_vectors as mrv  # noqa: E402

NAME = 'antsac_O27_A8_H64.npz'


def main():
    refs = mrv.load_reference()
    got = {}

    def keep(path, out):   # sac_case's save: take the case instead of writing ref_sac_<name>.npz
        got.update(out)

    orig, mrv.save_split = mrv.save_split, keep
    try:
        mrv.sac_case(refs, 'ant', 27, 8, 64, 64, 33, steps=2, compact=True)
    finally:
        mrv.save_split = orig
    arrays = {k: np.asarray(v) for k, v in got.items()}
    assert sum(v.nbytes for v in arrays.values()) <= mrv.PART_BYTES, 'the case must fit one committed file'
    np.savez_compressed(os.path.join(HERE, NAME), **arrays)
    print('ok', NAME, len(arrays), 'arrays')


if __name__ == '__main__':
    main()
