#!/usr/bin/env python3
"""The REAL reference's answer to every call the frozen screen of make_goldens_r2.py (CRITERION_VERSION 2) makes on the
rows of ref_extra.npz's live-pair fixture that tests/test_gn_oracle.py::test_committed_screen_is_what_the_generator_produces
re-screens - so that test replays the screen on the reference's own answers wherever the reference is absent.

Runs only where the reference is present (make_goldens.REF); writes ``ref_screen_calls.npz`` next to this file.
Only arrays are stored - never reference source text:
  calls_g [K, 2]       the two counts of the pixel handed to ``optimize_sino_cpu`` (matdecomp.py:87-127)
  calls_n_iters [K]    its n_iters
  calls_raised [K]     the reference raised LinAlgError
  calls_a [K, 2]       its answer for that pixel (NaN where it raised)
  views                the views of the fixture screened ([first, end))

    python tests/golden/make_goldens_screen.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens  # noqa: E402
import make_goldens_r2 as r2  # noqa: E402

VIEWS = (0, 2)          # what the test re-screens (a third of the fixture's views: a few seconds)


def main():
    e = np.load(os.path.join(HERE, 'ref_extra.npz'))
    assert int(e['uns_criterion_version']) == r2.CRITERION_VERSION
    ref = make_goldens.load_reference()
    ref.xc.mixatten = make_goldens.load_pkg_module('xcompy').mixatten
    calls = {}

    def recording(gp, ee, i0_1, mus, n_iters, verbose=False):
        key = (float(gp[0, 0, 0]), float(gp[1, 0, 0]), int(n_iters))
        try:
            a = ref.optimize_sino_cpu(gp, ee, i0_1, mus, n_iters, verbose=verbose)
        except np.linalg.LinAlgError:
            calls[key] = (True, np.full(2, np.nan))
            raise
        calls[key] = (False, np.asarray(a, dtype=np.float64)[0, 0].copy())
        return a

    sel = slice(*VIEWS)
    got = r2.screen(recording, e['uns_g'][:, sel], e['uns_ee'], e['uns_i0'], e['uns_mus'], int(e['uns_n_iters']))
    for name, mine, committed in zip(('raised', 'raised_at', 'a50', 'ill', 'cond'), got,
                                     (e['uns_raised'], e['uns_raised_at'], e['uns_a50'], e['uns_ill'], e['uns_cond'])):
        assert np.array_equal(mine, committed[sel], equal_nan=True), name
    keys = list(calls)
    np.savez_compressed(os.path.join(HERE, 'ref_screen_calls.npz'),
                        calls_g=np.array([k[:2] for k in keys], dtype=np.float64),
                        calls_n_iters=np.array([k[2] for k in keys], dtype=np.int32),
                        calls_raised=np.array([calls[k][0] for k in keys], dtype=bool),
                        calls_a=np.array([calls[k][1] for k in keys], dtype=np.float64),
                        views=np.array(VIEWS, dtype=np.int32))
    print(f'{len(keys)} calls recorded ({sum(calls[k][0] for k in keys)} raised)')


if __name__ == '__main__':
    main()
