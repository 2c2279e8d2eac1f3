#!/usr/bin/env python
"""Eight restarts of the coarse qutrit X gate (ten slices of 1 ns, examples/coarse_qutrit_x_gate.py), each its own L-BFGS run on the GPU.

    python examples/lbfgs_restarts.py [--restarts R] [--slices N]

Grape(..., restarts=8, method='LBFGS', exact_gradient=True) runs the device-resident L-BFGS loop: every control set keeps its own curvature
history and line search, one kernel launch per evaluation takes all their decisions, and the host only polls.  scipy's 'L-BFGS-B' optimises one
control set per call with a host round trip per evaluation; here the restarts are independent quasi-Newton runs and the best one is returned.
With ten long slices the first-order gradient is not the derivative of the loss the Armijo test sees, hence exact_gradient=True.
The script prints every restart's final infidelity and evaluation count, and the infidelity of the returned pulse re-simulated with exact
propagators."""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'quantum-optimal-control_amd'))
import coarse_qutrit_x_gate as coarse  # noqa: E402
from quantum_optimal_control.main_grape.grape import Grape  # noqa: E402

CONVERGENCE = {'update_step': 1000, 'max_iterations': 400, 'conv_target': 1e-12, 'lbfgs_history': 8}


def run(restarts=8, steps=coarse.STEPS, quiet=True, seed=4, **grape_kwargs):
    """dict(uks, infidelity of the returned pulse, per-restart loss and iterations, seconds)."""
    H0, Hops, Hnames, U = coarse.problem()
    kw = dict(total_time=coarse.TOTAL_TIME, steps=steps, states_concerned_list=[0, 1], maxA=coarse.MAXA, reg_coeffs={}, method='LBFGS',
              show_plots=False, save=False, Taylor_terms=coarse.TAYLOR, convergence=dict(CONVERGENCE), exact_gradient=True, restarts=restarts)
    kw.update(grape_kwargs)
    np.random.seed(seed)
    finals = {}
    out = io.StringIO()
    t0 = time.time()
    with contextlib.redirect_stdout(out if quiet else sys.stdout):
        uks, _ = Grape(H0, Hops, Hnames, U, _restart_info=finals, **kw)
    return dict(uks=uks, seconds=time.time() - t0, infidelity=coarse.infidelity(H0, Hops, U, uks, coarse.TOTAL_TIME), log=out.getvalue(), **finals)


def main(restarts=8, steps=coarse.STEPS, quiet=False):
    r = run(restarts, steps)
    if not quiet:
        print('%d restarts, %d slices of %.2f ns, L-BFGS on the device to an infidelity of %.0e (%.2f s):' % (
            restarts, steps, coarse.TOTAL_TIME / steps, CONVERGENCE['conv_target'], r['seconds']))
        for b in range(restarts):
            print('  restart %d: infidelity %.3e after %d evaluations' % (b, r['loss'][b], r['iterations'][b]))
    print('returned pulse: infidelity %.3e (exact propagators)' % r['infidelity'])
    return r['infidelity']


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--restarts', type=int, default=8)
    ap.add_argument('--slices', type=int, default=coarse.STEPS)
    args = ap.parse_args()
    main(args.restarts, args.slices)
