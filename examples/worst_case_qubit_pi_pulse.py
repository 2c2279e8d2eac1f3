#!/usr/bin/env python
"""Worst-case single-qubit pi pulse: the ensemble of examples/robust_qubit_pi_pulse.py (+-5 MHz detuning x {0.95, 1, 1.05} drive amplitude, 9
members), optimised once for the weighted mean of the members' infidelities and once for their soft worst case (`risk`, DESIGN.md 6b'), from the
same seeds with the same iteration budget (method='LBFGS').

The gate is short here -- 10 ns in 20 slices at 0.1 GHz, twice the time of a bare pi pulse -- so that no pulse serves every member at once and
the edge of the ensemble has to be paid for by its centre.  With the 40 ns and 100 slices of the robust example the mean objective alone
keeps pulling every member down, and a risk bought nothing within the same budget (DESIGN.md 6b').

    python examples/worst_case_qubit_pi_pulse.py [--iterations N] [--risk BETA] [--restarts R]

Both pulses are re-simulated on every member with exact propagators (scipy.linalg.expm); the script prints the worst-member and the mean
infidelity 1 - |tr(U_target^dagger U)|^2 / 4 of each."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'quantum-optimal-control_amd'))
from quantum_optimal_control.main_grape.grape import Grape  # noqa: E402
from robust_qubit_pi_pulse import SX, member_fidelities, problem  # noqa: E402

TOTAL_TIME, STEPS, MAXA = 10.0, 20, [0.1, 0.1]
# beta times the spread of the members' infidelities decides how far the objective leans to the worst member: the mean pulse leaves a spread
# of about 5e-3 here, so 1000 puts most of the weight on the edge of the ensemble and still lets the other members steer
RISK = 1000.0


def main(iterations=100, risk=RISK, restarts=1, quiet=False):
    """Returns dict(ens, uks_mean, uks_risk, infidelity_mean, infidelity_risk): the two pulses and their per-member infidelities."""
    H0, Hops, Hnames, ens = problem()
    kw = dict(total_time=TOTAL_TIME, steps=STEPS, states_concerned_list=[0, 1], maxA=MAXA, reg_coeffs={}, method='LBFGS', show_plots=not quiet,
              save=False, restarts=restarts, convergence={'update_step': 50, 'max_iterations': iterations, 'conv_target': 1e-10})
    np.random.seed(2)
    uks_mean, _ = Grape(H0, Hops, Hnames, SX, robust=dict(ens, risk=0.0), **kw)
    np.random.seed(2)
    uks_risk, _ = Grape(H0, Hops, Hnames, SX, robust=dict(ens, risk=risk), **kw)
    i_mean = 1.0 - member_fidelities(H0, Hops, ens, uks_mean, TOTAL_TIME, SX)
    i_risk = 1.0 - member_fidelities(H0, Hops, ens, uks_risk, TOTAL_TIME, SX)
    w = ens['weights']
    print('mean objective:       worst-member infidelity %.3e, mean infidelity %.3e' % (i_mean.max(), float(np.dot(w, i_mean))))
    print('risk %-6g objective: worst-member infidelity %.3e, mean infidelity %.3e' % (risk, i_risk.max(), float(np.dot(w, i_risk))))
    return dict(ens=ens, uks_mean=uks_mean, uks_risk=uks_risk, infidelity_mean=i_mean, infidelity_risk=i_risk)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--iterations', type=int, default=100)
    ap.add_argument('--risk', type=float, default=RISK)
    ap.add_argument('--restarts', type=int, default=1)
    a = ap.parse_args()
    main(a.iterations, a.risk, a.restarts)
