#!/usr/bin/env python
"""Robust single-qubit pi pulse: one pulse optimised over +-5 MHz detuning x {0.95, 1, 1.05} drive amplitude (9 members), beside a
plain pulse for the nominal qubit with the same iteration budget.

    python examples/robust_qubit_pi_pulse.py [--iterations N]

Both pulses are re-simulated on every member with exact propagators (scipy.linalg.expm); the script prints the worst-member gate
fidelity |tr(U_target^dagger U)|^2 / 4 of each."""
import argparse
import os
import sys

import numpy as np
from scipy.linalg import expm

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'quantum-optimal-control_amd'))
from quantum_optimal_control.helper_functions.robust import ensemble_grid, member_hamiltonians  # noqa: E402
from quantum_optimal_control.main_grape.grape import Grape  # noqa: E402

SZ = np.array([[1, 0], [0, -1]], dtype=complex)
SX = np.array([[0, 1], [1, 0]], dtype=complex)
SY = np.array([[0, -1j], [1j, 0]], dtype=complex)


def problem():
    H0 = 0.0 * SZ                                              # rotating frame, on resonance
    Hops, Hnames = [2 * np.pi * SX / 2, 2 * np.pi * SY / 2], ['x', 'y']
    ens = ensemble_grid(operators=[2 * np.pi * SZ / 2], offsets=np.array([-0.005, 0.0, 0.005])[:, None],   # detuning +-5 MHz (GHz units)
                        amp_scales=[0.95, 1.0, 1.05], k=len(Hops))                                        # drive amplitude error
    return H0, Hops, Hnames, ens


def member_fidelities(H0, Hops, ens, uks, total_time, U):
    """Gate fidelity of the pulse `uks` (k x steps) on every member, by exact propagators."""
    steps = uks.shape[1]
    dt = total_time / steps
    out = []
    for e in range(len(ens['weights'])):
        H0e, Hopse = member_hamiltonians(H0, Hops, ens, e)
        X = np.eye(len(H0))
        for t in range(steps):
            X = expm(-1j * dt * (H0e + sum(uks[j, t] * Hopse[j] for j in range(len(Hops))))) @ X
        out.append(abs(np.trace(U.conj().T @ X)) ** 2 / len(H0) ** 2)
    return np.array(out)


def main(iterations=300, quiet=False):
    H0, Hops, Hnames, ens = problem()
    total_time, steps, U = 40.0, 100, SX
    kw = dict(total_time=total_time, steps=steps, states_concerned_list=[0, 1], maxA=[0.1, 0.1], reg_coeffs={}, method='Adam', show_plots=not quiet,
              save=False, convergence={'rate': 0.01, 'update_step': 100, 'max_iterations': iterations, 'conv_target': 1e-10,
                                       'learning_rate_decay': 1000})
    np.random.seed(2)
    uks_nominal, _ = Grape(H0, Hops, Hnames, U, **kw)
    np.random.seed(2)
    uks_robust, _ = Grape(H0, Hops, Hnames, U, robust=ens, **kw)
    f_nominal = member_fidelities(H0, Hops, ens, uks_nominal, total_time, U)
    f_robust = member_fidelities(H0, Hops, ens, uks_robust, total_time, U)
    print('nominal pulse: worst-member fidelity %.6f (nominal member %.6f)' % (f_nominal.min(), f_nominal[0]))
    print('robust pulse:  worst-member fidelity %.6f (nominal member %.6f)' % (f_robust.min(), f_robust[0]))
    return f_nominal, f_robust


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--iterations', type=int, default=300)
    main(ap.parse_args().iterations)
