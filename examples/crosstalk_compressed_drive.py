#!/usr/bin/env python
"""Two qubits, one drive line each, with crosstalk and amplifier compression: 10 % of each line reaches the other qubit, and every line
delivers u - 0.1 u^3 / maxA^2 of the amplitude u it is asked for.  The gate is X on the first qubit and sqrt(X) on the second.

    python examples/crosstalk_compressed_drive.py [--iterations N]

Two pulses with the same iteration budget:
  naive  optimised as if each line drove its own qubit, linearly (no map), then scored through the true map:
         Grape(..., method='EVOLVE', initial_guess=naive pulse, control_map=cm);
  aware  optimised through the map, Grape(..., control_map=cm).
The script prints the gate infidelity 1 - |tr(U_target^dagger U)|^2 / 16 of each, as the engine propagates it through the true map."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'quantum-optimal-control_amd'))
from quantum_optimal_control.helper_functions import control_map as cmap  # noqa: E402
from quantum_optimal_control.main_grape.grape import Grape  # noqa: E402

TOTAL_TIME, STEPS = 10.0, 40
MAXA = [0.12, 0.12]           # GHz
CROSSTALK, COMPRESSION = 0.1, 0.1
ZZ = 0.002                    # always-on coupling, GHz


def problem():
    sx, sz, one = np.array([[0, 1], [1, 0]], dtype=complex), np.diag([1.0, -1.0]).astype(complex), np.eye(2, dtype=complex)
    H0 = 2 * np.pi * ZZ * np.kron(sz, sz) / 4
    Hops, Hnames = [2 * np.pi * np.kron(sx, one) / 2, 2 * np.pi * np.kron(one, sx) / 2], ['line1', 'line2']
    half = (one - 1j * sx) / np.sqrt(2)                                # sqrt(X) up to a phase
    return H0, Hops, Hnames, np.kron(-1j * sx, half)


def true_map():
    """What stands between the two lines and the two qubits: each line compresses, then 10 % of it leaks to the other qubit."""
    lines = cmap.polynomial([[1.0, 0.0, -COMPRESSION / a ** 2] for a in MAXA])
    return cmap.compose(cmap.linear([[1.0, CROSSTALK], [CROSSTALK, 1.0]]), lines)


def infidelity(U, Uf):
    return 1.0 - abs(np.trace(U.conj().T @ Uf)) ** 2 / len(U) ** 2


def main(iterations=400, quiet=False):
    H0, Hops, Hnames, U = problem()
    cm = true_map()
    kw = dict(total_time=TOTAL_TIME, steps=STEPS, states_concerned_list=[0, 1, 2, 3], maxA=MAXA, reg_coeffs={}, show_plots=not quiet, save=False,
              convergence={'rate': 0.02, 'update_step': 100, 'max_iterations': iterations, 'conv_target': 1e-13, 'learning_rate_decay': 1000})
    np.random.seed(3)
    uks_naive, Uf_model = Grape(H0, Hops, Hnames, U, method='Adam', **kw)                                   # the model: no map
    _, Uf_naive = Grape(H0, Hops, Hnames, U, method='EVOLVE', initial_guess=uks_naive, control_map=cm, **kw)   # ... scored through the true map
    np.random.seed(3)
    _, Uf_aware = Grape(H0, Hops, Hnames, U, method='Adam', control_map=cm, **kw)                            # optimised through the map
    inf_naive, inf_aware = infidelity(U, Uf_naive), infidelity(U, Uf_aware)
    print('naive pulse: infidelity as modelled %.3e, through the true map %.3e' % (infidelity(U, Uf_model), inf_naive))
    print('aware pulse: infidelity through the true map %.3e' % inf_aware)
    print('coefficients of the aware pulse: largest |c| = %.4f GHz on lines limited to %.2f GHz' % (np.max(np.abs(cm.coefficients)), max(MAXA)))
    return inf_naive, inf_aware


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--iterations', type=int, default=400)
    main(ap.parse_args().iterations)
