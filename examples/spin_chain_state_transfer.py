#!/usr/bin/env python
"""An excitation moved along a 10-spin XX chain (n = 2^10 = 1024 levels) by local z fields -- the sparse state-transfer route.

    python examples/spin_chain_state_transfer.py [--spins L] [--iterations N] [--restarts B]

The Hamiltonians are scipy.sparse matrices built from Kronecker products; because `H0` / `Hops` are sparse, Grape() keeps them sparse from here
to the GPU (ELLPACK mat-vecs, csrc/qoc_sparse.h) and never forms an n x n array: the drift of this chain has 9 entries per row at most, a dense
copy would have 1024.  The script prints the fidelity the returned pulse reaches when it is re-simulated with scipy's expm_multiply."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'quantum-optimal-control_amd'))
from quantum_optimal_control.helper_functions.synthetic_systems import xx_chain  # noqa: E402
from quantum_optimal_control.main_grape.grape import Grape  # noqa: E402


def main(spins=10, iterations=300, restarts=1, steps=200, quiet=False):
    coupling = 1.0
    H0, Hops, Hnames, excitation = xx_chain(spins, coupling=coupling)       # z control on every site
    start, target = excitation(0), excitation(spins - 1)
    total_time = 2.0 * spins / coupling                                     # a few transit times of the bare chain
    convergence = {'rate': 0.05, 'update_step': 50, 'max_iterations': iterations, 'conv_target': 1e-4, 'learning_rate_decay': 1000}
    np.random.seed(1)
    uks, U_final = Grape(H0, Hops, Hnames, [target], total_time=total_time, steps=steps, states_concerned_list=[start], convergence=convergence,
                         reg_coeffs={'dwdt': 0.001}, maxA=[2.0] * spins, method='Adam', state_transfer=True, show_plots=not quiet, save=False,
                         restarts=restarts)
    assert U_final == []                                                    # state transfer returns no unitary, as in the reference
    # re-simulate the returned pulse with exact slice propagators applied to the vector (still no dense matrix)
    from scipy.sparse.linalg import expm_multiply
    dt, psi = total_time / steps, start.copy()
    for t in range(steps):
        H = H0
        for j in range(len(Hops)):
            H = H + uks[j, t] * Hops[j]
        psi = expm_multiply(-1j * dt * H, psi)
    fidelity = float(abs(np.vdot(target, psi)) ** 2)
    print('%d spins, n = %d, pulse shape %s: transfer fidelity %.6f after at most %d iterations' % (spins, 2 ** spins, uks.shape, fidelity, iterations))
    return fidelity


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--spins', type=int, default=10)
    ap.add_argument('--iterations', type=int, default=300)
    ap.add_argument('--restarts', type=int, default=1)
    args = ap.parse_args()
    main(args.spins, args.iterations, args.restarts)
