#!/usr/bin/env python
"""One photon into a lossy cavity: |g,0> -> |g,1> on a qubit dispersively coupled to a cavity mode, optimised once as a closed system and once
under the master equation.

    python examples/cavity_fock_state_under_loss.py [--cavity N] [--slices N] [--iterations N]

A qubit (2 levels) next to a cavity truncated at 20 levels is 40 levels -- past the 32 that the LDS-resident open-system kernels hold, so
Grape(..., collapse_ops=[...]) runs on the tiled path (QOC_PATH_LINDBLAD_TILED: 16 x 16 matrix-instruction tiles, operators in global scratch;
DESIGN.md 6n) without being asked to.  In the frame rotating with both drives H0 = chi |e><e| a^dagger a; the four controls are the two quadratures of a
qubit drive and of a cavity drive.  A Fock state needs the qubit: displacements alone only make coherent states.  The cavity loses photons at
rate KAPPA and the qubit relaxes with lifetime T1, so the time the pulse spends with the qubit excited, or with more than one photon in the
cavity, costs fidelity that the closed model does not see.  Both pulses are scored under decay with method='EVOLVE', and the script prints the two
infidelities 1 - <g,1|rho(T)|g,1> (about five minutes on an MI355X at the default sizes)."""
import argparse
import contextlib
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'quantum-optimal-control_amd'))
from quantum_optimal_control.helper_functions import open_system  # noqa: E402
from quantum_optimal_control.main_grape.grape import Grape  # noqa: E402

CAVITY, STEPS, ITERATIONS = 20, 100, 300
TOTAL_TIME = 4.0              # |chi| TOTAL_TIME = 2.4 pi: a little over one dispersive period
CHI = -2.0 * np.pi * 0.3      # dispersive shift
KAPPA = 0.05                  # photon loss rate of the cavity
T1 = 15.0                     # qubit lifetime
MAXA = [1.5, 1.5, 0.8, 0.8]   # qubit x, qubit y, cavity x, cavity y
UNITARY_ERROR = 1e-10         # Taylor remainder of the Lindblad slice map over the whole pulse: the trace of rho(T) is 1 to this


def problem(cavity=CAVITY):
    """(H0, Hops, Hnames, start, target, collapse_ops) on the 2 x cavity levels |qubit> (x) |photons>, index = qubit * cavity + photons."""
    a = np.diag(np.sqrt(np.arange(1, cavity)), 1).astype(complex)
    sm = np.array([[0, 1], [0, 0]], dtype=complex)                  # |g><e|
    iq, ic = np.eye(2), np.eye(cavity)
    H0 = CHI * np.kron(sm.conj().T @ sm, a.conj().T @ a)
    Hops = [0.5 * np.kron(sm + sm.conj().T, ic), 0.5 * np.kron(1j * (sm.conj().T - sm), ic),
            0.5 * np.kron(iq, a + a.conj().T), 0.5 * np.kron(iq, 1j * (a.conj().T - a))]

    def ket(q, photons):
        v = np.zeros(2 * cavity, dtype=complex)
        v[q * cavity + photons] = 1.0
        return v
    collapse = [np.kron(iq, open_system.relaxation(cavity, 1.0 / KAPPA)), np.sqrt(1.0 / T1) * np.kron(sm, ic)]
    return H0, Hops, ['qubit_x', 'qubit_y', 'cavity_x', 'cavity_y'], ket(0, 0), ket(0, 1), collapse


def initial_guess(steps=STEPS):
    """A fixed, unremarkable start: every drive on, slowly varying, no two alike."""
    t = (np.arange(steps) + 0.5) / steps
    return np.stack([0.5 * np.sin(np.pi * t), 0.3 * np.cos(2 * np.pi * t), 0.3 * np.sin(2 * np.pi * t) + 0.1, 0.2 * np.cos(np.pi * t)])


def _grape(quiet, cavity, total_time, **kw):
    H0, Hops, Hnames, start, target, _ = problem(cavity)
    if 'collapse_ops' in kw:
        kw.setdefault('unitary_error', UNITARY_ERROR)
    with contextlib.redirect_stdout(io.StringIO() if quiet else sys.stdout):
        return Grape(H0, Hops, Hnames, [target], total_time, kw.pop('steps'), [start], state_transfer=True, maxA=MAXA, reg_coeffs={},
                     show_plots=False, save=False, **kw)


def optimise(aware, cavity=CAVITY, steps=STEPS, iterations=ITERATIONS, total_time=TOTAL_TIME, quiet=True, **grape_kwargs):
    """The pulse (4 x steps) Adam finds: aware=False for the closed model, True under the master equation."""
    conv = {'rate': 0.03, 'update_step': 50, 'max_iterations': int(iterations), 'conv_target': 1e-6, 'learning_rate_decay': 1e6}
    kw = dict(steps=steps, method='Adam', convergence=conv, initial_guess=initial_guess(steps))
    if aware:
        kw['collapse_ops'] = problem(cavity)[5]
    kw.update(grape_kwargs)
    return _grape(quiet, cavity, total_time, **kw)[0]


def final_density(uks, cavity=CAVITY, total_time=TOTAL_TIME, quiet=True):
    """rho(T) (n x n) of the pulse `uks` under the master equation (one evaluation: method='EVOLVE')."""
    uks = np.asarray(uks, dtype=np.float64)
    _, rho = _grape(quiet, cavity, total_time, steps=uks.shape[1], method='EVOLVE', initial_guess=uks, collapse_ops=problem(cavity)[5])
    return rho[0, 0]


def score(uks, cavity=CAVITY, total_time=TOTAL_TIME, quiet=True):
    """Infidelity 1 - <g,1|rho(T)|g,1> of the pulse `uks` under the master equation."""
    target = problem(cavity)[4]
    return 1.0 - float(np.real(np.conj(target) @ final_density(uks, cavity, total_time, quiet) @ target))


def main(cavity=CAVITY, steps=STEPS, iterations=ITERATIONS, total_time=TOTAL_TIME, quiet=False):
    closed = score(optimise(False, cavity, steps, iterations, total_time), cavity, total_time)
    aware = score(optimise(True, cavity, steps, iterations, total_time), cavity, total_time)
    if not quiet:
        print('%d levels, %d slices over %.1f time units, %d iterations; photon loss %.3f, qubit T1 %.1f; infidelity under the master equation:'
              % (2 * cavity, steps, total_time, iterations, KAPPA, T1))
        print('  pulse optimised for the closed system      %.4f' % closed)
        print('  pulse optimised under the master equation  %.4f' % aware)
    return closed, aware


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--cavity', type=int, default=CAVITY)
    ap.add_argument('--slices', type=int, default=STEPS)
    ap.add_argument('--iterations', type=int, default=ITERATIONS)
    main(ap.parse_args().cavity, ap.parse_args().slices, ap.parse_args().iterations)
