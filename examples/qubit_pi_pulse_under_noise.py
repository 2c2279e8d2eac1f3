#!/usr/bin/env python
"""Qubit pi pulse under detuning noise that moves DURING the gate: Ornstein-Uhlenbeck noise of 5 MHz rms whose correlation time (10 ns) is a quarter
of the 40 ns pulse.  Three pulses with the same iteration budget:

  nominal       the qubit without noise;
  quasi-static  a robust ensemble of constant detunings of the same variance (what `robust=` modelled so far);
  traces        an ensemble of sampled noise trajectories (helper_functions.noise.ornstein_uhlenbeck, the `traces` key of the robust dict), started
                from the nominal pulse with initial_guess=.

    python examples/qubit_pi_pulse_under_noise.py [--iterations N] [--members E] [--heldout H]

All three are scored with method='EVOLVE' on a held-out set of fresh traces (every member in one call); the script prints the held-out mean
infidelity of each and, for the nominal and the trace pulse, the mean infidelity on the training traces -- the number the trace ensemble
minimises.  One Taylor order for every call, so that all figures belong to one propagator."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'quantum-optimal-control_amd'))
from quantum_optimal_control.helper_functions import noise  # noqa: E402
from quantum_optimal_control.main_grape.grape import Grape  # noqa: E402

SZ = np.array([[1, 0], [0, -1]], dtype=complex)
SX = np.array([[0, 1], [1, 0]], dtype=complex)
SY = np.array([[0, -1j], [1j, 0]], dtype=complex)

TOTAL_TIME, STEPS = 40.0, 100                  # ns, slices
SIGMA, TAU = 0.005, 10.0                       # GHz rms detuning, ns correlation time
DETUNING = 2 * np.pi * SZ / 2                  # a detuning of delta GHz is delta x this operator


def main(iterations=300, members=32, heldout=256, quiet=False):
    H0 = 0.0 * SZ                                                       # rotating frame, on resonance
    Hops, Hnames = [2 * np.pi * SX / 2, 2 * np.pi * SY / 2], ['x', 'y']
    dt = TOTAL_TIME / STEPS
    k = len(Hops)
    train = noise.ensemble([DETUNING], [noise.ornstein_uhlenbeck(members, STEPS, dt, SIGMA, TAU, 11)], k=k)
    static = noise.ensemble([DETUNING], [noise.quasi_static(members, STEPS, SIGMA, 12)], k=k)
    fresh = noise.ensemble([DETUNING], [noise.ornstein_uhlenbeck(heldout, STEPS, dt, SIGMA, TAU, 13)], k=k)
    kw = dict(total_time=TOTAL_TIME, steps=STEPS, states_concerned_list=[0, 1], maxA=[0.1, 0.1], reg_coeffs={}, show_plots=not quiet, save=False,
              Taylor_terms=[12, 1])
    conv = {'rate': 0.01, 'update_step': 100, 'max_iterations': iterations, 'conv_target': 1e-10, 'learning_rate_decay': 1000}
    np.random.seed(2)
    uks_nominal, _ = Grape(H0, Hops, Hnames, SX, method='Adam', convergence=conv, **kw)
    np.random.seed(2)
    uks_static, _ = Grape(H0, Hops, Hnames, SX, method='Adam', convergence=conv, robust=static, **kw)
    uks_traces, _ = Grape(H0, Hops, Hnames, SX, method='Adam', convergence=conv, robust=train, initial_guess=uks_nominal, **kw)

    def score(uks, ens):
        """The mean infidelity of the pulse over the members of ens: one EVOLVE call."""
        info = {}
        Grape(H0, Hops, Hnames, SX, method='EVOLVE', initial_guess=uks, robust=ens, _restart_info=info, **kw)
        return float(np.mean(info['member_losses'][0]))

    held = [score(u, fresh) for u in (uks_nominal, uks_static, uks_traces)]
    trained = [score(u, train) for u in (uks_nominal, uks_traces)]
    print('held-out mean infidelity over %d fresh traces: nominal %.3e, quasi-static %.3e, traces %.3e' % ((heldout,) + tuple(held)))
    print('training-set mean infidelity over %d traces:   nominal %.3e, traces %.3e' % ((members,) + tuple(trained)))
    return held[0], held[1], held[2], trained[0], trained[1]


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--iterations', type=int, default=300)
    ap.add_argument('--members', type=int, default=32)
    ap.add_argument('--heldout', type=int, default=256)
    a = ap.parse_args()
    main(a.iterations, a.members, a.heldout)
