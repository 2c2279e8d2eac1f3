#!/usr/bin/env python
"""What the running costs of the open-system engine cost per iteration (profiles/running_costs.txt), on the shapes of
profiles/open_system.txt: one control set, k = 2, (T, s) = (6, 1).  The same engine, made through qoc_create_open_costs, with L = 0, 1 and 4
observables (dense Hermitian, power 2), alternating within one process: ROUNDS rounds over the three engines, each timing ITERS enqueued
iterations between device events (qoc_time_iterations) after a warm-up.

    python tools/running_cost_overhead.py [--rounds 3] [--iters 20]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'quantum-optimal-control_amd')):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

from quantum_optimal_control.core import hip_engine  # noqa: E402
from quantum_optimal_control.helper_functions import open_system  # noqa: E402
from quantum_optimal_control.helper_functions.synthetic_systems import herm, random_unitary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    args = ap.parse_args()
    WARM, COUNTS = 5, (0, 1, 4)
    SHAPES = [(3, 2, 100, 2), (9, 4, 200, 4), (32, 2, 100, 2)]        # n, m, slices, c
    k, T, s, dt = 2, 6, 1, 0.4
    params = hip_engine.HipEngine.adam_params(rate=0.01, conv_target=-1.0, min_grad=-1.0, max_iterations=10 ** 6, poll_every=10 ** 6)
    for n, m, steps, c in SHAPES:
        rng = np.random.default_rng(5)
        H0, Hops = herm(rng, n), [0.5 * herm(rng, n) for _ in range(k)]
        Hs = np.stack([-1j * dt * H0] + [-1j * dt * h for h in Hops])
        U0, target = np.eye(n, dtype=complex), random_unitary(rng, n)
        V = np.ascontiguousarray(np.eye(n, dtype=complex)[:, :m])
        W = np.ascontiguousarray(target[:, :m])
        a = np.diag(np.sqrt(np.arange(1, n)), 1).astype(complex)
        pool = [a, a.conj().T @ a] + [rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n)) for _ in range(c - 2)]
        ops = [np.sqrt(0.1) * x / np.linalg.norm(x, 2) for x in pool[:c]]
        obs = [herm(rng, n) for _ in range(max(COUNTS))]
        engines = {}
        try:
            for L in COUNTS:
                costs = [open_system.observable_cost(o / np.linalg.norm(o, 2), 1.0) for o in obs[:L]]
                eng = hip_engine.HipEngine(Hs, U0, V, W, np.array([1.0, 1.25]), dt, dt * steps, steps, T, s, reg_coeffs={}, n_seeds=1, collapse_ops=ops,
                                           running_costs=costs)
                engines[L] = eng
                eng.set_base(np.random.default_rng(6).normal(0.0, 0.5, size=(1, k, steps)))
                eng.iterate(params, WARM)
                eng.sync()
            times = {L: [] for L in COUNTS}
            for _ in range(args.rounds):
                for L in COUNTS:
                    times[L].append(engines[L].time_iterations(params, args.iters) / args.iters)
            base = float(np.median(times[0]))
            for L in COUNTS:
                t = times[L]
                print('n=%d m=%d slices=%d c=%d k=%d T=%d s=%d L=%d: ms per iteration median %.4f min %.4f max %.4f (%+.2f %% against L=0; %d x %d iterations '
                      'after %d warm-up, alternating)' % (n, m, steps, c, k, T, s, L, np.median(t), min(t), max(t), 100.0 * (np.median(t) / base - 1.0),
                                                          args.rounds, args.iters, WARM), flush=True)
        finally:                                                  # (also when an engine cannot be made or a launch fails)
            for eng in engines.values():
                eng.close()


if __name__ == '__main__':
    main()
