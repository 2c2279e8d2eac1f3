#!/usr/bin/env python
"""What a table of noise traces costs (profiles/noise_traces.txt): per loop iteration, the same ensemble engine without a table
(k_ens_expand) and with one (k_ens_expand_traces), alternating, REPS repetitions of --iters iterations each after a warm-up; device events around
the enqueued iterations (qoc_time_iterations).  Two configurations: the C2 x 64-member ensemble of tools/robust_bench.py (n = 32, k = 4, 500 slices)
and a qubit with 1024 members (100 slices).  This tool only times; it never looks at a result.

    python tools/noise_traces_bench.py [--config c2|qubit|both] [--mode both|no_table|table] [--iters N] [--root DIR]

--root DIR: take the package and the library from another checkout (the parent commit, built there: its engines know no table, so only no_table
runs).  Under `rocprofv3 --kernel-trace --stats -- python tools/noise_traces_bench.py --mode table --reps 1` the expand kernel's own time is the
row k_ens_expand_traces of the kernel statistics (k_ens_expand with --mode no_table)."""
import argparse
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument('--config', default='both', choices=['c2', 'qubit', 'both'])
ap.add_argument('--mode', default='both', choices=['both', 'no_table', 'table'])
ap.add_argument('--iters', type=int, default=0, help='iterations per repetition (0: 20 for c2, 200 for the qubit)')
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path[:0] = [ROOT, os.path.join(ROOT, 'quantum-optimal-control_amd')]
from quantum_optimal_control.core import hip_engine  # noqa: E402
from quantum_optimal_control.helper_functions.robust import ensemble_grid, validate  # noqa: E402
from quantum_optimal_control.helper_functions.synthetic_systems import case_c2, herm  # noqa: E402

SZ = np.array([[1, 0], [0, -1]], dtype=complex)
SX = np.array([[0, 1], [1, 0]], dtype=complex)
SY = np.array([[0, -1j], [1j, 0]], dtype=complex)
HAS_TABLE = hasattr(hip_engine.HipEngine, 'set_traces')


def inputs(H0, Hops, U, total_time, steps, m, maxA):
    n, dt = len(H0), total_time / steps
    Hs = np.stack([-1j * dt * np.asarray(H0)] + [-1j * dt * np.asarray(h) for h in Hops]).astype(np.complex128)
    V = np.eye(n, dtype=np.complex128)[:, :m]
    return Hs, np.eye(n), V, U @ V, np.asarray(maxA, dtype=np.float64), dt, total_time, steps


def configurations():
    out = {}
    if args.config in ('c2', 'both'):
        c = case_c2()
        ens = ensemble_grid(operators=[2 * np.pi * 0.01 * herm(np.random.default_rng(1), 32)], offsets=np.linspace(-1, 1, 8)[:, None],
                            amp_scales=np.linspace(0.95, 1.05, 8), k=4)
        out['C2 (n = 32, k = 4, 500 slices), E = 64'] = (inputs(c['H0'], c['Hops'], c['U'], c['total_time'], c['steps'], 8, c['maxA']),
                                                         tuple(c['Taylor_terms']), ens, args.iters or 20, 0.2)
    if args.config in ('qubit', 'both'):
        rng = np.random.default_rng(2)
        ens = validate(dict(operators=[2 * np.pi * SZ / 2], offsets=rng.normal(0, 0.005, size=(1024, 1)), amp_scales=np.ones((1024, 2))), 2, 2)
        out['qubit, 100 slices, E = 1024'] = (inputs(0 * SZ, [2 * np.pi * SX / 2, 2 * np.pi * SY / 2], SX, 40.0, 100, 2, [0.1, 0.1]), (12, 2), ens,
                                              args.iters or 200, 0.005)
    return out


def main():
    print('# noise traces: ms per loop iteration (qoc_time_iterations, %d x alternating), %s, tree %s' % (args.reps, hip_engine.device_info()['name'],
                                                                                                     'given by --root' if args.root != ap.get_default('root') else 'this one'))
    modes = [m for m in ('no_table', 'table') if args.mode in ('both', m) and (m == 'no_table' or HAS_TABLE)]
    for name, (a, taylor, ens, iters, scale) in configurations().items():
        E, q, steps = len(ens['weights']), len(ens['operators']), a[7]
        engines = {}
        for mode in modes:
            eng = hip_engine.HipEngine(*a, taylor[0], taylor[1], reg_coeffs={}, n_seeds=1, ensemble=ens)
            if mode == 'table':
                eng.set_traces(np.random.default_rng(3).normal(0, scale, size=(E, q, steps)))
            eng.set_base(np.random.default_rng(0).normal(0, 0.1, size=(1, eng.k, eng.steps)))
            engines[mode] = eng
            print('%s  %s plan: %s' % (name, mode, ' '.join('%s=%s' % kv for kv in eng.plan.items())))
        p = hip_engine.HipEngine.adam_params(rate=0.01, conv_target=-1.0, min_grad=-1.0, max_iterations=10 ** 9, poll_every=10 ** 9)
        for eng in engines.values():
            eng.time_iterations(p, max(5, iters // 4))
        times = {mode: [] for mode in engines}
        for _ in range(args.reps):
            for mode, eng in engines.items():
                times[mode].append(eng.time_iterations(p, iters) / iters)
        for mode, t in times.items():
            print('%s  %-8s ms per iteration: median %.4f  min %.4f  max %.4f   (%s)' % (name, mode, np.median(t), min(t), max(t), ' '.join('%.4f' % x for x in t)))
        if len(times) == 2:
            print('%s  table - no_table: %+.4f ms (medians); the table holds %d doubles = %.1f KiB' % (
                name, np.median(times['table']) - np.median(times['no_table']), E * q * steps, E * q * steps * 8 / 1024.0))
        for eng in engines.values():
            eng.close()


if __name__ == '__main__':
    main()
