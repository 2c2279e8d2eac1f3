#!/usr/bin/env python
"""Robust GRAPE cost: us per iteration (qoc_time_iterations) of an ensemble engine beside a plain engine of G E control sets on the same
path and plan -- a qubit ensemble (E = 9, 100 slices) and a C2-sized one (n = 32, k = 4, 500 slices, E = 64, one control set).

This tool only times; it never looks at a result.  The C2 x 64 ensemble it times (plan: path=mfma nt=2 expm=8 chunks=16 sweeps=downup) is checked
against the ensemble composed from the CPU oracle by tests/test_robust_families.py (row headline_c2_x64_downup_lazy_final: scalars, gradient,
every member's loss and final unitary, the vectors at every slice, an Adam step), as is every other kernel family an ensemble can run on.

    python tools/robust_bench.py [--iters N]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'quantum-optimal-control_amd')]
from quantum_optimal_control.core import hip_engine  # noqa: E402
from quantum_optimal_control.helper_functions.robust import ensemble_grid  # noqa: E402
from quantum_optimal_control.helper_functions.synthetic_systems import case_c2, herm  # noqa: E402

SZ = np.array([[1, 0], [0, -1]], dtype=complex)
SX = np.array([[0, 1], [1, 0]], dtype=complex)
SY = np.array([[0, -1j], [1j, 0]], dtype=complex)


def inputs(H0, Hops, U, total_time, steps, m, maxA):
    n, dt = len(H0), total_time / steps
    Hs = np.stack([-1j * dt * np.asarray(H0)] + [-1j * dt * np.asarray(h) for h in Hops]).astype(np.complex128)
    V = np.eye(n, dtype=np.complex128)[:, :m]
    return Hs, np.eye(n), V, U @ V, np.asarray(maxA, dtype=np.float64), dt, total_time, steps


def timed(args, taylor, G, ens, path, iters, plan_seeds=0):
    eng = hip_engine.HipEngine(*args, taylor[0], taylor[1], reg_coeffs={}, n_seeds=G, path=path, ensemble=ens, plan_seeds=plan_seeds)
    try:
        rng = np.random.default_rng(0)
        eng.set_base(rng.normal(0, 0.1, size=(G, eng.k, eng.steps)))
        p = eng.adam_params(rate=0.01, conv_target=-1.0, min_grad=-1.0, max_iterations=10 ** 9)
        eng.time_iterations(p, 20)
        ms = min(eng.time_iterations(p, iters) for _ in range(3))
        return 1e3 * ms / iters, ' '.join('%s=%s' % kv for kv in eng.plan.items())
    finally:
        eng.close()


def row(name, args, taylor, G, ens, iters):
    E = len(ens['weights'])
    us_e, plan_e = timed(args, taylor, G, ens, hip_engine.PATH_AUTO, iters)
    path = {'mfma': hip_engine.PATH_MFMA, 'gemm': hip_engine.PATH_GEMM, 'st_fused': hip_engine.PATH_ST_FUSED}.get(plan_e.split()[0][5:],
                                                                                                             hip_engine.PATH_GENERIC)
    # the plain batch: G E control sets, k + q controls (the perturbation rows become ordinary controls), on the ensemble's path
    Hs = args[0]
    q = len(ens['operators'])
    Hs_p = np.concatenate([Hs] + ([np.stack([-1j * args[5] * p for p in ens['operators']])] if q else []))
    pargs = (Hs_p,) + args[1:4] + (np.concatenate([args[4], np.ones(q)]),) + args[5:]
    us_p, plan_p = timed(pargs, taylor, G * E, None, path, iters)
    print('%-34s ensemble %9.1f us  plain G*E=%-4d %9.1f us  ratio %.3f' % (name, us_e, G * E, us_p, us_e / us_p))
    print('    ensemble plan: %s' % plan_e)
    print('    plain plan:    %s' % plan_p)


def main(iters=200):
    print('# robust GRAPE: us per iteration (qoc_time_iterations, best of 3 x %d), %s' % (iters, hip_engine.device_info()['name']))
    ens_q = ensemble_grid(operators=[2 * np.pi * SZ / 2], offsets=np.array([-0.005, 0.0, 0.005])[:, None], amp_scales=[0.95, 1.0, 1.05], k=2)
    row('qubit, 100 slices, E = 9, G = 1', inputs(0 * SZ, [2 * np.pi * SX / 2, 2 * np.pi * SY / 2], SX, 40.0, 100, 2, [0.1, 0.1]), (12, 2),
        1, ens_q, iters)
    c = case_c2()
    rng = np.random.default_rng(1)
    ens_c2 = ensemble_grid(operators=[2 * np.pi * 0.01 * herm(rng, 32)], offsets=np.linspace(-1, 1, 8)[:, None],
                           amp_scales=np.linspace(0.95, 1.05, 8), k=4)
    row('C2 (n = 32, k = 4, 500 slices), E = 64, G = 1', inputs(c['H0'], c['Hops'], c['U'], c['total_time'], c['steps'], 8, c['maxA']),
        tuple(c['Taylor_terms']), 1, ens_c2, max(20, iters // 10))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    main(ap.parse_args().iters)
