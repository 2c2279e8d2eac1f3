#!/usr/bin/env python
"""Transfer-function GRAPE: what the response glue (k_shape_expand / k_shape_reduce) costs beside the heavy kernels, at the bench size --
C2 (n = 32, k = 4, 500 slices, m = 8, Taylor (5, 3)), 64 control sets, MFMA path.  One process, qoc_time_iterations, three alternating rounds
after a warm-up:

    (a) a one-member nominal ensemble engine (k_ens_expand / k_ens_reduce: the glue that moves the same bytes without a matrix)
    (b) hold, P = 125
    (c) gaussian_filter, P = 125, sigma = 2 slices
    (d) a dense P = 125 response (recorded only)

This tool only times; tests/test_transfer_gpu.py checks what the engines compute.

    python tools/transfer_overhead.py [--iters N] [--package DIR] [--only-ensemble]

--package DIR: import quantum_optimal_control (and with it its lib/libqoc_hip.so) from DIR instead of this tree, e.g. a build of an earlier
commit; with --only-ensemble only (a) is timed, which every commit since the ensemble engine can do."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(iters, package, only_ensemble):
    sys.path[:0] = [ROOT, package or os.path.join(ROOT, 'quantum-optimal-control_amd')]
    from quantum_optimal_control.core import hip_engine
    from quantum_optimal_control.helper_functions.synthetic_systems import case_c2
    c = case_c2()
    n, k, steps, m, G, Pn = 32, 4, c['steps'], 8, 64, 125
    dt = c['total_time'] / steps
    Hs = np.stack([-1j * dt * np.asarray(c['H0'])] + [-1j * dt * np.asarray(h) for h in c['Hops']]).astype(np.complex128)
    V = np.eye(n, dtype=np.complex128)[:, :m]
    args = (Hs, np.eye(n), V, c['U'] @ V, np.asarray(c['maxA'], dtype=np.float64), dt, c['total_time'], steps, c['Taylor_terms'][0],
            c['Taylor_terms'][1])
    nominal = dict(operators=[], offsets=np.zeros((1, 0)), amp_scales=np.ones((1, k)), weights=np.ones(1))
    rows = [('a ensemble of one nominal member', dict(ensemble=nominal), steps)]
    if not only_ensemble:
        from quantum_optimal_control.helper_functions import transfer as tf
        dense = np.random.default_rng(2).uniform(-1.0, 1.0, size=(steps, Pn))
        dense = 0.9 * dense / np.sum(np.abs(dense), axis=1)[:, None]
        rows += [('b hold P=125', dict(transfer=tf.hold(steps, Pn).matrix), Pn),
                 ('c gaussian P=125 sigma=2 slices', dict(transfer=tf.gaussian_filter(steps, Pn, c['total_time'], 2 * dt).matrix), Pn),
                 ('d dense P=125', dict(transfer=dense), Pn)]
    engines = []
    try:
        for name, kw, width in rows:
            eng = hip_engine.HipEngine(*args, reg_coeffs={}, n_seeds=G, path=hip_engine.PATH_MFMA, **kw)
            eng.set_base(np.random.default_rng(0).normal(0, 0.1, size=(G, k, width)))
            engines.append((name, eng, eng.adam_params(rate=0.01, conv_target=-1.0, min_grad=-1.0, max_iterations=10 ** 9)))
        print('# transfer overhead: ms per iteration (qoc_time_iterations, %d iterations per round), C2 x %d control sets, %s, library %s' % (
            iters, G, hip_engine.device_info()['name'], hip_engine.LIB_PATH))
        for name, eng, p in engines:
            eng.time_iterations(p, 20)                                       # warm-up
        times = {name: [] for name, _, _ in engines}
        for _ in range(3):                                                   # alternating rounds
            for name, eng, p in engines:
                times[name].append(eng.time_iterations(p, iters) / iters)
        base = min(times[engines[0][0]])
        for name, eng, p in engines:
            t = times[name]
            print('%-34s rounds %s ms  best %.4f ms  vs (a) %+.2f %%' % (name, ' '.join('%.4f' % x for x in t), min(t), 100.0 * (min(t) / base - 1.0)))
            print('    plan: %s' % ' '.join('%s=%s' % kv for kv in eng.plan.items()))
    finally:
        for _, eng, _ in engines:
            eng.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=500)
    ap.add_argument('--package', default=None)
    ap.add_argument('--only-ensemble', action='store_true')
    a = ap.parse_args()
    main(a.iters, a.package, a.only_ensemble)
