#!/usr/bin/env python
"""What the exact gradient (HipEngine(exact_gradient=True), csrc/qoc_exact_grad.h) costs beside the first-order one.

Four configurations, three engines each: first-order on the generic path, exact on the generic path, first-order as AUTO plans it.

    (a) C2, one trajectory: n = 32, k = 4, 500 slices, m = 8, (T, s) = (5, 3)
    (b) the same, 64 control sets
    (c) C3-shaped state transfer: n = 64, k = 6, 1000 slices, one trajectory, T = 10
    (d) the 10-slice qutrit X gate of examples/coarse_qutrit_x_gate.py, (T, s) = (12, 3)

Reported: milliseconds per evaluation, the median of `--samples` hipEvent timings (qoc_time_iterations) after a warm-up.  An "evaluation" is one
loop iteration with the learning rate 0: controls, forward, loss, backward, the tail -- the launches of qoc_eval -- at a point that does not
move.  Beside each ratio exact / first-order the arithmetic estimate of DESIGN.md ("Exact gradient", cost model) in complex FMAs per slice.
This tool only times; tests/test_exact_gradient_gpu.py checks what the engines compute.

    python tools/exact_gradient_cost.py [--samples N] [--only a,b,c,d] [--engines first,exact,auto]

--engines exact under rocprofv3 --kernel-trace --stats shows the share of k_exact_grad in an evaluation."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'quantum-optimal-control_amd'), os.path.join(ROOT, 'examples')]


def unitary_args(c, n, m):
    steps = c['steps']
    dt = c['total_time'] / steps
    Hs = np.stack([-1j * dt * np.asarray(c['H0'])] + [-1j * dt * np.asarray(h) for h in c['Hops']]).astype(np.complex128)
    V = np.eye(n, dtype=np.complex128)[:, :m]
    return (Hs, np.eye(n), V, np.asarray(c['U']) @ V, np.asarray(c['maxA'], dtype=np.float64), dt, c['total_time'], steps, c['Taylor_terms'][0],
            c['Taylor_terms'][1]), dict(reg_coeffs={})


def state_args(c):
    steps = c['steps']
    dt = c['total_time'] / steps
    Hs = np.stack([-1j * dt * np.asarray(c['H0'])] + [-1j * dt * np.asarray(h) for h in c['Hops']]).astype(np.complex128)
    V = np.stack(c['states_concerned_list'], axis=1).astype(np.complex128)
    W = np.stack(c['U'], axis=1).astype(np.complex128)
    return (Hs, None, V, W, np.asarray(c['maxA'], dtype=np.float64), dt, c['total_time'], steps, c['Taylor_terms'][0], 0), dict(
        reg_coeffs=c['reg_coeffs'], state_transfer=True)


def estimate(n, k, m, T, s, state_transfer):
    """Complex FMAs per slice: (first-order generic, exact generic)."""
    if state_transfer:
        D, N = T - 1, 1
        forward, sweep = D * n * n * m, D * n * n * m
        first = forward + sweep + k * n * n * m
    else:
        D, N = T, 1 << s
        forward, sweep = (T - 1 + s) * n ** 3 + n ** 3 + n * n * m, n * n * m
        first = forward + sweep + k * n * n * m
    # sub-states (N - 1 chains of D products), per sub-step the x chain (D - 1), the y chain (D) and the accumulator (D); k contractions with M
    exact = forward + sweep + ((N - 1) * D + N * (3 * D - 1)) * n * n * m + k * n * n
    return first, exact


def configurations():
    from quantum_optimal_control.helper_functions.synthetic_systems import case_c2, case_c3
    import coarse_qutrit_x_gate as ex
    c2 = case_c2()
    a_args, a_kw = unitary_args(c2, 32, 8)
    c3 = case_c3()
    c_args, c_kw = state_args(c3)
    H0, Hops, _, U = ex.problem()
    q = dict(H0=H0, Hops=Hops, U=U, total_time=ex.TOTAL_TIME, steps=ex.STEPS, maxA=ex.MAXA, Taylor_terms=ex.TAYLOR)
    d_args, d_kw = unitary_args(q, 3, 2)
    return [('a', 'C2 n=32 k=4 500 slices m=8 (5,3), 1 control set', a_args, a_kw, 1, (32, 4, 8, 5, 3, False)),
            ('b', 'C2 n=32 k=4 500 slices m=8 (5,3), 64 control sets', a_args, a_kw, 64, (32, 4, 8, 5, 3, False)),
            ('c', 'C3 state transfer n=64 k=6 1000 slices m=1 T=10, 1 control set', c_args, c_kw, 1, (64, 6, 1, 10, 0, True)),
            ('d', 'qutrit X gate n=3 k=2 10 slices m=2 (12,3), 1 control set', d_args, d_kw, 1, (3, 2, 2, 12, 3, False))]


def main(samples, only, engines):
    from quantum_optimal_control.core import hip_engine
    P = hip_engine
    print('# exact gradient: ms per evaluation (median of %d hipEvent timings after warm-up), %s' % (samples, P.device_info()['name']))
    for tag, text, args, kw, G, shape in configurations():
        if only and tag not in only:
            continue
        print('(%s) %s' % (tag, text))
        k, steps = args[0].shape[0] - 1, args[7]
        base = np.random.default_rng(0).normal(0, 1.0 / np.sqrt(steps), size=(G, k, steps))
        med = {}
        for key, name, ekw in (('first', 'first-order generic', dict(path=P.PATH_GENERIC)),
                               ('exact', 'exact generic', dict(path=P.PATH_GENERIC, exact_gradient=True)),
                               ('auto', 'first-order AUTO', dict(path=P.PATH_AUTO))):
            if engines and key not in engines:
                continue
            eng = P.HipEngine(*args, n_seeds=G, **kw, **ekw)
            try:
                eng.set_base(base)
                p = eng.adam_params(rate=0.0, conv_target=-1.0, min_grad=-1.0, max_iterations=10 ** 9)
                eng.time_iterations(p, 3)                                    # warm-up
                ts = sorted(eng.time_iterations(p, 1) for _ in range(samples))
                med[name] = ts[len(ts) // 2]
                print('    %-20s median %9.4f ms   min %9.4f   max %9.4f   plan: %s' % (name, med[name], ts[0], ts[-1],
                                                                                         ' '.join('%s=%s' % kv for kv in eng.plan.items())))
            finally:
                eng.close()
        if len(med) < 3:
            continue
        first, exact = estimate(*shape)
        print('    exact / first-order on the generic path: measured %.2f, arithmetic estimate %.2f (%.3g / %.3g complex FMAs per slice)' % (
            med['exact generic'] / med['first-order generic'], exact / first, exact, first))
        print('    exact generic / first-order AUTO: measured %.2f' % (med['exact generic'] / med['first-order AUTO']))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=21)
    ap.add_argument('--only', default='')
    ap.add_argument('--engines', default='')
    a = ap.parse_args()
    main(a.samples, [x for x in a.only.split(',') if x], [x for x in a.engines.split(',') if x])
