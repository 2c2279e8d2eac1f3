#!/usr/bin/env python
"""Risk-sensitive robust GRAPE cost: us per iteration (qoc_time_iterations) of the two ensembles of tools/robust_bench.py -- a qubit (E = 9, 100
slices) and C2 x 64 members (n = 32, k = 4, 500 slices, one control set) -- with the mean objective (risk 0: the launches of an engine that
never heard of a risk) and with risk 200 (one k_ens_tilt launch more, the reduce reads the tilted weights).  This tool only times.

    python tools/risk_bench.py [--iters N]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import robust_bench as rbench  # noqa: E402
from robust_bench import SX, SY, SZ, case_c2, ensemble_grid, herm, hip_engine, inputs  # noqa: E402


def row(name, args, taylor, ens, iters, risks=(0.0, 200.0)):
    out = []
    for beta in risks:
        us, plan = rbench.timed(args, taylor, 1, dict(ens, risk=beta), hip_engine.PATH_AUTO, iters)
        out.append(us)
    print('%-46s %s   +%.1f us' % (name, '  '.join('risk %-5g %9.1f us' % (b, u) for b, u in zip(risks, out)), out[-1] - out[0]))
    print('    plan: %s' % plan)


def main(iters=200):
    print('# risk-sensitive robust GRAPE: us per iteration (qoc_time_iterations, best of 3 x %d), %s' % (iters, hip_engine.device_info()['name']))
    ens_q = ensemble_grid(operators=[2 * np.pi * SZ / 2], offsets=np.array([-0.005, 0.0, 0.005])[:, None], amp_scales=[0.95, 1.0, 1.05], k=2)
    row('qubit, 100 slices, E = 9, G = 1', inputs(0 * SZ, [2 * np.pi * SX / 2, 2 * np.pi * SY / 2], SX, 40.0, 100, 2, [0.1, 0.1]), (12, 2), ens_q, iters)
    c = case_c2()
    rng = np.random.default_rng(1)
    ens_c2 = ensemble_grid(operators=[2 * np.pi * 0.01 * herm(rng, 32)], offsets=np.linspace(-1, 1, 8)[:, None],
                           amp_scales=np.linspace(0.95, 1.05, 8), k=4)
    row('C2 (n = 32, k = 4, 500 slices), E = 64, G = 1', inputs(c['H0'], c['Hops'], c['U'], c['total_time'], c['steps'], 8, c['maxA']),
        tuple(c['Taylor_terms']), ens_c2, max(20, iters // 10))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    main(ap.parse_args().iters)
