#!/usr/bin/env python
"""What the device axis of the member table costs (profiles/fleet.txt): C2 x 64, per-iteration time of a one-member nominal
ensemble and of a fleet of 64 devices x 1 nominal member (one control set per device: every control set reads its own block of the table).
Alternating, REPS repetitions of ITERS iterations each after a warm-up; device events around the enqueued iterations (qoc_time_iterations).

    python tools/fleet_overhead.py                      # both engines side by side
    python tools/fleet_overhead.py --kinds ensemble     # one of them (a kernel trace of its own; a tree without fleets)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'quantum-optimal-control_amd')):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

import bench  # noqa: E402
from quantum_optimal_control.core import hip_engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--kinds', default='ensemble,fleet')
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--iters', type=int, default=200)
args = ap.parse_args()
REPS, ITERS, WARM = args.reps, args.iters, 50
c, Hs, U0, V, W, dt = bench.build_problem()
k, G = bench.K_OPS, bench.SEEDS_PER_GPU
maxA = np.asarray(c['maxA'], dtype=np.float64)
nominal = dict(operators=[], offsets=np.zeros((1, 0)), amp_scales=np.ones((1, k)), weights=np.ones(1))
kinds = {'ensemble': dict(ensemble=nominal), 'fleet': dict(ensemble=nominal, fleet=dict(amp_scales=np.ones((G, 1, k))))}
engines = {}
for name in args.kinds.split(','):
    eng = hip_engine.HipEngine(Hs, U0, V, W, maxA, dt, c['total_time'], bench.SLICES, bench.TAYLOR[0], bench.TAYLOR[1], reg_coeffs={},
                               n_seeds=G, **kinds[name])
    eng.set_base(bench.seed_bases(0, G))
    engines[name] = eng
    print(name, 'plan:', ' '.join('%s=%s' % kv for kv in eng.plan.items()))
params = hip_engine.HipEngine.adam_params(rate=0.01, conv_target=-1.0, min_grad=-1.0, max_iterations=10 ** 6, poll_every=10 ** 6)
for eng in engines.values():
    eng.iterate(params, WARM)
    eng.sync()
times = {name: [] for name in engines}
for rep in range(REPS):
    for name, eng in engines.items():
        times[name].append(eng.time_iterations(params, ITERS) / ITERS)
for name, t in times.items():
    print('%-9s ms per iteration: median %.4f  min %.4f  max %.4f   (%s)' % (name, np.median(t), min(t), max(t), ' '.join('%.4f' % x for x in t)))
if len(engines) == 2:
    s_e, s_f = engines['ensemble'].scalars(), engines['fleet'].scalars()
    print('device axis: %+.4f ms; fleet of nominal devices equal to the ensemble after %d iterations: %s'
          % (float(np.median(times['fleet'])) - float(np.median(times['ensemble'])), WARM + REPS * ITERS,
             all(np.array_equal(s_e[key], s_f[key]) for key in s_e)))
for eng in engines.values():
    eng.close()
