#!/usr/bin/env python
"""What a control map costs (profiles/control_map.txt): C2 x 64, per-iteration time of the plain engine, a one-member nominal
ensemble, and the same ensemble with an identity control map.  Alternating, REPS repetitions of ITERS iterations each after a warm-up; device
events around the enqueued iterations (qoc_time_iterations).

    python tools/control_map_overhead.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'quantum-optimal-control_amd')):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402

import bench  # noqa: E402
from quantum_optimal_control.core import hip_engine  # noqa: E402
from quantum_optimal_control.helper_functions import control_map as cmap  # noqa: E402

REPS, ITERS, WARM = 7, 200, 50
c, Hs, U0, V, W, dt = bench.build_problem()
k, G = bench.K_OPS, bench.SEEDS_PER_GPU
maxA = np.asarray(c['maxA'], dtype=np.float64)
nominal = dict(operators=[], offsets=np.zeros((1, 0)), amp_scales=np.ones((1, k)), weights=np.ones(1))
kinds = {'plain': {}, 'ensemble': dict(ensemble=nominal), 'identity_map': dict(ensemble=nominal, control_map=cmap.identity(k))}
engines = {}
for name, kw in kinds.items():
    eng = hip_engine.HipEngine(Hs, U0, V, W, maxA, dt, c['total_time'], bench.SLICES, bench.TAYLOR[0], bench.TAYLOR[1], reg_coeffs={},
                               n_seeds=G, **kw)
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
    print('%-13s ms per iteration: median %.4f  min %.4f  max %.4f   (%s)' % (name, np.median(t), min(t), max(t), ' '.join('%.4f' % x for x in t)))
med = {name: float(np.median(t)) for name, t in times.items()}
print('ensemble glue (k_ens_expand + k_ens_reduce): %+.4f ms; map glue (k_map_expand + k_map_reduce): %+.4f ms'
      % (med['ensemble'] - med['plain'], med['identity_map'] - med['ensemble']))
s_e, s_m = engines['ensemble'].scalars(), engines['identity_map'].scalars()
print('identity map equal to no map after %d iterations: %s' % (WARM + REPS * ITERS, all(np.array_equal(s_e[key], s_m[key]) for key in s_e)))
for eng in engines.values():
    eng.close()
