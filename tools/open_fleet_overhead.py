#!/usr/bin/env python
"""What the member axis of the open-system engine costs (profiles/open_fleet.txt): n = 3, k = 2, m = 2, c = 2, 100 slices, (T, s) =
(6, 1), per-iteration time of ONE engine per process -- a fleet of F devices x E members with decay, or the plain open engine with n_seeds = F E
(the same workgroup count).  A process is one side of an A/B run: the caller alternates processes, the library under QOC_HIP_LIBRARY deciding which
commit a 'plain' process measures.  Device events around the enqueued iterations (qoc_time_iterations), REPS repetitions of ITERS iterations after a
warm-up.

    python tools/open_fleet_overhead.py --kind fleet --members 1        # F = 16, E = 1
    python tools/open_fleet_overhead.py --kind plain --members 9        # n_seeds = 144
    rocprofv3 --kernel-trace --stats ... -- python tools/open_fleet_overhead.py --kind fleet --reps 1 --iters 120     # the glue launches"""
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

ap = argparse.ArgumentParser()
ap.add_argument('--kind', choices=['fleet', 'plain'], default='fleet')
ap.add_argument('--devices', type=int, default=16)
ap.add_argument('--members', type=int, default=1)
ap.add_argument('--perturb', type=int, default=1, choices=[0, 1], help='q: drift perturbations of a fleet (a frozen control row each)')
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--iters', type=int, default=100)
args = ap.parse_args()
F, E, REPS, ITERS, WARM = args.devices, args.members, args.reps, args.iters, 20
n, k, m, steps, T, s, dt = 3, 2, 2, 100, 6, 1, 0.4
rng = np.random.default_rng(5)
H0, Hops = herm(rng, n), [0.5 * herm(rng, n) for _ in range(k)]
Hs = np.stack([-1j * dt * H0] + [-1j * dt * h for h in Hops])
U0, target = np.eye(n, dtype=complex), random_unitary(rng, n)
V = np.ascontiguousarray(np.eye(n, dtype=complex)[:, :m])
W = np.ascontiguousarray(target[:, :m])
ops = [open_system.relaxation(n, 50.0), open_system.dephasing(n, 80.0)]
maxA = np.array([1.0, 1.25])
common = dict(reg_coeffs={}, n_seeds=F if args.kind == 'fleet' else F * E)
if args.kind == 'fleet':
    q = args.perturb
    P = [herm(rng, n)][:q]
    ens = dict(operators=P, offsets=np.zeros((E, q)), amp_scales=np.ones((E, k)), weights=np.full(E, 1.0 / E))
    fleet = dict(offsets=rng.uniform(-0.2, 0.2, size=(F, E, q)), amp_scales=rng.uniform(0.9, 1.1, size=(F, E, k)), collapse_ops=ops,
                 rate_scales=rng.uniform(0.5, 2.0, size=(F, E, len(ops))))
    eng = hip_engine.HipEngine(Hs, U0, V, W, maxA, dt, dt * steps, steps, T, s, ensemble=ens, fleet=fleet, **common)
else:
    eng = hip_engine.HipEngine(Hs, U0, V, W, maxA, dt, dt * steps, steps, T, s, collapse_ops=ops, **common)
eng.set_base(np.random.default_rng(6).normal(0.0, 0.5, size=(eng.n_seeds, k, steps)))
params = hip_engine.HipEngine.adam_params(rate=0.01, conv_target=-1.0, min_grad=-1.0, max_iterations=10 ** 6, poll_every=10 ** 6)
eng.iterate(params, WARM)
eng.sync()
t = [eng.time_iterations(params, ITERS) / ITERS for _ in range(REPS)]
print('%s F=%d E=%d q=%d trajectories=%d library=%s plan: %s' % (args.kind, F, E, args.perturb if args.kind == 'fleet' else 0, F * E, os.environ.get('QOC_HIP_LIBRARY', 'in-tree'),
                                                            ' '.join('%s=%s' % kv for kv in eng.plan.items())))
print('%s F=%d E=%d ms per iteration: median %.4f  min %.4f  max %.4f   (%s; %d x %d iterations after %d warm-up)'
      % (args.kind, F, E, np.median(t), min(t), max(t), ' '.join('%.4f' % x for x in t), REPS, ITERS, WARM))
eng.close()
