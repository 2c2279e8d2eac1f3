#!/usr/bin/env python
"""What an iteration of the device-resident L-BFGS loop (qoc_iterate_lbfgs, csrc/qoc_lbfgs.h) costs beside an iteration of the Adam loop on the
same engine, and what the loop needs on the coarse qutrit gate beside scipy's L-BFGS-B.

    python tools/lbfgs_cost.py cost      four engines: a qubit (workgroup-resident path), one C2 trajectory (latency mode), C2 x 64, an open engine
                                         (n = 9, four collapse operators, 200 slices).  Microseconds per loop iteration, stop rules that never fire.
                                         Adam (qoc_iterate): wall clock around `iters` enqueued iterations between two qoc_sync calls, five repeats
                                         after a warm-up of 20, and the same through qoc_time_iterations' hipEvent bracket -- the C ABI has no such
                                         bracket for the L-BFGS loop, the pair shows what the wall clock adds.  L-BFGS (qoc_iterate_lbfgs, history 8),
                                         wall clock: `early` = the first 12 iterations after qoc_set_base, five repeats from the same start (accepted
                                         steps); `late` = `iters` iterations after 300 more (rejected trials dominate).  Beside them a host-driven
                                         evaluation (qoc_eval without the gradient download) as the scipy route pays it
    python tools/lbfgs_cost.py wall      examples/coarse_qutrit_x_gate.py to 1e-10 with exact_gradient=True: method='L-BFGS-B' (scipy) and
                                         method='LBFGS', wall seconds of the whole Grape call (engine creation included), three repeats
    python tools/lbfgs_cost.py trace     60 L-BFGS iterations on each of the four engines and nothing else: the workload for ONE
                                         rocprofv3 --kernel-trace run
    python tools/lbfgs_cost.py summarise DIR      k_lbfgs_step's own time per engine from the kernel trace CSV under DIR (dispatches in launch
                                         order, 60 per engine, the first 10 of each dropped)

This tool only times; tests/test_lbfgs_gpu.py checks what the loop computes."""
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'quantum-optimal-control_amd'), os.path.join(ROOT, 'examples')]

NAMES = ['qubit (small)', 'C2 x 1 (latency)', 'C2 x 64', 'open n=9 c=4']
TRACE_ITERS = 60


def engines():
    from quantum_optimal_control.core import hip_engine as P
    from tests.golden import cases
    from tests.helpers import oracle_system
    from tests.test_open_system import open_case

    def engine(sp, n_seeds, **kw):
        return P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, state_transfer=sp.state_transfer,
                           reg_coeffs=sp.reg_coeffs, one_minus_gauss=sp.one_minus_gauss, n_seeds=n_seeds, **kw)
    sp, sp2 = oracle_system(cases.case_c1()), oracle_system(cases.case_c2())
    spo, ops = open_case(9, 2, 4, 200, (6, 1), 4, seed=24)
    b64 = np.stack([sp2.base0 * (1 + 0.01 * i) for i in range(64)])
    return [(NAMES[0], lambda: engine(sp, 1), sp.base0[None], 200), (NAMES[1], lambda: engine(sp2, 1), sp2.base0[None], 200),
            (NAMES[2], lambda: engine(sp2, 64), b64, 40), (NAMES[3], lambda: engine(spo, 1, collapse_ops=ops), spo.base0[None], 10)]


def loop_params():
    from quantum_optimal_control.core import hip_engine as P
    adam = P.HipEngine.adam_params(rate=1e-4, learning_rate_decay=1e9, conv_target=-1.0, min_grad=-1.0, max_iterations=10 ** 9, poll_every=100)
    lb = P.HipEngine.lbfgs_params(conv_target=-1.0, min_grad=-1.0, max_iterations=10 ** 9, history=8)
    return adam, lb


def timed(fn, eng, iters, reps=5):
    out = []
    for _ in range(reps):
        eng.sync()
        t0 = time.perf_counter()
        fn(iters)
        eng.sync()
        out.append((time.perf_counter() - t0) / iters * 1e6)
    return out


def cost():
    adam, lb = loop_params()
    early_iters = 12                                   # from a fresh start: accepted steps (the history fills to 8 pairs), few rejected trials
    for name, make, bases, iters in engines():
        eng = make()
        eng.set_base(bases)
        eng.iterate(adam, 20)
        a = timed(lambda n: eng.iterate(adam, n), eng, iters)
        # the same iterations inside the engine's own hipEvent bracket (qoc_time_iterations): what the wall clock around two syncs adds
        a_ev = [eng.time_iterations(adam, iters) * 1e3 / iters for _ in range(5)]
        ev = timed(lambda n: [eng.evaluate(want_grad=False) for _ in range(n)], eng, min(iters, 50), 3)
        early = []
        for _ in range(5):                             # every repeat from the same start: the same steps, accepted ones
            eng.set_base(bases)
            early += timed(lambda n: eng.iterate_lbfgs(lb, n), eng, min(early_iters, iters), 1)
        eng.iterate_lbfgs(lb, 300 if iters >= 100 else 3 * iters)       # ... and far into the run: rejected trials dominate
        late = timed(lambda n: eng.iterate_lbfgs(lb, n), eng, iters)
        print(json.dumps(dict(config=name, path=eng.plan.get('path'), tail=eng.plan.get('tail'), iters=iters, adam_wall_us=[round(x, 2) for x in a],
                              adam_event_us=[round(x, 2) for x in a_ev], host_eval_us=[round(x, 2) for x in ev],
                              lbfgs_early_us=[round(x, 2) for x in early], lbfgs_early_iters=min(early_iters, iters), lbfgs_late_us=[round(x, 2) for x in late],
                              adam_median=round(float(np.median(a)), 2), adam_event_median=round(float(np.median(a_ev)), 2),
                              lbfgs_early_median=round(float(np.median(early)), 2), lbfgs_late_median=round(float(np.median(late)), 2))), flush=True)
        eng.close()


def wall():
    import coarse_qutrit_x_gate as coarse
    import lbfgs_restarts
    conv = dict(coarse.CONVERGENCE, conv_target=1e-10)
    for rep in range(3):
        r = coarse.run(True, convergence=dict(conv))
        q = lbfgs_restarts.run(restarts=1, convergence=dict(conv))
        print(json.dumps(dict(rep=rep, scipy_evaluations=r['evaluations'], scipy_seconds=round(r['seconds'], 4), scipy_infidelity=r['infidelity'],
                              lbfgs_evaluations=int(q['iterations'][0]) + 1, lbfgs_seconds=round(q['seconds'], 4), lbfgs_loss=float(q['loss'][0]),
                              lbfgs_infidelity=q['infidelity'])), flush=True)


def trace():
    _, lb = loop_params()
    for name, make, bases, _ in engines():
        eng = make()
        eng.set_base(bases)
        eng.iterate_lbfgs(lb, TRACE_ITERS)
        eng.sync()
        eng.close()


def summarise(directory):
    rows = []
    for f in glob.glob(os.path.join(directory, '**', '*kernel_trace.csv'), recursive=True):
        for r in csv.DictReader(open(f)):
            if 'k_lbfgs_step' in r['Kernel_Name']:
                rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']) - int(r['Start_Timestamp']), r.get('Workgroup_Size_X', r.get('Workgroup_Size', '?')),
                             r.get('Grid_Size_X', r.get('Grid_Size', '?')), r.get('VGPR_Count', '?'), r.get('Scratch_Size', r.get('Private_Segment_Size', '?'))))
    rows.sort()
    print('k_lbfgs_step dispatches: %d' % len(rows))
    for i, name in enumerate(NAMES):
        part = rows[TRACE_ITERS * i:TRACE_ITERS * (i + 1)]
        if part:
            d = np.array([p[1] for p in part[10:]]) / 1e3
            print('%-18s workgroup %s grid %s vgpr %s scratch %s: median %.2f us  mean %.2f  min %.2f  max %.2f' % (
                name, part[0][2], part[0][3], part[0][4], part[0][5], np.median(d), d.mean(), d.min(), d.max()))


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'cost'
    if mode == 'summarise':
        summarise(sys.argv[2])
    else:
        {'cost': cost, 'wall': wall, 'trace': trace}[mode]()
