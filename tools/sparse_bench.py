#!/usr/bin/env python
"""What the sparse state-transfer engine (qoc_create_sparse, csrc/qoc_sparse.h) costs on XX spin chains beside the dense engine AUTO picks for the same
problem, from the same library -- the numbers of profiles/sparse_state_transfer.txt and DESIGN.md 6g.

    python tools/sparse_bench.py compare   chains of 6, 8 and 10 spins (n = 64, 256, 1024), z controls on both ends, 200 slices, the reference's Taylor
                                           rule; one and 64 control sets; ms per loop iteration (qoc_time_iterations: hipEvents around iterations whose
                                           stop rule never fires), sparse against dense.  A dense engine that cannot be created is recorded with its error
    python tools/sparse_bench.py large     the sparse engine alone at 12 and 14 spins, and whether the dense engine can be created there at all (14 spins:
                                           attempted only when the host has the 13 GB its three dense operators take)
    python tools/sparse_bench.py threads   the sweeps' workgroup size: 256 against 1024 threads (QOC_EXPERIMENTAL=1 QOC_SP_THREADS) at every size above,
                                           one and 64 control sets -- what QOC_SP_WIDE_FROM in csrc/qoc_sparse.h rests on
    python tools/sparse_bench.py ensemble [--spins 6,8,10,12] [--members 1,8] [--q 0,bonds] [--layouts 1,2] [--rounds 3]
                                           sparse ensembles (qoc_create_sparse_fleet): the same chains with E members and q perturbation
                                           operators (bonds: one per bond of the chain, spins - 1 of them, offsets of +-5 %), one control set; per-operator
                                           rows (row_layout 1) against merged rows (2), the two engines alive side by side and timed alternately `rounds`
                                           times -- the numbers of profiles/sparse_ensemble.txt and what QOC_SP_MERGED_AUTO in csrc/qoc_sparse.h rests on
    python tools/sparse_bench.py plain     the plain sparse rows at 6 and 10 spins (n = 64, 1024), one and 64 control sets: the figures to hold against
                                           the same rows of another build of the library

This tool only times; tests/test_sparse_gpu.py and tests/test_sparse_ensemble_gpu.py check what the engines compute."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'quantum-optimal-control_amd')]

STEPS = 200


def problem(spins):
    from quantum_optimal_control.core.sparse_parameters import SparseSystemParameters
    from quantum_optimal_control.helper_functions.synthetic_systems import xx_chain
    H0, Hops, names, exc = xx_chain(spins, control_sites=[0, spins - 1])
    np.random.seed(0)
    sp = SparseSystemParameters(H0, Hops, names, [exc(spins - 1)], 2.0 * spins, STEPS, [exc(0)], [2.0, 2.0], None, None, False, 1e-4, {'dwdt': 0.001}, False, None,
                                None, True, True)
    return sp


def engine(sp, n_seeds, dense=False, **kw):
    from quantum_optimal_control.core import hip_engine as P
    ops, _, V, W, _ = sp.engine_inputs()
    common = dict(state_transfer=True, reg_coeffs=sp.reg_coeffs, n_seeds=n_seeds)
    common.update(kw)
    if dense:
        Hs = np.stack([o.toarray() for o in ops])
        return P.HipEngine(Hs, None, V, W, sp.ops_max_amp, sp.dt, sp.total_time, sp.steps, sp.exp_terms, 0, **common)
    return P.HipEngine(None, None, V, W, sp.ops_max_amp, sp.dt, sp.total_time, sp.steps, sp.exp_terms, 0, sparse_ops=ops, **common)


def ms_per_iteration(eng, sp, n_seeds, budget_ms=1500.0):
    from quantum_optimal_control.core import hip_engine as P
    rng = np.random.default_rng(1)
    eng.set_base(rng.normal(0, 1.0 / np.sqrt(sp.steps), size=(n_seeds, sp.ops_len, sp.steps)))
    params = P.HipEngine.adam_params(rate=1e-4, learning_rate_decay=1e9, conv_target=-1.0, min_grad=-1.0, max_iterations=10 ** 9, poll_every=100)
    first = eng.time_iterations(params, 1)                                      # warm-up, and the size of the timed window
    if first > budget_ms:                                                       # (a dense engine far out of its range: that one iteration is the figure)
        return first, first, 1
    iters = int(max(3, min(200, budget_ms / max(first, 1e-3))))
    times = [eng.time_iterations(params, iters) / iters for _ in range(3)]
    return min(times), max(times), iters


def report(tag, eng, sp, n_seeds):
    lo, hi, iters = ms_per_iteration(eng, sp, n_seeds)
    print('%-44s %9.4f ms per iteration (max of 3: %9.4f; %d iterations each)   %s' % (tag, lo, hi, iters, ' '.join('%s=%s' % kv for kv in eng.plan.items())),
          flush=True)


def try_dense(sp, n_seeds, tag):
    from quantum_optimal_control.core import hip_engine as P
    try:
        eng = engine(sp, n_seeds, dense=True)
    except (P.QocError, MemoryError) as exc:
        print('%-44s could not be created: %s' % (tag, str(exc)[:300]), flush=True)
        return
    try:
        report(tag, eng, sp, n_seeds)
    finally:
        eng.close()


def compare():
    for spins in (6, 8, 10):
        sp = problem(spins)
        print('--- %d spins, n = %d, %d slices, Taylor terms %d, stored entries %s' % (spins, 2 ** spins, STEPS, sp.exp_terms, [o.nnz for o in sp.ops_sparse]), flush=True)
        for n_seeds in (1, 64):
            eng = engine(sp, n_seeds)
            try:
                report('sparse %2d spins x %2d control sets' % (spins, n_seeds), eng, sp, n_seeds)
            finally:
                eng.close()
            try_dense(sp, n_seeds, 'dense  %2d spins x %2d control sets' % (spins, n_seeds))


def host_available_bytes():
    with open('/proc/meminfo') as f:
        for line in f:
            if line.startswith('MemAvailable'):
                return int(line.split()[1]) * 1024
    return 0


def large():
    for spins in (12, 14):
        sp = problem(spins)
        print('--- %d spins, n = %d, %d slices, Taylor terms %d, stored entries %s' % (spins, 2 ** spins, STEPS, sp.exp_terms, [o.nnz for o in sp.ops_sparse]), flush=True)
        for n_seeds in (1, 64):
            eng = engine(sp, n_seeds)
            try:
                report('sparse %2d spins x %2d control sets' % (spins, n_seeds), eng, sp, n_seeds)
            finally:
                eng.close()
        need = 3 * (2 ** spins) ** 2 * 16
        if need * 3 > host_available_bytes():
            print('dense  %2d spins: not attempted -- its three dense operators are %.1f GB on the host before anything reaches the GPU' % (spins, need / 1e9), flush=True)
        else:
            try_dense(sp, 1, 'dense  %2d spins x  1 control set' % spins)


def threads():
    os.environ['QOC_EXPERIMENTAL'] = '1'
    for spins in (6, 8, 9, 10, 12, 14):
        sp = problem(spins)
        for n_seeds in (1, 64):
            for t in (256, 1024):
                os.environ['QOC_SP_THREADS'] = str(t)
                eng = engine(sp, n_seeds)
                try:
                    assert eng.plan['threads'] == str(t), eng.plan
                    lo, hi, iters = ms_per_iteration(eng, sp, n_seeds, budget_ms=600.0)
                    print('n = %5d x %2d control sets, %4d threads: %9.4f ms per iteration (max of 3: %9.4f)' % (2 ** spins, n_seeds, t, lo, hi), flush=True)
                finally:
                    eng.close()


def plain():
    for spins in (6, 10):
        sp = problem(spins)
        for n_seeds in (1, 64):
            eng = engine(sp, n_seeds)
            try:
                lo, hi, iters = ms_per_iteration(eng, sp, n_seeds)
                print('plain sparse n = %5d x %2d control sets: %9.4f ms per iteration (max of 3: %9.4f; %d iterations each)' % (2 ** spins, n_seeds, lo, hi, iters), flush=True)
            finally:
                eng.close()


def ensemble_of(spins, E, q):
    """E members over the first q bonds of the chain: member 0 nominal, the others with coupling errors of +-5 %."""
    from quantum_optimal_control.helper_functions import robust
    from quantum_optimal_control.helper_functions.synthetic_systems import xx_bonds
    rng = np.random.default_rng(2)
    off = np.vstack([np.zeros(q), rng.uniform(-0.05, 0.05, size=(E - 1, q))]) if q else np.zeros((E, 0))
    return robust.validate(dict(operators=xx_bonds(spins)[:q], offsets=off, amp_scales=np.ones((E, 2))), 2 ** spins, 2, sparse=True)


def ensemble(argv):
    import argparse
    ap = argparse.ArgumentParser(prog='sparse_bench.py ensemble')
    ap.add_argument('--spins', default='6,8,10,12')
    ap.add_argument('--members', default='1,8')
    ap.add_argument('--q', default='0,bonds')
    ap.add_argument('--layouts', default='1,2')
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args(argv)
    layouts = [int(x) for x in args.layouts.split(',')]
    names = {0: 'auto', 1: 'per_operator', 2: 'merged'}
    for spins in [int(x) for x in args.spins.split(',')]:
        sp = problem(spins)
        print('--- %d spins, n = %d, %d slices, Taylor terms %d' % (spins, 2 ** spins, STEPS, sp.exp_terms), flush=True)
        for qname in args.q.split(','):
            q = spins - 1 if qname == 'bonds' else int(qname)
            for E in [int(x) for x in args.members.split(',')]:
                ens = ensemble_of(spins, E, q)
                engines = {lay: engine(sp, 1, ensemble=ens, row_layout=lay) for lay in layouts}
                try:
                    times = {lay: [] for lay in layouts}
                    for _ in range(args.rounds):                                    # alternating: a drift of the machine hits both alike
                        for lay in layouts:
                            lo, hi, iters = ms_per_iteration(engines[lay], sp, 1, budget_ms=400.0)
                            times[lay] += [lo, hi]
                    for lay in layouts:
                        t = times[lay]
                        print('n = %5d  operators = %2d (q = %2d)  E = %d  %-12s %9.4f ms per iteration (min; max %9.4f over %d windows)  rows=%s merged_width=%s lds=%s'
                              % (2 ** spins, 3 + q, q, E, names[lay], min(t), max(t), len(t), engines[lay].plan['rows'], engines[lay].plan['merged_width'],
                                 engines[lay].plan['lds']), flush=True)
                finally:
                    for eng in engines.values():
                        eng.close()


if __name__ == '__main__':
    if sys.argv[1] == 'ensemble':
        ensemble(sys.argv[2:])
    else:
        {'compare': compare, 'large': large, 'threads': threads, 'plain': plain}[sys.argv[1]]()
