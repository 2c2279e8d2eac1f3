"""The memory policy of k_mfma_expm_inplace and k_mfma_downup (csrc/qoc_mfma_frag.h: QocMem; QOC_EXPM_KSTORE, QOC_DOWNUP_*) moves the same values.

QOC_EXPERIMENTAL=1 QOC_MEM_POLICY=0 (read when the engine is created) runs the plain accesses, the default runs the policy instances where the
library has them (k <= 4; qoc_plan_describe: mem_policy=<0|1>).  Both must agree BIT FOR BIT in everything read back -- scalars(), get_base,
get_uks(evaluated=True), get_final_unitary, inter_vecs -- after one evaluation and after three iterations of the device loop; policy 0 is also
held against the CPU oracle at the tolerances of tests/test_hip_parity.py (1e-12 x max|entry| for loss, final unitary and inter_vecs, 1e-11 x
max|g| for the gradient).

Unitary engines on the MFMA batch path (fused sweep), chunks pinned:
  (n, k, m, steps, seeds, chunks) = (32, 4, 8, 37, 3, 4)   chunks of 10, 10, 10 and 7 slices: odd chunk lengths, unequal halves
                                    (32, 4, 8, 9, 2, 8)    four chunks of two slices and one of one slice: a pair whose second half is empty
                                    (20, 5, 3, 40, 2, 4)   QA = 5, KC = 5 (no policy instance: mem_policy=0 either way), m < 8
  and the first shape with a stop value between the two losses: one control set finishes at the first iteration (QocDev::skip_done), the other runs on.
"""
import contextlib
import os

import numpy as np
import pytest

from oracle import grape_oracle as go
from tests.golden import cases
from tests.helpers import oracle_system

pytestmark = pytest.mark.gpu

U_ATOL, G_RTOL, S_RTOL = 1e-12, 1e-11, 1e-12
MFMA = 2
SHAPES = {'odd_chunks': (32, 4, 8, 37, 3, 4), 'one_and_two_slices': (32, 4, 8, 9, 2, 8), 'five_strips_five_controls': (20, 5, 3, 40, 2, 4),
          'finished_set': (32, 4, 8, 37, 2, 4)}
# what qoc_plan_describe reports per policy request: the policy instances are built for k <= 4
HAS_POLICY = {'odd_chunks': True, 'one_and_two_slices': True, 'five_strips_five_controls': False, 'finished_set': True}
SCALARS = ('loss', 'reg_loss', 'grad_squared', 'unitary_scale', 'iterations', 'done')


@contextlib.contextmanager
def mem_policy(policy):
    """The switch is read inside qoc_create: set around the constructor only."""
    old = {key: os.environ.get(key) for key in ('QOC_EXPERIMENTAL', 'QOC_MEM_POLICY')}
    os.environ['QOC_EXPERIMENTAL'], os.environ['QOC_MEM_POLICY'] = '1', str(policy)
    try:
        yield
    finally:
        for key, v in old.items():
            if v is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = v


def problem(name):
    n, k, m, steps, seeds, chunks = SHAPES[name]
    sp = oracle_system(cases.case_c2(n=n, k=k, steps=steps, m=m, taylor=(5, 3), seed=len(name)))
    rng = np.random.default_rng(steps)
    bases = [sp.base0] + [2.0 * rng.normal(size=sp.base0.shape) / np.sqrt(sp.steps) - 0.2 for _ in range(seeds - 1)]
    return sp, bases, chunks


def read_back(eng):
    out = dict(eng.scalars())
    out.update(base=eng.get_base(), uks=eng.get_uks(evaluated=True), U_final=eng.get_final_unitary(), inter_vecs=eng.get_inter_vecs())
    return out


def run(name, policy, sp, bases, chunks, conv):
    from quantum_optimal_control.core import hip_engine
    with mem_policy(policy):
        eng = hip_engine.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling,
                                   reg_coeffs={}, n_seeds=len(bases), path=MFMA, chunks=chunks)
    try:
        L = -(-sp.steps // chunks)                          # slices per chunk of the pinned chunk count; the engine reports the chunks that are not empty
        assert eng.path == MFMA and eng.chunks == -(-sp.steps // L) and eng.plan['sweeps'] == 'downup' and eng.plan['expm'] == '8', eng.plan
        assert eng.plan['mem_policy'] == str(policy if HAS_POLICY[name] else 0), eng.plan
        eng.set_base(np.stack(bases))
        r = eng.evaluate()
        first = read_back(eng)
        eng.iterate(eng.adam_params(poll_every=3, **conv), 3)
        eng.sync()
        return dict(eval=r, first=first, after=read_back(eng))
    finally:
        eng.close()


@pytest.fixture(scope='module', params=list(SHAPES))
def both(request):
    """One problem under policy 0 and policy 1 (an engine each, same inputs), and its oracle evaluations."""
    name = request.param
    sp, bases, chunks = problem(name)
    oracle = [go.evaluate(sp, base, want_inter=True) for base in bases]
    conv = dict(rate=0.01, learning_rate_decay=2500, conv_target=1e-8, min_grad=1e-25, max_iterations=3)
    if name == 'finished_set':
        # a stop value between the two losses, a rate that cannot carry the other set across it in three iterations
        lo, hi = sorted(o['loss'] for o in oracle)
        assert hi - lo > 1e-6, (lo, hi)
        conv = dict(conv, rate=1e-5, conv_target=0.5 * (lo + hi))
    return name, sp, bases, oracle, {policy: run(name, policy, sp, bases, chunks, conv) for policy in (0, 1)}


def test_policy_0_against_the_oracle(both):
    name, sp, bases, oracle, out = both
    r, first = out[0]['eval'], out[0]['first']
    for b, o in enumerate(oracle):
        gmax = np.max(np.abs(o['grad']))
        figures = (abs(r['loss'][b] - o['loss']), np.max(np.abs(r['grad'][b] - o['grad'])) / gmax, np.max(np.abs(first['U_final'][b] - o['U_final'])),
                   np.max(np.abs(first['inter_vecs'][b] - o['inter_vecs'])))
        print('  %s set %d: |loss - oracle| %.2e  gradient %.2e of max|g| = %.2e  U_final %.2e  inter_vecs %.2e' % ((name, b) + figures[:2] + (gmax,) + figures[2:]))
        assert figures[0] <= S_RTOL * max(1.0, abs(o['loss'])), ('loss', b, r['loss'][b], o['loss'])
        assert figures[1] <= G_RTOL, ('grad', b, figures[1], gmax)
        assert figures[2] <= U_ATOL * max(1.0, np.max(np.abs(o['U_final']))), ('U_final', b, figures[2])
        assert figures[3] <= U_ATOL * max(1.0, np.max(np.abs(o['inter_vecs']))), ('inter_vecs', b, figures[3])


def test_policies_agree_bit_for_bit(both):
    name, sp, bases, oracle, out = both
    for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale', 'grad'):
        assert np.array_equal(out[0]['eval'][key], out[1]['eval'][key]), ('evaluate', key)
    for when in ('first', 'after'):
        for key in SCALARS + ('base', 'uks', 'U_final', 'inter_vecs'):
            assert np.array_equal(out[0][when][key], out[1][when][key]), (when, key)
    done = out[0]['after']['done']
    if name == 'finished_set':
        assert sorted(done) == [0, 1], done                  # one set stopped inside the loop (the kernels skipped it from then on), the other ran on
    else:
        assert not np.any(done), done
