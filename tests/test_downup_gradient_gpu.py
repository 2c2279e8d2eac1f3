"""The control gradient of the fused sweep k_mfma_downup (csrc/qoc_mfma_downup.h), against the CPU oracle and against the separate sweeps.

Pass B of the kernel forms Q = conj(Lambda_{t+1}) Psi_{t+1}^T per slice and contracts it with the control images in LDS, whose rows it reads a control
at a time (QOC_DOWNUP_AHEAD).  Built with -DQOC_DOWNUP_Q444=1 it forms Q strip by strip on v_mfma_f64_4x4x4_4b, the left 4 x 4 blocks read from the
wave's LDS image (wave 0 reads the image its next product multiplies from, wave 1 stores Lambda_{t+1} over the dead image of Psi_t), and skips the
strips of padded sizes that are never contracted; the same cases hold that build (point QOC_HIP_LIBRARY at it), which is not the default because it
measured slower (profiles/downup_q444_ab.txt).  Every case runs 12 control sets with fewer than 64 slices -- more than the 8 sets up to which
a batch may go elsewhere, fewer slices than the latency mode takes -- on the MFMA path, and asserts from the plan that the fused sweep ran.

Cases, each the smallest shape at which one branch can go wrong:
  full_auto_chunks      n = 32, k = 4, m = 8, 40 slices, AUTO chunks
  full_one_slice_tail   13 slices in 4 pinned chunks: 4, 4, 4, 1 -- the last chunk has no second half (n = 0 in wave 1)
  full_odd_halves       40 slices in 6 pinned chunks: 7 x 5 + 5 -- halves of 4 / 3 and 3 / 2 slices, odd counts in the two-slice loops
  n20, n27              QA = 5 and QA = 7: the skipped strips (13 slices in chunks of 7 and 6)
  k1, k5                one control; the KC = 5 instances
  m3, m5                zero vector columns inside MQ = 2
For each: one evaluation against oracle.grape_oracle (gradient 1e-11 x max|g|, scalars 1e-12 relative: tests/test_hip_parity.py), the same against an
engine on the separate sweeps (QOC_EXPERIMENTAL=1 QOC_UPDOWN=0, same process), and three iterations of the device loop against the oracle's loop
(tests/test_bench_config_parity.py).  Reference semantics: core/tensorflow_state.py:49-65 (gradient), :204-242 (chain), core/run_session.py:47-69.
"""
import functools

import numpy as np
import pytest

from oracle import grape_oracle as go
from tests.helpers import oracle_system

pytestmark = pytest.mark.gpu

G_RTOL, S_RTOL = 1e-11, 1e-12
MFMA, SETS = 2, 12
CONV = dict(rate=0.01, learning_rate_decay=2500, conv_target=1e-8, min_grad=1e-25, max_iterations=3)

#            n   k  m  slices  chunks asked (0: AUTO)  chunks planned (None: whatever AUTO makes of it)
CASES = {
    'full_auto_chunks':    (32, 4, 8, 40, 0, None),
    'full_one_slice_tail': (32, 4, 8, 13, 4, 4),
    'full_odd_halves':     (32, 4, 8, 40, 6, 6),
    'n20':                 (20, 4, 8, 13, 2, 2),
    'n27':                 (27, 4, 8, 13, 2, 2),
    'k1':                  (32, 1, 8, 13, 2, 2),
    'k5':                  (32, 5, 8, 13, 2, 2),
    'm3':                  (32, 4, 3, 13, 2, 2),
    'm5':                  (32, 4, 5, 13, 2, 2),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The problem, its 12 control sets and the oracle's evaluation of each: computed once per case, shared by the tests, never modified."""
    from quantum_optimal_control.helper_functions import synthetic_systems
    n, k, m, steps, _, _ = CASES[name]
    c = synthetic_systems.case_c2(n=n, k=k, steps=steps, m=m, taylor=(5, 3), seed=sorted(CASES).index(name))
    assert c['reg_coeffs'] == {}
    sp = oracle_system(c)
    rng = np.random.default_rng(100 + sorted(CASES).index(name))
    bases = np.stack([sp.base0] + [2.0 * rng.normal(size=sp.base0.shape) / np.sqrt(sp.steps) - 0.2 for _ in range(SETS - 1)])
    bases.setflags(write=False)
    return sp, bases, tuple(go.evaluate(sp, b) for b in bases)


def make_engine(name, sp):
    from quantum_optimal_control.core import hip_engine
    return hip_engine.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling,
                                reg_coeffs={}, n_seeds=SETS, path=MFMA, chunks=CASES[name][4])


def assert_sweeps(eng, name, sweeps):
    """The sweeps the engine resolved (qoc_plan_describe): without this a fallback to other kernels would make the comparison vacuous."""
    assert eng.path == MFMA and eng.plan['path'] == 'mfma' and eng.plan['nt'] == '2', eng.plan
    assert eng.plan['sweeps'] == sweeps, eng.plan
    if CASES[name][5] is not None:
        assert int(eng.plan['chunks']) == eng.chunks == CASES[name][5], eng.plan


def compare_evaluation(r, expected, what):
    """`expected`: per control set a dict with loss, reg_loss, grad_squared, unitary_scale, grad."""
    for b, o in enumerate(expected):
        gmax = np.max(np.abs(o['grad']))
        gd = np.max(np.abs(r['grad'][b] - o['grad'])) / gmax
        sd = {key: abs(r[key][b] - o[key]) / max(1.0, abs(o[key])) for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale')}
        print('  %s, set %2d: gradient %.2e of max|g| = %.2e  %s' % (what, b, gd, gmax, '  '.join('%s %.2e' % kv for kv in sd.items())))
        assert gd <= G_RTOL, (what, 'grad', b, gd, gmax)
        for key, v in sd.items():
            assert v <= S_RTOL, (what, key, b, r[key][b], o[key])


@pytest.mark.parametrize('name', list(CASES))
def test_one_evaluation_against_the_oracle(name):
    sp, bases, ref = reference(name)
    eng = make_engine(name, sp)
    try:
        assert_sweeps(eng, name, 'downup')
        print('  plan: %s' % eng.plan)
        eng.set_base(bases)
        compare_evaluation(eng.evaluate(), ref, 'oracle')
    finally:
        eng.close()


@pytest.mark.parametrize('name', list(CASES))
def test_one_evaluation_against_the_separate_sweeps(name, monkeypatch):
    """QOC_EXPERIMENTAL=1 QOC_UPDOWN=0 is read when an engine is created: the forward and the backward sweep as kernels of their own."""
    sp, bases, _ = reference(name)
    fused = make_engine(name, sp)
    try:
        assert_sweeps(fused, name, 'downup')
        monkeypatch.setenv('QOC_EXPERIMENTAL', '1')
        monkeypatch.setenv('QOC_UPDOWN', '0')
        apart = make_engine(name, sp)
        try:
            assert_sweeps(apart, name, 'pair')
            fused.set_base(bases)
            apart.set_base(bases)
            r, s = fused.evaluate(), apart.evaluate()
            compare_evaluation(r, [dict(grad=s['grad'][b], **{key: s[key][b] for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale')})
                                   for b in range(SETS)], 'separate sweeps')
        finally:
            apart.close()
    finally:
        fused.close()


@pytest.mark.parametrize('name', list(CASES))
def test_three_iterations_of_the_device_loop(name):
    sp, bases, _ = reference(name)
    eng = make_engine(name, sp)
    try:
        assert_sweeps(eng, name, 'downup')
        eng.set_base(bases)
        eng.iterate(eng.adam_params(poll_every=3, **CONV), 3)
        eng.sync()
        base = eng.get_base()
        for b in range(SETS):
            o = go.run_adam(sp, CONV, base=bases[b])
            assert o['iterations'] == 3
            print('  set %2d: base %.2e' % (b, np.max(np.abs(base[b] - o['base']))))
            np.testing.assert_allclose(base[b], o['base'], rtol=0, atol=1e-10)
    finally:
        eng.close()
