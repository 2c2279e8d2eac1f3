"""Two live engines of different shape on one device, used in turn (include/qoc.h hands out independent handles).

What they can share without knowing it is a kernel instance: hipFuncSetAttribute(..., hipFuncAttributeMaxDynamicSharedMemorySize, bytes) holds
per kernel instance for the whole process, and an engine asks for its own byte count when it is created.  Where that count depends on the
engine's shape, creating a second engine with a smaller count while the first lives leaves the first to launch with more than the instance
was last granted.  The pairs below meet on every such instance, small count created last and first:

  k_exact_grad<true>        (D + 4) n m + n^2 complex numbers          csrc/qoc_exact_grad.h: qoc_exact_lds_opt_in
  k_mfma_grad_rt<NT, MQ>    ((k + 3) & ~3) NT 256 complex numbers      csrc/qoc_mfma_backward.hip: qoc_mfma_setup
  k_mfma_grad<NT, MQ>       min(k, 4 or 2) control images              the same call; varies only behind QOC_GRAD_RT=0 (k <= 8 takes the row-tile kernel)
  k_mfma_backward<NT, true> pads + k control images                    variant 1 (and n <= 16), while the images fit the LDS
  k_lb_forward / k_lb_backward  (c + 4) n (n | 1) complex numbers      csrc/qoc_lindblad.h: qoc_lb_lds_opt_in asks for the size rule's limit, not the engine's
                            count; open engines beside open and closed ones: tests/test_open_system_edges.py::test_open_engine_beside_another

The other call sites ask for a constant of the instance and need no pair: the latency mode's gradient kernels (csrc/qoc_mfma_latency.hip:
the image count KC and NT are template arguments, NT = 4 always takes two), k_mfma_backward3 and k_mfma_downup (qoc_mfma_setup: KC = 4 | 5, MQ
and NT = 2 are template arguments), k_mfma_expm_rows (qoc_expm_rows_lds<NT>()), the GEMM path's kernels and the workgroup-resident path's
(160 KiB always).  Two pairs of those and one mixed pair run as controls.

Every comparison is np.array_equal against the same engine running alone."""
import functools

import numpy as np
import pytest

from quantum_optimal_control.core import hip_engine
from tests import exact_gradient_reference as xr
from tests.golden import cases
from tests.helpers import oracle_system
from tests.test_exact_gradient_gpu import assert_gradient, assert_scalar, make_engine
from tests.test_hip_parity import check_eval

pytestmark = pytest.mark.gpu

P = hip_engine
G = 2
GRAD_RT_OFF = (('QOC_EXPERIMENTAL', '1'), ('QOC_GRAD_RT', '0'))       # (read when an engine is created; only beside QOC_EXPERIMENTAL=1)


def _c2(**kw):
    return lambda: cases.case_c2(**kw)


# name: (recipe, keywords of HipEngine, environment, plan entries the engine must report)
SPECS = {
    'exact_lds_152k': (_c2(n=64, k=2, steps=5, m=8, taylor=(7, 1), seed=26), dict(exact_gradient=True), (),
                       dict(exact_variant='lds', exact_lds='155648')),
    'exact_lds_90k': (_c2(n=48, k=2, steps=5, m=8, taylor=(5, 1), seed=28), dict(exact_gradient=True), (),
                      dict(exact_variant='lds', exact_lds='92160')),
    'exact_global': (_c2(n=64, k=2, steps=5, m=8, taylor=(8, 1), seed=26), dict(exact_gradient=True), (), dict(exact_variant='global')),
    'rt_n64_k6': (_c2(n=64, k=6, steps=13, m=8, taylor=(5, 2), seed=70), dict(path=P.PATH_MFMA, variant=7), (),
                  dict(path='mfma', nt='4', sweeps='row_tile_gradient')),
    'rt_n64_k3': (_c2(n=64, k=3, steps=13, m=8, taylor=(5, 2), seed=67), dict(path=P.PATH_MFMA, variant=7), (),
                  dict(path='mfma', nt='4', sweeps='row_tile_gradient')),
    'grad_n48_k4': (_c2(n=48, k=4, steps=13, m=8, taylor=(5, 2), seed=52), dict(path=P.PATH_MFMA, variant=7), GRAD_RT_OFF,
                    dict(path='mfma', nt='3', sweeps='split')),
    'grad_n48_k1': (_c2(n=48, k=1, steps=13, m=8, taylor=(5, 2), seed=49), dict(path=P.PATH_MFMA, variant=7), GRAD_RT_OFF,
                    dict(path='mfma', nt='3', sweeps='split')),
    'one_wave_n48_k3': (_c2(n=48, k=3, steps=13, m=4, taylor=(5, 2), seed=51), dict(path=P.PATH_MFMA, variant=1), (),
                        dict(path='mfma', nt='3', sweeps='one_wave')),
    'one_wave_n48_k1': (_c2(n=48, k=1, steps=13, m=4, taylor=(5, 2), seed=49), dict(path=P.PATH_MFMA, variant=1), (),
                        dict(path='mfma', nt='3', sweeps='one_wave')),
    'small_n4': (_c2(n=4, k=2, steps=12, m=3, taylor=(6, 1), seed=2), dict(path=P.PATH_SMALL), (), dict(path='small')),
    'small_n12': (_c2(n=12, k=2, steps=16, m=3, taylor=(5, 2), seed=3), dict(path=P.PATH_SMALL), (), dict(path='small')),
    'gemm_n128': (_c2(n=128, k=2, steps=8, m=8, taylor=(5, 2), seed=41), dict(path=P.PATH_GEMM), (), dict(path='gemm')),
    'gemm_n40': (_c2(n=40, k=2, steps=16, m=4, taylor=(5, 2), seed=3), dict(path=P.PATH_GEMM), (), dict(path='gemm')),
    'gemm_direct_st': (lambda: cases.case_c3(n=24, k=2, steps=16, taylor=(6, 0)), dict(path=P.PATH_GEMM, chunks=1), (),
                       dict(path='gemm', route='direct')),
}

# (the engine with the larger count on the shared instance, the smaller one)
PAIRS = [('exact_lds_152k', 'exact_lds_90k'), ('exact_lds_152k', 'exact_global'), ('rt_n64_k6', 'rt_n64_k3'), ('grad_n48_k4', 'grad_n48_k1'),
         ('one_wave_n48_k3', 'one_wave_n48_k1'), ('small_n12', 'small_n4'), ('gemm_n128', 'gemm_n40'), ('small_n4', 'gemm_direct_st')]
LOOP = dict(rate=0.02, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=1000, poll_every=5)


@functools.lru_cache(maxsize=None)
def problem(name):
    sp = oracle_system(SPECS[name][0]())
    rng = np.random.default_rng(17)
    return sp, np.stack([sp.base0, 2.0 * rng.normal(size=sp.base0.shape) / np.sqrt(sp.steps) + 0.2])


def create(name, monkeypatch):
    _, kw, env, plan = SPECS[name]
    sp, bases = problem(name)
    with monkeypatch.context() as mp:
        for key, value in env:
            mp.setenv(key, value)
        eng = make_engine(sp, G, **kw)
    try:
        for key, value in plan.items():
            assert eng.plan[key] == value, (name, eng.plan)
        eng.set_base(bases)
    except Exception:
        eng.close()
        raise
    return eng


def loop_state(eng):
    s = eng.scalars()
    return dict(s, base=eng.get_base(), inter_vecs=eng.get_inter_vecs())


def assert_same(tag, got, want):
    assert sorted(got) == sorted(want)
    for key in want:
        assert np.array_equal(got[key], want[key]), (tag, key)


_SOLO = {}


def solo(name, monkeypatch):
    """The engine on its own, once per spec: its first evaluation (checked against the oracle, or the exact reference), its state after
    iterate(3), and one more evaluation where the loop left it."""
    if name in _SOLO:
        return _SOLO[name]
    sp, bases = problem(name)
    eng = create(name, monkeypatch)
    try:
        first = eng.evaluate()
        if SPECS[name][1].get('exact_gradient'):
            for g, b in enumerate(bases):
                o = xr.evaluate(sp, b)
                for key in ('loss', 'reg_loss', 'unitary_scale', 'grad_squared'):
                    assert_scalar('%s %s[%d]' % (name, key, g), first[key][g], o[key])
                assert_gradient('%s grad[%d]' % (name, g), first['grad'][g], o['grad'])
        else:
            check_eval(eng, sp, bases)
    finally:
        eng.close()
    # The workgroup-resident path is the one path on which a burst is not its single launches bit for bit: inside a launch the learning rate
    # and beta^t advance by running products (tests/test_small_path.py: test_small_path_explicit_step_and_iterate, atol 1e-13).  Alone it runs
    # the launches of the interleaved run, and iterate(3) is held to that test's 1e-13.
    single = SPECS[name][1].get('path') == P.PATH_SMALL
    eng = create(name, monkeypatch)
    try:
        p = eng.adam_params(**LOOP)
        for _ in range(3 if single else 1):
            eng.iterate(p, 1 if single else 3)
        eng.sync()
        looped = loop_state(eng)
        after = eng.evaluate()
    finally:
        eng.close()
    assert list(looped['iterations']) == [3] * G, looped['iterations']
    if single:
        eng = create(name, monkeypatch)
        try:
            eng.iterate(eng.adam_params(**LOOP), 3)
            eng.sync()
            np.testing.assert_allclose(eng.get_base(), looped['base'], rtol=0, atol=1e-13)
        finally:
            eng.close()
    _SOLO[name] = (first, looped, after)
    return _SOLO[name]


def run_pair(a, b, monkeypatch):
    """a is created first, b while a lives."""
    a0, a_loop, _ = solo(a, monkeypatch)
    b0, b_loop, b_after = solo(b, monkeypatch)
    A = B = None
    try:
        A = create(a, monkeypatch)
        assert_same('%s alone' % a, A.evaluate(), a0)
        B = create(b, monkeypatch)
        assert_same('%s beside %s' % (b, a), B.evaluate(), b0)
        assert_same('%s after %s was created' % (a, b), A.evaluate(), a0)
        pa, pb = A.adam_params(**LOOP), B.adam_params(**LOOP)
        for _ in range(3):
            A.iterate(pa, 1)
            B.iterate(pb, 1)
        A.sync()
        B.sync()
        assert_same('%s interleaved with %s' % (a, b), loop_state(A), a_loop)
        assert_same('%s interleaved with %s' % (b, a), loop_state(B), b_loop)
        A.close()
        assert_same('%s after %s was closed' % (b, a), B.evaluate(), b_after)
    finally:
        for eng in (A, B):
            if eng is not None:
                eng.close()


@pytest.mark.parametrize('order', ['large_first', 'small_first'])
@pytest.mark.parametrize('pair', PAIRS, ids=['%s+%s' % p for p in PAIRS])
def test_two_engines_in_turn(pair, order, monkeypatch):
    large, small = pair
    if order == 'large_first':
        run_pair(large, small, monkeypatch)
    else:
        run_pair(small, large, monkeypatch)
