"""Robust GRAPE, CPU side: validation of Grape(robust=...) and ensemble_grid, the (T, s) choice over the members, and the engine's
refusals that come before any device is touched."""
import numpy as np
import pytest

from quantum_optimal_control.helper_functions import robust as rb
from quantum_optimal_control.helper_functions.robust import ensemble_grid

SZ = np.array([[1, 0], [0, -1]], dtype=complex)
SX = np.array([[0, 1], [1, 0]], dtype=complex)
SY = np.array([[0, -1j], [1j, 0]], dtype=complex)


def test_grid_is_the_cartesian_product_with_the_nominal_point_first():
    ens = ensemble_grid(operators=[SZ / 2], offsets=np.array([-0.005, 0.0, 0.005])[:, None], amp_scales=[0.95, 1.0, 1.05], k=2)
    assert ens['offsets'].shape == (9, 1) and ens['amp_scales'].shape == (9, 2)
    assert ens['offsets'][0, 0] == 0.0 and np.all(ens['amp_scales'][0] == 1.0)
    pts = {(o[0], a[0]) for o, a in zip(ens['offsets'], ens['amp_scales'])}
    assert pts == {(o, a) for o in (-0.005, 0.0, 0.005) for a in (0.95, 1.0, 1.05)}
    assert np.all(ens['amp_scales'][:, 0] == ens['amp_scales'][:, 1])          # a scalar row applies to every control
    np.testing.assert_allclose(ens['weights'], np.full(9, 1 / 9), rtol=1e-15)


def test_grid_without_the_nominal_point_keeps_product_order_and_normalises_weights():
    ens = ensemble_grid(operators=[SZ], offsets=[[0.1], [0.2]], amp_scales=[[0.9, 1.1], [1.2, 0.8]], k=2, weights=[1, 2, 3, 4])
    np.testing.assert_array_equal(ens['offsets'][:, 0], [0.1, 0.1, 0.2, 0.2])
    np.testing.assert_array_equal(ens['amp_scales'][:, 0], [0.9, 1.2, 0.9, 1.2])
    np.testing.assert_allclose(ens['weights'], np.array([1, 2, 3, 4]) / 10.0)
    ens = ensemble_grid(amp_scales=[0.9, 1.0], k=3)                               # no operators: amplitude errors only
    assert ens['offsets'].shape == (2, 0) and np.all(ens['amp_scales'][0] == 1.0)


@pytest.mark.parametrize('robust,match', [
    (dict(operators=[SZ], offsets=[[0.1, 0.2]]), 'offsets have shape'),
    (dict(operators=[SZ]), 'offsets'),
    (dict(operators=[SZ + 1j * SX], offsets=[[0.1]]), 'not Hermitian'),
    (dict(operators=[np.eye(3)], offsets=[[0.1]]), 'shape'),
    (dict(amp_scales=[[1.0]]), 'amp_scales have shape'),
    (dict(operators=[SZ], offsets=[[0.1], [0.2]], amp_scales=np.ones((3, 2))), 'amp_scales have shape'),
    (dict(amp_scales=np.ones((2, 2)), weights=[1.0, -0.5]), 'weights'),
    (dict(amp_scales=np.ones((2, 2)), weights=[0.0, 0.0]), 'sum to zero'),
    (dict(amp_scales=np.ones((2, 2)), weights=[1.0]), 'weights for 2 members'),
    (dict(), 'no members'),
    (dict(amp_scales=np.ones((1, 2)), extra=1), 'unknown keys'),
    ([1, 2], 'a dict'),
])
def test_validation_errors(robust, match):
    with pytest.raises(ValueError, match=match):
        rb.validate(robust, 2, 2)


def test_grape_rejects_a_bad_ensemble_and_time_sharding_before_any_device_work():
    from quantum_optimal_control.main_grape.grape import Grape, GrapeSharded
    args = (0 * SZ, [SX / 2, SY / 2], ['x', 'y'], SX, 10.0, 20, [0, 1])
    with pytest.raises(ValueError, match='not Hermitian'):
        Grape(*args, robust=dict(operators=[1j * SZ], offsets=[[0.1]]), save=False, show_plots=False)
    with pytest.raises(ValueError, match='time-sharded'):
        Grape(*args, robust=dict(amp_scales=np.ones((2, 2))), time_comm=object(), save=False, show_plots=False)
    with pytest.raises(ValueError, match='GrapeSharded: robust'):
        GrapeSharded(*args, restarts=2, robust=dict(amp_scales=np.ones((2, 2))), save=False, show_plots=False)


def test_taylor_choice_is_the_member_maximum():
    from quantum_optimal_control.core.system_parameters import SystemParameters
    H0, Hops, maxA, U0 = 2 * np.pi * 0.05 * SZ / 2, [2 * np.pi * SX / 2], np.array([0.2]), np.eye(2)
    ens = ensemble_grid(operators=[2 * np.pi * SZ / 2], offsets=[[-2.0], [0.0], [3.0]], amp_scales=[1.0, 4.0], k=1)
    chosen = rb.choose_taylor(H0, Hops, ens, maxA, U0, 10.0, 100, 1e-4, False, False)
    per = []
    for e in range(len(ens['weights'])):
        H0e, Hopse = rb.member_hamiltonians(H0, Hops, ens, e)
        np.random.seed(0)
        sp = SystemParameters(H0e, Hopse, ['x'], SX, U0, 10.0, 100, [0, 1], None, maxA, None, None, False, 1e-4, False, False, {},
                              False, None, None, True, True, False, False, False)
        per.append((sp.exp_terms, sp.scaling))
    assert chosen == (max(t for t, _ in per), max(s for _, s in per))
    assert len(set(per)) > 1                                # the members disagree, so the maximum is a real choice


def test_ensemble_engine_refuses_excluded_paths_before_touching_a_device():
    from quantum_optimal_control.core import hip_engine
    n, k, m, steps = 2, 1, 2, 4
    Hs = np.zeros((k + 1, n, n), dtype=np.complex128)
    ens = dict(operators=[SZ], offsets=np.zeros((2, 1)), amp_scales=np.ones((2, 1)), weights=np.full(2, 0.5))
    base = (Hs, np.eye(n), np.eye(n)[:, :m], np.eye(n)[:, :m], [1.0], 0.1, 0.4, steps, 3, 0)
    for kw, match in ((dict(path=hip_engine.PATH_SMALL), 'workgroup-resident'), (dict(variant=5), 'latency mode'),
                      (dict(time_shards=2, time_rank=-1), 'time-sharded'),
                      (dict(path=hip_engine.PATH_MFMA, ensemble=dict(ens, operators=[SZ] * 8, offsets=np.zeros((2, 8)))), 'k \\+ q = 9')):
        kw = dict(dict(ensemble=ens, reg_coeffs={}), **kw)
        with pytest.raises(hip_engine.QocError, match=match):
            hip_engine.HipEngine(*base, **kw)
