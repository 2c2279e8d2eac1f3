"""The exact gradient without a GPU: the NumPy reference (tests/exact_gradient_reference.py) against central differences of the oracle's
reg_loss on nine rows, on each of which the oracle's first-order gradient is visibly something else; and the static side of the feature
(the ABI field, Grape's signature, the refusal of time sharding)."""
import ctypes
import inspect

import numpy as np
import pytest

from tests import exact_gradient_reference as xr
from tests.helpers import oracle_system

ROWS = xr.table_rows()


@pytest.mark.parametrize('name,c', ROWS, ids=[n for n, _ in ROWS])
def test_reference_against_central_differences(name, c):
    """h = 1e-6: the truncation error of the difference quotient is O(h^2 |f'''|) ~ 1e-12, its rounding noise ~ eps |f| / h ~ 1e-10 of a loss of
    order one -- both far below 1e-7 of the gradient's largest entry.  Measured on the CPU: <= 4.8e-9 on every row.  The first-order gradient
    differs from the same quotient by 1.6e-2 .. 1.9 of the largest entry."""
    sp = oracle_system(c)
    base = xr.perturbed_base(sp)
    r = xr.evaluate(sp, base)
    fd = xr.central_differences(sp, base)
    gmax = float(np.max(np.abs(fd)))
    exact = float(np.max(np.abs(r['grad'] - fd)))
    first = float(np.max(np.abs(r['first_order_grad'] - fd)))
    print('%s (T, s) = (%d, %d): |exact - fd| / gmax = %.2e, |first - fd| / gmax = %.2e, gmax = %.3e' % (
        name, sp.exp_terms, sp.scaling, exact / gmax, first / gmax, gmax))
    assert exact <= 1e-7 * max(gmax, 1e-3), (exact, gmax)
    assert first >= 1e-2 * gmax, (first, gmax)
    assert r['grad_squared'] == 0.5 * float(np.sum(r['grad'] ** 2))


def test_config_has_the_gradient_field_at_the_size_it_had():
    from quantum_optimal_control.core.hip_engine import QocConfig
    names = [f[0] for f in QocConfig._fields_]
    assert 'gradient' in names and names.index('gradient') == names.index('time_rank') + 1 and names[-1] == 'reserved'
    assert QocConfig.gradient.size == 4 and QocConfig.reserved.size == 8
    # 8 ints, dt and total_time, 6 flags, 6 coefficients, 14 ints (the last three were `reserved[3]`)
    assert ctypes.sizeof(QocConfig) == 8 * 4 + 2 * 8 + 6 * 4 + 6 * 8 + 14 * 4 == 176
    assert QocConfig().gradient == 0


def test_grape_signature():
    from quantum_optimal_control.core.hip_engine import HipEngine
    from quantum_optimal_control.core.hip_state import HipState
    from quantum_optimal_control.main_grape.grape import Grape
    params = inspect.signature(Grape).parameters
    p = params['exact_gradient']
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    names = list(params)
    assert names.index('exact_gradient') == names.index('transfer') + 1
    for fn in (HipEngine.__init__, HipState.__init__):
        assert inspect.signature(fn).parameters['exact_gradient'].default is False


def test_grape_refuses_time_sharding_before_any_engine_is_built(monkeypatch):
    from quantum_optimal_control.core import hip_engine
    from quantum_optimal_control.main_grape.grape import Grape

    def no_engine(*a, **kw):
        raise AssertionError('an engine was built')
    monkeypatch.setattr(hip_engine.HipEngine, '__init__', no_engine)
    SX = np.array([[0, 1], [1, 0]], dtype=complex)
    with pytest.raises(ValueError, match='exact gradient'):
        Grape(0.0 * SX, [2 * np.pi * SX / 2], ['x'], SX, 10.0, 10, [0, 1], reg_coeffs={}, maxA=[0.1], show_plots=False, save=False,
              exact_gradient=True, time_comm=object())


def test_convergence_takes_an_optional_ftol():
    from quantum_optimal_control.core.convergence import Convergence
    assert Convergence(None, 'ns', {}).ftol is None
    assert Convergence(None, 'ns', {'ftol': 0.0, 'rate': 0.02}).ftol == 0.0
