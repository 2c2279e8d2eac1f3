"""The L-BFGS loop's specification (tests/lbfgs_reference.py) on problems with known answers, against the oracle's Adam loop, and the Python side of
the device-resident loop -- binding, routing, refusals -- without a GPU.  The kernel itself is tested in tests/test_lbfgs_gpu.py against the same
reference."""
import ctypes
from collections import Counter

import numpy as np
import pytest

from oracle import grape_oracle as go
from quantum_optimal_control.core import hip_engine
from tests import lbfgs_reference as ref
from tests.golden import cases
from tests.helpers import oracle_system


# ---- problems with known answers ---------------------------------------------------------------------------------------------------------------

def _quadratic(N=50, cond=1e4, seed=0):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(N, N)))
    A = (Q * np.logspace(0, np.log10(cond), N)) @ Q.T
    A = 0.5 * (A + A.T)
    xs = rng.normal(size=N)
    b = A @ xs
    fs = 0.5 * xs @ A @ xs - b @ xs

    def evaluate(x):
        g = A @ x - b
        f = 0.5 * x @ A @ x - b @ x
        return dict(reg_loss=f, grad=g, loss=f - fs, grad_squared=0.5 * g @ g)
    return evaluate, fs, rng.normal(size=N)


def rosenbrock(x):
    f = np.sum(100 * (x[1:] - x[:-1] ** 2) ** 2 + (1 - x[:-1]) ** 2)
    g = np.zeros_like(x)
    g[:-1] += -400 * x[:-1] * (x[1:] - x[:-1] ** 2) - 2 * (1 - x[:-1])
    g[1:] += 200 * (x[1:] - x[:-1] ** 2)
    return dict(reg_loss=f, grad=g, loss=f, grad_squared=0.5 * g @ g)


QUADRATIC_EVALUATIONS = 524         # measured: the first evaluation within 1e-12 |f*| of the optimum (f* = -20083.6) is number 524, counting from 0


def test_convex_quadratic_descends_and_reaches_the_optimum():
    evaluate, fs, x0 = _quadratic()
    rec = ref.run(evaluate, x0, dict(conv_target=-1.0, min_grad=-1.0, max_iterations=2000), 700)
    f = np.array(rec['f'])
    accepted = f[[i for i, b in enumerate(rec['branch']) if b == ref.ACCEPT]]
    assert len(accepted) > 100 and np.all(np.diff(accepted) <= 0)
    reached = np.nonzero(f - fs <= 1e-12 * abs(fs))[0]
    assert len(reached) and reached[0] <= QUADRATIC_EVALUATIONS, reached[:1]


def test_rosenbrock_takes_the_rejection_skip_and_wrap_branches():
    """M = 3 in 10 dimensions from the classic start: 131 accepted and 18 rejected trials, one pair refused for its curvature, the history wraps."""
    rec = ref.run(rosenbrock, np.array([-1.2, 1.0] * 5), dict(history=3, conv_target=1e-18, min_grad=1e-30, max_iterations=1000))
    count = Counter(rec['branch'])
    assert count[ref.REJECT] >= 1 and count[ref.ACCEPT] >= 10
    assert sum(p is False for p in rec['pushed']) >= 1                      # sy <= 1e-10 yy: the pair is not kept
    assert len(rec['wrapped']) >= 1 and len(rec['state'].S) == 3
    assert rec['state'].done and rec['branch'][-1] == ref.STOP
    assert rec['loss'][-1] < 1e-18 and np.max(np.abs(rec['x'] - 1.0)) < 1e-8


@pytest.mark.parametrize('max_iterations, expected', [
    (3, [ref.ACCEPT, ref.REJECT, ref.ACCEPT, ref.RESTORE, ref.STOP]),
    (10, [ref.ACCEPT, ref.REJECT, ref.ACCEPT, ref.REJECT, ref.RESET, ref.REJECT, ref.ACCEPT, ref.REJECT, ref.RESET, ref.REJECT, ref.RESTORE, ref.STOP]),
    (15, [ref.ACCEPT, ref.REJECT, ref.ACCEPT, ref.REJECT, ref.RESET, ref.REJECT, ref.ACCEPT, ref.REJECT, ref.RESET, ref.REJECT, ref.STALL, ref.STOP]),
])
def test_small_parameters_reset_stall_and_restore(max_iterations, expected):
    """max_ls = 1 and c1 = 0.9 refuse almost every trial: the direction is reset after two of them, a steepest-descent search that fails too stalls,
    and a run that hits max_iterations on a refused trial goes back.  Every run ends with its last evaluation at the point it returns: an accepted one."""
    rec = ref.run(rosenbrock, np.array([3.0, -2.0] * 5), dict(history=3, max_ls=1, c1=0.9, conv_target=1e-18, max_iterations=max_iterations))
    assert rec['branch'] == expected
    st = rec['state']
    assert st.done and len(rec['points']) <= max_iterations + 2
    assert np.array_equal(rec['points'][-1], rec['x']) and np.array_equal(rec['x'], st.x_acc) and rec['f'][-1] == st.f_acc
    accepted = [f for f, b in zip(rec['f'], rec['branch']) if b == ref.ACCEPT]
    assert np.all(np.diff(accepted) < 0)


def test_first_evaluation_that_meets_the_stop_rule_moves_nothing():
    x0 = np.ones(10)
    rec = ref.run(rosenbrock, x0, dict(conv_target=1e-8))
    assert rec['branch'] == [ref.STOP] and np.array_equal(rec['x'], x0) and rec['state'].iters == 0


def test_a_nan_objective_is_a_rejection():
    calls = []

    def evaluate(x):
        r = rosenbrock(x)
        calls.append(1)
        if len(calls) == 2:
            r['reg_loss'] = float('nan')
        return r
    rec = ref.run(evaluate, np.array([-1.2, 1.0] * 5), dict(conv_target=1e-18), 3)
    assert rec['branch'][:2] == [ref.ACCEPT, ref.REJECT]


# ---- against the oracle's Adam loop -----------------------------------------------------------------------------------------------------------------

def test_forty_evaluations_beat_forty_adam_iterations_on_the_oracle():
    """case_c2(3, 2, 24 slices of 0.02: short slices, where the first-order gradient is accurate to the line search's needs), from the same start.
    Measured: L-BFGS 2.335e-02 at its last accepted point within 40 evaluations, the oracle's Adam loop (default rate 0.01) 4.168e-01 at its 40th."""
    c = cases.case_c2(3, 2, steps=24, m=2, taylor=(6, 1), seed=7)
    c['total_time'] = 0.02 * 24
    sp = oracle_system(c)
    rec = ref.run(lambda x: go.evaluate(sp, x), sp.base0, dict(conv_target=-1.0, min_grad=-1.0, max_iterations=1000), 40)
    assert len(rec['loss']) == 40
    lbfgs = [l for l, b in zip(rec['loss'], rec['branch']) if b == ref.ACCEPT][-1]
    adam = go.run_adam(sp, dict(max_iterations=39, conv_target=-1.0, min_grad=-1.0), history=True)['history']
    assert len(adam) == 40
    print('L-BFGS %.6e  Adam %.6e' % (lbfgs, adam[-1, 0]))
    assert lbfgs < adam[-1, 0]


# ---- binding and routing (no library call) ------------------------------------------------------------------------------------------------------------

def test_binding_declares_the_loop():
    for name in ('qoc_iterate_lbfgs', 'qoc_run_lbfgs'):
        assert name in hip_engine.EXPORTED_SYMBOLS
    fields = [(n, t) for n, t in hip_engine.QocLbfgsParams._fields_]
    assert fields == [('conv_target', ctypes.c_double), ('min_grad', ctypes.c_double), ('c1', ctypes.c_double), ('shrink', ctypes.c_double),
                      ('max_iterations', ctypes.c_int32), ('history', ctypes.c_int32), ('max_ls', ctypes.c_int32), ('poll_every', ctypes.c_int32)]
    assert ctypes.sizeof(hip_engine.QocLbfgsParams) == 4 * 8 + 4 * 4
    res, args = hip_engine._SIGNATURES['qoc_iterate_lbfgs']
    assert res is ctypes.c_int and args[1] is ctypes.POINTER(hip_engine.QocLbfgsParams) and args[2] is ctypes.c_int32
    p = hip_engine.HipEngine.lbfgs_params()
    assert (p.conv_target, p.min_grad, p.c1, p.shrink, p.max_iterations, p.history, p.max_ls) == (1e-8, 1e-25, 1e-4, 0.5, 5000, 8, 20)


class _FakeEngine(object):
    """What run_session touches of an engine, recording the loop's calls: every control set finishes at the third evaluation."""
    n_seeds, samples, members, open_system = 2, None, 0, False
    lbfgs_params = staticmethod(hip_engine.HipEngine.lbfgs_params)

    def __init__(self):
        self.bursts, self.params, self.evaluations = [], None, 0

    def iterate_lbfgs(self, params, iters):
        self.params = params
        self.bursts.append(int(iters))
        self.evaluations += int(iters)

    def scalars(self):
        done = int(self.evaluations >= 3)
        return dict(loss=np.array([0.5, 0.25]), reg_loss=np.array([0.5, 0.25]), grad_squared=np.array([1.0, 1.0]), unitary_scale=np.array([1.0, 1.0]),
                    iterations=np.array([self.evaluations - done] * 2, dtype=np.int32), done=np.array([done, done], dtype=np.int32))

    def get_uks(self, evaluated=False):
        return np.zeros((2, 1, 4))

    def get_final_unitary(self):
        return np.stack([np.eye(2, dtype=complex)] * 2)

    def get_inter_vecs(self):
        return np.zeros((2, 5, 2, 2), dtype=complex)

    def close(self):
        pass


def _fake_grape(monkeypatch):
    from quantum_optimal_control.main_grape import grape
    monkeypatch.setattr(hip_engine, 'load_library', lambda: pytest.fail('the library was called'))
    made = []

    class FakeState(object):
        def __init__(self, sys_para, **kwargs):
            self.engine = _FakeEngine()
            made.append(self.engine)

        def build_graph(self):
            return self.engine

        def close(self):
            pass
    monkeypatch.setattr(grape, 'HipState', FakeState)
    return grape, made


def _qubit():
    sx = np.array([[0, 1], [1, 0]], dtype=complex)
    sz = np.array([[1, 0], [0, -1]], dtype=complex)
    return 0.1 * sz, [sx], ['x'], sx


def test_grape_routes_lbfgs_and_maps_the_convergence_keys(monkeypatch):
    grape, made = _fake_grape(monkeypatch)
    H0, Hops, names, U = _qubit()
    conv = dict(conv_target=1e-9, min_grad=1e-20, max_iterations=7, update_step=2, lbfgs_history=5, lbfgs_c1=1e-3, lbfgs_max_ls=11)
    out = grape.Grape(H0, Hops, names, U, 1.0, 4, [0, 1], convergence=conv, method='LBFGS', restarts=2, save=False, show_plots=False, reg_coeffs={})
    assert out is not None and len(made) == 1
    p = made[0].params
    assert (p.conv_target, p.min_grad, p.max_iterations, p.history, p.c1, p.max_ls, p.shrink, p.poll_every) == (1e-9, 1e-20, 7, 5, 1e-3, 11, 0.5, 2)
    assert made[0].bursts == [1, 2]                        # evaluation 0, then to the next multiple of update_step; all done at the third
    # defaults, and the method's name in any case
    made.clear()
    grape.Grape(H0, Hops, names, U, 1.0, 4, [0, 1], convergence=dict(max_iterations=1), method='lbfgs', save=False, show_plots=False, reg_coeffs={})
    p = made[0].params
    assert (p.history, p.c1, p.max_ls, p.max_iterations) == (8, 1e-4, 20, 1)
    assert sum(made[0].bursts) == 3                        # the budget: max_iterations + 2 evaluations


def test_sharded_entry_points_refuse_lbfgs(monkeypatch):
    grape, made = _fake_grape(monkeypatch)
    H0, Hops, names, U = _qubit()
    with pytest.raises(ValueError, match="GrapeSharded: method='LBFGS'"):
        grape.GrapeSharded(H0, Hops, names, U, 1.0, 4, [0, 1], method='LBFGS', restarts=2, save=False, show_plots=False, reg_coeffs={})
    with pytest.raises(ValueError, match="GrapeTimeSharded: method='LBFGS'"):
        grape.GrapeTimeSharded(H0, Hops, names, U, 1.0, 4, [0, 1], method='lbfgs', comm=object(), save=False, show_plots=False, reg_coeffs={})
    with pytest.raises(ValueError, match='time_comm'):
        grape.Grape(H0, Hops, names, U, 1.0, 4, [0, 1], method='LBFGS', time_comm=object(), save=False, show_plots=False, reg_coeffs={})
    assert not made
