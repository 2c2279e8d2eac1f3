"""Open-system GRAPE on the GPU (HipEngine(collapse_ops=...), qoc_create_open, csrc/qoc_lindblad.h) against the NumPy reference of
tests/lindblad_reference.py: parity on the smallest shapes at which each code path can go wrong, for 1 and 3 control sets; the closed limit
against the closed-system oracle; determinism; the device Adam loop; what is refused; and Grape(collapse_ops=...) end to end on the lossy
Lambda system of examples/lossy_lambda_transfer.py."""
import ctypes as C
import functools
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import grape_oracle as go
from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.helper_functions import open_system
from tests import lindblad_reference as lr
from tests.test_adam_tail import LOOP_ATOL, _choose_target
from tests.test_hip_parity import G_RTOL, S_RTOL
from tests.test_open_system import bases_of, open_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
P = hip_engine

# name: (n, k, m, steps, (T, s), c, state_transfer, reg_coeffs)
ROWS = {
    'n3_c1': (3, 1, 2, 17, (4, 0), 1, False, None),
    'n4_c2': (4, 2, 3, 7, (14, 2), 2, False, None),                                     # four sub-steps
    'one_step': (4, 2, 2, 1, (6, 1), 2, False, None),
    'n9_c2': (9, 2, 4, 5, (6, 1), 2, False, None),                                      # two qutrits, ten pairs
    'st_n16_c1': (16, 2, 1, 9, (8, 0), 1, True, None),
    'n32_c4': (32, 4, 2, 3, (5, 1), 4, False, None),                                    # LDS past 64 KiB: the opt-in is needed
    'n32_c5': (32, 4, 2, 3, (5, 1), 5, False, None),                                    # the largest LDS footprint the size rule allows
    'regs': (4, 2, 3, 7, (14, 2), 2, False, {'amplitude': 0.3, 'dwdt': 0.02, 'd2wdt2': 0.001}),
    'band': (4, 2, 3, 16, (14, 2), 2, False, {'bandpass': 0.1, 'band': [0.4, 1.0]}),
}


@functools.lru_cache(maxsize=None)
def system(name):
    n, k, m, steps, taylor, c, st, rc = ROWS[name]
    return open_case(n, k, m, steps, taylor, c, seed=20 + list(ROWS).index(name), state_transfer=st, reg_coeffs=rc)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference at the row's three bases: computed once, shared by every test that needs it."""
    sp, ops = system(name)
    return [lr.evaluate(sp, ops, b) for b in bases_of(sp)]


def make_engine(sp, ops, n_seeds=1, reg_coeffs=None, **kw):
    return hip_engine.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling,
                                state_transfer=sp.state_transfer, reg_coeffs=sp.reg_coeffs if reg_coeffs is None else reg_coeffs,
                                one_minus_gauss=sp.one_minus_gauss, n_seeds=n_seeds, collapse_ops=ops, **kw)


def assert_gradient(tag, got, ref):
    gmax = float(np.max(np.abs(ref)))
    err = float(np.max(np.abs(got - ref)))
    print('%s: max gradient error %.3e, largest entry %.3e' % (tag, err, gmax))
    assert err <= G_RTOL * max(gmax, 1e-3), (tag, err, gmax)


def assert_scalar(tag, got, want):
    print('%s: engine %.17g reference %.17g' % (tag, got, want))
    assert abs(got - want) <= S_RTOL * max(1.0, abs(want)), (tag, got, want)


def assert_eval(name, r, refs):
    for g, o in enumerate(refs):
        for key in ('loss', 'reg_loss', 'unitary_scale', 'grad_squared'):
            assert_scalar('%s %s[%d]' % (name, key, g), r[key][g], o[key])
        assert_gradient('%s grad[%d]' % (name, g), r['grad'][g], o['grad'])


# ---- 1. parity with the reference -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('G', [1, 3])
@pytest.mark.parametrize('name', list(ROWS))
def test_parity_with_the_reference(name, G):
    (sp, ops), refs = system(name), reference(name)
    bases = np.stack(bases_of(sp)[:G] if G > 1 else bases_of(sp)[1:2])       # (one control set: the perturbed base)
    refs = refs[:G] if G > 1 else refs[1:2]
    n, k, m, steps, taylor, c, st, rc = ROWS[name]
    eng = make_engine(sp, ops, G)
    try:
        assert eng.path == P.PATH_LINDBLAD, eng.plan
        plan = eng.plan
        assert (plan['path'], plan['collapse'], plan['pairs'], plan['gradient']) == ('lindblad', str(c), str(m * (m + 1) // 2), 'first_order'), plan
        if name.startswith('n32'):
            assert int(plan['lds']) > 64 * 1024
        eng.set_base(bases)
        r = eng.evaluate()
        assert_eval(name, r, refs)
        if name == 'n4_c2':
            rho, pop = eng.get_final_density(), eng.get_populations()
            assert rho.shape == (G, m, m, n, n) and pop.shape == (G, steps + 1, n, m)
            for g, o in enumerate(refs):
                assert np.max(np.abs(rho[g] - o['rho_final'])) <= S_RTOL                  # every pair, the mirrored ones included
                assert np.max(np.abs(pop[g] - o['populations'])) <= S_RTOL
                assert np.array_equal(rho[g][1, 0], rho[g][0, 1].conj().T)
    finally:
        eng.close()


def test_the_rows_see_the_collapse_operators():
    """The closed-system oracle is far from the open reference on a parity row: the rows cannot pass with the dissipator left out."""
    (sp, ops), refs = system('n4_c2'), reference('n4_c2')
    o = go.evaluate(sp, bases_of(sp)[1])
    assert abs(o['loss'] - refs[1]['loss']) > 1e-3 and refs[1]['unitary_scale'] < 1.0 + 1e-9


# ---- 2. the closed limit, determinism ---------------------------------------------------------------------------------------------------

def test_closed_limit_against_the_closed_oracle():
    sp, _ = system('n4_c2')
    bases = bases_of(sp)
    eng = make_engine(sp, [], 3)
    try:
        assert eng.plan['collapse'] == '0', eng.plan
        eng.set_base(np.stack(bases))
        r = eng.evaluate()
        for g, b in enumerate(bases):
            o = go.evaluate(sp, b)
            for key in ('loss', 'reg_loss', 'grad_squared'):
                assert_scalar('closed limit %s[%d]' % (key, g), r[key][g], o[key])
            assert_gradient('closed limit grad[%d]' % g, r['grad'][g], o['grad'])
            assert abs(r['unitary_scale'][g] - 1.0) <= 1e-9
    finally:
        eng.close()


@pytest.mark.parametrize('name', ['n9_c2', 'n32_c5', 'band'])
def test_two_evaluations_are_bit_identical(name):
    sp, ops = system(name)
    eng = make_engine(sp, ops, 3)
    try:
        eng.set_base(np.stack(bases_of(sp)))
        a = eng.evaluate()
        rho_a = eng.get_final_density()
        b = eng.evaluate()
        for key in ('grad', 'grad_squared', 'loss', 'reg_loss', 'unitary_scale'):
            assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(rho_a, eng.get_final_density())
    finally:
        eng.close()


# ---- 3. the device Adam loop ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _loop_reference():
    sp, ops = system('n4_c2')
    bases = bases_of(sp)
    max_it = 11                                                              # (poll every 5: never a divisor)
    conv = dict(rate=0.02, max_iterations=max_it, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0)
    free = [lr.run_adam(sp, ops, conv, b) for b in bases]
    target, stops = _choose_target([r['history'] for r in free], max_it)
    conv = dict(conv, conv_target=target)
    refs = [lr.run_adam(sp, ops, conv, b) if s < max_it else r for b, r, s in zip(bases, free, stops)]
    assert [r['iterations'] for r in refs] == stops and len(set(stops)) >= 2
    return sp, ops, bases, conv, refs, stops


def test_device_adam_loop_against_the_reference():
    """qoc_run_adam with control sets that stop at different iterations inside one polling burst; a finished set's read-backs stay those of its
    last evaluation."""
    sp, ops, bases, conv, refs, stops = _loop_reference()
    eng = make_engine(sp, ops, 3)
    try:
        eng.set_base(np.stack(bases))
        its = eng.run_adam(eng.adam_params(poll_every=5, **conv))
        assert list(its) == stops
        s = eng.scalars()
        assert list(s['iterations']) == stops and list(s['done']) == [1, 1, 1]
        base, uks, uks_ev, rho = eng.get_base(), eng.get_uks(), eng.get_uks(evaluated=True), eng.get_final_density()
        for g, ref in enumerate(refs):
            print('set %d: %d iterations, max |base - reference| %.3e' % (g, stops[g], np.max(np.abs(base[g] - ref['base']))))
            np.testing.assert_allclose(base[g], ref['base'], rtol=0, atol=LOOP_ATOL)
            np.testing.assert_allclose(uks[g], ref['uks'], rtol=0, atol=LOOP_ATOL)
            np.testing.assert_allclose(uks_ev[g], ref['uks'], rtol=0, atol=LOOP_ATOL)
            for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale'):
                assert abs(s[key][g] - ref['last'][key]) <= LOOP_ATOL * max(1.0, abs(ref['last'][key])), (key, g)
            np.testing.assert_allclose(rho[g], ref['last']['rho_final'], rtol=0, atol=LOOP_ATOL)
    finally:
        eng.close()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------

def _raw_create(n=4, k=1, m=2, steps=4, c=1, T=6, s=1, **fields):
    """qoc_create_open through the bare C ABI: (status, message)."""
    lib = hip_engine.load_library()
    cfg = hip_engine.QocConfig()
    cfg.n, cfg.k, cfg.steps, cfg.m, cfg.taylor_terms, cfg.scaling, cfg.n_seeds = n, k, steps, m, T, s, 1
    cfg.dt, cfg.total_time = 0.1, 0.1 * steps
    for key, value in fields.items():
        setattr(cfg, key, value)
    Hs = np.zeros((k + 1, n, n), dtype=np.complex128)
    eye = np.eye(n, dtype=np.complex128)
    V = np.ascontiguousarray(eye[:, :min(m, n)] if m <= n else np.zeros((n, m), dtype=np.complex128))
    D = np.ones((max(c, 1), n, n), dtype=np.complex128)
    op = hip_engine.QocOpen()
    op.n_collapse, op.C = c, hip_engine._dp(D.view(np.float64))
    maxA = np.ones(k)
    h = C.c_void_p()
    rc = lib.qoc_create_open(C.byref(cfg), C.byref(op), hip_engine._dp(Hs.view(np.float64)), hip_engine._dp(eye.view(np.float64)),
                             hip_engine._dp(V.view(np.float64)), hip_engine._dp(V.view(np.float64)), hip_engine._dp(maxA), None, C.byref(h))
    msg = lib.qoc_last_error().decode()
    if rc == 0:
        lib.qoc_destroy(h)
    return rc, msg


@pytest.mark.parametrize('kw, msg', [
    (dict(n_forbidden=1), 'forbidden levels'), (dict(has_speed_up=1), 'speed_up'), (dict(forbid_dressed=1), 'forbid_dressed'),
    (dict(gradient=1), 'exact gradient'), (dict(time_shards=2), 'time-sharded'), (dict(path=P.PATH_GENERIC), 'QOC_PATH_LINDBLAD'),
    (dict(path=P.PATH_SMALL), 'QOC_PATH_LINDBLAD'), (dict(n=33), 'n = 33'), (dict(n=32, c=6), 'bytes of LDS'), (dict(n=4, c=9), 'at most 8'),
    (dict(n=4, m=5), 'states of interest'), (dict(T=0), 'taylor_terms'), (dict(T=61), 'taylor_terms'), (dict(s=13), 'scaling')])
def test_create_open_refuses(kw, msg):
    rc, text = _raw_create(**kw)
    assert rc == -1 and msg in text and text.startswith('qoc_create_open'), (rc, text)


def test_create_open_accepts_the_lindblad_path_by_name():
    assert _raw_create(path=P.PATH_LINDBLAD)[0] == 0
    assert _raw_create(n=32, c=5)[0] == 0


def test_read_backs_refuse_the_wrong_kind_of_engine():
    sp, ops = system('n3_c1')
    eng = make_engine(sp, ops, 1)
    closed = hip_engine.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, reg_coeffs={})
    try:
        for e in (eng, closed):
            e.set_base(sp.base0[None])
            e.evaluate()
        for call in (eng.get_final_unitary, eng.get_inter_vecs, eng.member_scalars, eng.member_final_unitary, eng.get_pulse,
                     closed.get_final_density, closed.get_populations):
            with pytest.raises(hip_engine.QocError, match='status -4'):
                call()
        assert 'collapse' not in closed.plan and closed.plan['path'] != 'lindblad', closed.plan
        closed.get_final_unitary()
    finally:
        eng.close()
        closed.close()


def test_create_destroy_twenty_times():
    sp, ops = system('n9_c2')
    first = None
    for _ in range(20):
        eng = make_engine(sp, ops, 2)
        eng.set_base(np.stack(bases_of(sp)[:2]))
        r = eng.evaluate()
        eng.close()
        first = r if first is None else first
        assert np.array_equal(r['grad'], first['grad'])


# ---- 5. Grape, end to end ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _lambda_runs():
    import lossy_lambda_transfer as ex
    assert ex.STEPS == 40 and ex.CONVERGENCE['max_iterations'] == 300
    closed, aware = ex.optimise(False), ex.optimise(True)
    return ex.score(closed), ex.score(aware), closed, aware


def test_grape_finds_the_route_around_the_lossy_level():
    """Both pulses scored with method='EVOLVE' under the master equation: the aware pulse's infidelity is at most half the closed-optimised one's
    (the NumPy reference driven the same way, tests/test_open_system.py::test_reference_finds_the_route_around_the_lossy_level: 0.038 against 0.78 after 100 iterations)."""
    inf_closed, inf_aware, closed, aware = _lambda_runs()
    print('infidelity under decay: closed-optimised %.4f, optimised under the master equation %.4f' % (inf_closed, inf_aware))
    assert closed.shape == aware.shape == (2, 40)
    assert 2.0 * inf_aware <= inf_closed, (inf_aware, inf_closed)


def test_grape_evolve_agrees_with_the_reference():
    import lossy_lambda_transfer as ex
    _, inf_aware, _, aware = _lambda_runs()
    H0, Hops, _, start, target, ops = ex.problem()
    T, s = open_system.choose_taylor(H0, Hops, ex.MAXA, ops, ex.TOTAL_TIME / ex.STEPS, ex.STEPS, 1e-4)
    sp = go.OracleSystem(H0, Hops, [target], ex.TOTAL_TIME, ex.STEPS, [start], maxA=ex.MAXA, initial_guess=aware, state_transfer=True,
                         Taylor_terms=[T, s], reg_coeffs={})
    assert abs(lr.evaluate(sp, ops, sp.base0, want_grad=False)['loss'] - inf_aware) <= 1e-10


def test_grape_restarts_return_the_best_set(monkeypatch):
    """Grape(restarts=3, collapse_ops=...) from a poor first start (the pump saturated, the Stokes drive off): every set's final loss and pulse
    are read from the engine just before Grape closes it; the returned pair is the set with the lowest loss, and that is not set 0 (the NumPy
    reference driven the same way ends at 0.865, 0.213, 0.241)."""
    import contextlib
    import io
    import lossy_lambda_transfer as ex
    from quantum_optimal_control.main_grape.grape import Grape
    H0, Hops, names, start, target, ops = ex.problem()
    seen = {}
    close = hip_engine.HipEngine.close

    def recording_close(self):
        if getattr(self, '_h', None) is not None and self._h.value and not seen:
            seen.update(loss=self.scalars()['loss'].copy(), uks=self.get_uks(evaluated=True).copy(), rho=self.get_final_density().copy())
        close(self)
    monkeypatch.setattr(hip_engine.HipEngine, 'close', recording_close)
    guess = np.stack([np.full(12, 1.9), np.full(12, 0.02)])
    with contextlib.redirect_stdout(io.StringIO()):
        uks, rho, loss = Grape(H0, Hops, names, [target], ex.TOTAL_TIME, 12, [start], state_transfer=True, maxA=ex.MAXA, reg_coeffs={}, show_plots=False,
                               save=False, convergence=dict(ex.CONVERGENCE, max_iterations=20), restarts=3, initial_guess=guess, collapse_ops=ops,
                               _return_session=True)
    print('final losses of the three sets: %s; returned %.6f' % (seen['loss'], loss))
    best = int(np.argmin(seen['loss']))
    assert seen['loss'].shape == (3,) and len(set(seen['loss'])) == 3 and best != 0
    assert loss == seen['loss'][best] and np.array_equal(uks, seen['uks'][best]) and np.array_equal(rho, seen['rho'][best])
    assert uks.shape == (2, 12) and rho.shape == (1, 1, 4, 4)
    assert abs(loss - (1.0 - rho[0, 0][2, 2].real)) <= 1e-12 and abs(np.trace(rho[0, 0]) - 1.0) <= 1e-3


def test_grape_run_log_holds_the_open_system_datasets(tmp_path):
    """tests/open_system_h5_script.py in an interpreter with h5py: this one, else the one tests/test_h5_log.py falls back to."""
    from tests import test_h5_log
    if importlib.util.find_spec('h5py') is not None:
        exe = sys.executable
    elif os.path.exists(test_h5_log.CONDA):
        exe = test_h5_log.CONDA
    else:
        pytest.skip('no interpreter with h5py available')
    env = dict(os.environ)
    sys_cxx = '/usr/lib/x86_64-linux-gnu/libstdc++.so.6'
    if exe == test_h5_log.CONDA and os.path.exists(sys_cxx):
        env['LD_PRELOAD'] = ':'.join(x for x in (sys_cxx, env.get('LD_PRELOAD', '')) if x)
    r = subprocess.run([exe, '-W', 'ignore', os.path.join(ROOT, 'tests', 'open_system_h5_script.py'), str(tmp_path)], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0 and 'OK grape_open_system_save' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
