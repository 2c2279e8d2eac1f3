"""The exact gradient on the GPU (HipEngine(exact_gradient=True), qoc_config.gradient = 1, csrc/qoc_exact_grad.h) against the NumPy reference of
tests/exact_gradient_reference.py: parity on the generic path and through AUTO for 1 and 3 control sets, with the forward's scalars bit-equal to a
first-order engine's; determinism; the default untouched; composition with ensembles and pulse responses; the device Adam loop; what is
refused; and Grape(exact_gradient=True) with L-BFGS-B on the coarse qutrit gate of examples/coarse_qutrit_x_gate.py."""
import functools
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import grape_oracle as go
from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.helper_functions import transfer as tf
from tests import exact_gradient_reference as xr
from tests.golden import cases
from tests.helpers import oracle_system
from tests.robust_reference import composed, composed_shaped
from tests.test_adam_tail import LOOP_ATOL
from tests.test_hip_parity import G_RTOL, S_RTOL, check_eval
from tests.test_robust_gpu import ensemble, member_systems, nominal_system
from tests.test_transfer_gpu import split_regs, systems

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
P = hip_engine


# ---- rows -------------------------------------------------------------------------------------------------------------------------------

def _rows():
    rows = list(xr.table_rows())                                                        # the nine rows of tests/test_exact_gradient.py
    c2, c3 = cases.case_c2, cases.case_c3
    rows.append(('n3_k1_T4s0', c2(n=3, k=1, steps=17, m=2, taylor=(4, 0), seed=11)))
    rows.append(('n18_T2s1', c2(n=18, k=2, steps=21, m=5, taylor=(2, 1), seed=12)))     # T = 2: no inner sum beyond a + b <= 1
    rows.append(('n8_m1_T7s1', c2(n=8, k=1, steps=9, m=1, taylor=(7, 1), seed=5)))
    rows.append(('n32_T5s3', c2(n=32, k=4, steps=12, m=8, taylor=(5, 3), seed=0)))      # eight sub-steps
    rows.append(('n33_T5s2', c2(n=33, k=2, steps=7, m=8, taylor=(5, 2), seed=13)))      # just past a 32 tile
    c = c2(n=64, k=3, steps=5, m=8, taylor=(5, 2), seed=14)
    c['reg_coeffs'] = {'forbidden_coeff_list': [5.0], 'states_forbidden_list': [63]}
    rows.append(('n64_forbidden', c))                                                   # the largest LDS-resident generator
    rows.append(('n70_T4s1', c2(n=70, k=2, steps=5, m=4, taylor=(4, 1), seed=15)))      # past any LDS-resident size: global scratch
    rows.append(('n25_k8_T7s2', c2(n=25, k=8, steps=6, m=6, taylor=(7, 2), seed=16)))
    rows.append(('one_step', c2(n=4, k=2, steps=1, m=2, taylor=(6, 1), seed=6)))
    rows.append(('st_T2', dict(c3(n=6, k=3, steps=9, taylor=(2, 0)))))                  # K = I + B
    rows.append(('st_T1', dict(c3(n=6, k=3, steps=9, taylor=(1, 0)))))                  # K = I: the fidelity part of dL_du is exactly zero
    rows.append(('st_n40_T6', dict(c3(n=40, k=2, steps=6, taylor=(6, 0)))))
    rows.append(('st_n70_T5', dict(c3(n=70, k=2, steps=5, taylor=(5, 0)))))
    return rows


ROWS = dict(_rows())


@functools.lru_cache(maxsize=None)
def system(name):
    return oracle_system(ROWS[name])


def bases_of(sp):
    b1 = xr.perturbed_base(sp)
    return [sp.base0, b1, -0.5 * b1 + 0.1]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference at the row's three bases: computed once, shared by every path and batch size."""
    sp = system(name)
    return [xr.evaluate(sp, b) for b in bases_of(sp)]


def make_engine(sp, n_seeds=1, path=P.PATH_AUTO, reg_coeffs=None, **kw):
    return hip_engine.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling,
                                state_transfer=sp.state_transfer, reg_coeffs=sp.reg_coeffs if reg_coeffs is None else reg_coeffs,
                                one_minus_gauss=sp.one_minus_gauss, Vs=sp.Vs, n_seeds=n_seeds, path=path, **kw)


def assert_gradient(tag, got, ref):
    gmax = float(np.max(np.abs(ref)))
    err = float(np.max(np.abs(got - ref)))
    print('%s: max gradient error %.3e, largest entry %.3e, ratio %.3e' % (tag, err, gmax, err / max(gmax, 1e-3)))
    assert err <= G_RTOL * max(gmax, 1e-3), (tag, err, gmax)


def assert_scalar(tag, got, want):
    print('%s: engine %.17g reference %.17g' % (tag, got, want))
    assert abs(got - want) <= S_RTOL * max(1.0, abs(want)), (tag, got, want)


# ---- 1. parity with the reference -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('G', [1, 3])
@pytest.mark.parametrize('path', [P.PATH_GENERIC, P.PATH_AUTO], ids=['generic', 'auto'])
@pytest.mark.parametrize('name', list(ROWS))
def test_parity_with_the_reference(name, path, G):
    sp, refs = system(name), reference(name)
    bases = np.stack(bases_of(sp)[:G] if G > 1 else bases_of(sp)[1:2])       # (one control set: the perturbed base)
    refs = refs[:G] if G > 1 else refs[1:2]
    eng = make_engine(sp, G, path, exact_gradient=True)
    first = None
    try:
        assert eng.path == P.PATH_GENERIC and eng.plan['gradient'] == 'exact', eng.plan
        first = make_engine(sp, G, eng.path)
        assert first.plan['gradient'] == 'first_order'
        eng.set_base(bases)
        first.set_base(bases)
        r, f = eng.evaluate(), first.evaluate()
        for key in ('loss', 'reg_loss', 'unitary_scale'):                     # the forward is shared
            assert np.array_equal(r[key], f[key]), (key, r[key], f[key])
        for g, o in enumerate(refs):
            for key in ('loss', 'reg_loss', 'unitary_scale', 'grad_squared'):
                assert_scalar('%s %s[%d]' % (name, key, g), r[key][g], o[key])
            assert_scalar('%s grad_squared[%d] of its own gradient' % (name, g), r['grad_squared'][g], 0.5 * float(np.sum(r['grad'][g] ** 2)))
            assert_gradient('%s grad[%d]' % (name, g), r['grad'][g], o['grad'])
            if name == 'st_T1':
                assert not np.any(o['dL_du'])                                  # K = I: only the pulse regulariser (dwdt) is left in the gradient
    finally:
        eng.close()
        if first is not None:
            first.close()


def test_the_rows_tell_the_two_gradients_apart():
    """On a first-order engine the same comparison fails by orders of magnitude: the parity test cannot pass by accident."""
    name = 'n8_T3s2'
    sp, refs = system(name), reference(name)
    eng = make_engine(sp, 1, P.PATH_GENERIC)
    try:
        eng.set_base(bases_of(sp)[1][None])
        r = eng.evaluate()
        gmax = float(np.max(np.abs(refs[1]['grad'])))
        assert np.max(np.abs(r['grad'][0] - refs[1]['grad'])) >= 1e-2 * gmax
    finally:
        eng.close()


# ---- 2. determinism, and the default untouched ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['n32_T5s3', 'n70_T4s1', 'state_transfer_allreg'])
def test_two_evaluations_are_bit_identical(name):
    sp = system(name)
    eng = make_engine(sp, 3, exact_gradient=True)
    try:
        eng.set_base(np.stack(bases_of(sp)))
        a = eng.evaluate()
        b = eng.evaluate()
        for key in ('grad', 'grad_squared', 'loss', 'reg_loss'):
            assert np.array_equal(a[key], b[key]), key
    finally:
        eng.close()


@pytest.mark.parametrize('name', ['n4_allreg', 'n32_T5s3', 'state_small'])
def test_off_is_off(name):
    sp = system(name)
    bases = bases_of(sp)[:2]
    off = make_engine(sp, 2, exact_gradient=False)
    plain = make_engine(sp, 2)
    try:
        assert off.plan == plain.plan and off.path == plain.path and plain.plan['gradient'] == 'first_order'
        off.set_base(np.stack(bases))
        plain.set_base(np.stack(bases))
        a, b = off.evaluate(), plain.evaluate()
        for key in a:
            assert np.array_equal(a[key], b[key]), key
        check_eval(off, sp, bases)
    finally:
        off.close()
        plain.close()


# ---- 3. composition with ensembles and pulse responses ----------------------------------------------------------------------------------

def _response(kind, steps, total_time):
    if kind == 'hold':
        return tf.hold(steps, 4).matrix
    M = tf.gaussian_filter(steps, 4, total_time, 1.5 * total_time / steps).matrix
    return M / np.maximum(1.0, np.sum(np.abs(M), axis=1))[:, None]                    # rows of l1 norm <= 1: arcsin of the pulse is defined


@pytest.mark.parametrize('name', ['n4_allreg', 'state_transfer_allreg'])
def test_composes_with_an_ensemble(name):
    c = dict(ROWS[name])
    ens = ensemble(c, 3, 1)
    nominal = nominal_system(c)
    sps = member_systems(c, ens, (nominal.exp_terms, nominal.scaling))
    bases = bases_of(nominal)[:2]
    eng = make_engine(nominal, 2, ensemble=ens, exact_gradient=True)
    try:
        assert eng.plan['gradient'] == 'exact' and eng.plan['members'] == '3' and eng.path == P.PATH_GENERIC, eng.plan
        eng.set_base(np.stack(bases))
        r = eng.evaluate()
        for g, b in enumerate(bases):
            o = composed(sps, ens['weights'], b, evaluate=xr.evaluate)
            for key in ('loss', 'reg_loss', 'unitary_scale', 'grad_squared'):
                assert_scalar('%s %s[%d]' % (name, key, g), r[key][g], o[key])
            assert_gradient('%s ensemble grad[%d]' % (name, g), r['grad'][g], o['grad'])
    finally:
        eng.close()


@pytest.mark.parametrize('with_ensemble', [False, True], ids=['nominal', 'ensemble'])
@pytest.mark.parametrize('kind', ['hold', 'gaussian_filter'])
@pytest.mark.parametrize('name', ['n4_allreg', 'state_transfer_allreg'])
def test_composes_with_a_response(name, kind, with_ensemble):
    c = dict(ROWS[name])
    ens = ensemble(c, 3, 1) if with_ensemble else None
    nominal, sps, w = systems(c, ens)
    T = _response(kind, nominal.steps, nominal.total_time)
    _, pulse_rc = split_regs(c['reg_coeffs'])
    thetas = np.random.default_rng(77).normal(0.0, 0.7, size=(2, nominal.k, 4))
    eng = make_engine(nominal, 2, ensemble=ens, transfer=T, exact_gradient=True)
    try:
        assert eng.plan['gradient'] == 'exact' and eng.plan['samples'] == '4' and eng.path == P.PATH_GENERIC, eng.plan
        eng.set_base(thetas)
        r = eng.evaluate()
        for g in range(2):
            o = composed_shaped(sps, w, T, thetas[g], pulse_rc, nominal.total_time, evaluate=xr.evaluate)
            for key in ('loss', 'reg_loss', 'unitary_scale', 'grad_squared'):
                assert_scalar('%s %s[%d]' % (name, key, g), r[key][g], o[key])
            assert_gradient('%s %s grad[%d]' % (name, kind, g), r['grad'][g], o['grad'])
    finally:
        eng.close()


# ---- 4. the device Adam loop ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['n4_allreg', 'state_small'])
def test_device_adam_loop_follows_the_exact_gradient(name):
    """25 loop iterations against go.Adam driven on the host by the reference gradient with the loop's learning-rate schedule; the final bases
    agree to the tolerance of tests/test_adam_tail.py: test_loop_against_the_oracle."""
    sp = system(name)
    rate, decay, iters = 0.02, 50.0, 25
    base = np.array(sp.base0, dtype=np.float64)
    opt = go.Adam(base.shape)
    for it in range(1, iters + 1):
        base = opt.step(base, xr.evaluate(sp, base)['grad'], rate * np.exp(-float(it) / decay))
    eng = make_engine(sp, 1, exact_gradient=True)
    try:
        eng.set_base(sp.base0[None])
        eng.iterate(eng.adam_params(rate=rate, learning_rate_decay=decay, conv_target=-1.0, min_grad=-1.0, max_iterations=1000, poll_every=5), iters)
        eng.sync()
        s = eng.scalars()
        assert list(s['iterations']) == [iters] and list(s['done']) == [0]
        got = eng.get_base()[0]
        print('%s: max |base - reference| after %d iterations %.3e' % (name, iters, np.max(np.abs(got - base))))
        np.testing.assert_allclose(got, base, rtol=0, atol=LOOP_ATOL)
    finally:
        eng.close()


# ---- 5. capability ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('path', [P.PATH_SMALL, P.PATH_MFMA, P.PATH_GEMM, P.PATH_ST_FUSED], ids=['small', 'mfma', 'gemm', 'st_fused'])
def test_other_paths_refuse_the_exact_gradient(path):
    sp = system('state_small' if path == P.PATH_ST_FUSED else 'n4_T6s1')
    with pytest.raises(hip_engine.QocError, match='exact gradient'):
        make_engine(sp, 1, path, exact_gradient=True)


def test_time_sharding_refuses_the_exact_gradient():
    with pytest.raises(hip_engine.QocError, match='exact gradient'):
        make_engine(system('n4_T6s1'), 1, exact_gradient=True, time_shards=2, time_rank=-1)


def test_auto_resolves_to_the_generic_path():
    sp = system('n3_k1_T4s0')
    plain = make_engine(sp, 1)
    eng = make_engine(sp, 1, exact_gradient=True)
    try:
        assert plain.path == P.PATH_SMALL                                      # what AUTO picks for this shape otherwise
        assert eng.path == P.PATH_GENERIC and eng.plan['path'] == 'generic' and eng.plan['gradient'] == 'exact', eng.plan
    finally:
        plain.close()
        eng.close()


# ---- 6. Grape, end to end ---------------------------------------------------------------------------------------------------------------

def _final_error(log):
    errors = [float(line.split('Error = :')[1].split(';')[0]) for line in log.splitlines() if line.startswith('Error = :')]
    return errors[-1]


@functools.lru_cache(maxsize=None)
def _lbfgs_runs():
    """The 10-slice qutrit X gate of examples/coarse_qutrit_x_gate.py (Taylor_terms [12, 3], np.random.seed(4), method 'L-BFGS-B', conv_target 1e-12,
    max_iterations 400), once per gradient: run once, shared by the tests below.  The example's convergence dict carries 'ftol': 0, which takes
    scipy's relative-reduction stop (default 2.2e-9) out of both runs, so that conv_target, min_grad and the 400 evaluations alone end them: with
    the default the first-order run gives up at 5.64e-8 after 189 evaluations (the CPU oracle driven the same way: 188, 5.637e-8) and there
    would be no converged run to compare evaluation counts with."""
    import coarse_qutrit_x_gate as ex
    assert ex.CONVERGENCE['conv_target'] == 1e-12 and ex.CONVERGENCE['max_iterations'] == 400 and ex.TAYLOR == [12, 3]
    first, exact = ex.run(False), ex.run(True)
    for name, r in (('first-order', first), ('exact', exact)):
        print('%s: %d evaluations, final loss %.3e, infidelity by exact propagators %.3e; %s' % (
            name, r['evaluations'], _final_error(r['log']), r['infidelity'],
            ' / '.join(line for line in r['log'].splitlines() if line.startswith(('CONVERGENCE', 'STOP', 'ABNORMAL')))))
    return first, exact


def test_grape_lbfgs_reaches_the_target_with_either_gradient():
    """Both runs reach a loss below 1e-10 (the engine's own loss, and the infidelity re-simulated with exact propagators)."""
    first, exact = _lbfgs_runs()
    assert _final_error(exact['log']) < 1e-10 and exact['infidelity'] < 1e-10
    assert _final_error(first['log']) < 1e-10 and first['infidelity'] < 1e-10, (_final_error(first['log']), first['evaluations'])


def test_grape_lbfgs_needs_fewer_evaluations_with_the_exact_gradient():
    """The exact run uses at most half the engine evaluations of the first-order run (counted by wrapping HipEngine.evaluate).  The CPU oracle
    driven the same way needs 14 against 219; the factor of two leaves room for line searches that branch differently under GPU rounding."""
    first, exact = _lbfgs_runs()
    assert 2 * exact['evaluations'] <= first['evaluations'], (exact['evaluations'], first['evaluations'])


def test_lbfgs_default_stop_is_scipys_unless_ftol_is_given():
    """Without 'ftol' the driver passes what it always passed: the first-order run of the same problem ends on scipy's relative-reduction test."""
    import coarse_qutrit_x_gate as ex
    conv = {key: v for key, v in ex.CONVERGENCE.items() if key != 'ftol'}
    r = ex.run(False, convergence=conv)
    print('default ftol, first-order: %d evaluations, final loss %.3e' % (r['evaluations'], _final_error(r['log'])))
    assert 'RELATIVE REDUCTION OF F' in r['log'] and _final_error(r['log']) > 1e-10


@pytest.mark.parametrize('method', ['Adam', 'EVOLVE'])
def test_grape_other_drivers_take_the_keyword(method):
    import coarse_qutrit_x_gate as ex
    conv = dict(ex.CONVERGENCE, max_iterations=30, rate=0.02)
    r = ex.run(True, method=method, convergence=conv, restarts=2 if method == 'Adam' else 1)
    assert r['uks'].shape == (2, ex.STEPS) and np.all(np.isfinite(r['uks'])) and 0.0 <= r['infidelity'] <= 1.0


def test_grape_run_log_holds_the_flag(tmp_path):
    """tests/exact_gradient_h5_script.py in an interpreter with h5py: this one, else the one tests/test_h5_log.py falls back to."""
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
    r = subprocess.run([exe, '-W', 'ignore', os.path.join(ROOT, 'tests', 'exact_gradient_h5_script.py'), str(tmp_path)], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0 and 'OK grape_exact_gradient_save' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_coarse_qutrit_example():
    import coarse_qutrit_x_gate as ex
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        inf_first, inf_exact = ex.main(quiet=True)
    assert inf_exact < 1e-9
