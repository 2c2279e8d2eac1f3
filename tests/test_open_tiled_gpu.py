"""The tiled open-system path on the GPU (path=PATH_LINDBLAD_TILED, csrc/qoc_lindblad_tiled.h) against the NumPy references the LDS path is tested with
(tests/lindblad_reference.py, tests/open_fleet_reference.py, tests/running_cost_reference.py), on the rows of tests/open_tiled_cases.py for one and
three control sets: parity and the plan line; the closed limit against the closed oracle; both open paths on one problem; zero pads and determinism
across evaluations and engines; member rows; running costs; the device Adam loop; the refusals of the bare C ABI; and the cavity example end to end
at a reduced size.

Tolerances: S_RTOL, G_RTOL and LOOP_ATOL, applied as tests/test_open_system_gpu.py applies them (its assert_scalar, assert_gradient, assert_eval)."""
import contextlib
import functools
import io
import os
import sys

import numpy as np
import pytest

from oracle import grape_oracle as go
from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.helper_functions import open_system
from tests import lindblad_reference as lr
from tests import open_fleet_reference as ofr
from tests import open_tiled_cases as tc
from tests import running_cost_reference as rc
from tests.test_adam_tail import LOOP_ATOL
from tests.test_hip_parity import S_RTOL
from tests.test_open_system import bases_of, open_case
from tests.test_open_system_gpu import _raw_create, assert_eval, assert_gradient, assert_scalar
from tests.test_running_costs import dense_observable

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
P = hip_engine
TILED = P.PATH_LINDBLAD_TILED
KEYS = ('loss', 'reg_loss', 'unitary_scale', 'grad_squared')


def make_engine(sp, ops, n_seeds=1, path=TILED, **kw):
    return P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, state_transfer=sp.state_transfer,
                       reg_coeffs=sp.reg_coeffs, one_minus_gauss=sp.one_minus_gauss, n_seeds=n_seeds, collapse_ops=ops, path=path, **kw)


def np_of(n):
    return 16 * ((n + 15) // 16)


def assert_plan(eng, n, m, c, trajectories):
    """path=lindblad_tiled collapse=<c> pairs=<R> np=<NP> work=<bytes>: five NP x NP complex matrices per (trajectory, pair)."""
    plan, R = eng.plan, m * (m + 1) // 2
    assert eng.path == TILED and list(plan)[:5] == ['path', 'collapse', 'pairs', 'np', 'work'], plan
    assert (plan['path'], plan['collapse'], plan['pairs'], plan['np'], plan['gradient']) == ('lindblad_tiled', str(c), str(R), str(np_of(n)), 'first_order'), plan
    assert int(plan['work']) == trajectories * R * 5 * np_of(n) ** 2 * 16 and 'lds' not in plan, plan


def sets_of(sp, refs, G):
    """(bases, references) of a row for G control sets (one control set: the perturbed base), as tests/test_open_system_gpu.py picks them."""
    return (np.stack(bases_of(sp)[:G]), refs[:G]) if G > 1 else (np.stack(bases_of(sp)[1:2]), refs[1:2])


# ---- 1. parity with the reference -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('G', [1, 3])
@pytest.mark.parametrize('name', list(tc.ROWS))
def test_parity_with_the_reference(name, G):
    (sp, ops), (_, n, k, m, steps, taylor, c) = tc.system(name), tc.ROWS[name]
    bases, refs = sets_of(sp, tc.reference(name), G)
    eng = make_engine(sp, ops, G)
    try:
        assert_plan(eng, n, m, c, G)
        eng.set_base(bases)
        r = eng.evaluate()
        assert_eval(name, r, refs)
        if name in ('n16', 'near33'):
            rho, pop = eng.get_final_density(), eng.get_populations()
            assert rho.shape == (G, m, m, n, n) and pop.shape == (G, steps + 1, n, m)
            for g, o in enumerate(refs):
                assert np.max(np.abs(rho[g] - o['rho_final'])) <= S_RTOL                  # every pair, the mirrored ones included
                assert np.max(np.abs(pop[g] - o['populations'])) <= S_RTOL
                assert np.array_equal(rho[g][1, 0], rho[g][0, 1].conj().T)
    finally:
        eng.close()


# ---- 2. the closed limit ----------------------------------------------------------------------------------------------------------------

def test_closed_limit_against_the_closed_oracle():
    """n = 33 without collapse operators: the closed engine's loss and gradient ((T, s) = (14, 2): the two Taylor conventions agree to rounding)."""
    sp, _ = open_case(33, 2, 2, 3, (14, 2), 0, seed=230)
    bases = bases_of(sp)
    eng = make_engine(sp, [], 3)
    try:
        assert_plan(eng, 33, 2, 0, 3)
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


# ---- 3. both paths on one problem -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', tc.BOTH_PATHS)
def test_both_paths_agree(name):
    sp, ops = tc.system(name)
    bases = np.stack(bases_of(sp))
    out = {}
    for path in (P.PATH_LINDBLAD, TILED):
        eng = make_engine(sp, ops, 3, path=path)
        try:
            assert eng.path == path and eng.plan['path'] == ('lindblad' if path == P.PATH_LINDBLAD else 'lindblad_tiled'), eng.plan
            eng.set_base(bases)
            out[path] = (eng.evaluate(), eng.get_final_density(), eng.get_populations())
        finally:
            eng.close()
    (a, rho_a, pop_a), (b, rho_b, pop_b) = out[P.PATH_LINDBLAD], out[TILED]
    for g in range(3):
        for key in KEYS:
            assert_scalar('%s %s[%d] tiled against LDS' % (name, key, g), b[key][g], a[key][g])
        assert_gradient('%s grad[%d] tiled against LDS' % (name, g), b['grad'][g], a['grad'][g])
    assert np.max(np.abs(rho_a - rho_b)) <= S_RTOL and np.max(np.abs(pop_a - pop_b)) <= S_RTOL


# ---- 4. pads and determinism ------------------------------------------------------------------------------------------------------------

def _evaluate_at(eng, base):
    eng.set_base(base[None])
    r = eng.evaluate()
    return {key: np.array(r[key]) for key in KEYS + ('grad',)}, eng.get_final_density().copy()


@pytest.mark.parametrize('name', ['n17', 'near33'])
def test_pads_stay_zero_and_evaluations_are_bit_identical(name):
    """Base A, base B, base A on one engine: what B left in the scratch (pads included) does not reach the third evaluation.  Then A on a second
    engine made after an n = 128 engine ran and was closed: its scratch may be the memory that engine wrote all over."""
    sp, ops = tc.system(name)
    A, B = bases_of(sp)[1], bases_of(sp)[2]
    eng = make_engine(sp, ops, 1)
    try:
        first, rho_first = _evaluate_at(eng, A)
        other, _ = _evaluate_at(eng, B)
        third, rho_third = _evaluate_at(eng, A)
    finally:
        eng.close()
    assert not np.array_equal(first['grad'], other['grad'])
    for key in first:
        assert np.array_equal(first[key], third[key]), key
    assert np.array_equal(rho_first, rho_third)
    big_sp, big_ops = tc.system('n128')
    big = make_engine(big_sp, big_ops, 3)
    try:
        big.set_base(np.stack(bases_of(big_sp)))
        big.evaluate()
    finally:
        big.close()
    eng = make_engine(sp, ops, 1)
    try:
        again, rho_again = _evaluate_at(eng, A)
    finally:
        eng.close()
    for key in first:
        assert np.array_equal(first[key], again[key]), key
    assert np.array_equal(rho_first, rho_again)


# ---- 5. member rows ---------------------------------------------------------------------------------------------------------------------

def test_members_with_their_own_rates():
    """An ensemble of two members at n = 33 with different rate scales (and drifts and amplitude scales): k_lbt_forward<true> / k_lbt_backward<true>
    on the rows of H0 and of the scaled, padded D_j."""
    n, k, m, steps, c = 33, 2, 2, 2, 2
    p = ofr.problem(n, k, steps, m, c, taylor=(5, 1), seed=40)
    ens = ofr.make_fleet(p, 1, 2, 1, zero=False).device(0)
    assert len(set(np.asarray(ens['rate_scales']).reshape(-1))) == 2 * c
    xs = np.random.default_rng(6100).normal(0.0, 0.7, size=(2, k, steps))
    sp = ofr.engine_system(p)
    eng = P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, p['maxA'], sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, state_transfer=sp.state_transfer,
                      reg_coeffs=p['reg_coeffs'], n_seeds=2, ensemble=ens, path=TILED)
    try:
        assert_plan(eng, n, m, c, 4)
        assert eng.plan['members'] == '2' and eng.open_system and eng.members == 2, eng.plan
        eng.set_base(xs)
        r, ms, rho_m, rho0, pop = eng.evaluate(), eng.member_scalars(), eng.member_final_density(), eng.get_final_density(), eng.get_populations()
        assert rho_m.shape == (2, 2, m, m, n, n)
        for g in range(2):
            o = ofr.evaluate(p, None, ens, xs[g])
            for key in KEYS:
                assert_scalar('members %s[%d]' % (key, g), r[key][g], o[key])
            assert_gradient('members grad[%d]' % g, r['grad'][g], o['grad'])
            assert abs(o['member_loss'][0] - o['member_loss'][1]) > 1e-6
            assert np.max(np.abs(ms['loss'][g] - o['member_loss'])) <= S_RTOL * max(1.0, np.max(np.abs(o['member_loss'])))
            assert np.all(ms['reg_state'][g] == 0.0)
            assert np.max(np.abs(rho_m[g] - o['member_rho'])) <= S_RTOL
            assert np.max(np.abs(rho0[g] - o['rho_final'])) <= S_RTOL and np.max(np.abs(pop[g] - o['populations'])) <= S_RTOL
    finally:
        eng.close()


# ---- 6. running costs -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _costs_case():
    sp, ops = tc.system('near33')
    costs = [open_system.level_cost(33, 32, 0.8, 2), open_system.observable_cost(dense_observable(33, 33), -0.6, 1)]
    return sp, ops, costs, [rc.evaluate(sp, ops, costs, b) for b in bases_of(sp)]


@pytest.mark.parametrize('G', [1, 3])
def test_running_costs(G):
    sp, ops, costs, refs = _costs_case()
    bases, refs = sets_of(sp, refs, G)
    eng = make_engine(sp, ops, G, running_costs=costs)
    try:
        assert_plan(eng, 33, 2, 2, G)
        assert eng.plan['running_costs'] == '2' and list(eng.plan)[-1] == 'running_costs', eng.plan
        eng.set_base(bases)
        r = eng.evaluate()
        x, ms, rho = eng.get_expectations(), eng.member_scalars(), eng.get_final_density()
        assert x.shape == (G, sp.steps + 1, 2, 2)
        for g, o in enumerate(refs):
            for key in KEYS:
                assert_scalar('costs %s[%d]' % (key, g), r[key][g], o[key])
            assert_gradient('costs grad[%d]' % g, r['grad'][g], o['grad'])
            assert_scalar('costs reg_state[%d]' % g, ms['reg_state'][g, 0], o['reg_state'])
            assert np.max(np.abs(x[g] - o['expectations'])) <= S_RTOL * max(1.0, np.max(np.abs(o['expectations'])))
            assert np.max(np.abs(rho[g] - o['rho_final'])) <= S_RTOL
            assert abs(o['reg_state']) > 1e-3                                       # (the term is visible in reg_loss)
    finally:
        eng.close()


# ---- 7. the device Adam loop ------------------------------------------------------------------------------------------------------------

def test_device_adam_loop_against_the_reference():
    sp, ops = tc.system('near33')
    bases = bases_of(sp)[:2]
    conv = dict(rate=0.02, max_iterations=5, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0)
    refs = [lr.run_adam(sp, ops, conv, b) for b in bases]
    eng = make_engine(sp, ops, 2)
    try:
        eng.set_base(np.stack(bases))
        its = eng.run_adam(eng.adam_params(poll_every=5, **conv))
        assert list(its) == [ref['iterations'] for ref in refs] == [5, 5]
        s = eng.scalars()
        base, uks, rho = eng.get_base(), eng.get_uks(), eng.get_final_density()
        for g, ref in enumerate(refs):
            print('set %d: max |base - reference| %.3e' % (g, np.max(np.abs(base[g] - ref['base']))))
            assert not np.allclose(base[g], bases[g], rtol=0, atol=1e-3)             # (the loop moved the variable)
            np.testing.assert_allclose(base[g], ref['base'], rtol=0, atol=LOOP_ATOL)
            np.testing.assert_allclose(uks[g], ref['uks'], rtol=0, atol=LOOP_ATOL)
            for key in KEYS:
                assert abs(s[key][g] - ref['last'][key]) <= LOOP_ATOL * max(1.0, abs(ref['last'][key])), (key, g)
            np.testing.assert_allclose(rho[g], ref['last']['rho_final'], rtol=0, atol=LOOP_ATOL)
    finally:
        eng.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kw, msg', [
    (dict(n=129), 'qoc_create_open: n = 129 (1 .. 128 levels on QOC_PATH_LINDBLAD_TILED)'),
    (dict(n=0), 'qoc_create_open: n = 0 (1 .. 128 levels on QOC_PATH_LINDBLAD_TILED)'),
    (dict(n=4, c=9), 'at most 8'), (dict(n=4, m=5), 'm = 5 states of interest (1 .. n = 4)')])
def test_create_open_refuses_on_the_tiled_path(kw, msg):
    rc_, text = _raw_create(path=TILED, **kw)
    assert rc_ == -1 and msg in text and text.startswith('qoc_create_open'), (rc_, text)


def test_create_open_accepts_the_tiled_path_by_name_and_closed_engines_do_not():
    assert _raw_create(path=TILED)[0] == 0
    assert _raw_create(path=TILED, n=32, c=6)[0] == 0 and _raw_create(path=TILED, n=33, c=8)[0] == 0
    sp, _ = tc.system('n3')
    with pytest.raises(P.QocError, match='unknown path 8'):
        P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, reg_coeffs={}, path=TILED)


def test_auto_takes_the_tiled_path_where_the_lds_rule_ends():
    """HipEngine resolves AUTO through open_system.choose_path: an engine that ran before keeps PATH_LINDBLAD, n = 33 runs tiled."""
    for name, path in (('n17', P.PATH_LINDBLAD), ('n33_s2', TILED), ('n32_c6', TILED)):
        sp, ops = tc.system(name)
        eng = make_engine(sp, ops, 1, path=P.PATH_AUTO)
        try:
            assert eng.path == path, (name, eng.plan)
        finally:
            eng.close()


# ---- 9. Grape, end to end ---------------------------------------------------------------------------------------------------------------

def test_cavity_example_end_to_end(monkeypatch):
    """examples/cavity_fock_state_under_loss.py at cavity 17 (n = 34), 20 slices, 5 iterations: Grape(collapse_ops=...) lands on the tiled path unasked."""
    import cavity_fock_state_under_loss as ex
    plans = []
    close = P.HipEngine.close

    def recording_close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            plans.append(dict(self.plan))
        close(self)
    monkeypatch.setattr(P.HipEngine, 'close', recording_close)
    size = dict(cavity=17, total_time=1.0)
    closed = ex.optimise(False, steps=20, iterations=5, **size)
    assert [p['path'] == 'lindblad_tiled' for p in plans] == [False]
    aware = ex.optimise(True, steps=20, iterations=5, **size)
    assert plans[-1]['path'] == 'lindblad_tiled' and plans[-1]['np'] == '48' and plans[-1]['collapse'] == '2', plans[-1]
    assert closed.shape == aware.shape == (4, 20) and np.all(np.isfinite(closed)) and np.all(np.isfinite(aware))
    assert not np.array_equal(closed, aware)
    for uks in (closed, aware):
        rho = ex.final_density(uks, **size)
        assert plans[-1]['path'] == 'lindblad_tiled'
        assert rho.shape == (34, 34) and np.all(np.isfinite(rho)) and abs(np.trace(rho) - 1.0) <= 1e-9, abs(np.trace(rho) - 1.0)
        assert 0.0 <= ex.score(uks, **size) <= 1.0
