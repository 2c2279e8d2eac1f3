"""k_exact_grad (csrc/qoc_exact_grad.h) in the regimes tests/test_exact_gradient_gpu.py never enters, against the NumPy reference of
tests/exact_gradient_reference.py on three control sets per row:

  * more (trajectory, slice) items than workgroups -- the grid capped at 2048 and by the 256 MiB of scratch -- so that a workgroup takes a
    second and third item: the `item += gridDim.x` stride, the loop-top barrier in front of the reuse of A, PS and the factorial table, and the
    scratch offset blockIdx.x * per_wg, in the LDS and in the global variant, in unitary mode and in state transfer with sources;
  * the limits 2^12 sub-steps and Taylor degree 60, and the refusals just past them;
  * the largest LDS footprint and the first sizes past it at n <= 64;
  * the device Adam loop with control sets that stop at different iterations;
  * create / destroy cycles, refused creates included.

Which regime a row ran in is read from the engine's plan (exact_variant, exact_lds, exact_grid of qoc_plan_describe), never restated here.
The long rows use slices of 0.02 time units (tests/test_adam_tail.py's choice) and the degree-60 rows |A_t| <= ~0.5 (tests/test_hip_fuzz.py's):
with the recipes' 0.2 a low-order polynomial applied a thousand times shrinks the states to nothing and the comparison would be vacuous; every
row asserts that its reference gradient is not."""
import ctypes
import functools

import numpy as np
import pytest

from quantum_optimal_control.core import hip_engine
from tests import exact_gradient_reference as xr
from tests.composed_reference import run_adam
from tests.golden import cases
from tests.helpers import oracle_system
from tests.test_adam_tail import LOOP_ATOL, _choose_target
from tests.test_exact_gradient_gpu import assert_gradient, assert_scalar, bases_of, make_engine, system
from tests.test_hip_parity import G_RTOL, S_RTOL, check_eval  # noqa: F401  (the bounds assert_gradient / assert_scalar apply)

pytestmark = pytest.mark.gpu

P = hip_engine
B = 3


def _rows():
    """name -> (recipe, regime).  regime: variant / lds as the plan must report them; grid = the exact grid, capped = grid < B * steps."""
    c2, c3 = cases.case_c2, cases.case_c3
    rows = {}
    c = c2(n=3, k=2, steps=1400, m=2, taylor=(4, 1), seed=21); c['total_time'] = 0.02 * 1400
    rows['grid_cap_unitary'] = (c, dict(variant='lds', grid=2048))                       # 4200 items: three per workgroup for some
    c = c3(n=4, k=2, steps=700, taylor=(5, 0)); c['total_time'] = 0.02 * 700
    c['reg_coeffs'] = {'dwdt': 1e-3, 'forbidden_coeff_list': [50.0], 'states_forbidden_list': [3]}
    rows['grid_cap_state_transfer'] = (c, dict(variant='lds', grid=2048))                # 2100 items, k_st_bwd_store with sources
    rows['scratch_cap_lds'] = (c2(n=16, k=2, steps=45, m=8, taylor=(4, 10), seed=22), dict(variant='lds', capped=True))
    rows['scratch_cap_global'] = (c2(n=70, k=2, steps=70, m=4, taylor=(4, 8), seed=23), dict(variant='global', capped=True))
    rows['s12'] = (c2(n=8, k=2, steps=50, m=4, taylor=(3, 12), seed=24), dict(variant='lds', capped=True))
    c = c2(n=6, k=2, steps=5, m=3, taylor=(60, 1), seed=25); c['total_time'] = 0.03 * 5
    rows['T60_unitary'] = (c, dict(variant='lds'))
    c = c3(n=6, k=2, steps=5, taylor=(60, 0)); c['total_time'] = 0.015 * 5
    rows['T60_state_transfer'] = (c, dict())
    rows['largest_lds'] = (c2(n=64, k=2, steps=5, m=8, taylor=(7, 1), seed=26), dict(variant='lds', lds=155648))
    rows['n64_past_lds'] = (c2(n=64, k=2, steps=5, m=8, taylor=(8, 1), seed=26), dict(variant='global', lds=0))
    rows['n16_past_lds'] = (c2(n=16, k=2, steps=5, m=16, taylor=(35, 0), seed=27), dict(variant='global', lds=0))
    return rows


ROWS = _rows()


@functools.lru_cache(maxsize=None)
def row_system(name):
    return oracle_system(ROWS[name][0])


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference at the row's three bases: computed once, left unchanged."""
    sp = row_system(name)
    return [xr.evaluate(sp, b) for b in bases_of(sp)]


def assert_regime(name, eng, steps):
    want, plan = ROWS[name][1], eng.plan
    assert eng.path == P.PATH_GENERIC and plan['gradient'] == 'exact', plan
    grid, items = int(plan['exact_grid']), B * steps
    print('%s: exact_variant=%s exact_lds=%s exact_grid=%d items=%d' % (name, plan['exact_variant'], plan['exact_lds'], grid, items))
    assert 1 <= grid <= items
    if 'variant' in want:
        assert plan['exact_variant'] == want['variant'], plan
    if 'lds' in want:
        assert int(plan['exact_lds']) == want['lds'], plan
    if 'grid' in want:
        assert grid == want['grid'] < items, plan
    if want.get('capped'):
        assert grid < items, plan


@pytest.mark.parametrize('name', list(ROWS))
def test_regime_against_the_reference(name):
    """Scalars at S_RTOL, the gradient at G_RTOL of its largest entry, two evaluations bit for bit.  Largest gradient error per row on an MI355X,
    relative to the largest entry: grid_cap_unitary 8.4e-15, grid_cap_state_transfer 4.7e-15, scratch_cap_lds 6.1e-13, scratch_cap_global
    5.7e-13, s12 4.4e-12, T60_unitary 1.3e-15, T60_state_transfer 2.0e-16, largest_lds 4.3e-15, n64_past_lds 2.9e-15, n16_past_lds 5.5e-15.

    unitary_scale at s = 12: twelve squarings of I + E double the rounding of the 1 on the diagonal twelve times, 2^12 eps = 4.5e-13 per slice, and
    50 slices add up.  Against the oracle's own recursion restated in 80-bit extended precision (eps 1.1e-19) the oracle's fp64 value is off by
    +3.2e-13, -6.8e-13 and -1.7e-13 on the three sets; k_expm_generic squares E = P - I instead (E <- 2E + E E, the identity added at the
    end), which the same restatement puts within 2e-15, so the distance to the oracle is the oracle's own error and stays inside S_RTOL = 1e-12.
    (With I + E squared in the kernel as in the oracle, the engine sat at +2.1e-14, -1.6e-12, +1.2e-12 and missed the bound on the third set.)"""
    sp, refs = row_system(name), reference(name)
    eng = make_engine(sp, B, exact_gradient=True)
    try:
        assert_regime(name, eng, sp.steps)
        eng.set_base(np.stack(bases_of(sp)))
        r = eng.evaluate()
        again = eng.evaluate()
        for key in r:
            assert np.array_equal(r[key], again[key]), key                    # every sum in a fixed order, whichever workgroup takes the item
        worst = 0.0
        for g, o in enumerate(refs):
            gmax = float(np.max(np.abs(o['grad'])))
            assert gmax >= 1e-3 and np.isfinite(gmax), (name, g, gmax)        # the bound below is relative to an entry that is there
            for key in ('loss', 'reg_loss', 'unitary_scale', 'grad_squared'):
                assert_scalar('%s %s[%d]' % (name, key, g), r[key][g], o[key])
            worst = max(worst, float(np.max(np.abs(r['grad'][g] - o['grad']))) / gmax)
            assert_gradient('%s grad[%d]' % (name, g), r['grad'][g], o['grad'])
        print('%s: largest gradient error of the row, relative to the largest entry: %.3e (bound %.0e)' % (name, worst, G_RTOL))
    finally:
        eng.close()


@pytest.mark.parametrize('taylor,message', [((3, 13), 'scaling <= 12'), ((61, 1), 'taylor_terms <= 60')], ids=['s13', 'T61'])
def test_past_the_limits_is_refused(taylor, message):
    sp = oracle_system(cases.case_c2(n=8, k=2, steps=5, m=4, taylor=taylor, seed=24))
    with pytest.raises(hip_engine.QocError, match=message):
        make_engine(sp, B, exact_gradient=True)


def test_state_transfer_past_the_degree_limit_is_refused():
    sp = oracle_system(cases.case_c3(n=6, k=2, steps=5, taylor=(61, 0)))
    with pytest.raises(hip_engine.QocError, match='taylor_terms <= 60'):
        make_engine(sp, B, exact_gradient=True)


# ---- the device loop with unequal stops -------------------------------------------------------------------------------------------------

def python_loop(sp, base, conv):
    """tests/test_transfer_gpu.py: python_loop with the reference's exact gradient: go.Adam, run_adam's stop rule and learning-rate schedule."""
    return run_adam(lambda b: xr.evaluate(sp, b), base, conv)


@pytest.mark.parametrize('name', ['n4_allreg', 'state_small'])
def test_device_loop_with_unequal_stops(name):
    """Three control sets, 30 iterations at the most, polled every 4: conv_target lies between the reference's losses so that the sets stop at
    different iterations.  A stopped set stays in the batch while the others run on: k_bwd_store / k_st_bwd_store and k_exact_grad evaluate it
    again at its unmoved controls, and what is read back afterwards must still be its last evaluation."""
    sp = system(name)
    bases = [np.array(b, dtype=np.float64) for b in bases_of(sp)]
    conv = dict(rate=0.02, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=30)
    free = [python_loop(sp, b, conv) for b in bases]
    target, stops = _choose_target([f['history'] for f in free], 30)
    conv['conv_target'] = target
    refs = [f if s == 30 else python_loop(sp, b, conv) for f, s, b in zip(free, stops, bases)]
    assert [r['iterations'] for r in refs] == stops and len(set(stops)) >= 2 and 30 in stops, stops
    eng = make_engine(sp, B, exact_gradient=True)
    try:
        eng.set_base(np.stack(bases))
        its = eng.run_adam(eng.adam_params(poll_every=4, **conv))
        s = eng.scalars()
        base, inter = eng.get_base(), eng.get_inter_vecs()
        print('%s: stops %s (reference %s), conv_target %.6e' % (name, list(its), stops, target))
        assert list(its) == stops and list(s['iterations']) == stops and list(s['done']) == [1] * B
        for g, ref in enumerate(refs):
            print('%s set %d: max |base - reference| %.3e' % (name, g, np.max(np.abs(base[g] - ref['base']))))
            np.testing.assert_allclose(base[g], ref['base'], rtol=0, atol=LOOP_ATOL)
            o = ref['last']                                                       # the reference at this set's own final base
            for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale'):
                assert abs(s[key][g] - o[key]) <= LOOP_ATOL * max(1.0, abs(o[key])), (key, g, s[key][g], o[key])
            np.testing.assert_allclose(inter[g], o['inter_vecs'], rtol=0, atol=LOOP_ATOL * max(1.0, np.max(np.abs(o['inter_vecs']))))
    finally:
        eng.close()


# ---- create and destroy -----------------------------------------------------------------------------------------------------------------

def _free_bytes(hip):
    f, t = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(f), ctypes.byref(t)) == 0
    return f.value


@pytest.mark.parametrize('name', ['largest_lds', 'scratch_cap_global', 'refused'])
def test_create_destroy_releases_device_memory(name):
    """tests/test_hip_parity.py: test_create_destroy_releases_device_memory for an exact engine (its costates and its scratch, 256 MiB in the
    capped row) and for a create that is refused after the path's buffers were allocated: free HBM after 20 cycles is back at the level
    after the first, within the same 8 MiB."""
    hip = ctypes.CDLL('libamdhip64.so')
    sp = oracle_system(cases.case_c2(n=8, k=2, steps=50, m=4, taylor=(3, 13), seed=24)) if name == 'refused' else row_system(name)
    baseline = None
    for cycle in range(20):
        if name == 'refused':
            with pytest.raises(hip_engine.QocError, match='scaling <= 12'):
                make_engine(sp, B, exact_gradient=True)
        else:
            eng = make_engine(sp, B, exact_gradient=True)
            eng.set_base(np.stack([sp.base0] * B))
            eng.evaluate()
            eng.close()
        if cycle == 0:
            baseline = _free_bytes(hip)
    assert _free_bytes(hip) >= baseline - (8 << 20), (name, baseline, _free_bytes(hip))
