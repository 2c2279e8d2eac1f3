"""Device fleets without a GPU: the builders and validate of helper_functions/fleet.py, the start points and the NumPy stream of Grape(fleet=...),
every refusal of the Python layer before the library is loaded, the per-device selection rule and the Taylor rule."""
import numpy as np
import pytest

from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.core.hip_state import HipState
from quantum_optimal_control.helper_functions import fleet as fl_mod
from quantum_optimal_control.helper_functions import robust as rb
from quantum_optimal_control.main_grape import grape as grape_mod
from quantum_optimal_control.parallel_seeds import restart_guesses

SX = np.array([[0, 1], [1, 0]], dtype=complex)
SY = np.array([[0, -1j], [1j, 0]], dtype=complex)
SZ = np.array([[1, 0], [0, -1]], dtype=complex)
DETUNINGS = np.array([[0.010], [-0.004], [0.007]]) * 2 * np.pi
SCALES = np.array([[0.95, 1.0], [1.05, 0.9], [1.0, 1.1]])


def qubit_call(**kw):
    args = dict(H0=0.0 * SZ, Hops=[2 * np.pi * SX / 2, 2 * np.pi * SY / 2], Hnames=['x', 'y'], U=SX, total_time=20.0, steps=16, states_concerned_list=[0, 1],
                maxA=[0.1, 0.1], reg_coeffs={}, save=False, show_plots=False)
    args.update(kw)
    return args


def qubit_fleet():
    return fl_mod.devices([SZ / 2], DETUNINGS, SCALES, k=2)


def grid():
    return rb.ensemble_grid(operators=[SZ / 2], offsets=[[-0.003], [0.0], [0.003]], amp_scales=[0.97, 1.0, 1.03], k=2, risk=20.0)


# ---- builders and validate ----------------------------------------------------------------------------------------------------------------------

def test_devices_builds_one_member_per_device():
    fl = qubit_fleet()
    assert fl.offsets.shape == (3, 1, 1) and fl.amp_scales.shape == (3, 1, 2) and fl.n_devices == 3 and fl.n_members == 1
    assert np.array_equal(fl.offsets[:, 0], DETUNINGS) and np.array_equal(fl.amp_scales[:, 0], SCALES)
    assert np.array_equal(fl.weights, [1.0]) and fl.risk == 0.0 and len(fl.operators) == 1
    only_scales = fl_mod.devices(amp_scales=SCALES, k=2)
    assert only_scales.offsets.shape == (3, 1, 0) and only_scales.operators == []
    only_offsets = fl_mod.devices([SZ / 2], DETUNINGS, None, k=2)
    assert np.array_equal(only_offsets.amp_scales, np.ones((3, 1, 2)))
    dev = fl.device(1)
    assert dev['offsets'].shape == (1, 1) and dev['amp_scales'].shape == (1, 2) and dev['offsets'][0, 0] == DETUNINGS[1, 0]
    assert rb.validate(dev, 2, 2)['weights'][0] == 1.0                    # a device is a robust dict


def test_around_composes_offsets_by_sum_and_scales_by_product():
    ens = grid()
    fl = fl_mod.around([SZ / 2], DETUNINGS, SCALES, robust=ens)
    E = len(ens['weights'])
    assert E == 9 and fl.offsets.shape == (3, 9, 1) and fl.amp_scales.shape == (3, 9, 2)
    for f in range(3):
        for e in range(E):
            for qq in range(1):
                assert fl.offsets[f, e, qq] == DETUNINGS[f, qq] + ens['offsets'][e, qq]
            for j in range(2):
                assert fl.amp_scales[f, e, j] == SCALES[f, j] * ens['amp_scales'][e, j]
    assert np.array_equal(fl.weights, ens['weights']) and fl.risk == 20.0
    with pytest.raises(ValueError, match="the fleet's own operators"):
        fl_mod.around([SZ], DETUNINGS, SCALES, robust=ens)
    with pytest.raises(ValueError, match='robust'):
        fl_mod.around([SZ / 2], DETUNINGS, SCALES)


@pytest.mark.parametrize('change,match', [
    (lambda fl: setattr(fl, 'operators', [np.array([[0, 1], [0, 0]], dtype=complex)]), 'not Hermitian'),
    (lambda fl: fl.offsets.__setitem__((1, 0, 0), np.nan), 'finite'),
    (lambda fl: fl.amp_scales.__setitem__((2, 0, 1), np.inf), 'finite'),
    (lambda fl: setattr(fl, 'amp_scales', fl.amp_scales[:, :, :1]), r'amp_scales have shape \(3, 1, 1\)'),
    (lambda fl: setattr(fl, 'offsets', fl.offsets[:2]), r'offsets have shape \(2, 1, 1\)'),
    (lambda fl: setattr(fl, 'operators', [np.eye(3)]), 'operator 0 has shape'),
    (lambda fl: setattr(fl, 'weights', np.array([1.0, 1.0])), 'weights'),
    (lambda fl: setattr(fl, 'risk', -1.0), 'risk'),
])
def test_validate_names_the_cause(change, match):
    fl = qubit_fleet()
    change(fl)
    with pytest.raises(ValueError, match=match) as err:
        fl_mod.validate(fl, 2, 2)
    assert 'fleet' in str(err.value)


def test_validate_and_the_builders_refuse_what_is_no_fleet():
    with pytest.raises(ValueError, match='Fleet'):
        fl_mod.validate(dict(offsets=DETUNINGS), 2, 2)
    with pytest.raises(ValueError, match='k '):
        fl_mod.devices([SZ], DETUNINGS)
    with pytest.raises(ValueError, match='without operators'):
        fl_mod.devices([], DETUNINGS, SCALES, k=2)
    with pytest.raises(ValueError, match='required with operators'):
        fl_mod.devices([SZ], None, SCALES, k=2)
    with pytest.raises(ValueError, match='no devices'):
        fl_mod.devices(k=2)
    with pytest.raises(ValueError, match=r'amp_scales have shape \(2, 2\), expected \(3, 2\)'):
        fl_mod.devices([SZ], DETUNINGS, SCALES[:2], k=2)


# ---- start points and the NumPy stream ------------------------------------------------------------------------------------------------------------

class LibraryTouched(Exception):
    pass


@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise LibraryTouched()
    monkeypatch.setattr(hip_engine, 'load_library', boom)


def test_tiled_start_points():
    rng = np.random.default_rng(0)
    base = rng.normal(size=(2, 16))
    shared = np.concatenate([base[None], restart_guesses(2, 16, 1, 2)], axis=0)             # what Grape(restarts=3) starts from
    tiled = fl_mod.tile_bases(shared, 4)
    assert tiled.shape == (12, 2, 16)
    for f in range(4):
        for r in range(3):
            assert np.array_equal(tiled[3 * f + r], shared[r])
    own = rng.normal(size=(4, 3, 2, 16))
    assert np.array_equal(fl_mod.tile_bases(own, 4).reshape(4, 3, 2, 16), own)


class _FakeEngine(object):
    def __init__(self, *a, **kw):
        self.kw = kw

    def set_base(self, base):
        self.base = np.array(base)


def test_hip_state_tiles_the_restarts_over_the_devices(monkeypatch):
    """Control set (f, r) starts where control set r of the same state without a fleet starts; a per-device first point replaces r = 0 only."""
    from types import SimpleNamespace
    monkeypatch.setattr(hip_engine, 'HipEngine', _FakeEngine)
    base0 = np.random.default_rng(1).normal(size=(2, 16))
    sp = SimpleNamespace(reg_coeffs={}, use_gpu=True, state_transfer=False, use_inter_vecs=True, ops_max_amp=[0.1, 0.1], dt=1.0, total_time=16.0, steps=16,
                         exp_terms=5, scaling=1, one_minus_gauss=None, ops_weight_base=base0, engine_inputs=lambda: (None, None, None, None, None))
    plain = HipState(sp, n_seeds=3).build_graph().base
    fl = qubit_fleet()
    tiled = HipState(sp, n_seeds=9, fleet=fl).build_graph()
    assert tiled.kw['fleet'] is fl and tiled.kw['n_seeds'] == 9
    assert np.array_equal(tiled.base.reshape(3, 3, 2, 16), np.broadcast_to(plain[None], (3, 3, 2, 16)))
    firsts = np.random.default_rng(2).normal(size=(3, 2, 16))
    own = HipState(sp, n_seeds=9, fleet=fl, fleet_base=firsts).build_graph().base.reshape(3, 3, 2, 16)
    assert np.array_equal(own[:, 0], firsts) and np.array_equal(own[:, 1:], np.broadcast_to(plain[None, 1:], (3, 2, 2, 16)))


@pytest.mark.parametrize('extra', [dict(), dict(transfer='hold'), dict(control_map='identity'), dict(initial_guess='per_device'),
                                   dict(control_map='identity', initial_guess='per_device')])
def test_grape_consumes_the_numpy_stream_as_without_a_fleet(no_library, extra):
    from quantum_optimal_control.helper_functions import control_map as cmap
    from quantum_optimal_control.helper_functions import transfer as tf
    states = []
    for fleet in (None, qubit_fleet()):
        kw = dict(extra)
        if kw.get('transfer'):
            kw['transfer'] = tf.hold(16, 4)
        if kw.get('control_map'):
            kw['control_map'] = cmap.identity(2)
        if kw.get('initial_guess'):
            guess = 0.05 * np.cos(np.arange(3 * 2 * 16)).reshape(3, 2, 16)
            kw['initial_guess'] = guess if fleet is not None else guess[0]
        np.random.seed(123)
        with pytest.raises(LibraryTouched):                                # a valid call gets as far as the engine
            grape_mod.Grape(**qubit_call(fleet=fleet, restarts=2, Taylor_terms=[6, 1], **kw))
        states.append(np.random.get_state())
    assert states[0][0] == states[1][0] and np.array_equal(states[0][1], states[1][1]) and states[0][2:] == states[1][2:]


# ---- refusals of the Python layer, before the library is loaded -----------------------------------------------------------------------------------

def test_grape_refuses_before_the_library_loads(no_library):
    import scipy.sparse as sps
    fl = qubit_fleet()
    refused = dict(robust=grid(), collapse_ops=[], time_comm=object(), plan_seeds=4, _first_seed=1)
    for key, val in refused.items():
        with pytest.raises(ValueError, match='fleet') as err:
            grape_mod.Grape(**qubit_call(fleet=fl, **{key: val}))
        print(key, '->', err.value)
    for method in ('L-BFGS-B', 'BFGS'):
        with pytest.raises(ValueError, match="fleet runs under method='Adam', 'LBFGS' or 'EVOLVE'"):
            grape_mod.Grape(**qubit_call(fleet=fl, method=method))
    with pytest.raises(ValueError, match='fleet does not combine with scipy.sparse'):
        grape_mod.Grape(**qubit_call(fleet=fl, H0=sps.csr_matrix(0.0 * SZ), state_transfer=True, U=[np.array([0, 1.0])], states_concerned_list=[np.array([1.0, 0])]))
    for entry in (grape_mod.GrapeSharded, grape_mod.GrapeTimeSharded):
        with pytest.raises(ValueError, match='fleet'):
            entry(**qubit_call(fleet=fl))
    with pytest.raises(ValueError, match='fleet: amp_scales have shape'):
        grape_mod.Grape(**qubit_call(fleet=fl_mod.devices([SZ / 2], DETUNINGS, np.ones((3, 3)), k=3)))
    with pytest.raises(ValueError, match=r'per-device initial guess of a fleet is \(3, 2, ...\)'):
        grape_mod.Grape(**qubit_call(fleet=fl, initial_guess=np.zeros((2, 2, 16))))
    with pytest.raises(ValueError, match='strength > max_amp for op 1'):
        guess = np.zeros((3, 2, 16))
        guess[2, 1, 5] = 0.2
        grape_mod.Grape(**qubit_call(fleet=fl, initial_guess=guess, Taylor_terms=[6, 1]))
    for method in ('Adam', 'LBFGS', 'EVOLVE'):
        with pytest.raises(LibraryTouched):
            grape_mod.Grape(**qubit_call(fleet=fl, method=method))


def test_hip_engine_refuses_before_the_library_loads(no_library):
    fl = qubit_fleet()

    def make(**kw):
        args = dict(Hs=np.zeros((3, 2, 2)), U0=np.eye(2), V=np.eye(2), W=np.eye(2), maxA=[0.1, 0.1], dt=1.0, total_time=4.0, steps=4, taylor_terms=5, scaling=1,
                    reg_coeffs={}, n_seeds=3, fleet=fl)
        args.update(kw)
        return hip_engine.HipEngine(**args)
    with pytest.raises(LibraryTouched):
        make()
    for kw in (dict(collapse_ops=[]), dict(sparse_ops=[None] * 3), dict(time_comm=object()), dict(time_shards=2)):
        with pytest.raises(ValueError, match='fleet does not combine with'):
            make(**kw)


def test_fleet_arrays_checks_shapes():
    off, amp = hip_engine.fleet_arrays(qubit_fleet(), 1, 1, 2)
    assert off.shape == (3, 1, 1) and amp.shape == (3, 1, 2) and off.flags.c_contiguous and amp.flags.c_contiguous
    off, amp = hip_engine.fleet_arrays(dict(amp_scales=np.ones((4, 2, 3))), 2, 0, 3)
    assert off.shape == (4, 2, 0)
    with pytest.raises(ValueError, match='fleet amp_scales'):
        hip_engine.fleet_arrays(dict(amp_scales=np.ones((4, 2, 3))), 3, 0, 3)
    with pytest.raises(ValueError, match='fleet offsets'):
        hip_engine.fleet_arrays(dict(amp_scales=np.ones((4, 2, 3)), offsets=np.ones((4, 2, 2))), 2, 1, 3)


# ---- the per-device selection rule ----------------------------------------------------------------------------------------------------------------

def test_selection_takes_the_first_smallest_loss_of_every_device_and_never_a_nan():
    nan = np.nan
    loss = np.array([0.3, 0.1, 0.1, 0.2,          # a tie: the first of the equals
                     nan, 0.5, 0.4, nan,          # NaNs never win
                     nan, nan, nan, nan,          # ... unless all are NaN: restart 0
                     0.9, 0.8, 0.7, 0.6])
    best, sets = fl_mod.select_best(loss, 4)
    assert list(best) == [1, 2, 0, 3] and list(sets) == [1, 6, 8, 15]
    best, sets = fl_mod.select_best([0.5, 0.2, 0.7], 3)                   # one restart per device
    assert list(best) == [0, 0, 0] and list(sets) == [0, 1, 2]
    best, sets = fl_mod.select_best([0.5, 0.2, 0.7], 1)                   # one device: run_session's rule for restarts
    assert list(best) == [1] and list(sets) == [1]


# ---- the Taylor rule ------------------------------------------------------------------------------------------------------------------------------

def test_taylor_order_is_the_maximum_over_the_devices():
    """Devices spread over three decades of detuning: the per-device choices differ, and the fleet takes their maximum."""
    a = qubit_call(total_time=40.0, steps=20)
    ens = grid()
    fl = fl_mod.around([SZ / 2], np.array([[0.001], [0.3], [3.0]]) * 2 * np.pi, np.array([[1.0, 1.0], [2.0, 1.0], [1.0, 6.0]]), robust=ens)
    args = (a['maxA'], np.eye(2), a['total_time'], a['steps'], 1e-4, False, False)
    per_device = [rb.choose_taylor(a['H0'], a['Hops'], fl.device(f), *args) for f in range(3)]
    assert len(set(per_device)) > 1, per_device
    want = (max(t for t, _ in per_device), max(s for _, s in per_device))
    assert fl_mod.choose_taylor(fl, a['H0'], a['Hops'], None, *args) == want
    from quantum_optimal_control.helper_functions import control_map as cmap
    cm = cmap.validate(cmap.linear(np.array([[1.0, 0.3], [0.2, 1.0]])), k=2, r=2, steps=a['steps'])
    mapped = [cmap.choose_taylor(cm, a['H0'], a['Hops'], fl.device(f), *args) for f in range(3)]
    assert fl_mod.choose_taylor(fl, a['H0'], a['Hops'], cm, *args) == (max(t for t, _ in mapped), max(s for _, s in mapped))
