"""How an engine is constructed, in both languages.

A. HipEngine's dispatch against a recording stand-in for the library: for every combination of keywords the creation symbol, which of its
   arguments are NULL, every field of every struct passed (scalars, NULL pointers, the arrays behind the others read back through the recorded
   pointers) and the attributes the engine derives from them.  The expected table is written out below from the raw inputs.
B. The order of the library's refusals, through the real library and ctypes: inputs with two defects that belong to different stages of the
   construction funnel of csrc/qoc_engine.hip are refused with the message of the earlier stage.  Every call is refused on the host, before any
   device is touched, so this part needs no GPU (and creates nothing where there is one).
C. (gpu) The combinations of A built for real: one evaluation each, the plan's words, the shapes of the read-backs.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

from quantum_optimal_control.core import hip_engine as P
from quantum_optimal_control.helper_functions import control_map as cmap_mod
from quantum_optimal_control.helper_functions import fleet as fleet_mod

N, K, M, STEPS, SEEDS, E, Q, NP, F, NC, L = 3, 2, 1, 4, 2, 2, 1, 2, 2, 1, 1
R, D = 3, 2                       # a control map: R operators fed by the K pulses, degree D
DT, TOTAL, TAYLOR, SCALING = 0.1, 0.4, 3, 1

_rng = np.random.RandomState(7)


def _herm():
    a = _rng.randn(N, N) + 1j * _rng.randn(N, N)
    return (a + a.conj().T) / 2


H = np.stack([-1j * DT * _herm() for _ in range(R + 1)])            # -i dt H_j: the first K + 1 without a map, all R + 1 with one
U0 = np.eye(N, dtype=np.complex128)
V = np.ascontiguousarray(np.eye(N, dtype=np.complex128)[:, :M])
W = np.ascontiguousarray(np.eye(N, dtype=np.complex128)[:, 1:1 + M])
MAXA = np.array([1.0, 0.5])
PERT = [_herm() for _ in range(Q)]
ENS_OFF = np.array([[-0.2], [0.3]])
ENS_AMP = np.array([[0.9, 1.1], [1.0, 0.8]])
ENS_W = np.array([0.25, 0.75])
FL_OFF = np.array([[[-0.1], [0.1]], [[0.2], [-0.3]]])
FL_AMP = np.array([[[1.0, 0.9], [0.8, 1.2]], [[1.1, 1.0], [0.7, 0.95]]])
FL_AMP1 = np.array([[[1.0, 0.9]], [[1.1, 0.7]]])                  # a fleet of one member per device
TR = np.array([[1.0, 0.0], [0.5, 0.5], [0.0, 1.0], [0.0, 0.25]])
ALPHA = 0.1 * (1.0 + np.arange(R * K * D, dtype=np.float64).reshape(R, K, D))
MIX = 1.0 + 0.01 * np.arange(R * K * STEPS, dtype=np.float64).reshape(R, K, STEPS)
FIXED = 0.02 * np.arange(R * STEPS, dtype=np.float64).reshape(R, STEPS)
COLLAPSE = [np.sqrt(0.2) * np.diag(np.sqrt(np.arange(1, N)), 1).astype(np.complex128)]
RATES_E = np.array([[1.0], [2.5]])
RATES_F = np.array([[[1.0], [0.5]], [[2.0], [0.0]]])
COST_O = np.diag([0.0, 0.0, 1.0]).astype(np.complex128)
COSTS = [(COST_O, 0.3, 2)]
SP_DIAG = np.array([[1.0, -0.5, 0.25], [0.3, 0.7, -0.2], [0.6, 0.1, 0.9], [-0.4, 0.8, 0.5]])       # the diagonals of R + 1 sparse operators
SP_OPS = [sps.diags(-1j * DT * d).tocsr() for d in SP_DIAG]
SP_PERT_DIAG = np.array([[0.5, -1.0, 0.75]])
SP_PERT = [sps.diags(d).tocsr() for d in SP_PERT_DIAG]

ARGS = {
    'qoc_create': 'cfg Hs U0 V W maxA omg fs fc Vs out',
    'qoc_create_ensemble': 'cfg ens Hs U0 V W maxA omg fs fc Vs out',
    'qoc_create_shaped': 'cfg ens tr Hs U0 V W maxA omg fs fc Vs out',
    'qoc_create_mapped': 'cfg ens tr map Hs U0 V W maxA omg fs fc Vs out',
    'qoc_create_fleet': 'cfg ens fleet tr map Hs U0 V W maxA omg fs fc Vs out',
    'qoc_create_open': 'cfg open Hs U0 V W maxA omg out',
    'qoc_create_open_fleet': 'cfg decay ens fleet tr map Hs U0 V W maxA omg out',
    'qoc_create_open_costs': 'cfg decay costs ens fleet tr map Hs U0 V W maxA omg out',
    'qoc_create_sparse': 'cfg sparse V W maxA omg fs fc out',
    'qoc_create_sparse_fleet': 'cfg sparse plan ens fleet tr map V W maxA omg fs fc out',
}
ARGS = {name: names.split() for name, names in ARGS.items()}


def test_the_argument_names_match_the_signatures():
    for name, names in ARGS.items():
        assert len(names) == len(P._SIGNATURES[name][1]), name


# ---- A. the expected table --------------------------------------------------------------------------------------------------------------------

def _cfg(**over):
    want = dict(n=N, k=K, steps=STEPS, m=M, taylor_terms=TAYLOR, scaling=SCALING, state_transfer=0, n_seeds=SEEDS, dt=DT, total_time=TOTAL,
                has_amplitude=0, has_envelope=0, has_dwdt=0, has_d2wdt2=0, has_speed_up=0, has_bandpass=0, c_amplitude=0.0, c_envelope=0.0, c_dwdt=0.0,
                c_d2wdt2=0.0, c_speed_up=0.0, c_bandpass=0.0, band_lo=0, band_hi=0, n_forbidden=0, forbid_dressed=0, device=0, path=0, chunks=0, variant=0,
                plan_seeds=0, time_shards=0, time_rank=-1, gradient=0)
    want.update(over)
    return want


def _ens(off=ENS_OFF, amp=ENS_AMP, wt=ENS_W, dense=True):
    return dict(members=E, n_perturb=Q, P=np.stack([-1j * DT * p for p in PERT]) if dense else None, offsets=off, amp_scales=amp, weights=wt)


TR_S = dict(n_samples=NP, T=TR)
MAP_A = dict(n_terms=R, degree=D, poly=ALPHA, mix=None, fixed=None)
MAP_B = dict(n_terms=R, degree=D, poly=ALPHA, mix=MIX, fixed=FIXED)
FLEET_S = dict(devices=F, offsets=FL_OFF, amp_scales=FL_AMP)
SQRT_DT_C = np.sqrt(DT) * np.stack(COLLAPSE)
COSTS_S = dict(n_obs=L, O=COST_O[None], coeffs=np.array([0.3]), powers=np.array([2], dtype=np.int32))


def _sparse(n_ops, pert=False):
    """The COO arrays of the first n_ops diagonal operators, the perturbation -i dt P behind them."""
    diags = [-1j * DT * d for d in SP_DIAG[:n_ops]] + ([-1j * DT * d for d in SP_PERT_DIAG] if pert else [])
    idx = np.tile(np.arange(N, dtype=np.int32), len(diags))
    return dict(indptr=N * np.arange(len(diags) + 1, dtype=np.int64), row=idx, col=idx, val=np.concatenate(diags), vector_home=0)


def _dense(Hs=H[:K + 1]):
    return dict(Hs=Hs, U0=U0, V=V, W=W, maxA=MAXA, omg=None, fs=None, fc=None, Vs=None, out='handle')


def _lean(Hs=H[:K + 1]):
    return dict(Hs=Hs, U0=U0, V=V, W=W, maxA=MAXA, omg=None, out='handle')


SPARSE_ARGS = dict(V=V, W=W, maxA=MAXA, omg=None, fs=None, fc=None, out='handle')
ATTRS = dict(samples=None, devices=0, members=0, perturbations=0, row_layout=None, n_costs=0, terms=K, open_system=False)


def _ensemble(**more):
    return dict(dict(operators=PERT, offsets=ENS_OFF, amp_scales=ENS_AMP, weights=ENS_W), **more)


def _fleet(**more):
    return fleet_mod.Fleet(PERT, FL_OFF, FL_AMP, **more)


def _map(full=False):
    return cmap_mod.ControlMap(ALPHA, MIX, FIXED) if full else cmap_mod.ControlMap(ALPHA)


def _case(name, kw, symbol, expect, read, ens_kind, plan, **attrs):
    """kw: HipEngine's keywords (Hs: the dense operators, H[:K + 1] by default); expect: argument name -> None, an array, or a struct's fields;
    read: the read-back the flavour has; ens_kind: the library made an ensemble engine (member_scalars); plan: words of qoc_plan_describe."""
    return pytest.param(kw, symbol, expect, dict(ATTRS, **attrs), read, ens_kind, plan, id=name)


SPARSE_KW = dict(Hs=None, U0=None, state_transfer=True)
CASES = [
    _case('plain', {}, 'qoc_create', dict(_dense(), cfg=_cfg()), 'unitary', False, {}),
    _case('ensemble', dict(ensemble=_ensemble()), 'qoc_create_ensemble', dict(_dense(), cfg=_cfg(), ens=_ens()), 'unitary', True,
          {}, members=E, perturbations=Q),
    _case('transfer', dict(transfer=TR), 'qoc_create_shaped', dict(_dense(), cfg=_cfg(), ens=None, tr=TR_S), 'unitary', True,
          dict(samples=NP), samples=NP),
    _case('ensemble+transfer', dict(ensemble=_ensemble(), transfer=TR), 'qoc_create_shaped', dict(_dense(), cfg=_cfg(), ens=_ens(), tr=TR_S), 'unitary',
          True, dict(samples=NP), samples=NP, members=E, perturbations=Q),
    _case('map', dict(Hs=H, control_map=_map()), 'qoc_create_mapped', dict(_dense(H), cfg=_cfg(), ens=None, tr=None, map=MAP_A), 'unitary', True,
          dict(terms=R), terms=R),
    _case('map+ensemble+transfer', dict(Hs=H, control_map=_map(True), ensemble=_ensemble(), transfer=TR), 'qoc_create_mapped',
          dict(_dense(H), cfg=_cfg(), ens=_ens(), tr=TR_S, map=MAP_B), 'unitary', True, dict(samples=NP, terms=R),
          terms=R, samples=NP, members=E, perturbations=Q),
    _case('fleet', dict(fleet=_fleet()), 'qoc_create_fleet',
          dict(_dense(), cfg=_cfg(), ens=_ens(FL_OFF[0], FL_AMP[0], np.ones(E)), fleet=FLEET_S, tr=None, map=None), 'unitary', True,
          dict(devices=F), devices=F, members=E, perturbations=Q),
    _case('fleet+ensemble', dict(fleet=_fleet(), ensemble=_ensemble()), 'qoc_create_fleet',
          dict(_dense(), cfg=_cfg(), ens=_ens(), fleet=FLEET_S, tr=None, map=None), 'unitary', True, dict(devices=F),
          devices=F, members=E, perturbations=Q),
    _case('fleet-dict', dict(fleet=dict(amp_scales=FL_AMP1)), 'qoc_create_fleet',
          dict(_dense(), cfg=_cfg(), ens=None, fleet=dict(devices=F, offsets=None, amp_scales=FL_AMP1), tr=None, map=None), 'unitary', True,
          dict(devices=F), devices=F, members=1),
    _case('fleet-dict+ensemble', dict(fleet=dict(offsets=FL_OFF, amp_scales=FL_AMP), ensemble=_ensemble()), 'qoc_create_fleet',
          dict(_dense(), cfg=_cfg(), ens=_ens(), fleet=FLEET_S, tr=None, map=None), 'unitary', True, dict(devices=F),
          devices=F, members=E, perturbations=Q),
    _case('fleet+map+transfer', dict(Hs=H, fleet=_fleet(), control_map=_map(), transfer=TR), 'qoc_create_fleet',
          dict(_dense(H), cfg=_cfg(), ens=_ens(FL_OFF[0], FL_AMP[0], np.ones(E)), fleet=FLEET_S, tr=TR_S, map=MAP_A), 'unitary', True,
          dict(devices=F, samples=NP, terms=R), devices=F, members=E, perturbations=Q, samples=NP, terms=R),
    _case('collapse_ops', dict(collapse_ops=COLLAPSE), 'qoc_create_open', dict(_lean(), cfg=_cfg(), open=dict(n_collapse=NC, C=SQRT_DT_C)), 'density',
          False, {}, open_system=True),
    _case('collapse_ops-empty', dict(collapse_ops=[]), 'qoc_create_open', dict(_lean(), cfg=_cfg(), open=dict(n_collapse=0, C=None)), 'density', False,
          {}, open_system=True),
    _case('collapse_ops+costs', dict(collapse_ops=COLLAPSE, running_costs=COSTS), 'qoc_create_open_costs',
          dict(_lean(), cfg=_cfg(), decay=dict(n_collapse=NC, C=SQRT_DT_C, rate_scales=None), costs=COSTS_S, ens=None, fleet=None, tr=None, map=None),
          'density', True, dict(running_costs=L), open_system=True, n_costs=L),
    _case('ensemble-decay', dict(ensemble=_ensemble(collapse_ops=COLLAPSE, rate_scales=RATES_E)), 'qoc_create_open_fleet',
          dict(_lean(), cfg=_cfg(), decay=dict(n_collapse=NC, C=SQRT_DT_C, rate_scales=RATES_E[None]), ens=_ens(), fleet=None, tr=None, map=None),
          'density', True, {}, open_system=True, members=E, perturbations=Q),
    _case('fleet-decay', dict(fleet=_fleet(collapse_ops=COLLAPSE, rate_scales=RATES_F)), 'qoc_create_open_fleet',
          dict(_lean(), cfg=_cfg(), decay=dict(n_collapse=NC, C=SQRT_DT_C, rate_scales=RATES_F), ens=_ens(FL_OFF[0], FL_AMP[0], np.ones(E)),
               fleet=FLEET_S, tr=None, map=None), 'density', True, dict(devices=F), open_system=True, devices=F, members=E,
          perturbations=Q),
    _case('decay+costs', dict(ensemble=_ensemble(collapse_ops=COLLAPSE), running_costs=COSTS), 'qoc_create_open_costs',
          dict(_lean(), cfg=_cfg(), decay=dict(n_collapse=NC, C=SQRT_DT_C, rate_scales=np.ones((1, E, NC))), costs=COSTS_S, ens=_ens(), fleet=None,
               tr=None, map=None), 'density', True, dict(running_costs=L), open_system=True, members=E, perturbations=Q,
          n_costs=L),
    _case('decay+transfer+map', dict(Hs=H, ensemble=_ensemble(collapse_ops=COLLAPSE, rate_scales=RATES_E), transfer=TR, control_map=_map(True)),
          'qoc_create_open_fleet', dict(_lean(H), cfg=_cfg(), decay=dict(n_collapse=NC, C=SQRT_DT_C, rate_scales=RATES_E[None]), ens=_ens(), fleet=None,
                                        tr=TR_S, map=MAP_B), 'density', True, dict(samples=NP, terms=R), open_system=True,
          members=E, perturbations=Q, samples=NP, terms=R),
    _case('sparse', dict(SPARSE_KW, sparse_ops=SP_OPS[:K + 1]), 'qoc_create_sparse',
          dict(SPARSE_ARGS, cfg=_cfg(state_transfer=1), sparse=_sparse(K + 1)), 'inter', False, {}),
    _case('sparse+row_layout', dict(SPARSE_KW, sparse_ops=SP_OPS[:K + 1], row_layout='merged'), 'qoc_create_sparse_fleet',
          dict(SPARSE_ARGS, cfg=_cfg(state_transfer=1), sparse=_sparse(K + 1), plan=dict(row_layout=2), ens=None, fleet=None, tr=None, map=None), 'inter',
          True, dict(rows='merged'), row_layout=2, members=1),
    _case('sparse+ensemble', dict(SPARSE_KW, sparse_ops=SP_OPS[:K + 1], ensemble=_ensemble(operators=SP_PERT)), 'qoc_create_sparse_fleet',
          dict(SPARSE_ARGS, cfg=_cfg(state_transfer=1), sparse=_sparse(K + 1, True), plan=dict(row_layout=0), ens=_ens(dense=False), fleet=None, tr=None,
               map=None), 'inter', True, dict(rows=None), row_layout=0, members=E, perturbations=Q),
    _case('sparse+fleet+map', dict(SPARSE_KW, sparse_ops=SP_OPS, fleet=dict(amp_scales=FL_AMP1), control_map=_map()), 'qoc_create_sparse_fleet',
          dict(SPARSE_ARGS, cfg=_cfg(state_transfer=1), sparse=_sparse(R + 1), plan=dict(row_layout=0), ens=None,
               fleet=dict(devices=F, offsets=None, amp_scales=FL_AMP1), tr=None, map=MAP_A), 'inter', True,
          dict(devices=F, terms=R, rows=None), row_layout=0, members=1, devices=F, terms=R),
]


def _engine(kw, **more):
    kw = dict(dict(Hs=H[:K + 1], U0=U0), **kw)
    Hs, U0_ = kw.pop('Hs'), kw.pop('U0')
    return P.HipEngine(Hs, U0_, V, W, MAXA, DT, TOTAL, STEPS, TAYLOR, SCALING, reg_coeffs={}, n_seeds=SEEDS, **dict(kw, **more))


class Recorder(object):
    """Stands where the loaded library stands: every entry point succeeds and is written down.  A creation symbol's arguments are looked at
    by `inspect` while the call lasts: the binding keeps the arrays behind its structs alive across the call, not beyond it."""

    def __init__(self, inspect):
        self.calls, self.inspect = [], inspect

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            if name.startswith('qoc_create'):
                self.inspect(name, args)
            return 0
        return call


def _read(pointer, like):
    """What stands behind a recorded pointer, as many numbers as the expected array has."""
    like = np.ascontiguousarray(like)
    flat = like.view(np.float64).ravel() if np.iscomplexobj(like) else like.ravel()
    return np.ctypeslib.as_array(pointer, shape=(flat.size,)), flat


def _check_value(where, got, want):
    if want is None:
        assert not got, where + ' is not NULL'
    elif isinstance(want, np.ndarray):
        assert got, where + ' is NULL'
        seen, flat = _read(got, want)
        assert seen.dtype == flat.dtype, where
        np.testing.assert_array_equal(seen, flat, err_msg=where)
    else:
        assert got == want and type(got) is type(want), (where, got, want)


@pytest.mark.parametrize('kw, symbol, expect, attrs, read, ens_kind, plan', CASES)
def test_dispatch_against_a_recording_library(monkeypatch, kw, symbol, expect, attrs, read, ens_kind, plan):
    def inspect(called, args):
        assert called == symbol
        assert len(args) == len(ARGS[symbol]) and set(expect) == set(ARGS[symbol])
        for name, arg in zip(ARGS[symbol], args):
            want = expect[name]
            if name == 'out':
                assert isinstance(arg._obj, C.c_void_p)
            elif isinstance(want, dict):
                struct = arg._obj
                assert set(want) == {f for f, _ in struct._fields_} - {'reserved'}, name
                for field, value in want.items():
                    _check_value('%s.%s' % (name, field), getattr(struct, field), value)
            else:
                _check_value(name, arg, want)

    lib = Recorder(inspect)
    monkeypatch.setattr(P, 'load_library', lambda: lib)
    eng = _engine(kw)
    assert [name for name in lib.calls if name.startswith('qoc_create')] == [symbol]
    assert eng.plan == {}
    assert {key: getattr(eng, key) for key in attrs} == attrs
    assert (eng.n, eng.k, eng.m, eng.steps, eng.n_seeds) == (N, K, M, STEPS, SEEDS)


# ---- B. the order of the library's refusals -----------------------------------------------------------------------------------------------------

def _dp(a):
    return a.ctypes.data_as(P._DP)


class Inputs(object):
    """Valid arguments for every creation symbol, as ctypes structs over arrays this object keeps; a test spoils two of them."""

    def __init__(self, sparse=False):
        self.keep = keep = dict(H=H.copy(), U0=U0.copy(), V=V.copy(), W=W.copy(), maxA=MAXA.copy(), P=np.stack([-1j * DT * p for p in PERT]),
                                off=ENS_OFF.copy(), amp=ENS_AMP.copy(), wt=ENS_W.copy(), foff=FL_OFF.copy(), famp=FL_AMP.copy(), T=TR.copy(),
                                alpha=ALPHA.copy(), C=SQRT_DT_C.copy(), rates=np.ones((F, E, NC)), O=COST_O.copy(), coeffs=np.array([0.3]),
                                powers=np.array([2], dtype=np.int32))
        sp = _sparse(R + 1, True)
        keep.update(indptr=sp['indptr'], row=sp['row'].copy(), col=sp['col'].copy(), val=sp['val'].copy())
        self.cfg = P.QocConfig(n=N, k=K, steps=STEPS, m=M, taylor_terms=TAYLOR, scaling=SCALING, state_transfer=int(sparse), n_seeds=SEEDS, dt=DT,
                               total_time=TOTAL, time_rank=-1)
        self.ens = P.QocEnsemble(members=E, n_perturb=Q, P=None if sparse else _dp(keep['P'].view(np.float64)), offsets=_dp(keep['off']),
                                 amp_scales=_dp(keep['amp']), weights=_dp(keep['wt']))
        self.fleet = P.QocFleet(devices=F, offsets=_dp(keep['foff']), amp_scales=_dp(keep['famp']))
        self.tr = P.QocTransfer(n_samples=NP, T=_dp(keep['T']))
        self.map = P.QocControlMap(n_terms=R, degree=D, poly=_dp(keep['alpha']))
        self.open = P.QocOpen(n_collapse=NC, C=_dp(keep['C'].view(np.float64)))
        self.decay = P.QocDecay(n_collapse=NC, C=_dp(keep['C'].view(np.float64)), rate_scales=_dp(keep['rates']))
        self.costs = P.QocRunningCosts(n_obs=L, O=_dp(keep['O'].view(np.float64)), coeffs=_dp(keep['coeffs']), powers=keep['powers'].ctypes.data_as(P._IP))
        self.sparse = P.QocSparse(indptr=keep['indptr'].ctypes.data_as(C.POINTER(C.c_int64)), row=keep['row'].ctypes.data_as(P._IP),
                                  col=keep['col'].ctypes.data_as(P._IP), val=_dp(keep['val'].view(np.float64)), vector_home=0)
        self.plan = P.QocSparsePlan(row_layout=0)
        self.handle = C.c_void_p()
        self.Hs, self.U0, self.V, self.W = (_dp(keep[key].view(np.float64)) for key in ('H', 'U0', 'V', 'W'))
        self.maxA = _dp(keep['maxA'])
        self.omg = self.fs = self.fc = self.Vs = None

    def refusal(self, symbol):
        """Calls `symbol` of the real library and returns its message; nothing may have been created."""
        lib = P.load_library()
        args = []
        for name in ARGS[symbol]:
            value = self.handle if name == 'out' else getattr(self, name)
            args.append(C.byref(value) if isinstance(value, C.Structure) or name == 'out' else value)
        rc = getattr(lib, symbol)(*args)
        assert rc != 0 and not self.handle.value, 'the library accepted a spoiled input'
        return lib.qoc_last_error().decode()


def _spoil_amp(i):
    i.keep['famp'][1, 0, 1] = np.nan


def _zero_column(i):
    i.keep['T'][:, 1] = 0.0


def _bad_degree(i):
    i.map.degree = 0


def _negative_weight(i):
    i.keep['wt'][0] = -1.0


def _no_maxA(i):
    i.maxA = None


def _no_m(i):
    i.cfg.m = 0


def _d2_without_d1(i):
    i.cfg.has_d2wdt2 = 1


def _set(**fields):
    def spoil(i):
        for key, value in fields.items():
            obj, _, field = key.partition('__')
            setattr(getattr(i, obj), field, value) if field else setattr(i, obj, value)
    return spoil


def _negative_rate(i):
    i.keep['rates'][1, 0, 0] = -0.5


# (symbol, sparse inputs, the two defects -- the earlier stage first --, the message; recorded from the library before the funnel was one function)
PRECEDENCE = [
    # null arguments before the fleet; the fleet before the map, before the response matrix and before the members
    ('qoc_create_fleet', False, (_no_maxA, _spoil_amp), 'qoc_create_fleet: null argument'),
    ('qoc_create_fleet', False, (_spoil_amp, _bad_degree), 'qoc_create_fleet: amp_scales[1][0][1] is not finite'),
    ('qoc_create_fleet', False, (_spoil_amp, _zero_column), 'qoc_create_fleet: amp_scales[1][0][1] is not finite'),
    ('qoc_create_fleet', False, (_set(fleet__devices=3), _negative_weight), 'qoc_create_fleet: n_seeds = 2 is no multiple of devices = 3'),
    # the map before the response matrix and before the members
    ('qoc_create_mapped', False, (_bad_degree, _zero_column), 'qoc_create_mapped: degree = 0 (1 .. 8)'),
    ('qoc_create_mapped', False, (_bad_degree, _negative_weight), 'qoc_create_mapped: degree = 0 (1 .. 8)'),
    ('qoc_create_fleet', False, (_bad_degree, _zero_column), 'qoc_create_fleet: degree = 0 (1 .. 8)'),
    # the response matrix before the members
    ('qoc_create_shaped', False, (_zero_column, _negative_weight), 'qoc_create_shaped: column 1 of T is zero (the sample never reaches the pulse)'),
    ('qoc_create_shaped', False, (_set(tr__n_samples=0), _set(cfg__path=P.PATH_SMALL)), 'qoc_create_shaped: n_samples = 0 (>= 1)'),
    ('qoc_create_mapped', False, (_zero_column, _set(cfg__time_shards=2)), 'qoc_create_mapped: column 1 of T is zero (the sample never reaches the pulse)'),
    # the members before create_engine, which speaks as qoc_create
    ('qoc_create_ensemble', False, (_negative_weight, _no_m), 'qoc_create_ensemble: weight 0 is -1'),
    ('qoc_create_ensemble', False, (_set(cfg__path=P.PATH_SMALL), _set(U0=None)), 'qoc_create_ensemble: the workgroup-resident path (QOC_PATH_SMALL) runs its '
     "tail inside its launch, where the members' gradients cannot be reduced first"),
    ('qoc_create_ensemble', False, (_no_m, _no_m), 'qoc_create: n, k, steps, m, n_seeds must be >= 1'),
    ('qoc_create_shaped', False, (_negative_weight, _no_m), 'qoc_create_shaped: weight 0 is -1'),
    # an open entry point's own checks before the funnel, the funnel's stages behind them in their order
    ('qoc_create_open_fleet', False, (_negative_rate, _set(cfg__path=P.PATH_SMALL)),
     'qoc_create_open_fleet: an open system runs on QOC_PATH_LINDBLAD (or AUTO), not on path 5'),
    ('qoc_create_open_fleet', False, (_spoil_amp, _negative_rate), 'qoc_create_open_fleet: amp_scales[1][0][1] is not finite'),
    ('qoc_create_open_fleet', False, (_zero_column, _negative_rate), 'qoc_create_open_fleet: column 1 of T is zero (the sample never reaches the pulse)'),
    ('qoc_create_open_fleet', False, (_negative_rate, _set(U0=None)), 'qoc_create_open_fleet: rate_scales[1][0][0] is -0.5 (finite, >= 0)'),
    ('qoc_create_open_costs', False, (_set(costs__n_obs=17), _set(fleet__devices=3)), 'qoc_create_open_costs: n_obs = 17 (0 .. 16 running costs)'),
    ('qoc_create_open_costs', False, (_set(cfg__has_speed_up=1), _set(costs__n_obs=-1)),
     'qoc_create_open_costs: the speed_up regulariser is not available under a master equation'),
    ('qoc_create_open_costs', False, (_set(fleet__devices=3), _bad_degree), 'qoc_create_open_costs: n_seeds = 2 is no multiple of devices = 3'),
    ('qoc_create_open', False, (_set(cfg__has_speed_up=1), _d2_without_d1), 'qoc_create_open: the speed_up regulariser is not available under a master equation'),
    ('qoc_create_open', False, (_d2_without_d1, _d2_without_d1), 'qoc_create: d2wdt2 needs dwdt (reference: NameError new_weights)'),
    # a sparse entry point's own checks -- the map among them, which gives it the number of operators -- before the funnel
    ('qoc_create_sparse', True, (_set(sparse__vector_home=5), _d2_without_d1), 'qoc_create_sparse: vector_home = 5 (0 auto, 1 LDS, 2 global scratch)'),
    ('qoc_create_sparse_fleet', True, (_set(plan__row_layout=3), _bad_degree), 'qoc_create_sparse_fleet: row_layout = 3 (0 auto, 1 per operator, 2 merged)'),
    ('qoc_create_sparse_fleet', True, (_bad_degree, _spoil_amp), 'qoc_create_sparse_fleet: degree = 0 (1 .. 8)'),
    ('qoc_create_sparse_fleet', True, (_set(sparse__vector_home=5), _spoil_amp), 'qoc_create_sparse_fleet: vector_home = 5 (0 auto, 1 LDS, 2 global scratch)'),
    ('qoc_create_sparse_fleet', True, (_spoil_amp, _zero_column), 'qoc_create_sparse_fleet: amp_scales[1][0][1] is not finite'),
    ('qoc_create_sparse_fleet', True, (_zero_column, _negative_weight),
     'qoc_create_sparse_fleet: column 1 of T is zero (the sample never reaches the pulse)'),
]


@pytest.mark.parametrize('symbol, sparse, defects, message', PRECEDENCE, ids=['%s-%d' % (c[0][11:], i) for i, c in enumerate(PRECEDENCE)])
def test_the_earlier_stage_names_the_refusal(symbol, sparse, defects, message):
    inputs = Inputs(sparse)
    for spoil in defects:
        spoil(inputs)
    assert inputs.refusal(symbol) == message


def test_every_creation_symbol_but_the_plain_one_is_covered():
    assert {c[0] for c in PRECEDENCE} == set(ARGS) - {'qoc_create'}


# ---- C. the combinations of A, built for real -----------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_every_combination_builds_and_evaluates():
    for case in CASES:
        kw, symbol, _, attrs, read, ens_kind, plan = case.values
        eng = _engine(kw)
        try:
            assert {key: getattr(eng, key) for key in attrs} == attrs, case.id
            eng.set_base(0.3 * np.cos(np.arange(np.prod(eng._seed_shape()), dtype=np.float64)).reshape(eng._seed_shape()))
            r = eng.evaluate()
            assert r['loss'].shape == (SEEDS,) and np.all(np.isfinite(r['loss'])) and np.all(np.isfinite(r['grad'])), case.id
            if ens_kind:        # (an ensemble engine in the library, of one nominal member where there is no ensemble)
                plan = dict(plan, members=max(attrs['members'], 1), perturbations=attrs['perturbations'])
            for word in ('members', 'perturbations', 'devices', 'samples', 'terms', 'running_costs', 'rows'):
                if word in plan and plan[word] is None:
                    assert word in eng.plan, (case.id, word, eng.plan)             # (rows: what AUTO chose)
                elif word in plan:
                    assert eng.plan[word] == str(plan[word]), (case.id, word, eng.plan)
                else:
                    assert word not in eng.plan or (word == 'rows' and eng.plan['path'] == 'small'), (case.id, word, eng.plan)
            if ens_kind:
                ms = eng.member_scalars()
                assert ms['loss'].shape == ms['reg_state'].shape == (SEEDS, max(attrs['members'], 1)) and np.all(np.isfinite(ms['loss'])), case.id
            out = dict(unitary=eng.get_final_unitary, density=eng.get_final_density, inter=eng.get_inter_vecs)[read]()
            assert out.shape == dict(unitary=(SEEDS, N, N), density=(SEEDS, M, M, N, N), inter=(SEEDS, STEPS + 1, N, M))[read], case.id
            assert np.all(np.isfinite(out)), case.id
        finally:
            eng.close()
