"""Sparse ensembles without a GPU: the composed sparse reference of tests/sparse_ensemble_reference.py against the dense composed
references; the merged-row builder of csrc/qoc_sparse_host.h through its stand-alone driver under the address and undefined-behaviour sanitizers; what
Grape and HipEngine still refuse on the sparse route before the library is loaded; the host side of a 14-spin ensemble inside the memory bound of
tests/test_sparse.py; and the Taylor rule over members."""
import functools
import os
import shutil
import subprocess
import tracemalloc

import numpy as np
import pytest
import scipy.sparse as sps

from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.core import sparse_parameters as spp
from quantum_optimal_control.helper_functions import control_map as cmap
from quantum_optimal_control.helper_functions import fleet as fl_mod
from quantum_optimal_control.helper_functions import robust as rb
from quantum_optimal_control.helper_functions.synthetic_systems import xx_bonds, xx_chain
from quantum_optimal_control.main_grape import grape as grape_mod
from tests import control_map_reference as ref
from tests import fleet_reference as fr
from tests import sparse_ensemble_reference as ser
from tests.test_hip_parity import G_RTOL, S_RTOL, U_ATOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'quantum-optimal-control_amd', 'csrc')


# ---- the sparse composed reference against the dense composed references, n = 16 -----------------------------------------------------------------

def dense_problem(k=2, r=None, steps=6):
    """A dense state-transfer problem of n = 16 (a forbidden level, speed_up and dwdt) and the same problem with every operator as CSR."""
    c = fr.problem('state', n=16, k=k, r=r, steps=steps, m=2)
    p = ser.Problem(sps.csr_matrix(c['H0']), [sps.csr_matrix(h) for h in c['Hops']], np.stack(c['states_concerned_list'], axis=1), np.stack(c['U'], axis=1),
                    c['total_time'], c['steps'], c['Taylor_terms'][0], c['maxA'], c['reg_coeffs'])
    return c, p


def sparse_members(ens):
    return dict(ens, operators=[sps.csr_matrix(op) for op in ens['operators']])


def close(name, got, want):
    for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale'):
        print('%s %s: sparse %.17g dense %.17g' % (name, key, got[key], want[key]))
        assert abs(got[key] - want[key]) <= S_RTOL * max(1.0, abs(want[key])), (name, key)
    gmax, gerr = np.max(np.abs(want['grad'])), np.max(np.abs(got['grad'] - want['grad']))
    print('%s: gradient error %.3e, largest entry %.3e' % (name, gerr, gmax))
    assert gmax > 1e-3 and gerr <= G_RTOL * max(gmax, 1e-3)
    assert np.max(np.abs(got['member_loss'] - want['member_loss'])) <= S_RTOL
    assert np.max(np.abs(got['inter_vecs'] - want['inter_vecs'])) <= U_ATOL * max(1.0, np.max(np.abs(want['inter_vecs'])))
    assert np.max(np.abs(got['coefficients'] - want['coefficients'])) <= U_ATOL * max(1.0, np.max(np.abs(want['coefficients'])))


@pytest.mark.parametrize('name', ['ensemble', 'risk', 'line', 'map', 'fleet'])
def test_sparse_composed_reference_against_the_dense_ones(name):
    k, r = (2, 3) if name == 'map' else (2, 2)
    c, p = dense_problem(k=k, r=r)
    steps = c['steps']
    cm = ref.make_map(k, r, 3, steps, mix=True, fixed=True) if name == 'map' else None
    dense_cm = cm if cm is not None else cmap.validate(cmap.identity(k), k=k, r=k, steps=steps)
    T = None
    if name == 'line':
        rng = np.random.default_rng(4)
        T = np.abs(rng.normal(size=(steps, 4))) + 0.1
    x = ref.variables(k, steps if T is None else T.shape[1], 1)[0]
    if name == 'fleet':
        fl = fr.make_fleet(c, 3, 2, 2)
        sparse_fl = fl_mod.validate(fl_mod.Fleet([sps.csr_matrix(op) for op in fl.operators], fl.offsets, fl.amp_scales, weights=fl.weights), 16, k, sparse=True)
        assert all(sps.issparse(op) for op in sparse_fl.operators)
        values = []
        for f in range(3):
            got, want = ser.evaluate_fleet(p, sparse_fl, f, x), fr.evaluate(c, dense_cm, fl, f, x)
            close('fleet device %d' % f, got, want)
            values.append(want['loss'])
        assert fr.swapped_apart(values)
        return
    ens = ref.ensemble(c, 3, 2)
    beta = 4.0 if name == 'risk' else 0.0
    got = ser.evaluate(p, sparse_members(ens), x, cm=cm, T=T, beta=beta)
    want = ref.evaluate(c, dense_cm, ens, x, T=T, beta=beta)
    close(name, got, want)
    if name == 'risk':
        assert np.max(np.abs(got['weights'] - want['weights'])) <= S_RTOL and np.max(np.abs(got['weights'] - ens['weights'])) > 1e-3


# ---- the merged-row builder, through its stand-alone driver under the sanitizers -----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def merge_driver(tmp):
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    if cxx is None:
        return None
    exe = os.path.join(tmp, 'sparse_merge_main')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', CSRC,
                           os.path.join(ROOT, 'tests', 'sparse_merge_main.cpp'), '-o', exe])
    return exe


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    exe = merge_driver(str(tmp_path_factory.mktemp('sparse_merge')))
    if exe is None:
        pytest.skip('no C++ compiler found')
    return exe


def run_merge(driver, tmp_path, n, operators):
    """operators: a list of entry lists [(row, col, value), ...].  Returns the driver's error line, or (Wm, len, col, op, val)."""
    path = os.path.join(str(tmp_path), 'ops.txt')
    with open(path, 'w') as f:
        f.write('%d %d\n' % (n, len(operators)))
        for entries in operators:
            f.write('%d\n' % len(entries))
            for r, c, v in entries:
                f.write('%d %d %r %r\n' % (r, c, float(np.real(v)), float(np.imag(v))))
    out = subprocess.run([driver, path], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)   # (a sanitizer report ends it non-zero)
    lines = out.stdout.split('\n')
    if lines[0].startswith('error'):
        return lines[0]
    Wm = int(lines[0].split()[1])
    length = np.array([int(x) for x in lines[1:1 + n]], dtype=np.int64)
    rows = [x.split() for x in lines[1 + n:1 + n + Wm * n]]
    col = np.array([int(x[0]) for x in rows], dtype=np.int64).reshape(Wm, n)
    op = np.array([int(x[1]) for x in rows], dtype=np.int64).reshape(Wm, n)
    val = np.array([complex(float(x[2]), float(x[3])) for x in rows]).reshape(Wm, n)
    return Wm, length, col, op, val


def expected_merge(n, operators):
    """The layout the header documents, restated: per row the entries of operator 0, then 1, ..: distinct columns ascending, duplicates summed in input
    order, explicit zeros kept, nothing for padding."""
    rows = [[] for _ in range(n)]
    for j, entries in enumerate(operators):
        per = [dict() for _ in range(n)]
        for r, c, v in entries:
            per[r][c] = per[r].get(c, 0j) + complex(v)
        for r in range(n):
            rows[r] += [(c, j, per[r][c]) for c in sorted(per[r])]
    return max([len(x) for x in rows] + [0]), rows


def check_merge(driver, tmp_path, n, operators):
    Wm, length, col, op, val = run_merge(driver, tmp_path, n, operators)
    eWm, rows = expected_merge(n, operators)
    assert Wm == eWm and np.array_equal(length, [len(x) for x in rows])
    for r in range(n):
        got = [(int(col[s, r]), int(op[s, r]), complex(val[s, r])) for s in range(length[r])]
        assert got == rows[r], r
        # behind len[r]: the row's own index under operator 0, value 0 (never read)
        assert all((col[s, r], op[s, r], val[s, r]) == (r, 0, 0) for s in range(length[r], Wm))
    return Wm, length


MERGE_CASES = {
    'empty_rows': (6, [[(0, 1, 1.0), (5, 0, 2j)], [(0, 0, 1j), (5, 5, 1.0)]]),                                   # rows 1 .. 4 have no entry in any operator
    'width_0_operator': (5, [[(r, r, 1.0 + r) for r in range(5)], [], [(r, (r + 1) % 5, 1j) for r in range(5)]]),
    'operator_missing_from_rows': (6, [[(r, r, 1.0) for r in range(6)], [(0, 3, 2.0), (0, 1, 1.0), (4, 4, 1j)], [(5, 0, 3.0)]]),
    'duplicates_and_zeros': (4, [[(1, 3, 1 + 2j), (1, 3, 0.25 - 1j), (2, 0, 0.0)], [(1, 3, 4.0), (3, 2, 2.0), (3, 2, -2.0), (0, 0, 0.0)]]),
    'no_operator': (3, []),
    'all_empty': (3, [[], []]),
}


@pytest.mark.parametrize('kind', list(MERGE_CASES))
def test_merged_builder(driver, tmp_path, kind):
    n, operators = MERGE_CASES[kind]
    Wm, length = check_merge(driver, tmp_path, n, operators)
    if kind == 'empty_rows':
        assert list(length) == [2, 0, 0, 0, 0, 2]
    if kind == 'duplicates_and_zeros':
        assert list(length) == [1, 2, 1, 1]                   # the stored zero of (2, 0), the summed-to-zero (3, 2) and the explicit (0, 0) stay
    if kind in ('no_operator', 'all_empty'):
        assert Wm == 0


def test_merged_builder_255_operators_and_its_limits(driver, tmp_path):
    rng = np.random.default_rng(3)
    n = 9
    operators = [[(int(r), int(c), complex(rng.normal(), rng.normal())) for r, c in zip(rng.integers(0, n, 2), rng.integers(0, n, 2))] for _ in range(255)]
    Wm, length = check_merge(driver, tmp_path, n, operators)
    assert Wm >= 255 * 2 // n
    assert 'at most 255' in run_merge(driver, tmp_path, n, operators + [[(0, 0, 1.0)]])
    out = subprocess.run([driver, 'roundtrip'], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout.split('\n')
    assert out[0].split() == [str(2 ** 24 - 1), '254'] and out[1].split() == ['0', '0']
    out = subprocess.run([driver, 'bign'], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
    assert out.startswith('error') and '24 bits' in out


# ---- Python: what stays refused on the sparse route, before the library is loaded ----------------------------------------------------------------

class LibraryTouched(Exception):
    pass


@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise LibraryTouched()
    monkeypatch.setattr(hip_engine, 'load_library', boom)


def chain_call(spins=4, **kw):
    H0, Hops, names, exc = xx_chain(spins)
    args = dict(H0=H0, Hops=Hops, Hnames=names, U=[exc(spins - 1)], total_time=4.0, steps=8, states_concerned_list=[exc(0)], reg_coeffs={},
                state_transfer=True, save=False, show_plots=False)
    args.update(kw)
    return args


def bond_ensemble(spins, E=3, spread=0.05, sparse=True, **kw):
    bonds = xx_bonds(spins)
    rng = np.random.default_rng(11)
    off = np.vstack([np.zeros(spins - 1), rng.uniform(-spread, spread, size=(E - 1, spins - 1))])
    return dict(operators=bonds if sparse else [b.toarray() for b in bonds], offsets=off, **kw)


def test_grape_keeps_its_refusals_on_the_sparse_route(no_library):
    """Grape() does not take the extensions on scipy.sparse Hamiltonians yet (the engine underneath does: HipEngine(sparse_ops=, ensemble=, ...)); what it
    refuses, it refuses before the library is loaded, and the helpers refuse decay and wrong-shaped tables on the sparse route themselves."""
    spins, k = 4, 4
    fleet = fl_mod.devices(xx_bonds(spins), offsets=np.random.default_rng(2).uniform(-0.05, 0.05, size=(3, spins - 1)), k=k)
    with pytest.raises(LibraryTouched):                                    # a plain sparse call gets as far as the engine
        grape_mod.Grape(**chain_call(Taylor_terms=[6, 0]))
    for kw in (dict(robust=bond_ensemble(spins)), dict(fleet=fleet), dict(transfer=np.eye(8)), dict(control_map=cmap.identity(k)), dict(exact_gradient=True),
               dict(collapse_ops=[]), dict(time_comm=object()), dict(dressed_info={'eigenvectors': None}), dict(U0=np.eye(16))):
        with pytest.raises(ValueError, match='sparse'):
            grape_mod.Grape(**chain_call(Taylor_terms=[6, 0], **kw))
    for decay in (dict(collapse_ops=[np.eye(16)]), dict(collapse_ops=[np.eye(16)], rate_scales=np.ones((3, 1)))):
        with pytest.raises(ValueError, match='sparse'):
            rb.validate(bond_ensemble(spins, **decay), 16, k, sparse=True)
    with pytest.raises(ValueError, match='sparse'):
        fl_mod.validate(fl_mod.Fleet(xx_bonds(spins), np.zeros((2, 1, 3)), np.ones((2, 1, k)), collapse_ops=[np.eye(16)]), 16, k, sparse=True)
    with pytest.raises(ValueError, match='offsets have shape'):            # a wrong-shaped table
        rb.validate(dict(operators=xx_bonds(spins), offsets=np.zeros((3, 2))), 16, k, sparse=True)
    with pytest.raises(ValueError, match='amp_scales have shape'):
        rb.validate(bond_ensemble(spins, amp_scales=np.ones((3, k + 1))), 16, k, sparse=True)
    with pytest.raises(ValueError, match='not Hermitian'):
        rb.validate(dict(operators=[sps.csr_matrix(([1.0], ([0], [1])), shape=(16, 16))], offsets=np.zeros((1, 1))), 16, k, sparse=True)


def test_hip_engine_sparse_ensemble_refusals(no_library):
    from tests import sparse_reference as sr
    sp = sr.sparse_case(8, 3)
    ens = dict(operators=[sr.random_sparse(np.random.default_rng(1), 8)], offsets=np.zeros((2, 1)), amp_scales=np.ones((2, sp.k)), weights=np.ones(2) / 2)

    def make(**kw):
        args = dict(Hs=None, U0=None, V=sp.V, W=sp.W, maxA=sp.maxA, dt=sp.dt, total_time=sp.total_time, steps=sp.steps, taylor_terms=sp.exp_terms, scaling=0,
                    state_transfer=True, reg_coeffs={}, sparse_ops=sp.ops)
        args.update(kw)
        return hip_engine.HipEngine(**args)
    for kw in (dict(ensemble=ens), dict(row_layout=2), dict(row_layout='merged', ensemble=ens), dict(control_map=cmap.identity(sp.k)),
               dict(fleet=dict(amp_scales=np.ones((2, 1, sp.k))), n_seeds=2)):
        with pytest.raises(LibraryTouched):
            make(**kw)
    for kw in (dict(ensemble=dict(ens, collapse_ops=[np.eye(8)])), dict(ensemble=dict(ens, rate_scales=np.ones((2, 1)))), dict(ensemble=ens, exact_gradient=True),
               dict(fleet=dict(amp_scales=np.ones((2, 1, sp.k)), collapse_ops=[np.eye(8)])), dict(row_layout=3), dict(row_layout='rows'), dict(transfer=np.eye(3)), dict(ensemble=ens, transfer=np.eye(3)),
               dict(ensemble=ens, collapse_ops=[]), dict(ensemble=ens, Vs=np.eye(8)), dict(ensemble=ens, time_shards=2)):
        with pytest.raises(ValueError):
            make(**kw)
    with pytest.raises(ValueError, match='row_layout'):                    # a dense engine has no rows to lay out
        make(sparse_ops=None, Hs=np.zeros((3, 8, 8)), U0=np.eye(8), row_layout=1)


def test_perturbation_operators_follow_the_route():
    """The sparse route keeps scipy.sparse perturbations sparse and converts dense ones to CSR; a dense route densifies sparse ones."""
    bonds = xx_bonds(4)
    for given in (bonds, [b.toarray() for b in bonds]):
        ens = rb.validate(dict(operators=given, offsets=np.zeros((2, 3))), 16, 4, sparse=True)
        assert all(sps.issparse(op) and op.dtype == np.complex128 for op in ens['operators'])
        out = hip_engine.sparse_perturbations(ens, 0.5)
        assert all(sps.issparse(op) for op in out) and (out[1] != -0.5j * bonds[1]).nnz == 0
        dense = rb.validate(dict(operators=given, offsets=np.zeros((2, 3))), 16, 4)
        assert all(isinstance(op, np.ndarray) and op.shape == (16, 16) for op in dense['operators'])
        P = hip_engine.ensemble_arrays(dict(dense, operators=given), 16, 4, 0.5)[0]
        assert P.shape == (3, 16, 16) and np.array_equal(P[2], -0.5j * bonds[2].toarray())
    grid = rb.ensemble_grid(bonds[:1], offsets=[[-0.05], [0.0], [0.05]], k=4)
    assert sps.issparse(grid['operators'][0]) and grid['offsets'][0, 0] == 0.0
    around = fl_mod.around(bonds[:1], offsets=[[0.1], [-0.1]], robust=grid, k=4)
    assert sps.issparse(around.operators[0]) and around.offsets.shape == (2, 3, 1)
    # the builders choose no route: sparse perturbations with decay build, a dense route densifies them and keeps the decay, the sparse route refuses it
    decay = rb.ensemble_grid(bonds[:1], offsets=[[0.0], [0.05]], k=4, collapse_ops=[np.eye(16)], rate_scales=[1.0, 2.0])
    assert sps.issparse(decay['operators'][0]) and decay['rate_scales'].shape == (4, 1)
    dense = rb.validate(decay, 16, 4)
    assert isinstance(dense['operators'][0], np.ndarray) and 'collapse_ops' in dense
    with pytest.raises(ValueError, match='sparse'):
        rb.validate(decay, 16, 4, sparse=True)
    fl = fl_mod.devices(bonds[:1], offsets=[[0.1], [-0.1]], k=4, collapse_ops=[np.eye(16)])
    assert sps.issparse(fl.operators[0]) and fl.has_decay
    assert isinstance(fl_mod.validate(fl, 16, 4).operators[0], np.ndarray)
    mixed = rb.ensemble_grid([bonds[0], bonds[1].toarray()], offsets=[[0.0, 0.0], [0.05, -0.05]], k=4)
    assert sps.issparse(mixed['operators'][0]) and isinstance(mixed['operators'][1], np.ndarray)


# ---- host memory and the Taylor rule ---------------------------------------------------------------------------------------------------------------

def test_host_side_of_a_14_spin_ensemble_stays_sparse():
    """n = 16384 with q = 13 bond perturbations: one densified operator is 4.3 GB; the host side of the ensemble, up to the arrays handed to the C ABI,
    stays below the 256 MB of tests/test_sparse.py."""
    tracemalloc.start()
    try:
        spins = 14
        H0, Hops, names, exc = xx_chain(spins, control_sites=[0, 13])
        ens = rb.validate(bond_ensemble(spins, E=3), 16384, 2, sparse=True)
        sys_para = spp.SparseSystemParameters(H0, Hops, names, [exc(13)], 8.0, 4, [exc(0)], [2.0, 2.0], None, None, False, 1e-4, {}, False, None, None, True, True,
                                              members=[ens])
        ops, U0, V, W, Vs = sys_para.engine_inputs()
        n, indptr, row, col, val = hip_engine.sparse_arrays(list(ops) + hip_engine.sparse_perturbations(ens, sys_para.dt))
        P, off, amp, wt = hip_engine.ensemble_arrays(ens, n, 2, sys_para.dt, dense=False)
        peak = tracemalloc.get_traced_memory()[1]
    finally:
        tracemalloc.stop()
    print('n = %d, %d operators, %d entries, peak %.1f MB, Taylor terms %d' % (n, len(indptr) - 1, indptr[-1], peak / 2 ** 20, sys_para.exp_terms))
    assert n == 16384 and P is None and len(indptr) == 1 + 3 + 13 and off.shape == (3, 13) and amp.shape == (3, 2)
    assert all(sps.issparse(op) for op in ens['operators'])
    assert peak < 256 * 2 ** 20


def test_taylor_rule_over_the_members():
    """The largest order any member's stored entries ask for wins: a member whose offset strengthens the couplings raises it, the nominal member
    alone reproduces the plain rule, and no dense array is formed."""
    H0, Hops, names, exc = xx_chain(6)
    args = (H0, Hops, names, [exc(5)], 2.0, 20, [exc(0)], 0.5 * np.ones(6), None, None, False, 1e-4, {}, False, None, None, True, True)
    np.random.seed(0)
    plain = spp.SparseSystemParameters(*args)
    bonds = xx_bonds(6)
    nominal = rb.validate(dict(operators=bonds, offsets=np.zeros((1, 5))), 64, 6, sparse=True)
    strong = rb.validate(dict(operators=bonds, offsets=np.vstack([np.zeros(5), 3.0 * np.ones(5)])), 64, 6, sparse=True)
    scaled = rb.validate(dict(operators=[], amp_scales=[np.ones(6), 4.0 * np.ones(6)]), 64, 6, sparse=True)
    orders = {}
    for name, ens in (('nominal', nominal), ('strong', strong), ('scaled', scaled)):
        np.random.seed(0)
        orders[name] = spp.SparseSystemParameters(*args, members=[ens]).exp_terms
    print('plain %d, members: %r' % (plain.exp_terms, orders))
    assert orders['nominal'] == plain.exp_terms
    assert orders['strong'] > plain.exp_terms and orders['scaled'] > plain.exp_terms
    # the rule by hand for the strong member: |H0| + 3 |sum of bonds| = 4 |H0| on the couplings' entries, past the diagonal's 1.5
    dt = 2.0 / 20
    x = dt * spp.member_max_abs_entry(H0, Hops, 0.5 * np.ones(6), bonds, 3.0 * np.ones(5))
    assert orders['strong'] == spp.choose_taylor_terms(x, 20, 1e-4)
    assert abs(spp.member_max_abs_entry(H0, Hops, 0.5 * np.ones(6)) - spp.max_abs_entry(H0, Hops, 0.5 * np.ones(6))) == 0.0
    # a fleet: the largest over its devices; a map: the coefficient bounds stand where maxA stands
    fleet = [nominal, strong]
    assert spp.choose_taylor_members(H0, Hops, 0.5 * np.ones(6), fleet, dt, 20, 1e-4) == orders['strong']
    double = cmap.validate(cmap.linear(2.0 * np.eye(6)), k=6, r=6, steps=20)       # (no constructor takes a map on this route: the rule alone)
    assert spp.choose_taylor_members(H0, Hops, 0.5 * np.ones(6), [None], dt, 20, 1e-4, control_map=double) == \
        spp.choose_taylor_terms(dt * spp.max_abs_entry(H0, Hops, 1.0 * np.ones(6)), 20, 1e-4)
