"""Sparse state transfer without a GPU: the scipy.sparse reference of tests/sparse_reference.py against the dense oracle; the COO -> ELLPACK builder of
csrc/qoc_sparse_host.h through its stand-alone driver, compiled under the address and undefined-behaviour sanitizers; what Grape and HipEngine refuse on
the sparse route before the library is loaded; and the host side of a 14-spin chain (n = 16384) inside a memory bound no dense operator could keep."""
import functools
import os
import shutil
import subprocess
import tracemalloc

import numpy as np
import pytest
import scipy.sparse as sps

from oracle import grape_oracle as go
from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.core import sparse_parameters as spp
from quantum_optimal_control.core.system_parameters import SystemParameters
from quantum_optimal_control.helper_functions.synthetic_systems import xx_chain
from quantum_optimal_control.main_grape import grape as grape_mod
from tests import sparse_reference as sr
from tests.test_hip_parity import G_RTOL, S_RTOL, U_ATOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'quantum-optimal-control_amd', 'csrc')

# name: sparse_case arguments.  Every pulse regulariser, bare forbidden levels and speed_up, one and three state columns, a non-Hermitian problem
ORACLE_ROWS = {
    'n16_plain': dict(n=16, steps=6, k=2, m=1, T=8),
    'n16_m3_allreg': dict(n=16, steps=16, k=2, m=3, T=7, reg_coeffs=sr.ALL_REGS, forbidden=True),
    'n16_nonhermitian': dict(n=16, steps=5, k=3, m=2, T=9, kind='nonhermitian', forbidden=True),
    'n64_m1_allreg': dict(n=64, steps=16, k=2, m=1, T=10, reg_coeffs=sr.ALL_REGS, forbidden=True),
    'n64_m3': dict(n=64, steps=4, k=4, m=3, T=6),
    'n64_nonhermitian_row': dict(n=64, steps=5, k=2, m=1, T=8, kind='nonhermitian', reg_coeffs={'speed_up': 0.4}),
}


@pytest.mark.parametrize('name', list(ORACLE_ROWS))
def test_sparse_reference_against_the_dense_oracle(name):
    sp = sr.sparse_case(seed=list(ORACLE_ROWS).index(name), **ORACLE_ROWS[name])
    dense = sr.dense_oracle(sp)
    for base in sr.bases_of(sp, 2):
        o, r = go.evaluate(dense, base, want_inter=True), sr.evaluate(sp, base)
        for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale'):
            print('%s %s: sparse %.17g dense %.17g' % (name, key, r[key], o[key]))
            assert abs(r[key] - o[key]) <= S_RTOL * max(1.0, abs(o[key])), (name, key)
        gmax, gerr = np.max(np.abs(o['grad'])), np.max(np.abs(r['grad'] - o['grad']))
        print('%s: gradient error %.3e, largest entry %.3e' % (name, gerr, gmax))
        assert gerr <= G_RTOL * max(gmax, 1e-3)
        assert np.max(np.abs(r['inter_vecs'] - o['inter_vecs'])) <= U_ATOL * max(1.0, np.max(np.abs(o['inter_vecs'])))
    assert gmax > 1e-3                                   # (the gradient check is a relative one: it must see a gradient)


# ---- the ELLPACK builder, through its stand-alone driver under the sanitizers ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def builder_driver(tmp):
    cxx = shutil.which('g++') or shutil.which('clang++') or shutil.which('c++')
    if cxx is None:
        return None
    exe = os.path.join(tmp, 'sparse_host_main')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-I', CSRC,
                           os.path.join(ROOT, 'tests', 'sparse_host_main.cpp'), '-o', exe])
    return exe


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    exe = builder_driver(str(tmp_path_factory.mktemp('sparse_host')))
    if exe is None:
        pytest.skip('no C++ compiler found')
    return exe


def run_builder(driver, tmp_path, n, entries):
    path = os.path.join(str(tmp_path), 'op.txt')
    with open(path, 'w') as f:
        f.write('%d %d\n' % (n, len(entries)))
        for r, c, v in entries:
            f.write('%d %d %r %r\n' % (r, c, float(np.real(v)), float(np.imag(v))))
    out = subprocess.run([driver, path], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)   # (a sanitizer report ends it non-zero)
    lines = out.stdout.split('\n')
    if lines[0].startswith('error'):
        return lines[0]
    _, W, stored = lines[0].split()
    W, stored = int(W), int(stored)
    col = np.array([int(x) for x in lines[1:1 + W * n]], dtype=np.int64).reshape(W, n)
    val = np.array([complex(*map(float, x.split())) for x in lines[1 + W * n:1 + 2 * W * n]]).reshape(W, n)
    return W, stored, col, val


def expected_ell(n, entries):
    """The layout the header documents, built independently: per row the distinct columns ascending, duplicates summed in input order, padding = (row, 0)."""
    rows = [dict() for _ in range(n)]
    for r, c, v in entries:
        rows[r][c] = rows[r].get(c, 0j) + complex(v)
    W = max([len(x) for x in rows] + [0])
    col = np.tile(np.arange(n), (W, 1))
    val = np.zeros((W, n), dtype=np.complex128)
    for r in range(n):
        for s, c in enumerate(sorted(rows[r])):
            col[s, r], val[s, r] = c, rows[r][c]
    return W, sum(len(x) for x in rows), col, val


def _entries_of(kind):
    rng = np.random.default_rng(5)
    n = 7
    if kind == 'duplicates':
        return n, [(1, 3, 1 + 2j), (1, 3, 0.25 - 1j), (1, 3, 4.0), (0, 0, 1j), (6, 2, 2.0), (6, 2, -2.0)]      # (6, 2) sums to a stored zero
    if kind == 'unsorted':
        e = [(r, c, complex(rng.normal(), rng.normal())) for r in range(n) for c in rng.choice(n, 3, replace=False)]
        return n, [e[i] for i in rng.permutation(len(e))]
    if kind == 'explicit_zeros':
        return n, [(0, 1, 0.0), (0, 2, 0.0), (0, 3, 1.0), (5, 5, 0.0)]
    if kind == 'empty_row':
        return n, [(r, (r + 1) % n, 1.0 + r) for r in range(n) if r != 3]
    if kind == 'all_zero_operator':
        return n, []
    if kind == 'width_1':
        return n, [(r, r, -1j * r) for r in range(n)]
    if kind == 'width_n':
        return n, [(r, c, complex(r, c)) for r in range(n) for c in range(n)]
    raise KeyError(kind)


@pytest.mark.parametrize('kind', ['duplicates', 'unsorted', 'explicit_zeros', 'empty_row', 'all_zero_operator', 'width_1', 'width_n'])
def test_ell_builder(driver, tmp_path, kind):
    n, entries = _entries_of(kind)
    W, stored, col, val = run_builder(driver, tmp_path, n, entries)
    eW, estored, ecol, eval_ = expected_ell(n, entries)
    assert (W, stored) == (eW, estored)
    assert {'width_1': 1, 'width_n': n, 'all_zero_operator': 0, 'explicit_zeros': 3}.get(kind, W) == W
    assert np.array_equal(col, ecol) and np.array_equal(val, eval_)
    # the matrix the layout stands for is the matrix the entries stand for
    A = np.zeros((n, n), dtype=np.complex128)
    for s in range(W):
        A[np.arange(n), col[s]] += val[s]
    B = np.zeros((n, n), dtype=np.complex128)
    for r, c, v in entries:
        B[r, c] += v
    assert np.array_equal(A, B)


def test_ell_builder_refusals(driver, tmp_path):
    assert 'outside 0 .. 3' in run_builder(driver, tmp_path, 4, [(0, 0, 1.0), (4, 0, 1.0)])
    assert 'outside 0 .. 3' in run_builder(driver, tmp_path, 4, [(0, -1, 1.0)])
    assert 'not finite' in run_builder(driver, tmp_path, 4, [(0, 0, 1.0), (1, 2, complex(0, np.inf))])
    assert 'not finite' in run_builder(driver, tmp_path, 4, [(1, 2, complex(np.nan, 0))])
    assert 'not finite' in run_builder(driver, tmp_path, 4, [(1, 2, 1e308), (1, 2, 1e308)])                    # the duplicates' sum overflows
    out = subprocess.run([driver, 'overflow', '50000'], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
    assert out.startswith('error') and 'does not fit 32-bit' in out                                          # n * W = 2.5e9


# ---- Python: the route, its refusals (before the library is loaded), its memory ------------------------------------------------------------------

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
                state_transfer=True, save=False, show_plots=False, Taylor_terms=[6, 0])
    args.update(kw)
    return args


def test_grape_takes_the_sparse_route_and_refuses_before_the_library_loads(no_library):
    n = 16
    with pytest.raises(LibraryTouched):                                    # a valid call gets as far as the engine
        grape_mod.Grape(**chain_call())
    with pytest.raises(LibraryTouched):                                    # one sparse operator among dense ones is enough
        a = chain_call()
        a['H0'] = a['H0'].toarray()
        grape_mod.Grape(**a)
    with pytest.raises(ValueError, match='state_transfer=True'):
        grape_mod.Grape(**chain_call(state_transfer=False, U=np.eye(n)))
    refused = dict(robust={'operators': [], 'amp_scales': np.ones((1, 4)), 'weights': [1.0]}, transfer=np.eye(8), exact_gradient=True,
                   collapse_ops=[], time_comm=object(), dressed_info={'eigenvectors': None}, U0=np.eye(n), plan_seeds=4, _first_seed=1)
    for key, val in refused.items():
        with pytest.raises(ValueError, match='sparse'):
            grape_mod.Grape(**chain_call(**{key: val}))
    a = chain_call()
    pos = [a.pop(key) for key in ('H0', 'Hops', 'Hnames', 'U', 'total_time', 'steps', 'states_concerned_list')]
    with pytest.raises(ValueError, match='sparse'):
        grape_mod.GrapeSharded(*pos, restarts=2, **a)
    with pytest.raises(ValueError, match='sparse'):
        grape_mod.GrapeSharded(restarts=2, **chain_call())
    with pytest.raises(ValueError, match='sparse'):
        grape_mod.GrapeTimeSharded(*pos, comm=object(), **a)


def test_hip_engine_refuses_before_the_library_loads(no_library):
    sp = sr.sparse_case(8, 3)

    def make(**kw):
        args = dict(Hs=None, U0=None, V=sp.V, W=sp.W, maxA=sp.maxA, dt=sp.dt, total_time=sp.total_time, steps=sp.steps, taylor_terms=sp.exp_terms, scaling=0,
                    state_transfer=True, reg_coeffs={}, sparse_ops=sp.ops)
        args.update(kw)
        return hip_engine.HipEngine(**args)
    with pytest.raises(LibraryTouched):
        make()
    for kw in (dict(ensemble={}), dict(transfer=np.eye(3)), dict(exact_gradient=True), dict(collapse_ops=[]), dict(time_comm=object()), dict(time_shards=2),
               dict(Vs=np.eye(8)), dict(Hs=np.zeros((3, 8, 8))), dict(U0=np.eye(8)), dict(path=hip_engine.PATH_GENERIC), dict(state_transfer=False),
               dict(vector_home='registers')):
        with pytest.raises(ValueError):
            make(**kw)
    with pytest.raises(ValueError, match='must all be'):
        make(sparse_ops=sp.ops[:2] + [sps.csr_matrix((9, 9), dtype=complex)])


def test_dense_inputs_are_untouched():
    """Dense operators never take the route, whatever the reference's sparse flags say."""
    assert not spp.is_sparse_problem(np.eye(4), [np.eye(4)])
    assert spp.is_sparse_problem(np.eye(4), [sps.identity(4)]) and spp.is_sparse_problem(sps.identity(4), [])


def test_taylor_rule_is_the_dense_rule_on_the_stored_entries():
    """n >= 10: SparseSystemParameters picks the Taylor order the dense SystemParameters picks for the same chain."""
    H0, Hops, names, exc = xx_chain(6)
    for total_time, steps in ((10.0, 40), (30.0, 20)):
        np.random.seed(0)
        sparse = spp.SparseSystemParameters(H0, Hops, names, [exc(5)], total_time, steps, [exc(0)], 4 * np.ones(6), None, None, False, 1e-4, {}, False, None, None,
                                            True, True)
        np.random.seed(0)
        dense = SystemParameters(H0.toarray(), [h.toarray() for h in Hops], names, [exc(5)], np.identity(64), total_time, steps, [exc(0)], None, 4 * np.ones(6), None,
                                 None, False, 1e-4, True, False, {}, False, None, None, True, True, False, False, False)
        assert (sparse.exp_terms, sparse.scaling) == (dense.exp_terms, dense.scaling)
        assert np.array_equal(sparse.ops_weight_base, dense.ops_weight_base)
        for a, b in zip(sparse.engine_inputs()[0], dense.Hs_c):
            assert np.array_equal(a.toarray(), b)
        assert np.array_equal(sparse.engine_inputs()[2], dense.engine_inputs()[2]) and np.array_equal(sparse.engine_inputs()[3], dense.engine_inputs()[3])


def test_host_side_of_a_14_spin_chain_stays_sparse():
    """n = 16384: one densified operator is 4.3 GB; the whole host-side problem, up to the arrays handed to the C ABI, stays below 256 MB."""
    tracemalloc.start()
    try:
        H0, Hops, names, exc = xx_chain(14, control_sites=[0, 13])
        sys_para = spp.SparseSystemParameters(H0, Hops, names, [exc(13)], 8.0, 4, [exc(0)], [2.0, 2.0], None, None, False, 1e-4, {}, False, None, None, True, True)
        ops, U0, V, W, Vs = sys_para.engine_inputs()
        n, indptr, row, col, val = hip_engine.sparse_arrays(ops)
        peak = tracemalloc.get_traced_memory()[1]
    finally:
        tracemalloc.stop()
    print('n = %d, %d entries, peak %.1f MB, Taylor terms %d' % (n, indptr[-1], peak / 2 ** 20, sys_para.exp_terms))
    assert n == 16384 and U0 is None and Vs is None and V.shape == (16384, 1)
    assert indptr[-1] == sum(o.nnz for o in ops) and len(row) == len(col) == len(val) == indptr[-1]
    assert peak < 256 * 2 ** 20


def test_dump_inputs_stores_sparse_operators_as_csr_arrays(monkeypatch):
    from quantum_optimal_control.helper_functions import data_management

    class FakeLog(object):
        stored = {}

        def __init__(self, path):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def add(self, key, data):
            FakeLog.stored[key] = np.array(data)

        def create_group(self, name):
            return self

        def create_dataset(self, key, data):
            FakeLog.stored[key] = np.array(data)
    monkeypatch.setattr(data_management, 'H5File', FakeLog)
    H0, Hops, names, exc = xx_chain(5)
    grape_mod._dump_inputs('log.h5', H0, Hops, names, [exc(4)], 4.0, 8, [exc(0)], True, False, False, False, None, None, 'Adam', {'rate': 0.01}, {}, None)
    got = FakeLog.stored
    for name, op in [('H0', H0)] + [('Hops_%d' % i, h) for i, h in enumerate(Hops)]:
        back = sps.csr_matrix((got[name + '_data'], got[name + '_indices'], got[name + '_indptr']), shape=(32, 32))
        assert (back != op).nnz == 0
    assert 'H0' not in got and 'Hops' not in got and all(v.size < 32 * 32 for v in got.values())
