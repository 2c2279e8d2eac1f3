"""Sparse state transfer on the GPU (HipEngine(sparse_ops=...), qoc_create_sparse, csrc/qoc_sparse.h): parity with the dense oracle on the smallest shapes at
which each code path can go wrong, for one and three control sets; both vector homes and the boundary of the rule that picks one; a 14-spin chain
(n = 16384) against the sparse reference of tests/sparse_reference.py; determinism; the device Adam and L-BFGS loops against the same loops on a dense
engine; what the C ABI refuses; create / destroy cycles; Grape() with sparse and with dense inputs of one problem; the example."""
import contextlib
import ctypes as C
import functools
import io
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sps

from oracle import grape_oracle as go
from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.helper_functions.synthetic_systems import xx_chain
from tests import sparse_reference as sr
from tests.test_adam_tail import LOOP_ATOL, _choose_target
from tests.test_hip_parity import G_RTOL, S_RTOL, U_ATOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'examples'))
P = hip_engine

# name: sparse_case arguments (random rows: 1 to 6 entries per row before the Hermitian part is taken)
ROWS = {
    'n1': dict(n=1, steps=3),
    'n2': dict(n=2, steps=4),
    'n5': dict(n=5, steps=6),
    'n33': dict(n=33, steps=5),
    'n256': dict(n=256, steps=3),                                       # the last size on 256 threads
    'n257': dict(n=257, steps=4),                                       # more rows than a 256-thread workgroup: the first size on 1024
    'n1025': dict(n=1025, steps=3),                                     # more rows than 1024 threads
    'dense_n8': dict(n=8, steps=4, kind='dense'),                       # width n
    'diagonal': dict(n=20, steps=4, kind='diagonal'),                   # width 1
    'zero_control': dict(n=20, steps=4, kind='zero_control'),           # width 0
    'disjoint': dict(n=20, steps=4, kind='disjoint'),
    'T1': dict(n=12, steps=4, T=1),                                     # the identity map
    'T2': dict(n=12, steps=4, T=2),
    'T20': dict(n=12, steps=4, T=20),
    'T60': dict(n=12, steps=3, T=60),
    'k1': dict(n=12, steps=5, k=1),
    'k8': dict(n=12, steps=3, k=8),
    'm3': dict(n=12, steps=5, m=3),
    'allreg': dict(n=24, steps=16, m=2, reg_coeffs=sr.ALL_REGS, forbidden=True),
    'nonhermitian': dict(n=24, steps=5, m=2, kind='nonhermitian', forbidden=True),
}


@functools.lru_cache(maxsize=None)
def system(name):
    return sr.sparse_case(seed=list(ROWS).index(name), **ROWS[name])


@functools.lru_cache(maxsize=None)
def reference(name):
    """The dense oracle at the row's three bases: computed once, shared by every test that needs it."""
    sp = system(name)
    dense = sr.dense_oracle(sp)
    return [go.evaluate(dense, b, want_inter=True) for b in sr.bases_of(sp)]


def make_engine(sp, n_seeds=1, **kw):
    return P.HipEngine(None, None, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, 0, state_transfer=True, reg_coeffs=sp.reg_coeffs,
                       one_minus_gauss=sp.one_minus_gauss if 'envelope' in sp.reg_coeffs else None, n_seeds=n_seeds, sparse_ops=sp.ops, **kw)


def make_dense_engine(sp, n_seeds=1, **kw):
    Hs = np.stack([o.toarray() for o in sp.ops])
    return P.HipEngine(Hs, None, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, 0, state_transfer=True, reg_coeffs=sp.reg_coeffs,
                       one_minus_gauss=sp.one_minus_gauss if 'envelope' in sp.reg_coeffs else None, n_seeds=n_seeds, **kw)


def assert_eval(tag, r, refs, inter=None):
    for g, o in enumerate(refs):
        for key in ('loss', 'reg_loss', 'unitary_scale', 'grad_squared'):
            print('%s %s[%d]: engine %.17g reference %.17g' % (tag, key, g, r[key][g], o[key]))
            assert abs(r[key][g] - o[key]) <= S_RTOL * max(1.0, abs(o[key])), (tag, key, g, r[key][g], o[key])
        gmax, err = float(np.max(np.abs(o['grad']))), float(np.max(np.abs(r['grad'][g] - o['grad'])))
        print('%s grad[%d]: max error %.3e, largest entry %.3e' % (tag, g, err, gmax))
        assert err <= G_RTOL * max(gmax, 1e-3), (tag, g, err, gmax)
        if inter is not None:
            ierr, imax = float(np.max(np.abs(inter[g] - o['inter_vecs']))), float(np.max(np.abs(o['inter_vecs'])))
            print('%s inter_vecs[%d]: max error %.3e, largest entry %.3e' % (tag, g, ierr, imax))
            assert ierr <= U_ATOL * max(1.0, imax), (tag, g, ierr)


# ---- 1. parity with the dense oracle ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('G', [1, 3])
@pytest.mark.parametrize('name', list(ROWS))
def test_parity_with_the_dense_oracle(name, G):
    sp, refs = system(name), reference(name)
    bases = np.stack(sr.bases_of(sp)[:G] if G > 1 else sr.bases_of(sp)[1:2])       # (one control set: a perturbed base)
    refs = refs[:G] if G > 1 else refs[1:2]
    eng = make_engine(sp, G)
    try:
        plan = eng.plan
        assert eng.path == P.PATH_SPARSE and (plan['path'], plan['vector_home'], plan['gradient']) == ('sparse', 'lds', 'first_order'), plan
        widths = [int(w) for w in plan['ell'].split(',')]
        assert widths == [int(np.max(np.diff(o.indptr))) if o.nnz else 0 for o in sp.ops], plan
        assert int(plan['nnz']) == sum(o.nnz for o in sp.ops) and int(plan['lds']) == 2 * sp.n * 16 and int(plan['grad_grid']) == G * sp.steps
        assert int(plan['threads']) == (1024 if sp.n > 256 else 256)
        if name == 'dense_n8':
            assert widths == [8] * (sp.k + 1)
        if name == 'diagonal':
            assert widths == [1] * (sp.k + 1)
        if name == 'zero_control':
            assert widths[1] == 0
        eng.set_base(bases)
        r = eng.evaluate()
        assert_eval(name, r, refs, eng.get_inter_vecs())
        assert np.array_equal(eng.get_base(), bases)
        np.testing.assert_allclose(eng.get_uks(evaluated=True), np.stack([o['uks'] for o in refs]), rtol=0, atol=1e-15 * 4)
        s = eng.scalars()
        assert np.array_equal(s['loss'], r['loss']) and np.array_equal(s['reg_loss'], r['reg_loss'])
        with pytest.raises(P.QocError, match='no final unitary'):
            eng.get_final_unitary()
        if name == 'T1':                                                         # the identity map: every time point is the start
            assert np.array_equal(eng.get_inter_vecs()[0], np.broadcast_to(sp.V, (sp.steps + 1,) + sp.V.shape))
    finally:
        eng.close()


def test_the_rows_see_every_operator():
    """Dropping the drift or a control moves the oracle far from the row's reference: the rows cannot pass with an operator left out."""
    sp, refs = system('n33'), reference('n33')
    for j in range(sp.k + 1):
        ops = list(sp.ops)
        ops[j] = sps.csr_matrix(ops[j].shape, dtype=np.complex128)
        cut = sr.SparseProblem(sp.H0_in, sp.Hops_in, sp.V, sp.W, sp.total_time, sp.steps, sp.exp_terms, sp.maxA, sp.reg_coeffs)
        cut.ops = ops
        o = sr.evaluate(cut, sr.bases_of(sp)[1])
        assert abs(o['loss'] - refs[1]['loss']) > 1e-4 or np.max(np.abs(o['grad'] - refs[1]['grad'])) > 1e-4


# ---- 2. the vector homes ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['n16_home', 'n257'])
def test_both_vector_homes(name):
    """LDS and global scratch, forced: each against the oracle, and the two bit for bit -- the homes run the same code through a pointer, every sum in
    the same order."""
    if name == 'n16_home':
        sp = sr.sparse_case(16, 5, m=2, seed=40, forbidden=True)
        refs = [go.evaluate(sr.dense_oracle(sp), b, want_inter=True) for b in sr.bases_of(sp)]
    else:
        sp, refs = system(name), reference(name)
    out = {}
    for home in ('lds', 'global'):
        eng = make_engine(sp, 3, vector_home=home)
        try:
            assert eng.plan['vector_home'] == home and int(eng.plan['lds']) == (2 * sp.n * 16 if home == 'lds' else 0), eng.plan
            eng.set_base(np.stack(sr.bases_of(sp)))
            r = eng.evaluate()
            inter = eng.get_inter_vecs()
            assert_eval('%s %s' % (name, home), r, refs, inter)
            out[home] = (r, inter)
        finally:
            eng.close()
    for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale', 'grad'):
        assert np.array_equal(out['lds'][0][key], out['global'][0][key]), key
    assert np.array_equal(out['lds'][1], out['global'][1])


@functools.lru_cache(maxsize=None)
def boundary_case(n):
    sp = sr.sparse_case(n, 2, k=2, m=1, T=3, seed=50)
    return sp, sr.evaluate(sp, sp.base0)


@pytest.mark.parametrize('n,home', [(5088, 'lds'), (5089, 'global')])
def test_the_boundary_of_the_home_rule(n, home):
    """2 n 16 B <= 159 KiB: n = 5088 is the last size in LDS (162816 bytes of dynamic LDS, far past the 64 KiB a kernel gets without opting in)."""
    sp, ref = boundary_case(n)
    eng = make_engine(sp, 1)
    try:
        assert eng.plan['vector_home'] == home and int(eng.plan['lds']) == (162816 if home == 'lds' else 0), eng.plan
        eng.set_base(sp.base0[None])
        assert_eval('n%d' % n, eng.evaluate(), [ref], eng.get_inter_vecs())
    finally:
        eng.close()
    if home == 'global':
        with pytest.raises(P.QocError, match='vector_home = 1'):
            make_engine(sp, 1, vector_home='lds')


@functools.lru_cache(maxsize=None)
def chain14():
    sp = sr.chain_problem(14, 4, 6, k=2, target_site=1)
    return sp, [sr.evaluate(sp, b) for b in sr.bases_of(sp, 2)]


def test_a_14_spin_chain():
    """n = 16384, the row no dense path can hold (one dense operator: 4.3 GB), against the sparse reference."""
    sp, refs = chain14()
    assert refs[0]['loss'] < 0.9 and np.max(np.abs(refs[0]['grad'])) > 1e-3       # (the excitation arrives: the comparison sees a gradient)
    eng = make_engine(sp, 2)
    try:
        assert eng.plan['vector_home'] == 'global' and eng.plan['threads'] == '1024', eng.plan
        eng.set_base(np.stack(sr.bases_of(sp, 2)))
        assert_eval('chain14', eng.evaluate(), refs, eng.get_inter_vecs())
    finally:
        eng.close()


# ---- 3. determinism, create / destroy ---------------------------------------------------------------------------------------------------------------

def test_two_evaluations_are_bit_identical():
    sp = system('n257')
    eng = make_engine(sp, 3)
    try:
        eng.set_base(np.stack(sr.bases_of(sp)))
        a, ia = eng.evaluate(), eng.get_inter_vecs()
        b, ib = eng.evaluate(), eng.get_inter_vecs()
    finally:
        eng.close()
    other = make_engine(sp, 3)
    try:
        other.set_base(np.stack(sr.bases_of(sp)))
        c, ic = other.evaluate(), other.get_inter_vecs()
    finally:
        other.close()
    for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale', 'grad'):
        assert np.array_equal(a[key], b[key]) and np.array_equal(a[key], c[key]), key
    assert np.array_equal(ia, ib) and np.array_equal(ia, ic)


def test_create_destroy_cycles():
    sp, refs = system('n33'), reference('n33')
    for cycle in range(12):
        eng = make_engine(sp, 1, vector_home=('lds', 'global')[cycle % 2])
        try:
            eng.set_base(sr.bases_of(sp)[0][None])
            r = eng.evaluate()
            assert abs(r['loss'][0] - refs[0]['loss']) <= S_RTOL
        finally:
            eng.close()
    big, small = make_engine(boundary_case(5088)[0], 1), make_engine(sp, 1)      # a small engine beside the largest LDS footprint, then that one again
    try:
        small.set_base(sr.bases_of(sp)[0][None])
        assert abs(small.evaluate()['loss'][0] - refs[0]['loss']) <= S_RTOL
        big.set_base(boundary_case(5088)[0].base0[None])
        assert abs(big.evaluate()['loss'][0] - boundary_case(5088)[1]['loss']) <= S_RTOL
    finally:
        big.close()
        small.close()


# ---- 4. the device loops against the same loops on a dense engine -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def loop_case():
    sp = sr.sparse_case(64, 12, k=3, m=1, T=9, seed=60, reg_coeffs={'dwdt': 0.02, 'amplitude': 0.1})
    return sp, np.stack(sr.bases_of(sp))


def _free_history(eng, bases, iterate, evaluations):
    """The loss of every control set at each of `evaluations` evaluations of a loop that nothing stops."""
    eng.set_base(bases)
    hist = []
    for _ in range(evaluations):
        iterate(1)
        hist.append(eng.scalars()['loss'].copy())
    hist = np.array(hist)                                                  # (evaluation, control set)
    return [hist[:, b:b + 1] for b in range(hist.shape[1])]


def _compare_loops(dense, sparse, its_d, its_s):
    assert list(its_d) == list(its_s) and len(set(its_d)) >= 2, (its_d, its_s)
    sd, ss = dense.scalars(), sparse.scalars()
    assert list(sd['done']) == list(ss['done']) == [1, 1, 1]
    np.testing.assert_allclose(sparse.get_base(), dense.get_base(), rtol=0, atol=LOOP_ATOL)
    np.testing.assert_allclose(sparse.get_uks(), dense.get_uks(), rtol=0, atol=LOOP_ATOL)
    np.testing.assert_allclose(sparse.get_uks(evaluated=True), dense.get_uks(evaluated=True), rtol=0, atol=LOOP_ATOL)
    for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale'):
        np.testing.assert_allclose(ss[key], sd[key], rtol=0, atol=LOOP_ATOL)
    np.testing.assert_allclose(sparse.get_inter_vecs(), dense.get_inter_vecs(), rtol=0, atol=LOOP_ATOL)


def test_adam_loop_against_the_dense_engine():
    sp, bases = loop_case()
    max_it = 11
    dense, sparse = make_dense_engine(sp, 3), make_engine(sp, 3)
    try:
        assert dense.path != P.PATH_SPARSE and sparse.path == P.PATH_SPARSE
        conv = dict(rate=0.05, max_iterations=max_it, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0)
        free = dense.adam_params(poll_every=1, **conv)
        hists = _free_history(dense, bases, lambda n: dense.iterate(free, n), max_it + 1)
        target, stops = _choose_target(hists, max_it)
        print('conv_target %.6e, expected stops %s' % (target, stops))
        conv['conv_target'] = target
        dense.set_base(bases)
        sparse.set_base(bases)
        its_d, its_s = dense.run_adam(dense.adam_params(poll_every=5, **conv)), sparse.run_adam(sparse.adam_params(poll_every=5, **conv))
        assert list(its_d) == stops
        _compare_loops(dense, sparse, its_d, its_s)
    finally:
        dense.close()
        sparse.close()


def test_lbfgs_loop_against_the_dense_engine():
    sp, bases = loop_case()
    max_it = 11
    dense, sparse = make_dense_engine(sp, 3), make_engine(sp, 3)
    try:
        p = dict(conv_target=-1.0, min_grad=-1.0, max_iterations=max_it, history=4)
        free = dense.lbfgs_params(poll_every=1, **p)
        hists = _free_history(dense, bases, lambda n: dense.iterate_lbfgs(free, n), max_it + 1)
        target, stops = _choose_target(hists, max_it)
        print('conv_target %.6e, first evaluations below it %s' % (target, stops))
        p['conv_target'] = target
        dense.set_base(bases)
        sparse.set_base(bases)
        its_d, its_s = dense.run_lbfgs(dense.lbfgs_params(poll_every=5, **p)), sparse.run_lbfgs(sparse.lbfgs_params(poll_every=5, **p))
        _compare_loops(dense, sparse, its_d, its_s)
    finally:
        dense.close()
        sparse.close()


# ---- 5. what the C ABI refuses ------------------------------------------------------------------------------------------------------------------------

def _raw_create(sp, mutate_cfg=None, entries=None, vector_home=0, V=True):
    """qoc_create_sparse through ctypes with a configuration the Python layer would not build; returns (status, message)."""
    lib = P.load_library()
    cfg = P.QocConfig()
    cfg.n, cfg.k, cfg.steps, cfg.m, cfg.taylor_terms, cfg.scaling, cfg.state_transfer, cfg.n_seeds = sp.n, sp.k, sp.steps, sp.m, sp.exp_terms, 0, 1, 1
    cfg.dt, cfg.total_time = sp.dt, sp.total_time
    if mutate_cfg:
        mutate_cfg(cfg)
    n, indptr, row, col, val = P.sparse_arrays(sp.ops)
    if entries:
        entries(row, col, val)
    s = P.QocSparse()
    s.indptr, s.row, s.col = indptr.ctypes.data_as(C.POINTER(C.c_int64)), row.ctypes.data_as(P._IP), col.ctypes.data_as(P._IP)
    s.val, s.vector_home = P._dp(val.view(np.float64)), vector_home
    Vc, Wc, maxA = np.ascontiguousarray(sp.V), np.ascontiguousarray(sp.W), np.ascontiguousarray(sp.maxA)
    h = C.c_void_p()
    rc = lib.qoc_create_sparse(C.byref(cfg), C.byref(s), P._dp(Vc.view(np.float64)) if V else None, P._dp(Wc.view(np.float64)), P._dp(maxA), None, None, None,
                               C.byref(h))
    msg = lib.qoc_last_error().decode()
    if rc == 0:
        lib.qoc_destroy(h)
    return rc, msg


def _set(**kw):
    def f(cfg):
        for key, val in kw.items():
            setattr(cfg, key, val)
    return f


def _entry(i, **kw):
    def f(row, col, val):
        if 'row' in kw:
            row[i] = kw['row']
        if 'col' in kw:
            col[i] = kw['col']
        if 'val' in kw:
            val[i] = kw['val']
    return f


REFUSALS = {
    'unitary_mode': (dict(mutate_cfg=_set(state_transfer=0)), 'state-transfer mode only'),
    'forbid_dressed': (dict(mutate_cfg=_set(forbid_dressed=1)), 'forbid_dressed'),
    'exact_gradient': (dict(mutate_cfg=_set(gradient=1)), 'exact gradient'),
    'time_shards': (dict(mutate_cfg=_set(time_shards=2)), 'time-sharded'),
    'path_generic': (dict(mutate_cfg=_set(path=P.PATH_GENERIC)), 'not on path 1'),
    'path_lindblad': (dict(mutate_cfg=_set(path=P.PATH_LINDBLAD)), 'not on path 6'),
    'taylor_0': (dict(mutate_cfg=_set(taylor_terms=0)), 'taylor_terms = 0'),
    'taylor_61': (dict(mutate_cfg=_set(taylor_terms=61)), 'taylor_terms = 61'),
    'm_0': (dict(mutate_cfg=_set(m=0)), 'm = 0'),
    'row_negative': (dict(entries=_entry(3, row=-1)), 'outside 0 .. 32'),
    'col_past_n': (dict(entries=_entry(0, col=33)), 'outside 0 .. 32'),
    'nan': (dict(entries=_entry(5, val=complex(np.nan, 0))), 'not finite'),
    'inf': (dict(entries=_entry(5, val=complex(0, np.inf))), 'not finite'),
    'vector_home_3': (dict(vector_home=3), 'vector_home = 3'),
    'null_V': (dict(V=False), 'null argument'),
}


@pytest.mark.parametrize('name', list(REFUSALS))
def test_c_level_refusals(name):
    kw, needle = REFUSALS[name]
    rc, msg = _raw_create(system('n33'), **kw)
    assert rc == -1 and msg.startswith('qoc_create_sparse') and needle in msg, (rc, msg)


def test_c_level_refusals_overflow_and_the_dense_entry_point():
    """n * W past int32: a row with n = 50000 entries (50000 stored numbers, not a matrix).  And path 7 belongs to qoc_create_sparse alone."""
    n = 50000
    wide = sps.csr_matrix((np.ones(n, dtype=np.complex128), (np.zeros(n, dtype=np.int64), np.arange(n))), shape=(n, n))
    sp = sr.SparseProblem(wide, [sps.identity(n, dtype=np.complex128, format='csr')], np.ones((n, 1)) / np.sqrt(n), np.ones((n, 1)) / np.sqrt(n), 1.0, 2, 3, [1.0])
    rc, msg = _raw_create(sp)
    assert rc == -1 and 'operator 0' in msg and 'does not fit 32-bit' in msg, (rc, msg)
    small = system('n5')
    with pytest.raises(P.QocError, match='unknown path 7'):
        make_dense_engine(small, 1, path=P.PATH_SPARSE)
    assert _raw_create(system('n33'))[0] == 0                                   # (the untouched arguments do create an engine)


# ---- 6. Grape end to end, the example -------------------------------------------------------------------------------------------------------------

def test_grape_with_sparse_and_with_dense_inputs():
    """One 6-spin problem (n = 64), 30 Adam iterations: the sparse route and the dense engine AUTO picks return the same pulse."""
    from quantum_optimal_control.main_grape.grape import Grape
    H0, Hops, names, exc = xx_chain(6, control_sites=[0, 2, 5])
    conv = {'rate': 0.05, 'update_step': 10, 'max_iterations': 30, 'conv_target': 1e-9, 'learning_rate_decay': 1000}
    kw = dict(Hnames=names, U=[exc(5)], total_time=12.0, steps=40, states_concerned_list=[exc(0)], convergence=conv, reg_coeffs={'dwdt': 0.001}, maxA=[2.0] * 3,
              method='Adam', state_transfer=True, show_plots=False, save=False)
    out = {}
    for kind, ops in (('sparse', (H0, Hops)), ('dense', (H0.toarray(), [h.toarray() for h in Hops]))):
        np.random.seed(3)
        with contextlib.redirect_stdout(io.StringIO()):
            uks, Uf = Grape(ops[0], ops[1], **kw)
        assert Uf == [] and uks.shape == (3, 40)
        out[kind] = uks
    print('largest amplitude %.3f, largest difference %.3e' % (np.max(np.abs(out['dense'])), np.max(np.abs(out['sparse'] - out['dense']))))
    assert np.max(np.abs(out['dense'])) > 0.1
    np.testing.assert_allclose(out['sparse'], out['dense'], rtol=0, atol=1e-10)


def test_grape_sparse_methods_and_restarts():
    """EVOLVE, the device L-BFGS loop and scipy's L-BFGS-B on the sparse route, and restarts=3 control sets."""
    from quantum_optimal_control.main_grape.grape import Grape
    H0, Hops, names, exc = xx_chain(4, control_sites=[0, 3])
    info = {}
    for method, restarts in (('EVOLVE', 1), ('LBFGS', 3), ('L-BFGS-B', 1), ('Adam', 3)):
        np.random.seed(4)
        conv = {'rate': 0.05, 'update_step': 10, 'max_iterations': 12, 'conv_target': 1e-9, 'learning_rate_decay': 1000}
        with contextlib.redirect_stdout(io.StringIO()):
            uks, Uf = Grape(H0, Hops, names, [exc(3)], 6.0, 20, [exc(0)], convergence=conv, reg_coeffs={}, maxA=[2.0, 2.0], method=method, state_transfer=True,
                            show_plots=False, save=False, restarts=restarts, _restart_info=info)
        assert Uf == [] and uks.shape == (2, 20) and np.all(np.isfinite(uks))
        assert info['loss'].shape == (restarts,) and np.all(info['loss'] < 1.0)


def test_spin_chain_example():
    """examples/spin_chain_state_transfer.py end to end on 6 spins in a short budget (the example's list of tests/test_examples.py, continued here): the
    re-simulated pulse brings nine tenths of the excitation to the last spin."""
    import spin_chain_state_transfer
    with contextlib.redirect_stdout(io.StringIO()):
        f = spin_chain_state_transfer.main(spins=6, iterations=150, steps=60, quiet=True)
    assert f > 0.9
