"""The device-resident Adam loop (qoc_run_adam / qoc_iterate) against the oracle's loop, on every flavour of the iteration's tail.

The tail -- pulse regularisers, chain rule through maxA sin(base), grad_squared, stop rule, learning-rate schedule, TF1 Adam and the controls of
the next evaluation (csrc/qoc_kernels_finish.h) -- runs in a kernel chosen by the element count ks = k steps of a control set, the path, the
regulariser set and the QOC_FINISH_SPLIT switch.  The engine reports its choice as plan['tail'] (qoc_plan_describe); expected_tail() below
restates the selection rules, and test_rows_cover_every_tail_flavour (CPU) checks that the rows name every flavour at every regulariser level
it accepts.  The oracle's loop does not depend on the path: it runs once per problem and every path's row compares against it.
"""
import math

import numpy as np
import pytest

from oracle import grape_oracle as go
from tests.golden import cases
from tests.helpers import oracle_system

U_ATOL = 1e-12
G_RTOL = 1e-11
S_RTOL = 1e-12
LOOP_ATOL = 1e-10

LEVELS = ('none', 'local', 'band')
LOCAL_REGS = {'amplitude': 0.02, 'dwdt': 0.001, 'd2wdt2': 1e-5, 'envelope': 0.01}
SPLIT_OFF = (('QOC_EXPERIMENTAL', '1'), ('QOC_FINISH_SPLIT', '0'))
GENERIC, MFMA, ST_FUSED, GEMM, SMALL = 1, 2, 3, 4, 5

# name: (system, n, m, k, steps, level); 'c2': case_c2(n, m, taylor=(4, 1), seed=41), 'st': state transfer with one forbidden level
PROBLEMS = {
    'k8x128_none': ('c2', 3, 2, 8, 128, 'none'),            # 1024
    'k8x128_local': ('c2', 3, 2, 8, 128, 'local'),
    'k8x128_band': ('c2', 3, 2, 8, 128, 'band'),
    'k5x205_none': ('c2', 3, 2, 5, 205, 'none'),            # 1025
    'k5x205_local': ('c2', 3, 2, 5, 205, 'local'),
    'k8x255_band': ('c2', 3, 2, 8, 255, 'band'),            # 2040
    'k7x292_none': ('c2', 3, 2, 7, 292, 'none'),            # 2044
    'k8x256_none': ('c2', 3, 2, 8, 256, 'none'),            # 2048
    'k8x256_local': ('c2', 3, 2, 8, 256, 'local'),
    'k8x512_band': ('c2', 3, 2, 8, 512, 'band'),            # 4096
    'k5x820_none': ('c2', 3, 2, 5, 820, 'none'),            # 4100
    'k5x820_local': ('c2', 3, 2, 5, 820, 'local'),
    'k5x820_band': ('c2', 3, 2, 5, 820, 'band'),
    'k8x1024_local': ('c2', 3, 2, 8, 1024, 'local'),        # 8192
    'k5x1639_none': ('c2', 3, 2, 5, 1639, 'none'),          # 8195
    'k5x1639_band': ('c2', 3, 2, 5, 1639, 'band'),
    'k8x2048_band': ('c2', 3, 2, 8, 2048, 'band'),          # 16384
    'k5x3277_local': ('c2', 3, 2, 5, 3277, 'local'),        # 16385
    'n10m9_k8x513_local': ('c2', 10, 9, 8, 513, 'local'),   # 4104, m > 8: the GEMM path launches its chains
    'st_k5x820_local': ('st', 4, 1, 5, 820, 'local'),       # 4100, state transfer, forbidden level 3
}

# (path, variant, env, problem, expected tail)
ROWS = [
    (GENERIC, 0, (), 'k8x128_none', 'finish256_regs'),
    (GENERIC, 0, (), 'k5x205_local', 'finish256_memory'),
    (GENERIC, 0, (), 'k8x255_band', 'finish256_memory'),
    (GENERIC, 0, (), 'k8x256_none', 'finish1024_regs'),
    (GENERIC, 0, (), 'k8x512_band', 'finish1024_regs'),
    (GENERIC, 0, (), 'k5x820_local', 'split17'),
    (GENERIC, 0, (), 'k5x1639_band', 'split33'),
    (GENERIC, 0, (), 'k8x2048_band', 'split64'),
    (MFMA, 8, (), 'k8x128_local', 'finish256_regs'),
    (MFMA, 8, (), 'k8x128_band', 'finish256_regs'),
    (MFMA, 8, (), 'k5x205_none', 'finish256_memory'),
    (MFMA, 8, (), 'k7x292_none', 'finish256_memory'),
    (MFMA, 8, (), 'k8x256_local', 'finish1024_regs'),
    (MFMA, 8, (), 'k5x820_none', 'split17'),
    (MFMA, 8, (), 'k5x3277_local', 'split64'),
    (MFMA, 5, (), 'k8x128_none', 'latency_fused_regs'),
    (MFMA, 5, (), 'k8x256_local', 'latency_fused_regs'),
    (MFMA, 5, (), 'k5x820_none', 'latency_fused_memory'),
    (MFMA, 5, (), 'k8x1024_local', 'latency_fused_memory'),
    (MFMA, 5, (), 'k5x3277_local', 'latency_fused_memory'),
    (MFMA, 5, (), 'k8x255_band', 'finish256_memory'),       # bandpass: the separate tail
    (MFMA, 5, (), 'k5x820_band', 'split17'),
    (GEMM, 0, (), 'k5x820_none', 'split17_partials'),
    (GEMM, 0, (), 'k8x1024_local', 'split32_partials'),
    (GEMM, 0, (), 'k5x1639_band', 'split33_partials'),
    (GEMM, 0, (), 'k5x3277_local', 'split64_partials'),
    (GEMM, 0, (), 'k8x512_band', 'finish1024_regs'),
    (GEMM, 0, (), 'n10m9_k8x513_local', 'split17'),
    (GENERIC, 0, SPLIT_OFF, 'k5x820_none', 'finish1024_regs8'),
    (GENERIC, 0, SPLIT_OFF, 'k8x1024_local', 'finish1024_regs8'),
    (MFMA, 8, SPLIT_OFF, 'k5x820_band', 'finish1024_regs8'),
    (GENERIC, 0, SPLIT_OFF, 'k5x1639_band', 'finish1024_memory'),
    (MFMA, 8, SPLIT_OFF, 'k5x1639_none', 'finish1024_memory'),
    (GEMM, 0, SPLIT_OFF, 'k5x3277_local', 'finish1024_memory'),
    (GENERIC, 0, (), 'st_k5x820_local', 'split17'),
    (ST_FUSED, 0, (), 'st_k5x820_local', 'split17'),
    (GEMM, 0, (), 'st_k5x820_local', 'split17_partials'),
    (SMALL, 0, (), 'k8x128_none', 'in_launch'),
    (SMALL, 0, (), 'k8x128_band', 'in_launch'),
    (SMALL, 0, (), 'k5x820_local', 'in_launch'),
    (SMALL, 0, (), 'k5x820_band', 'refused'),
]

# refusals of the workgroup-resident path (qoc_small.hip, qoc_small_supported): the bandpass DFT needs the whole pulse in one workgroup
SMALL_REFUSAL = 'the workgroup-resident path needs a pulse that fits 32 workgroups per control set'


def _ks(problem):
    _, _, _, k, steps, _ = PROBLEMS[problem]
    return k * steps


def expected_tail(path, ks, n, m, level, env, variant=0):
    """The selection rules of tail_kind (csrc/qoc_engine.hip) with the thread counts of finish_body's register branch, for n <= 32 (latency mode:
    one workgroup of 1024 threads, i.e. NT != 3)."""
    split = dict(env).get('QOC_EXPERIMENTAL') != '1' or dict(env).get('QOC_FINISH_SPLIT') != '0'
    if path == SMALL:
        return 'in_launch'
    if path == MFMA and variant == 5 and level != 'band':
        return 'latency_fused_regs' if ks <= 4 * 1024 else 'latency_fused_memory'
    if ks > 4096 and split:
        npad = 32 * math.ceil(n / 32)
        return 'split%d%s' % (min(64, math.ceil(ks / 256)), '_partials' if path == GEMM and npad <= 64 and m <= 8 else '')
    if 4096 < ks <= 8192:
        return 'finish1024_regs8'
    threads = 1024 if ks >= 2048 else 256
    return 'finish%d_%s' % (threads, 'regs' if ks <= 4 * threads else 'memory')


def _flavour(tail):
    """split<S>[_partials] -> split / split_partials; the others as they are."""
    if tail.startswith('split'):
        return 'split_partials' if tail.endswith('_partials') else 'split'
    return tail


# the regulariser levels each flavour accepts (the latency mode keeps its fused tail only without the bandpass DFT)
FLAVOUR_LEVELS = {
    'finish256_regs': LEVELS, 'finish256_memory': LEVELS, 'finish1024_regs': LEVELS, 'finish1024_regs8': LEVELS, 'finish1024_memory': LEVELS,
    'split': LEVELS, 'split_partials': LEVELS, 'latency_fused_regs': ('none', 'local'), 'latency_fused_memory': ('none', 'local'),
    'in_launch': LEVELS,
}


def _row_id(row):
    path, variant, env, problem, tail = row
    name = {GENERIC: 'generic', MFMA: 'mfma%d' % variant, ST_FUSED: 'st_fused', GEMM: 'gemm', SMALL: 'small'}[path]
    return '%s-%s-%s%s' % (name, problem, tail, '-splitoff' if env else '')


def test_rows_cover_every_tail_flavour():
    """CPU: every row's declared flavour follows the selection rules, and the rows cover every flavour at every level it accepts."""
    seen = set()
    for row in ROWS:
        path, variant, env, problem, tail = row
        system, n, m, k, steps, level = PROBLEMS[problem]
        if tail == 'refused':
            assert path == SMALL and level == 'band' and steps > 256, row
            continue
        assert tail == expected_tail(path, k * steps, n, m, level, env, variant), row
        seen.add((_flavour(tail), level))
    want = {(f, lv) for f, lvs in FLAVOUR_LEVELS.items() for lv in lvs}
    assert want <= seen, sorted(want - seen)
    # every threshold of the selection rules has a problem on both sides
    counts = {_ks(p) for p in PROBLEMS}
    for below, above in ((1024, 1025), (2047, 2048), (4096, 4097), (8192, 8193), (16384, 16385)):
        assert any(c <= below and c > below - 8 for c in counts) and any(c >= above and c < above + 8 for c in counts), (below, above)
    assert sum(PROBLEMS[p][4] % 256 != 0 for p in PROBLEMS) >= 3             # slice counts that are not multiples of 256


# ---- problems and the oracle's loop, once per problem ------------------------------------------------------------------------------------------

def _system(problem):
    system, n, m, k, steps, level = PROBLEMS[problem]
    if system == 'c2':
        c = cases.case_c2(n=n, k=k, steps=steps, m=m, taylor=(4, 1), seed=41)
        c['reg_coeffs'] = {}
    else:
        c = cases.case_c3(n=n, k=k, steps=steps, taylor=(6, 0), seed=43)
        c['reg_coeffs'] = {'forbidden_coeff_list': [50.0], 'states_forbidden_list': [n - 1]}
    c['total_time'] = 0.02 * steps
    if level != 'none':
        c['reg_coeffs'].update(LOCAL_REGS)
    if level == 'band':
        c['reg_coeffs'].update(bandpass=0.01, band=[0.5, 5.0])
    sp = oracle_system(c)
    bases = np.stack([sp.base0, 0.6 * sp.base0 + 0.1, -0.8 * sp.base0 + 0.05])       # three control sets, distinct starting points
    return sp, bases


def _max_iterations(problem):
    return 11 if _ks(problem) <= 4200 else 7             # (poll every 5: never a divisor)


def _choose_target(hists, max_it, accept=None):
    """A conv_target at which the control sets stop at >= 2 distinct iteration counts, one of them runs to max_iterations, and no loss of any
    history lies within 1e-8 relative of it (the stop never rests on the last bit).  Midpoints between the losses, the widest margin wins.
    accept(stops): a further condition on the stop counts a caller needs (tests/test_finished_sets_gpu.py)."""
    losses = np.sort(np.unique(np.concatenate([h[:, 0] for h in hists])))
    best = None
    for lo, hi in zip(losses[:-1], losses[1:]):
        t = 0.5 * (lo + hi)
        stops = []
        for h in hists:
            below = np.nonzero(h[:, 0] < t)[0]
            stops.append(int(below[0]) if len(below) else max_it)
        margin = min(np.min(np.abs(h[:, 0] - t)) / abs(t) for h in hists)
        inner = sum(0 < s < max_it for s in stops)
        key = (len(set(stops)), max_it in stops, inner, margin)
        if max_it in stops and len(set(stops)) >= 2 and (accept is None or accept(stops)) and (best is None or key > best[0]):
            best = (key, t, stops)
    assert best is not None, 'no conv_target splits the control sets'
    return best[1], best[2]


def _choose_min_grad(hists, max_it, accept=None):
    """_choose_target for the other stop rule: a min_grad between two grad_squared values of the free runs at which the control sets stop at
    >= 2 distinct iteration counts and no value of any history lies within 1e-8 relative of it.  The widest margin wins.  accept(stops): as
    above -- without it the distinct count ranks first, and a problem whose gradients only ever fall gives 0 and max_iterations alone."""
    values = np.sort(np.unique(np.concatenate([h[:, 2] for h in hists])))
    best = None
    for lo, hi in zip(values[:-1], values[1:]):
        t = 0.5 * (lo + hi)
        stops = []
        for h in hists:
            below = np.nonzero(h[:, 2] < t)[0]
            stops.append(int(below[0]) if len(below) else max_it)
        margin = min(np.min(np.abs(h[:, 2] - t)) / abs(t) for h in hists)
        key = (len(set(stops)), sum(0 < s < max_it for s in stops), margin)
        if len(set(stops)) >= 2 and margin > 1e-8 and (accept is None or accept(stops)) and (best is None or key > best[0]):
            best = (key, t, stops)
    assert best is not None, 'no min_grad splits the control sets'
    return best[1], best[2]


_ORACLE = {}


def oracle(problem):
    """Per problem: the system, the starting bases, the loop's parameters and per control set the oracle's run_adam result and its evaluation at the
    final base (inter_vecs included)."""
    if problem in _ORACLE:
        return _ORACLE[problem]
    sp, bases = _system(problem)
    max_it = _max_iterations(problem)
    conv = dict(rate=0.02, max_iterations=max_it, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0)
    free = [go.run_adam(sp, conv, base=b, history=True) for b in bases]
    target, stops = _choose_target([r['history'] for r in free], max_it)
    conv = dict(conv, conv_target=target)
    refs = []
    for b, r, s in zip(bases, free, stops):
        if s < max_it:
            r = go.run_adam(sp, conv, base=b, history=True)
        assert r['iterations'] == s
        assert np.min(np.abs(r['history'][:, 0] - target)) > 1e-8 * abs(target)
        refs.append(r)
    finals = [go.evaluate(sp, r['base'], want_inter=True) for r in refs]
    _ORACLE[problem] = (sp, bases, conv, refs, finals)
    return _ORACLE[problem]


def make_engine(sp, n_seeds, path, variant=0):
    from quantum_optimal_control.core import hip_engine
    return hip_engine.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling,
                                state_transfer=sp.state_transfer, reg_coeffs=sp.reg_coeffs, one_minus_gauss=sp.one_minus_gauss, Vs=sp.Vs,
                                n_seeds=n_seeds, path=path, variant=variant)


def _engine(row, monkeypatch, sp, n_seeds=3):
    path, variant, env, problem, tail = row
    for key, value in env:
        monkeypatch.setenv(key, value)                   # (read when the engine is created; only beside QOC_EXPERIMENTAL=1)
    eng = make_engine(sp, n_seeds, path, variant)
    assert eng.path == path
    assert eng.plan['tail'] == tail, (eng.plan, tail)
    return eng


def _compare_final(eng, sp, finals, r, u_atol=U_ATOL):
    """check_eval's comparison, against the cached oracle evaluations at the final bases (after a loop the bases themselves agree to LOOP_ATOL only)."""
    inter = eng.get_inter_vecs()
    Uf = None if sp.state_transfer else eng.get_final_unitary()
    for b, o in enumerate(finals):
        if r is not None:
            for key in ('loss', 'reg_loss', 'unitary_scale', 'grad_squared'):
                assert abs(r[key][b] - o[key]) <= S_RTOL * max(1.0, abs(o[key])), (key, b, r[key][b], o[key])
            gmax = max(1e-300, np.max(np.abs(o['grad'])))
            assert np.max(np.abs(r['grad'][b] - o['grad'])) <= G_RTOL * max(gmax, 1e-3), ('grad', b, np.max(np.abs(r['grad'][b] - o['grad'])), gmax)
        np.testing.assert_allclose(inter[b], o['inter_vecs'], rtol=0, atol=u_atol * max(1, np.max(np.abs(o['inter_vecs']))))
        if Uf is not None:
            np.testing.assert_allclose(Uf[b], o['U_final'], rtol=0, atol=u_atol * max(1, np.max(np.abs(o['U_final']))))


SMALL_ROWS = [r for r in ROWS if r[4] == 'refused']
LOOP_ROWS = [r for r in ROWS if r[4] != 'refused']


@pytest.mark.gpu
@pytest.mark.parametrize('row', SMALL_ROWS, ids=[_row_id(r) for r in SMALL_ROWS])
def test_small_path_refusal_is_an_error(row):
    from quantum_optimal_control.core.hip_engine import QocError
    sp, _ = _system(row[3])
    with pytest.raises(QocError, match=SMALL_REFUSAL):
        make_engine(sp, 3, row[0], row[1])


@pytest.mark.gpu
@pytest.mark.parametrize('row', LOOP_ROWS, ids=[_row_id(r) for r in LOOP_ROWS])
def test_loop_against_the_oracle(row, monkeypatch):
    """run_adam with seeds that stop at different iterations inside a burst (poll every 5), then every read-back and one more evaluation."""
    sp, bases, conv, refs, finals = oracle(row[3])
    stops = [r['iterations'] for r in refs]
    assert len(set(stops)) >= 2 and conv['max_iterations'] in stops, stops
    eng = _engine(row, monkeypatch, sp)
    eng.set_base(bases)
    its = eng.run_adam(eng.adam_params(poll_every=5, **conv))
    assert list(its) == stops
    s = eng.scalars()
    assert list(s['iterations']) == stops and list(s['done']) == [1, 1, 1]
    base, uks, uks_ev = eng.get_base(), eng.get_uks(), eng.get_uks(evaluated=True)
    for b, ref in enumerate(refs):
        np.testing.assert_allclose(base[b], ref['base'], rtol=0, atol=LOOP_ATOL)
        np.testing.assert_allclose(uks[b], ref['uks'], rtol=0, atol=LOOP_ATOL)
        np.testing.assert_allclose(uks_ev[b], ref['uks'], rtol=0, atol=LOOP_ATOL)      # (a stopped seed is not moved: current = evaluated)
        for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale'):
            assert abs(s[key][b] - ref[key]) <= LOOP_ATOL * max(1.0, abs(ref[key])), (key, b, s[key][b], ref[key])
    _compare_final(eng, sp, finals, None, LOOP_ATOL)
    # one more evaluation, at the oracle's final bases: dL/du re-formed through the same tail (on the GEMM path's persistent chains: from the
    # per-tile partials the split tail sums)
    eng.set_base(np.stack([r['base'] for r in refs]))
    _compare_final(eng, sp, finals, eng.evaluate())
    eng.close()


# one row per tail kind: explicit steps with a learning rate per control set
STEP_ROWS = [r for r in LOOP_ROWS if r[0] != SMALL]
STEP_ROWS = [next(r for r in STEP_ROWS if _flavour(r[4]) == f) for f in sorted({_flavour(r[4]) for r in STEP_ROWS})] + \
    [r for r in LOOP_ROWS if r[0] == SMALL][:1]


@pytest.mark.gpu
@pytest.mark.parametrize('row', STEP_ROWS, ids=[_row_id(r) for r in STEP_ROWS])
def test_explicit_steps_against_tf1_adam(row, monkeypatch):
    """qoc_adam_step (mode 2) three times, a different learning rate per control set and step, against tf.train.AdamOptimizer per control set.  The
    oracle's Adam steps from the device's gradient (itself checked against the oracle's): an element whose gradient is near eps / sqrt(1 - beta2)
    turns the gradient's last bits into the step's, which atol 1e-13 on the update must not depend on."""
    sp, bases = _system(row[3])
    lrs = np.array([0.01, 0.02, 0.005])
    eng = _engine(row, monkeypatch, sp)
    eng.set_base(bases)
    opts = [go.Adam(b.shape) for b in bases]
    base = bases.copy()
    for step in range(3):
        grad = eng.evaluate()['grad']
        for b in range(len(bases)):
            o = go.evaluate(sp, base[b])['grad']
            assert np.max(np.abs(grad[b] - o)) <= G_RTOL * max(np.max(np.abs(o)), 1e-3), (step, b)
        eng.adam_step(np.roll(lrs, step))
        base = np.stack([opt.step(x, g, lr) for opt, x, g, lr in zip(opts, base, grad, np.roll(lrs, step))])
        np.testing.assert_allclose(eng.get_base(), base, rtol=0, atol=1e-13)
        base = eng.get_base()
    eng.close()


READ_ROWS = [next(r for r in LOOP_ROWS if _flavour(r[4]) == f and not r[2])
             for f in ('split', 'split_partials', 'latency_fused_regs', 'latency_fused_memory')]


@pytest.mark.gpu
@pytest.mark.parametrize('row', READ_ROWS, ids=[_row_id(r) for r in READ_ROWS])
def test_reads_between_bursts_change_nothing(row, monkeypatch):
    """iterate 4, read current / evaluated pulses, final unitary, inter_vecs and scalars, iterate 3: bit for bit an uninterrupted iterate 7."""
    sp, bases = _system(row[3])
    conv = dict(rate=0.02, max_iterations=10 ** 6, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0)
    ref = _engine(row, monkeypatch, sp)
    ref.set_base(bases)
    ref.iterate(ref.adam_params(**conv), 7)
    ref.sync()
    eng = _engine(row, monkeypatch, sp)
    eng.set_base(bases)
    p = eng.adam_params(**conv)
    eng.iterate(p, 4)
    eng.get_uks()
    eng.get_uks(evaluated=True)
    eng.get_final_unitary()
    eng.get_inter_vecs()
    eng.scalars()
    eng.iterate(p, 3)
    eng.sync()
    np.testing.assert_array_equal(eng.get_base(), ref.get_base())
    np.testing.assert_array_equal(eng.get_uks(), ref.get_uks())
    np.testing.assert_array_equal(eng.get_uks(evaluated=True), ref.get_uks(evaluated=True))
    a, b = eng.scalars(), ref.scalars()
    for key in a:
        np.testing.assert_array_equal(a[key], b[key])
    np.testing.assert_array_equal(eng.get_inter_vecs(), ref.get_inter_vecs())
    eng.close()
    ref.close()
