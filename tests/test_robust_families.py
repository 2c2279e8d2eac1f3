"""Robust ensembles behind every kernel family they can run on.

An ensemble engine (qoc_create_ensemble, csrc/qoc_ensemble.h) turns G control sets x E members into G E trajectories of k + q controls and runs the
existing forward / loss / backward kernels on them, with a group view of G rows for the tail.  tests/test_robust_gpu.py checks that claim on toy
sizes (one kernel family); here every family the plain engine is tested on runs with an ensemble behind it and is compared with the ensemble
COMPOSED FROM THE UNCHANGED ORACLE: one go.OracleSystem per member (robust.member_hamiltonians, the engine's (T, s)), weighted sums of the members'
quantities (helpers of tests/test_robust_gpu.py).

  1. FAMILY_ROWS: one row per kernel family.  A row fixes the problem, (E, q, G), how the engine is requested and the plan keys it must resolve to;
     the plan is asserted BEFORE anything is compared, and a row never skips.  Compared per control set g and member e: loss, reg_loss,
     grad_squared, unitary_scale, the gradient, member_scalars()['loss'] and ['reg_state'], get_final_unitary() (member 0),
     member_final_unitary() (every member), get_inter_vecs() (member 0, every tau), get_uks(); then one explicit adam_step against go.Adam on the
     composed gradient (the group-view tail behind every family), and a second one followed by the read-backs of the stale, lazily formed buffers.
  2. test_rows_cover_every_reachable_plan (CPU): the plan values an ensemble can reach without QOC_EXPERIMENTAL, restated, and the rows must name
     each of them (the device of tests/test_adam_tail.py).  AUTO's table for ensembles itself: tests/test_auto_plan.py.
  3. LOOP_ROWS: run_adam with three control sets that stop at different iterations inside a burst, against python_loop over the composed oracle,
     on the families with lazy or shared state; after the loop every control set's read-backs are those of ITS last evaluation.
  4. the glue kernels' edges (a member of weight 0, one perturbed member, more items than one pass of k_ens_expand's grid, scales and offsets of
     either sign, a scale of exactly 0).
  5. Grape(robust=..., restarts=3) end to end against the winning seed of python_loop.

Tolerances (decided before anything was measured): the project's own.  TIGHT = 1e-12 (scalars, relative to max(1, |x|)), 1e-11 max(1, max|grad|),
1e-12 (vectors, unitaries) -- tests/test_robust_gpu.py -- for pulses of up to 200 slices (tests/test_auto_plan.py holds the plain engines to
these bounds at 130 slices and more); FULL = 1e-11 / 1e-10 / 1e-11 -- DESIGN.md section 2, test_hip_against_the_reference_text_at_baseline_sizes --
for the longer ones (the full-size C2 and C3 rows, the 820-slice split-tail row): round-off accumulates along the product chain.  1e-9 for a
base after an Adam step (tests/test_oracle_golden.py).  The weights sum to 1 (robust.validate), so a bound on one trajectory is a bound on the
weighted sum.
"""
import contextlib
import io
import re

import numpy as np
import pytest

from oracle import grape_oracle as go
from quantum_optimal_control.core import hip_engine
from quantum_optimal_control.helper_functions import robust as rb
from tests.golden import cases
from tests.test_adam_tail import _choose_target
from tests.test_auto_plan import _st_problem, expected_plan
from tests.test_robust_gpu import PULSE_REGS, bases_for, composed, ensemble, make_engine, member_systems, nominal_system, python_loop

P = hip_engine
TIGHT = dict(s=1e-12, g=1e-11, u=1e-12)
FULL = dict(s=1e-11, g=1e-10, u=1e-11)
STEP_ATOL = 1e-9
AUTO, GENERIC, MFMA, ST_FUSED, GEMM = P.PATH_AUTO, P.PATH_GENERIC, P.PATH_MFMA, P.PATH_ST_FUSED, P.PATH_GEMM
STATE_REGS = {'dwdt': 0.1, 'forbidden_coeff_list': [3.0, 2.0], 'speed_up': 0.4}


def tolerances(steps):
    return TIGHT if steps <= 200 else FULL


# ---- problems -----------------------------------------------------------------------------------------------------------------------------------

def c2(n, k, steps, m=8, taylor=(5, 2), seed=0, regs=None):
    """The C2 recipe at a short pulse (0.04 per slice: a well-conditioned gradient at every size, as tests/test_auto_plan.py)."""
    c = cases.case_c2(n=n, k=k, steps=steps, m=m, taylor=taylor, seed=seed)
    c['total_time'] = 0.04 * steps
    c['reg_coeffs'] = dict(regs or {})
    return c


def c2_state_reg(n, k, steps, m=8):
    return c2(n, k, steps, m, regs=dict(STATE_REGS, states_forbidden_list=[n - 1, n - 2]))


def st(n, k, m, steps, reg=False, hermitian=True, speed_up=False):
    """State transfer (tests/test_auto_plan.py: the C3 recipe, T = 8, 0.04 per slice; reg: C3's two forbidden levels)."""
    c = _st_problem(n, k, m, steps, hermitian, reg)
    if speed_up:
        c['reg_coeffs'] = dict(c['reg_coeffs'], speed_up=0.3)
    return c


def c3_shaped(k=6, steps=1000, n=64, taylor=(10, 0)):
    c = cases.case_c3(n=n, k=k, steps=steps, taylor=taylor)
    return c


def squared_chain_problem():
    c = cases.case_c3(n=64, k=3, steps=31, taylor=(10, 0))          # test_direct_route_on_the_squared_generator_chain: n64_T10_forbidden
    c['total_time'] = 3.1
    return c


def qubit(steps=400):
    sx = np.array([[0, 1], [1, 0]], dtype=complex)
    sy = np.array([[0, -1j], [1j, 0]], dtype=complex)
    sz = np.array([[1, 0], [0, -1]], dtype=complex)
    return dict(H0=2 * np.pi * 0.05 * sz / 2, Hops=[2 * np.pi * sx / 2, 2 * np.pi * sy / 2], Hnames=['x', 'y'], U=sx, total_time=10.0, steps=steps,
                states_concerned_list=[0, 1], maxA=[0.3, 0.2], reg_coeffs={'dwdt': 0.01}, Taylor_terms=[8, 2], state_transfer=False,
                initial_guess=None, dressed_info=None, U0=None, np_seed=11)


PROBLEMS = {
    'c2_full': lambda: cases.case_c2(n=32, k=4, steps=500, m=8, taylor=(5, 3), seed=0),
    'n24_k4_pulse_regs': lambda: c2(24, 4, 130, regs=PULSE_REGS),
    'n28_k4_state_regs': lambda: c2_state_reg(28, 4, 130),
    'n24_k4_m12': lambda: c2(24, 4, 130, m=12),
    'n40_k3': lambda: c2(40, 3, 60, regs={'dwdt': 0.1, 'amplitude': 0.05}),
    'n48_k3': lambda: c2(48, 3, 60),
    'n64_k4': lambda: c2(64, 4, 40),
    'n55_k4': lambda: c2(55, 4, 40, regs={'dwdt': 0.1}),
    'n32_k3_short': lambda: c2(32, 3, 40),
    'n20_k5': lambda: c2(20, 5, 40),
    'n20_k6': lambda: c2(20, 6, 40),
    'n16_k3': lambda: c2(16, 3, 40, m=4),
    'n40_k3_m6': lambda: c2(40, 3, 30, m=6, regs={'dwdt': 0.1}),
    'n40_k3_m12': lambda: c2(40, 3, 30, m=12),
    'n96_k2': lambda: c2(96, 2, 10, taylor=(6, 3)),
    'n130_k2': lambda: c2(130, 2, 12, taylor=(6, 3)),
    'n36_k5_820': lambda: c2(36, 5, 820, m=6, regs={'dwdt': 0.1, 'amplitude': 0.05}),
    'c3_full': lambda: c3_shaped(),
    'st_n40_k4': lambda: st(40, 4, 1, 100),
    'st_n47_k4': lambda: st(47, 4, 1, 100),
    'st_n50_k4': lambda: st(50, 4, 1, 100),
    'st_n40_k4_m2': lambda: st(40, 4, 2, 100),
    'st_n64_k3_sq': squared_chain_problem,
    'st_n64_k3_lossy': lambda: st(64, 3, 1, 30, hermitian=False),
    'st_n70_k3_m2': lambda: st(70, 3, 2, 20),
    'st_n20_k5': lambda: st(20, 5, 1, 40),
    'st_n32_k4': lambda: st(32, 4, 1, 100),
    'st_n32_k4_regs': lambda: st(32, 4, 1, 100, reg=True, speed_up=True),
    'st_n40_k3': lambda: st(40, 3, 1, 100),
    'st_n40_k3_regs': lambda: st(40, 3, 1, 100, reg=True, speed_up=True),
    'qubit_400': qubit,
    'n8_k2': lambda: c2(8, 2, 40, m=4, taylor=(6, 2), seed=21, regs={'dwdt': 0.01}),
}


def expected_tail(k, steps):
    """tail_kind (csrc/qoc_engine.hip) for an ensemble: the stand-alone tails on the group view of k controls -- never a path's own tail, and
    never the persistent chains' partials (k_ens_reduce leaves a plain gradient array)."""
    ks = k * steps
    if ks > 4096:
        return 'split%d' % min(64, -(-ks // 256))
    threads = 1024 if ks >= 2048 else 256
    return 'finish%d_%s' % (threads, 'regs' if ks <= 4 * threads else 'memory')


def row(name, problem, E, q, G, plan, path=AUTO, variant=0, chunks=0, ens=None):
    """ens: a callable that builds the row's ensemble; None: tests/test_robust_gpu.py's seeded ensemble(case, E, q)."""
    return dict(name=name, problem=problem, E=E, q=q, G=G, plan=plan, path=path, variant=variant, chunks=chunks, ens=ens)


def bench_ensemble():
    """The ensemble tools/robust_bench.py times on C2 (profiles/r07_robust.txt): one random Hermitian perturbation of 2 pi 0.01, 8 offsets x 8 amplitude
    scales, uniform weights."""
    from quantum_optimal_control.helper_functions.synthetic_systems import herm
    rng = np.random.default_rng(1)
    return rb.ensemble_grid(operators=[2 * np.pi * 0.01 * herm(rng, 32)], offsets=np.linspace(-1, 1, 8)[:, None], amp_scales=np.linspace(0.95, 1.05, 8), k=4)


def mfma(nt, expm, sweeps, **kw):
    return dict(path='mfma', nt=nt, expm=expm, sweeps=sweeps, **kw)


def gemm(route, chains, **kw):
    return dict(path='gemm', route=route, chains=chains, **kw)


# the exponential kernels a caller can force on an NT = 2 problem, and what qoc_plan_describe reports for each (7, the row-block kernel of the 48- and
# 64-wide problems, runs as the streamed kernel 4 there)
EXPM_REPORTED = {1: 1, 2: 2, 3: 3, 4: 4, 6: 6, 7: 4, 8: 8}

FAMILY_ROWS = [
    # ---- unitary mode, MFMA path ----
    row('headline_c2_x64_downup_lazy_final', 'c2_full', 64, 1, 1, mfma(2, 8, 'downup', chunks=16, tail='finish256_memory'), ens=bench_ensemble),
    row('downup_at_5_controls', 'n24_k4_pulse_regs', 8, 1, 3, mfma(2, 8, 'downup')),
    row('row_tile_gradient_nt2_at_6_controls', 'n24_k4_pulse_regs', 8, 2, 3, mfma(2, 8, 'row_tile_gradient')),
    row('pair_state_regulariser', 'n28_k4_state_regs', 4, 1, 3, mfma(2, 8, 'pair')),
    row('pair_m12', 'n24_k4_m12', 4, 1, 2, mfma(2, 8, 'pair')),
    row('nt3_n40_padded', 'n40_k3', 4, 1, 2, mfma(3, 7, 'row_tile_gradient')),
    row('nt3_n48', 'n48_k3', 4, 1, 2, mfma(3, 7, 'row_tile_gradient')),
    row('nt4_n64', 'n64_k4', 16, 1, 4, mfma(4, 7, 'row_tile_gradient')),
    row('nt4_n55_padded', 'n55_k4', 16, 1, 4, mfma(4, 7, 'row_tile_gradient')),
    row('nt1_n16', 'n16_k3', 4, 1, 2, mfma(1, 1, 'one_wave')),
] + [
    row('expm%d_chunks%d' % (v, ch), 'n32_k3_short', 3, 1, 2, mfma(2, EXPM_REPORTED[v], 'one_wave' if v == 1 else 'downup', chunks=40 if ch == 0 else 7),
        path=MFMA, variant=v, chunks=ch)
    for v in (1, 2, 3, 4, 6, 7, 8) for ch in (0, 7)
] + [
    row('eight_controls_mfma', 'n20_k5', 3, 3, 2, mfma(2, 8, 'row_tile_gradient'), path=MFMA),
    row('eight_controls_st_fused', 'st_n20_k5', 3, 3, 2, dict(path='st_fused'), path=ST_FUSED),
    row('nine_controls_auto_gemm', 'n20_k6', 3, 3, 2, gemm('unitary', 'persistent')),
    # ---- GEMM path ----
    row('gemm_unitary_persistent_n40', 'n40_k3_m6', 2, 1, 2, gemm('unitary', 'persistent')),
    row('gemm_unitary_launches_m12', 'n40_k3_m12', 2, 1, 2, gemm('unitary', 'launches')),
    row('gemm_n96_workgroup_tiles', 'n96_k2', 2, 1, 2, gemm('unitary', 'launches')),
    row('gemm_n130_padded', 'n130_k2', 2, 1, 2, gemm('unitary', 'launches')),
    row('gemm_persistent_split_tail', 'n36_k5_820', 2, 1, 2, gemm('unitary', 'persistent', tail='split17')),
    # ---- state transfer ----
    row('c3_direct_packed', 'c3_full', 4, 1, 6, gemm('direct', 'persistent', taylor_chain='packed')),
    row('c3_propagator', 'c3_full', 4, 1, 2, gemm('propagator', 'persistent')),
    row('direct_columns40', 'st_n40_k4', 4, 1, 3, gemm('direct', 'persistent', taylor_chain='columns40')),
    row('direct_columns48', 'st_n47_k4', 4, 1, 3, gemm('direct', 'persistent', taylor_chain='columns48')),
    row('direct_columns56', 'st_n50_k4', 4, 1, 3, gemm('direct', 'persistent', taylor_chain='columns56')),
    row('direct_butterfly_m2', 'st_n40_k4_m2', 8, 1, 6, gemm('direct', 'persistent', taylor_chain='butterfly')),
    row('direct_squared_chain', 'st_n64_k3_sq', 2, 2, 2, gemm('direct', 'persistent', taylor_chain='squared'), path=GEMM, variant=2, chunks=1),
    row('direct_full_lossy_drift', 'st_n64_k3_lossy', 2, 1, 2, gemm('direct', 'persistent', taylor_chain='full')),
    row('propagator_launches_n70', 'st_n70_k3_m2', 2, 1, 2, gemm('propagator', 'launches')),
    row('state_transfer_mfma_n32_downup', 'st_n32_k4', 3, 1, 3, mfma(2, 8, 'downup')),
    row('state_transfer_mfma_n32_regs_pair', 'st_n32_k4_regs', 3, 1, 3, mfma(2, 8, 'pair')),
    row('state_transfer_mfma_n40_nt3', 'st_n40_k3', 3, 1, 3, mfma(3, 7, 'row_tile_gradient')),
    row('state_transfer_mfma_n40_nt3_regs', 'st_n40_k3_regs', 3, 1, 3, mfma(3, 7, 'row_tile_gradient')),
]

# what an ensemble engine can report without QOC_EXPERIMENTAL (qoc_plan_describe; 'split' sweeps need QOC_GRAD_RT=0, expm=5 and the latency
# sweeps are the latency mode, which refuses ensembles)
REACHABLE_SWEEPS = {'one_wave', 'pair', 'row_tile_gradient', 'downup'}
REACHABLE_EXPM = {1, 2, 3, 4, 6, 7, 8}
REACHABLE_NT = {1, 2, 3, 4}
REACHABLE_GEMM = {('unitary', 'persistent', None), ('unitary', 'launches', None), ('propagator', 'persistent', None), ('propagator', 'launches', None)} | \
    {('direct', 'persistent', chain) for chain in ('packed', 'columns40', 'columns48', 'columns56', 'full', 'butterfly', 'squared')}
REACHABLE_PATHS = {'mfma', 'gemm', 'st_fused'}          # (+ generic: tests/test_robust_gpu.py runs it on every one of its problems)


def features(r):
    """What distinguishes a row: its problem's shape and regularisers, the request, and the plan it names."""
    c = PROBLEMS[r['problem']]()
    n, k, m, rc = len(c['H0']), len(c['Hops']), len(c['states_concerned_list']), c['reg_coeffs']
    f = dict(mode='st' if c['state_transfer'] else 'u', n=n, controls=k + r['q'], wide=m > 8, vectors=m, long=c['steps'] > 200, E=r['E'], G=r['G'],
             state_reg='forbidden_coeff_list' in rc or 'speed_up' in rc, padded=n % (16 if n <= 64 else 32) != 0, request=r['path'], variant=r['variant'],
             chunks_request=r['chunks'], split_tail=expected_tail(k, c['steps']).startswith('split'))
    f.update({key: r['plan'].get(key) for key in ('path', 'nt', 'expm', 'sweeps', 'route', 'chains', 'taylor_chain')})
    return f


U, ST = dict(mode='u'), dict(mode='st')
# the families an ensemble can run on: each entry must be matched by a row, and every row must be the ONLY match of some entry (so that no row can
# leave the table unnoticed)
FAMILIES = [
    dict(U, path='mfma', nt=2, expm=8, sweeps='downup', controls=5, long=True, E=64, n=32),                        # the measured headline
    dict(U, path='mfma', nt=2, sweeps='downup', controls=5, long=False, G=3, request=AUTO),                         # downup at the k' = 5 edge, several groups
    dict(U, path='mfma', nt=2, sweeps='row_tile_gradient', controls=6),                                             # ... q pushed k' to 6
    dict(U, path='mfma', nt=2, sweeps='pair', state_reg=True, wide=False),
    dict(U, path='mfma', nt=2, sweeps='pair', state_reg=False, wide=True),
    dict(U, path='mfma', nt=3, expm=7, padded=True), dict(U, path='mfma', nt=3, expm=7, n=48),
    dict(U, path='mfma', nt=4, expm=7, n=64, controls=5), dict(U, path='mfma', nt=4, expm=7, padded=True, controls=5),
    dict(U, path='mfma', nt=1, sweeps='one_wave'),
] + [dict(U, request=MFMA, variant=v, chunks_request=ch, expm=EXPM_REPORTED[v]) for v in sorted(REACHABLE_EXPM) for ch in (0, 7)] + [
    dict(U, request=MFMA, controls=8, path='mfma'), dict(ST, request=ST_FUSED, controls=8, path='st_fused'), dict(U, request=AUTO, controls=9, path='gemm'),
    dict(U, path='gemm', route='unitary', chains='persistent', n=40, split_tail=False),
    dict(U, path='gemm', route='unitary', chains='launches', wide=True, n=40),
    dict(U, path='gemm', route='unitary', chains='launches', n=96), dict(U, path='gemm', route='unitary', chains='launches', n=130, padded=True),
    dict(U, path='gemm', route='unitary', chains='persistent', split_tail=True),
    dict(ST, route='direct', taylor_chain='packed', n=64, vectors=1, long=True), dict(ST, route='propagator', chains='persistent', n=64, vectors=1, long=True),
    dict(ST, route='direct', taylor_chain='columns40', n=40), dict(ST, route='direct', taylor_chain='columns48', n=47),
    dict(ST, route='direct', taylor_chain='columns56', n=50), dict(ST, route='direct', taylor_chain='butterfly', vectors=2),
    dict(ST, route='direct', taylor_chain='squared', controls=5), dict(ST, route='direct', taylor_chain='full'),
    dict(ST, route='propagator', chains='launches'),
    dict(ST, path='mfma', nt=2, state_reg=False), dict(ST, path='mfma', nt=2, state_reg=True),
    dict(ST, path='mfma', nt=3, n=40, controls=4, state_reg=False), dict(ST, path='mfma', nt=3, n=40, controls=4, state_reg=True),
]


def test_rows_cover_every_reachable_plan():
    """CPU.  Every kernel family an ensemble can reach is named by a row of FAMILY_ROWS, every AUTO row's plan is what the restated table
    (tests/test_auto_plan.py: expected_plan(ensemble=)) gives for its sizes, and every row's tail is the group view's."""
    plans = [r['plan'] for r in FAMILY_ROWS]
    feats = [features(r) for r in FAMILY_ROWS]
    matches = [[i for i, f in enumerate(feats) if all(f[key] == v for key, v in fam.items())] for fam in FAMILIES]
    for fam, hit in zip(FAMILIES, matches):
        assert hit, 'no row for the family %s' % fam
    for i, r in enumerate(FAMILY_ROWS):
        assert [i] in matches, 'row %s is not the only row of any family' % r['name']
    on_mfma = [p for p in plans if p['path'] == 'mfma']
    assert {p['sweeps'] for p in on_mfma} == REACHABLE_SWEEPS, REACHABLE_SWEEPS - {p['sweeps'] for p in on_mfma}
    assert {p['expm'] for p in on_mfma} == REACHABLE_EXPM, REACHABLE_EXPM - {p['expm'] for p in on_mfma}
    assert {p['nt'] for p in on_mfma} == REACHABLE_NT, REACHABLE_NT - {p['nt'] for p in on_mfma}
    forced = {r['variant'] for r in FAMILY_ROWS if r['path'] == MFMA and r['variant']}
    assert forced == REACHABLE_EXPM, REACHABLE_EXPM - forced                  # every exponential kernel a caller can force
    on_gemm = {(p['route'], p['chains'], p.get('taylor_chain')) for p in plans if p['path'] == 'gemm'}
    assert on_gemm == REACHABLE_GEMM, REACHABLE_GEMM - on_gemm
    assert {p['path'] for p in plans} == REACHABLE_PATHS
    # the lazily formed final state: k_mfma_downup and the GEMM plans of qoc_gemm_lazy_final (unitary mode, chains by launches)
    assert any(p.get('sweeps') == 'downup' for p in plans) and any(p.get('route') == 'unitary' and p.get('chains') == 'launches' for p in plans)
    assert len({r['name'] for r in FAMILY_ROWS}) == len(FAMILY_ROWS)
    for r in FAMILY_ROWS:
        c = PROBLEMS[r['problem']]()
        n, k, steps = len(c['H0']), len(c['Hops']), c['steps']
        assert k + r['q'] <= 9 and r['q'] >= 1, r['name']
        if 'tail' in r['plan']:
            assert r['plan']['tail'] == expected_tail(k, steps), r['name']
        if r['path'] != AUTO:
            continue
        m = len(c['states_concerned_list'])
        rc = c['reg_coeffs']
        want = expected_plan(n, k, m, steps, c['Taylor_terms'][0], r['G'], state_transfer=c['state_transfer'],
                             state_reg='forbidden_coeff_list' in rc or 'speed_up' in rc, hermitian=r['problem'] != 'st_n64_k3_lossy',
                             s=c['Taylor_terms'][1], ensemble=(r['E'], r['q']))
        for key, value in r['plan'].items():
            if key in want:
                assert want[key] == value, (r['name'], key, value, want)
        assert want['path'] == r['plan']['path'], (r['name'], want)


# ---- the composed oracle, once per (problem, ensemble, control sets) ----------------------------------------------------------------------------

_SYSTEMS, _EXPECT = {}, {}


def start_bases(sp, G):
    """G distinct starting points: bases_for's three, then seeded draws of the same scale."""
    out = list(bases_for(sp, min(G, 3)))
    rng = np.random.default_rng(1000 + G)
    while len(out) < G:
        out.append(rng.normal(0, 1 / np.sqrt(sp.steps), sp.base0.shape))
    return np.stack(out)


def systems(problem, E, q, ens=None, key=None):
    """(case, validated ensemble, nominal system, member systems) of a problem, cached."""
    key = (problem, E, q) if key is None else key
    if key not in _SYSTEMS:
        c = PROBLEMS[problem]()
        ens = ensemble(c, E, q) if ens is None else ens
        nominal = nominal_system(c)
        _SYSTEMS[key] = (c, ens, nominal, member_systems(c, ens, (nominal.exp_terms, nominal.scaling)))
    return _SYSTEMS[key]


def expectation(sps, w, base):
    """composed() with what the read-backs need: every member's reg_state and final unitary, member 0's inter_vecs."""
    o = composed(sps, w, base, want_inter=True)
    reg = []
    for sp, r in zip(sps, o['members']):
        need = 'forbidden_coeff_list' in sp.reg_coeffs or 'speed_up' in sp.reg_coeffs
        reg.append(go.state_regularisers(sp, r['inter_vecs'])[0] if need else 0.0)
    o['member_reg_state'] = np.array(reg)
    o['member_U'] = None if sps[0].state_transfer else np.stack([r['U_final'] for r in o['members']])
    o['inter0'] = o['members'][0]['inter_vecs']
    del o['members']                                          # (the other members' vectors: 130 MB at C2 x 64)
    return o


def expected(key, sps, w, bases):
    if key not in _EXPECT:
        _EXPECT[key] = [expectation(sps, w, b) for b in bases]
    return _EXPECT[key]


def assert_plan(eng, r, c, ens):
    got = {key: (int(v) if v.lstrip('-').isdigit() else v) for key, v in eng.plan.items()}
    for key, want in r['plan'].items():
        assert got.get(key) == want, (r['name'], key, want, got)
    assert got['tail'] == expected_tail(len(c['Hops']), c['steps']), got
    assert got['members'] == len(ens['weights']) and got['perturbations'] == len(ens['operators']), got
    return got


def compare_group(tol, g, o, r, ms, Uf, mUf, inter, groups=None):
    """Control set g of an evaluation `r` (and the read-backs after it) against its expectation `o`."""
    i = g if groups is None else groups.index(g)             # (heavy read-backs may be sampled: `groups` lists the control sets they hold)
    for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale'):
        print('  group %d %s: |device - oracle| = %.3e (oracle %.6e)' % (g, key, abs(r[key][g] - o[key]), o[key]))
        assert abs(r[key][g] - o[key]) <= tol['s'] * max(1.0, abs(o[key])), (key, g, r[key][g], o[key])
    gm = max(1.0, float(np.max(np.abs(o['grad']))))
    print('  group %d gradient: %.3e (max|grad| %.3e)' % (g, np.max(np.abs(r['grad'][g] - o['grad'])), np.max(np.abs(o['grad']))))
    assert np.max(np.abs(r['grad'][g] - o['grad'])) <= tol['g'] * gm, (g, np.max(np.abs(r['grad'][g] - o['grad'])), gm)
    for key, want in (('loss', o['member_loss']), ('reg_state', o['member_reg_state'])):
        err = np.max(np.abs(ms[key][g] - want))
        print('  group %d member %s: %.3e' % (g, key, err))
        assert err <= tol['s'] * max(1.0, np.max(np.abs(want))), (key, g, ms[key][g], want)
    if inter is not None:
        err = np.max(np.abs(inter[i] - o['inter0']))
        print('  group %d inter_vecs: %.3e' % (g, err))
        assert err <= tol['u'] * max(1.0, np.max(np.abs(o['inter0']))), (g, err)
    if o['member_U'] is not None and Uf is not None:
        e0, ee = np.max(np.abs(Uf[i] - o['member_U'][0])), np.max(np.abs(mUf[i] - o['member_U']), axis=(1, 2))
        print('  group %d final unitary: member 0 %.3e, worst member %.3e' % (g, e0, ee.max()))
        assert e0 <= tol['u'] and np.all(ee <= tol['u']), (g, e0, ee)


def check_row(r, ens=None, key=None):
    if ens is None and r['ens'] is not None:
        ens, key = r['ens'](), (r['problem'], r['name'])
    c, ens, nominal, sps = systems(r['problem'], r['E'], r['q'], ens, key)
    assert (len(ens['weights']), len(ens['operators'])) == (r['E'], r['q']), r['name']
    G, w, tol = r['G'], ens['weights'], tolerances(c['steps'])
    eng = make_engine(nominal, G, ens, r['path'], r['variant'], r['chunks'])
    try:
        assert_plan(eng, r, c, ens)
        bases = start_bases(nominal, G)
        exp = expected((key or (r['problem'], r['E'], r['q']), G), sps, w, bases)
        eng.set_base(bases)
        res = eng.evaluate()
        ms = eng.member_scalars()
        unitary = not nominal.state_transfer
        Uf, mUf = (eng.get_final_unitary(), eng.member_final_unitary()) if unitary else (None, None)
        inter = eng.get_inter_vecs()
        uks = eng.get_uks()
        print(r['name'], eng.plan)
        for g in range(G):
            compare_group(tol, g, exp[g], res, ms, Uf, mUf, inter)
            want = nominal.maxA[:, None] * np.sin(bases[g])
            assert np.max(np.abs(uks[g] - want)) <= TIGHT['u'] * max(1.0, np.max(nominal.maxA)), (g, np.max(np.abs(uks[g] - want)))
        # one explicit step: the tail on the group view (after get_uks: the controls of the next evaluation are already formed)
        lrs = np.array([0.02, 0.01, 0.005, 0.03] * G)[:G]
        eng.adam_step(lrs)
        base = eng.get_base()
        for g in range(G):
            want = go.Adam(bases[g].shape).step(bases[g], exp[g]['grad'], lrs[g])
            print('  group %d base after one step: %.3e' % (g, np.max(np.abs(base[g] - want))))
            assert np.max(np.abs(base[g] - want)) <= STEP_ATOL, (g, np.max(np.abs(base[g] - want)))
        # a second step evaluates at the moved bases and leaves the lazily formed buffers stale: the members' final unitaries FIRST, then the
        # vectors and the members' scalars, of the last control set, against the oracle at the bases the device evaluated
        eng.adam_step(lrs)
        mUf = eng.member_final_unitary() if unitary else None
        inter, ms = eng.get_inter_vecs(), eng.member_scalars()
        Uf = eng.get_final_unitary() if unitary else None
        g = G - 1
        o = expectation(sps, w, base[g])
        for key, want in (('loss', o['member_loss']), ('reg_state', o['member_reg_state'])):
            assert np.max(np.abs(ms[key][g] - want)) <= tol['s'] * max(1.0, np.max(np.abs(want))), ('after steps', key, ms[key][g], want)
        err = np.max(np.abs(inter[g] - o['inter0']))
        print('  after two steps, group %d inter_vecs: %.3e' % (g, err))
        assert err <= tol['u'] * max(1.0, np.max(np.abs(o['inter0']))), ('after steps', err)
        if unitary:
            ee = np.max(np.abs(mUf[g] - o['member_U']), axis=(1, 2))
            print('  after two steps, group %d member final unitaries: %.3e' % (g, ee.max()))
            assert np.all(ee <= tol['u']) and np.max(np.abs(Uf[g] - o['member_U'][0])) <= tol['u'], ('after steps', ee)
    finally:
        eng.close()


# ---- 1. one row per kernel family ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('r', FAMILY_ROWS, ids=[r['name'] for r in FAMILY_ROWS])
def test_family_against_the_composed_oracle(r):
    check_row(r)


# ---- 3. the device loop on the families with lazy or shared state -------------------------------------------------------------------------------

# (row, learning rate, starting points: bases_for's three, or three near the nominal draw) -- chosen on the oracle alone so that the losses fall and cross
LOOP_ROWS = [
    (row('loop_downup', 'n24_k4_pulse_regs', 3, 1, 3, mfma(2, 8, 'downup')), 0.02, 'spread'),
    (row('loop_row_tile_gradient_nt3', 'n48_k3', 3, 1, 3, mfma(3, 7, 'row_tile_gradient')), 0.05, 'spread'),
    (row('loop_gemm_unitary_persistent', 'n40_k3_m6', 2, 1, 3, gemm('unitary', 'persistent')), 0.1, 'near'),
    (row('loop_gemm_unitary_lazy_final', 'n40_k3_m12', 2, 1, 3, gemm('unitary', 'launches')), 0.02, 'spread'),
    (row('loop_direct_state_transfer', 'st_n40_k4', 4, 1, 3, gemm('direct', 'persistent', taylor_chain='columns40')), 0.02, 'spread'),
]
LOOP_MAX = 11


@pytest.mark.gpu
@pytest.mark.parametrize('r,rate,spread', LOOP_ROWS, ids=[r[0]['name'] for r in LOOP_ROWS])
def test_loop_against_the_composed_oracle(r, rate, spread):
    """run_adam, three control sets, a conv_target (tests/test_adam_tail.py: _choose_target) at which they stop at different iterations inside a
    burst (poll_every divides none of them).  Iterations, bases (1e-9) and final scalars (1e-10) against python_loop over the composed oracle;
    then every control set's member_scalars / member_final_unitary / get_inter_vecs against the oracle AT THE DEVICE'S OWN final base of that
    control set (evaluation tolerances: a stopped control set is not moved, so these are the read-backs of its last evaluation -- one of a later
    iteration of the others would be off by a whole Adam step)."""
    c, ens, nominal, sps = systems(r['problem'], r['E'], r['q'])
    w, G, tol = ens['weights'], r['G'], tolerances(c['steps'])
    b0 = nominal.base0
    bases = start_bases(nominal, G) if spread == 'spread' else np.stack([b0, 0.85 * b0 + 0.03, 1.15 * b0 - 0.03])
    conv = dict(rate=rate, learning_rate_decay=50, conv_target=-1.0, min_grad=-1.0, max_iterations=LOOP_MAX)
    free = [python_loop(sps, w, b, conv) for b in bases]
    target, stops = _choose_target([f['history'] for f in free], LOOP_MAX)
    conv['conv_target'] = target
    refs = [f if s == LOOP_MAX else python_loop(sps, w, b, conv) for f, s, b in zip(free, stops, bases)]
    assert [ref['iterations'] for ref in refs] == stops and len(set(stops)) == 3 and 0 < min(stops) and max(stops) == LOOP_MAX, stops
    poll = next(p for p in (5, 4, 7, 3, 6) if all(s % p for s in stops if s))
    eng = make_engine(nominal, G, ens, r['path'], r['variant'], r['chunks'])
    try:
        assert_plan(eng, r, c, ens)
        eng.set_base(bases)
        its = eng.run_adam(eng.adam_params(poll_every=poll, **conv))
        # first read-back after the loop, before anything else refreshes the lazily formed final states (k_mfma_downup, qoc_gemm_lazy_final)
        unitary = not nominal.state_transfer
        mUf = eng.member_final_unitary() if unitary else None
        inter = eng.get_inter_vecs()
        s = eng.scalars()
        base = eng.get_base()
        print(r['name'], eng.plan, 'stops', stops, 'poll', poll)
        assert list(its) == stops and list(s['iterations']) == stops and list(s['done']) == [1] * G, (its, stops)
        for g, ref in enumerate(refs):
            print('  group %d base: %.3e' % (g, np.max(np.abs(base[g] - ref['base']))))
            assert np.max(np.abs(base[g] - ref['base'])) < STEP_ATOL, (g, np.max(np.abs(base[g] - ref['base'])))
            for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale'):
                assert abs(s[key][g] - ref['last'][key]) < 1e-10 * max(1.0, abs(ref['last'][key])), (key, g, s[key][g], ref['last'][key])
        ms = eng.member_scalars()
        Uf = eng.get_final_unitary() if unitary else None
        for g in range(G):
            o = expectation(sps, w, base[g])
            res = dict(s, grad=None)
            for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale'):
                assert abs(res[key][g] - o[key]) <= tol['s'] * max(1.0, abs(o[key])), (key, g, res[key][g], o[key])
            for key, want in (('loss', o['member_loss']), ('reg_state', o['member_reg_state'])):
                assert np.max(np.abs(ms[key][g] - want)) <= tol['s'] * max(1.0, np.max(np.abs(want))), (key, g, ms[key][g], want)
            err = np.max(np.abs(inter[g] - o['inter0']))
            print('  group %d (stopped at %d) inter_vecs: %.3e' % (g, stops[g], err))
            assert err <= tol['u'] * max(1.0, np.max(np.abs(o['inter0']))), (g, stops[g], err)
            if unitary:
                ee = np.max(np.abs(mUf[g] - o['member_U']), axis=(1, 2))
                print('  group %d member final unitaries: %.3e' % (g, ee.max()))
                assert np.all(ee <= tol['u']) and np.max(np.abs(Uf[g] - o['member_U'][0])) <= tol['u'], (g, stops[g], ee)
    finally:
        eng.close()


# ---- 4. edges of the glue kernels ---------------------------------------------------------------------------------------------------------------

def _custom(problem, operators_from, offsets, amp_scales, weights):
    c = PROBLEMS[problem]()
    n, k = len(c['H0']), len(c['Hops'])
    return rb.validate(dict(operators=operators_from['operators'], offsets=offsets, amp_scales=amp_scales, weights=weights), n, k)


@pytest.mark.gpu
def test_member_of_weight_zero():
    """A member of weight 0 changes nothing for its control sets (they equal the ensemble without it), and its own loss, reg_state and final unitary are
    still reported."""
    c = PROBLEMS['n8_k2']()
    full = ensemble(c, 3, 1)
    wt = full['weights'].copy()
    wt[1] = 0.0
    ens0 = _custom('n8_k2', full, full['offsets'], full['amp_scales'], wt)
    keep = [0, 2]
    ens2 = _custom('n8_k2', full, full['offsets'][keep], full['amp_scales'][keep], wt[keep])
    assert ens0['weights'][1] == 0.0 and np.array_equal(ens0['weights'][keep], ens2['weights'])
    r = row('weight_zero', 'n8_k2', 3, 1, 2, dict(path='mfma', nt=1))
    check_row(r, ens=ens0, key=('n8_k2', 'weight_zero'))               # (the composition carries the member with weight 0: its own quantities are compared)
    _, _, nominal, sps2 = systems('n8_k2', 2, 1, ens=ens2, key=('n8_k2', 'weight_zero_without'))
    bases = start_bases(nominal, 2)
    eng = make_engine(nominal, 2, ens0)
    try:
        eng.set_base(bases)
        res = eng.evaluate()
        for g in range(2):
            o = composed(sps2, ens2['weights'], bases[g])
            for key in ('loss', 'reg_loss', 'grad_squared', 'unitary_scale'):
                assert abs(res[key][g] - o[key]) <= TIGHT['s'] * max(1.0, abs(o[key])), (key, g, res[key][g], o[key])
            assert np.max(np.abs(res['grad'][g] - o['grad'])) <= TIGHT['g'] * max(1.0, np.max(np.abs(o['grad'])))
    finally:
        eng.close()


@pytest.mark.gpu
def test_one_perturbed_member_is_the_plain_oracle_of_the_perturbed_hamiltonian():
    """E = 1, q = 2, non-zero offsets and scales: not the nominal member."""
    c = PROBLEMS['n8_k2']()
    ens = _custom('n8_k2', ensemble(c, 2, 2), [[0.15, -0.1]], [[1.05, 0.93]], [1.0])
    H0e, Hopse = rb.member_hamiltonians(c['H0'], c['Hops'], ens, 0)
    assert np.max(np.abs(H0e - c['H0'])) > 1e-2 and ens['weights'][0] == 1.0
    check_row(row('one_perturbed_member', 'n8_k2', 1, 2, 3, dict(path='mfma', nt=1)), ens=ens, key=('n8_k2', 'one_perturbed'))


@pytest.mark.gpu
def test_scales_and_offsets_of_either_sign_and_a_scale_of_exactly_zero():
    """Scales that differ per control and per member, negative offsets, and amp_scales[1][0] == 0: member 1 then contributes EXACTLY nothing to the
    gradient of control 0 (k_ens_reduce multiplies by w_e a[e][j]) -- changing member 1's other scale and its offsets moves its trajectory, and row 0
    of the control sets' gradient keeps every bit while row 1 moves."""
    c = PROBLEMS['n8_k2']()
    src = ensemble(c, 3, 2)
    off = np.array([[0.2, -0.15], [-0.1, 0.05], [-0.2, -0.05]])
    amp = np.array([[1.1, 0.8], [0.0, 1.2], [0.95, -0.7]])
    wt = [0.5, 1.5, 1.0]
    ens_a = _custom('n8_k2', src, off, amp, wt)
    off_b, amp_b = off.copy(), amp.copy()
    off_b[1] = [0.17, -0.12]
    amp_b[1, 1] = 0.9
    ens_b = _custom('n8_k2', src, off_b, amp_b, wt)
    r = row('zero_scale', 'n8_k2', 3, 2, 3, dict(path='mfma', nt=1))
    check_row(r, ens=ens_a, key=('n8_k2', 'zero_scale_a'))
    check_row(r, ens=ens_b, key=('n8_k2', 'zero_scale_b'))
    nominal = nominal_system(c)
    bases = start_bases(nominal, 3)
    grads = []
    for ens in (ens_a, ens_b):
        eng = make_engine(nominal, 3, ens)
        try:
            eng.set_base(bases)
            grads.append(eng.evaluate()['grad'])
        finally:
            eng.close()
    assert np.array_equal(grads[0][:, 0], grads[1][:, 0])
    assert np.max(np.abs(grads[0][:, 1] - grads[1][:, 1])) > 1e-6


BIG_G, BIG_E = 512, 3


@pytest.mark.gpu
def test_more_items_than_one_pass_of_the_expand_grid():
    """k_ens_expand walks G (k + q) steps items with a grid capped at 2048 x 256 = 524 288 threads: 512 control sets x 3 rows x 400 slices = 614 400
    items, so the control sets from 436 on are written in the second pass.  Scalars (loss, reg_loss, unitary_scale; no gradient on the oracle side) of
    ALL control sets; the gradient and the full read-backs of eight of them -- the first, the last, and those around item 524 288 (control set 436)."""
    c, ens, nominal, sps = systems('qubit_400', BIG_E, 1)
    kp, steps = len(c['Hops']) + 1, c['steps']
    assert BIG_G * kp * steps > 2048 * 256
    edge = (2048 * 256) // (kp * steps)
    assert edge == 436
    sample = [0, 1, edge - 2, edge - 1, edge, edge + 1, BIG_G - 2, BIG_G - 1]
    w = ens['weights']
    bases = start_bases(nominal, BIG_G)
    eng = make_engine(nominal, BIG_G, ens)
    try:
        got = assert_plan(eng, row('big', 'qubit_400', BIG_E, 1, BIG_G, dict(path='mfma', nt=1, expm=1, sweeps='one_wave')), c, ens)
        want = expected_plan(2, 2, 2, steps, c['Taylor_terms'][0], BIG_G, ensemble=(BIG_E, 1))
        assert all(got[key] == v for key, v in want.items()), (got, want)
        eng.set_base(bases)
        res = eng.evaluate()
        ms = eng.member_scalars()
        Uf, mUf, inter = eng.get_final_unitary()[sample], eng.member_final_unitary()[sample], eng.get_inter_vecs()[sample]
        uks = eng.get_uks()
        assert np.max(np.abs(uks - nominal.maxA[None, :, None] * np.sin(bases))) <= TIGHT['u']
        tol = tolerances(steps)
        for g in range(BIG_G):
            if g in sample:
                compare_group(tol, g, expectation(sps, w, bases[g]), res, ms, Uf, mUf, inter, groups=sample)
                continue
            rs = [go.evaluate(sp, bases[g], want_grad=False) for sp in sps]
            for key in ('loss', 'reg_loss', 'unitary_scale'):
                o = sum(wi * r[key] for wi, r in zip(w, rs))
                assert abs(res[key][g] - o) <= tol['s'] * max(1.0, abs(o)), (key, g, res[key][g], o)
            assert np.max(np.abs(ms['loss'][g] - np.array([r['loss'] for r in rs]))) <= tol['s']
    finally:
        eng.close()


# ---- 5. Grape(robust=...) end to end ------------------------------------------------------------------------------------------------------------

def grape_problem():
    """Two-transmon-sized, a forbidden level (tests/test_robust_gpu.py: _auto_case('two_transmon')), automatic Taylor order."""
    c = cases.case_c2(n=9, k=2, steps=60, m=9, taylor=None, seed=3)
    c['total_time'] = 3.0
    c['reg_coeffs'] = {'forbidden_coeff_list': [10.0], 'states_forbidden_list': [8], 'dwdt': 0.01}
    return c


GRAPE_CONV = {'rate': 0.02, 'update_step': 7, 'max_iterations': 20, 'conv_target': 1e-12, 'learning_rate_decay': 100}


def grape_reference(c, ens, restarts, unitary_error=1e-4):
    """What Grape(robust=ens, restarts=R, method='Adam') must return, from python_loop over the composed oracle: the starting points are HipState's
    (restart 0: the reference's own draw; the others parallel_seeds.restart_guesses), the Taylor order robust.choose_taylor's."""
    from quantum_optimal_control.parallel_seeds import restart_guesses
    U0 = np.identity(len(c['H0']))
    taylor = rb.choose_taylor(c['H0'], c['Hops'], ens, c['maxA'], U0, c['total_time'], c['steps'], unitary_error, False, False)
    sps = member_systems(dict(c, Taylor_terms=list(taylor)), ens, taylor)
    k, steps = sps[0].base0.shape
    bases = np.concatenate([sps[0].base0[None], restart_guesses(k, steps, 1, restarts - 1)], axis=0)
    conv = dict(rate=GRAPE_CONV['rate'], learning_rate_decay=GRAPE_CONV['learning_rate_decay'], conv_target=GRAPE_CONV['conv_target'], min_grad=1e-25,
                max_iterations=GRAPE_CONV['max_iterations'])
    runs = [python_loop(sps, ens['weights'], b, conv) for b in bases]
    best = int(np.argmin([run['last']['loss'] for run in runs]))
    return sps, runs, best, taylor


@pytest.mark.gpu
def test_grape_robust_restarts_returns_the_winning_seed_of_the_composed_oracle():
    """uks and U_final of Grape(robust=, restarts=3, Taylor_terms=None) against the winner of three python_loop runs; the summary line names the
    oracle's worst member.  Bounds: a base after the loop agrees to 1e-9 (STEP_ATOL), so uks = maxA sin(base) to max(maxA) x 1e-9, and U_final, whose
    derivative with respect to one control value is bounded by dt ||H_j||, to 1e-12 + 1e-9 x dt x sum_j maxA_j ||H_j|| x slices."""
    from quantum_optimal_control.main_grape.grape import Grape
    from tests.helpers import grape_kwargs
    c = grape_problem()
    ens = ensemble(c, 4, 1)
    sps, runs, best, taylor = grape_reference(c, ens, 3)
    losses = sorted(run['last']['loss'] for run in runs)
    assert losses[1] - losses[0] > 1e-6, losses                        # the winner is not decided by round-off
    np.random.seed(c['np_seed'])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        uks, Uf = Grape(convergence=dict(GRAPE_CONV), method='Adam', restarts=3, robust=ens, **grape_kwargs(c))
    ref = runs[best]
    o = expectation(sps, ens['weights'], ref['base'])
    maxA = np.asarray(c['maxA'], dtype=float)
    err_u = np.max(np.abs(uks - maxA[:, None] * np.sin(ref['base'])))
    lip = (c['total_time'] / c['steps']) * sum(a * np.linalg.norm(h, 2) for a, h in zip(maxA, c['Hops'])) * c['steps']
    err_U = np.max(np.abs(Uf - o['member_U'][0]))
    print('Taylor %s, winner %d of losses %s; uks %.3e, U_final %.3e (bound %.3e)' % (taylor, best, losses, err_u, err_U, 1e-12 + STEP_ATOL * lip))
    assert err_u <= STEP_ATOL * maxA.max(), err_u
    assert err_U <= 1e-12 + STEP_ATOL * lip, (err_U, lip)
    line = [ln for ln in out.getvalue().splitlines() if ln.startswith('Robust ensemble:')]
    assert len(line) == 1, out.getvalue()
    mt = re.match(r'Robust ensemble: (\d+) members, weighted mean infidelity (\S+), worst member infidelity (\S+) \(member (\d+)\)', line[0])
    worst = int(np.argmax(o['member_loss']))
    margin = np.sort(o['member_loss'])
    assert margin[-1] - margin[-2] > 1e-6, margin                      # ... nor the worst member
    assert mt and int(mt.group(1)) == 4 and int(mt.group(4)) == worst, (line, o['member_loss'])
    assert abs(float(mt.group(2)) - o['loss']) <= 2e-3 * o['loss'] and abs(float(mt.group(3)) - o['member_loss'][worst]) <= 2e-3 * o['member_loss'][worst], line
