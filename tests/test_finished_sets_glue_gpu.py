"""Finished control sets beyond plain engines: ensembles, risk, lines, control maps, fleets, the exact gradient, sparse and open engines.

tests/test_finished_sets_gpu.py pins the contract of QocDev::skip_done on plain engines.  The features beside them added kernels that either carry
their own skip branch (k_ens_reduce, k_ens_tilt, k_ens_reduce_risk, k_shape_reduce<1|64>, k_shape_reduce_risk, k_sp_forward, k_sp_backward,
k_sp_grad, k_lb_forward, k_lb_backward, k_lb_reduce) or deliberately have none (k_ens_expand, k_shape_expand, k_map_expand, k_map_reduce,
k_exact_grad, k_bwd_store, the generic sweeps): those are right only if rewriting a finished set's rows from its kept controls gives the same bits at
every iteration.  Here every such kind runs the five checks of that module (check_row) through an Adapter whose reference is the kind's own:

  composed kinds (ensemble, risk, line, map, exact gradient, any mix of them)   tests/control_map_reference.py: evaluate, and run_adam over it
  fleets                                                                        tests/fleet_reference.py: the same with device g // R's rows
  ensembles on the MFMA and GEMM families                                       tests/test_robust_families.py: python_loop, expectation
  sparse                                                                        go.run_adam on sr.dense_oracle(sp); sr.evaluate for the read-backs
  open systems                                                                  tests/lindblad_reference.py: run_adam, evaluate

and whose snapshot holds the read-backs that exist only there, all of them frozen bit for bit (FROZEN): member_scalars, member_final_unitary (read
FIRST: it is lazily formed), member_weights, get_coefficients, get_pulse, get_final_density, get_populations.  Check 5 compares the whole snapshot
after set_base and the same loop, which includes the members' done flags k_ens_expand mirrors.

Tolerances are the project's: the loop's outcome at LOOP_ATOL where the kind's own loop test uses it (sparse, open), bases < 1e-9 and scalars < 1e-10
where tests/test_robust_families.py and tests/test_fleet_gpu.py use those (everything with members, lines, maps); the read-backs at TIGHT of
tests/test_robust_families.py, and at S_RTOL / U_ATOL of tests/test_hip_parity.py on sparse and open engines.

The second half holds the same contract under the L-BFGS loop, which evaluates with skip_done = 0: finished sets ARE evaluated again at every
iteration, on every path, and must come out with the same bits; and a run that ends by RESTORE must leave the read-backs of x_acc.

Shapes: n = 5, 8 slices, six control sets (a fleet: F = 3, R = 2), rate 0.1, starts drawn as default_rng(8).normal(0, 0.7); a family that needs
more has it (k_shape_reduce<64>: columns of 36 slices; the MFMA and GEMM rows: the loop problems of tests/test_robust_families.py; sparse: n = 24,
257 and 1025).  The stop values are chosen on the references alone and asserted without a device (test_stop_values_meet_the_conditions).
"""
import functools

import numpy as np
import pytest

from oracle import grape_oracle as go
from quantum_optimal_control.core import hip_engine as P
from quantum_optimal_control.helper_functions import control_map as cmap
from quantum_optimal_control.helper_functions import transfer as tf
from tests import control_map_reference as ref
from tests import fleet_reference as fr
from tests import lbfgs_reference as lb
from tests import lindblad_reference as lr
from tests import sparse_reference as sr
from tests import test_finished_sets_gpu as fs
from tests import test_lbfgs_gpu as lg
from tests import test_robust_families as rf
from tests.test_adam_tail import LOOP_ATOL
from tests.test_finished_sets_gpu import MAX_IT, RULES, Adapter, check_row, check_stop_values, snapshot, start_bases
from tests.test_hip_parity import S_RTOL, U_ATOL
from tests.test_robust_families import TIGHT
from tests.test_robust_gpu import make_engine as ensemble_engine
from tests.test_robust_gpu import python_loop

GLUE_LOOP = dict(vectors=1e-9, scalars=1e-10, strict=True)      # tests/test_robust_families.py, tests/test_fleet_gpu.py: `< 1e-9`, `< 1e-10 max(1, |x|)`
EXACT_LOOP = dict(vectors=LOOP_ATOL, scalars=LOOP_ATOL, strict=False)
SCALARS = ('loss', 'reg_loss', 'grad_squared', 'unitary_scale')
GLUE_READ = dict(dict.fromkeys(SCALARS, TIGHT['s']), member_loss=TIGHT['s'], weights=TIGHT['s'], final=TIGHT['u'], member_final=TIGHT['u'],
                 inter=TIGHT['u'], coefficients=TIGHT['g'], pulse=TIGHT['g'])
REGS = {'dwdt': 0.1, 'amplitude': 0.2, 'forbidden_coeff_list': [5.0], 'states_forbidden_list': [3], 'speed_up': 0.3}       # tests/test_control_map_gpu.py
N, STEPS, SETS, F, R = 5, 8, 6, 3, 2
CONV = dict(max_iterations=MAX_IT, learning_rate_decay=100, conv_target=-1.0, min_grad=-1.0)


# ---- 1. the composed kinds ------------------------------------------------------------------------------------------------------------------------

def glue(name, kernels, kind='unitary', steps=STEPS, Eq=None, beta=0.0, line=None, mapped=None, fleet=None, exact=False, path=P.PATH_GENERIC, plan=None,
         rate=0.1, seed=0, start=8):
    """One row of a composed kind.  Eq: (members, perturbations) of the ensemble, or of every device of the fleet; line: the samples P of tf.hold(steps,
    P); mapped: (k, r, D) of a map with M and F; fleet: (devices, control sets per device); kernels: the glue kernels the row is there for."""
    return dict(name=name, kernels=set(kernels), kind=kind, steps=steps, Eq=Eq, beta=beta, line=line, mapped=mapped, fleet=fleet, exact=exact, path=path,
                plan=dict(path='generic') if plan is None else plan, rate=rate, seed=seed, start=start)


ENS, RISK = {'k_ens_expand', 'k_ens_reduce'}, {'k_ens_expand', 'k_ens_tilt', 'k_ens_reduce_risk'}
ALL = {'k_shape_expand', 'k_map_expand', 'k_map_reduce', 'k_ens_tilt', 'k_shape_reduce_risk'}

GLUE_ROWS = [
    glue('ensemble_E3_q1', ENS, Eq=(3, 1)),
    glue('risk_beta4', RISK, Eq=(3, 1), beta=4.0),
    glue('line_hold_8_4', {'k_shape_expand', 'k_shape_reduce<1>'}, line=4),
    glue('line_columns_of_36_slices', {'k_shape_expand', 'k_shape_reduce<64>'}, steps=72, line=2),
    glue('map_k2_r3_D3_MF', {'k_map_expand', 'k_map_reduce'}, mapped=(2, 3, 3)),
    glue('fleet_F3_R2_E2_q1', ENS | {'fleet'}, Eq=(2, 1), fleet=(F, R)),
    glue('exact_gradient_unitary', {'k_exact_grad', 'k_bwd_store'}, exact=True),
    glue('exact_gradient_state_transfer', {'k_exact_grad', 'k_bwd_store'}, kind='state', exact=True),
    glue('all_map_E3_q1_risk_line', ALL, Eq=(3, 1), beta=4.0, line=4, mapped=(2, 3, 3)),
    glue('all_in_a_fleet', ALL | {'fleet'}, Eq=(3, 1), beta=4.0, line=4, mapped=(2, 3, 3), fleet=(F, R)),
    # the composition on the two matrix-instruction families an ensemble of n = 5 runs on (tests/test_control_map_gpu.py: FAMILIES)
    glue('all_on_mfma_nt1', ALL, Eq=(3, 1), beta=4.0, line=4, mapped=(2, 3, 3), path=P.PATH_MFMA, plan=dict(path='mfma', nt='1')),
    glue('all_on_gemm_unitary', ALL, Eq=(3, 1), beta=4.0, line=4, mapped=(2, 3, 3), path=P.PATH_GEMM, plan=dict(path='gemm', route='unitary')),
]


@functools.lru_cache(maxsize=None)
def glue_parts(name):
    """(problem, the reference's map, the engine's map, ensemble per control set, fleet, line matrix) of a row."""
    g = next(row for row in GLUE_ROWS if row['name'] == name)
    k, r, D = g['mapped'] or (2, 2, 1)
    state = g['kind'] == 'state'
    c = ref.problem(N, r, k, g['steps'], 2 if state else 3, state_transfer=state, taylor=(8, 0) if state else (6, 1), seed=30 + g['seed'], regs=REGS)
    cm = ref.make_map(k, r, D, g['steps'], mix=True, fixed=True) if g['mapped'] else None
    ref_map = cm if cm is not None else cmap.validate(cmap.identity(k), k=k, r=k, steps=g['steps'])     # (bit-identical to no map: tests/test_control_map_gpu.py)
    T = tf.hold(g['steps'], g['line']).matrix if g['line'] else None
    fl = None
    if g['fleet']:
        fl = fr.make_fleet(c, g['fleet'][0], *g['Eq'], risk=g['beta'])
        members = [fr.device(fl, b // g['fleet'][1]) for b in range(SETS)]
    else:
        members = [ref.ensemble(c, *g['Eq']) if g['Eq'] else ref.ensemble(c, 1, 0)] * SETS
    return g, c, ref_map, cm, members, fl, T


def glue_engine(name, n_sets):
    g, c, _, cm, members, fl, T = glue_parts(name)
    sp = ref.engine_system(c)
    ens = dict(members[0], risk=g['beta']) if g['Eq'] and fl is None else None
    eng = P.HipEngine(sp.Hs, sp.U0, sp.V, sp.W, c['maxA'], sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling, state_transfer=sp.state_transfer,
                      reg_coeffs=c['reg_coeffs'], n_seeds=n_sets, path=g['path'], ensemble=ens, transfer=T, exact_gradient=g['exact'], control_map=cm, fleet=fl)
    want = dict(g['plan'])
    if g['Eq']:
        want.update(members=str(g['Eq'][0]), perturbations=str(g['Eq'][1]))
    if fl is not None:
        want.update(devices=str(fl.n_devices))
    if cm is not None:
        want.update(terms=str(cm.n_terms), degree=str(cm.degree))
    if T is not None:
        want.update(samples=str(T.shape[1]))
    if g['exact']:
        want.update(gradient='exact')
    for key, word in want.items():
        assert eng.plan.get(key) == word, (name, key, word, eng.plan)
    assert eng.risk == (g['beta'] if g['Eq'] else 0.0) and eng.members == (g['Eq'][0] if g['Eq'] else 0), (eng.risk, eng.members)
    return eng


def glue_snapshot(eng):
    """The members' final unitaries FIRST (lazily formed, like the final unitary that snapshot() reads next), then what every engine has, then the
    read-backs of ensembles, maps and lines."""
    unitary = not eng.state_transfer
    out = {}
    if eng.members and unitary:
        out['member_final'] = eng.member_final_unitary()
    out.update(snapshot(eng, unitary))
    if eng.members:
        ms = eng.member_scalars()
        out.update(member_loss=ms['loss'], member_reg_state=ms['reg_state'], weights=eng.member_weights())
    if 'terms' in eng.plan:
        out['coefficients'] = eng.get_coefficients()
    if eng.samples is not None:
        out['pulse'] = eng.get_pulse()
    return out


def glue_adapter(name):
    g, c, ref_map, cm, members, fl, T = glue_parts(name)

    def evaluate(x, b):
        return ref.evaluate(c, ref_map, members[b], x, T=T, exact=g['exact'], beta=g['beta'])

    def loop(conv, x0, b):
        run = ref.run_adam(lambda x: evaluate(x, b), x0, conv)
        return dict(base=run['base'], iterations=run['iterations'], history=run['history'], vectors=dict(base=run['base']),
                    scalars={key: run['last'][key] for key in SCALARS})

    def at_base(base, b):
        o = evaluate(base, b)
        out = {key: o[key] for key in SCALARS}
        out['inter'] = o['inter_vecs']
        if not c['state_transfer']:
            out['final'] = o['U_final']
        if g['Eq']:
            out.update(member_loss=o['member_loss'], weights=o['weights'])
            if not c['state_transfer']:
                out['member_final'] = o['member_U']
        if cm is not None:
            out['coefficients'] = o['coefficients']
        if T is not None:
            out['pulse'] = o['pulse']
        return out

    width = g['line'] or g['steps']
    return Adapter(key=('glue', name), batch=SETS, starts=lambda: np.random.default_rng(g['start']).normal(0.0, 0.7, size=(SETS, len(c['maxA']), width)),
                   conv=dict(CONV, rate=g['rate']), build=lambda n_sets: glue_engine(name, n_sets), loop=loop, at=at_base, snapshot=glue_snapshot,
                   loop_tol=GLUE_LOOP, read_tol=GLUE_READ, full_again=True)


# ---- 2. an ensemble E3 q1 on the families of tests/test_robust_families.py: LOOP_ROWS (that file's problems and plan assertions) ------------------

# (six control sets of three members are 18 trajectories of n = 40, which AUTO gives to the MFMA path: the GEMM unitary route is asked for by name)
FAMILY_ROWS = [dict(row=dict(r, E=3, q=1, G=SETS, name='E3_q1_' + r['name'][len('loop_'):], path=P.PATH_GEMM if r['plan'].get('route') == 'unitary' else r['path']),
                    rate=rate, kernels=set(ENS)) for r, rate, _ in rf.LOOP_ROWS]
# name: another learning rate than the loop row's.  From the six starts of start_bases the gradients of these two problems only grow at the loop rows' rates
# (0.05, 0.02) and at 0.1 and 0.2, so that no min_grad stops a set inside the loop; at these rates they fall again (chosen on the composed oracle alone)
FAMILY_RATES = {'E3_q1_row_tile_gradient_nt3': 0.5, 'E3_q1_direct_state_transfer': 0.3}


def family_adapter(name):
    f = next(row for row in FAMILY_ROWS if row['row']['name'] == name)
    r = f['row']

    def parts():
        return rf.systems(r['problem'], r['E'], r['q'])

    def build(n_sets):
        c, ens, nominal, _ = parts()
        eng = ensemble_engine(nominal, n_sets, ens, r['path'], r['variant'], r['chunks'])
        rf.assert_plan(eng, r, c, ens)
        return eng

    def loop(conv, x0, b):
        _, ens, _, sps = parts()
        run = python_loop(sps, ens['weights'], x0, conv)
        return dict(base=run['base'], iterations=run['iterations'], history=run['history'], vectors=dict(base=run['base']),
                    scalars={key: run['last'][key] for key in SCALARS})

    def at(base, b):
        c, ens, nominal, sps = parts()
        o = rf.expectation(sps, ens['weights'], base)
        out = {key: o[key] for key in SCALARS}
        out.update(member_loss=o['member_loss'], member_reg_state=o['member_reg_state'], inter=o['inter0'])
        if not nominal.state_transfer:
            out.update(final=o['member_U'][0], member_final=o['member_U'])
        return out

    return Adapter(key=('family', name), batch=SETS, starts=lambda: start_bases(parts()[2], SETS),
                   conv=dict(CONV, rate=FAMILY_RATES.get(name, f['rate']), learning_rate_decay=50), build=build, loop=loop, at=at, snapshot=glue_snapshot,
                   loop_tol=GLUE_LOOP, read_tol=dict(GLUE_READ, member_reg_state=TIGHT['s']), full_again=True)


# ---- 3. sparse state transfer -----------------------------------------------------------------------------------------------------------------------

SPARSE_REGS = {'amplitude': 0.3, 'dwdt': 0.02, 'd2wdt2': 0.001, 'speed_up': 0.4}
SP_ALL = {'k_sp_forward', 'k_sp_backward', 'k_sp_grad'}
# name: (sparse_case arguments, vector_home, threads, learning rate)
SPARSE_ROWS = {
    'n24_m2_regs_forbidden_lds': (dict(n=24, steps=8, m=2, seed=70, reg_coeffs=SPARSE_REGS, forbidden=True), 'lds', 256, 0.05),
    'n24_m2_regs_forbidden_global': (dict(n=24, steps=8, m=2, seed=70, reg_coeffs=SPARSE_REGS, forbidden=True), 'global', 256, 0.05),
    'n257_1024_threads': (dict(n=257, steps=8, k=2, T=6, seed=71), 'lds', 1024, 0.05),
    'n1025_second_pass_over_the_rows': (dict(n=1025, steps=4, k=2, T=6, seed=72), 'lds', 1024, 0.05),
}
SPARSE_READ = dict(dict.fromkeys(SCALARS, S_RTOL), inter=U_ATOL)


@functools.lru_cache(maxsize=None)
def sparse_system(name):
    sp = sr.sparse_case(**SPARSE_ROWS[name][0])
    return sp, sr.dense_oracle(sp)


def sparse_adapter(name):
    args, home, threads, rate = SPARSE_ROWS[name]

    def build(n_sets):
        sp, _ = sparse_system(name)
        eng = P.HipEngine(None, None, sp.V, sp.W, sp.maxA, sp.dt, sp.total_time, sp.steps, sp.exp_terms, 0, state_transfer=True, reg_coeffs=sp.reg_coeffs,
                          n_seeds=n_sets, sparse_ops=sp.ops, vector_home=home)
        assert (eng.plan['path'], eng.plan['vector_home'], int(eng.plan['threads'])) == ('sparse', home, threads), (name, eng.plan)
        return eng

    def loop(conv, x0, b):
        res = go.run_adam(sparse_system(name)[1], conv, base=x0, history=True)
        return dict(base=res['base'], iterations=res['iterations'], history=res['history'], vectors=dict(base=res['base'], uks=res['uks'], evaluated=res['uks']),
                    scalars={key: res[key] for key in SCALARS})

    def at(base, b):
        o = sr.evaluate(sparse_system(name)[0], base)
        return dict({key: o[key] for key in SCALARS}, inter=o['inter_vecs'])

    # (the two homes run the same problem from the same starts: one reference serves both)
    return Adapter(key=('sparse', tuple(sorted((key, str(v)) for key, v in args.items()))), batch=SETS, starts=lambda: start_bases(sparse_system(name)[0], SETS),
                   conv=dict(CONV, rate=rate), build=build, loop=loop, at=at, snapshot=lambda eng: snapshot(eng, False), loop_tol=EXACT_LOOP,
                   read_tol=SPARSE_READ, full_again=True)


# ---- 4. open systems ------------------------------------------------------------------------------------------------------------------------------

OPEN_ROWS = {'n4_c2': 0.05, 'st_n16_c1': 0.05, 'regs': 0.05}            # rows of tests/test_open_system_gpu.py: learning rate
LB = {'k_lb_forward', 'k_lb_backward', 'k_lb_reduce'}
OPEN_READ = dict(loss=S_RTOL, reg_loss=S_RTOL, unitary_scale=S_RTOL, density=S_RTOL, populations=S_RTOL)


def open_system(name):
    from tests import test_open_system_gpu as og
    return og.system(name), og.ROWS[name]


def open_snapshot(eng):
    rho = eng.get_final_density()
    return dict(eng.scalars(), density=rho, populations=eng.get_populations(), base=eng.get_base(), uks=eng.get_uks(), evaluated=eng.get_uks(evaluated=True))


def open_adapter(name):
    def build(n_sets):
        from tests import test_open_system_gpu as og
        (sp, ops), shape = open_system(name)
        eng = og.make_engine(sp, ops, n_sets)
        m, c = shape[2], shape[5]
        assert (eng.plan['path'], eng.plan['collapse'], eng.plan['pairs']) == ('lindblad', str(c), str(m * (m + 1) // 2)), (name, eng.plan)
        return eng

    def loop(conv, x0, b):
        sp, ops = open_system(name)[0]
        res = lr.run_adam(sp, ops, conv, x0)
        return dict(base=res['base'], iterations=res['iterations'], history=res['history'],
                    vectors=dict(base=res['base'], uks=res['uks'], evaluated=res['uks'], density=res['last']['rho_final']),
                    scalars={key: res['last'][key] for key in SCALARS})

    def at(base, b):
        sp, ops = open_system(name)[0]
        o = lr.evaluate(sp, ops, base, want_grad=False)
        return dict(loss=o['loss'], reg_loss=o['reg_loss'], unitary_scale=o['unitary_scale'], density=o['rho_final'], populations=o['populations'])

    return Adapter(key=('open', name), batch=SETS, starts=lambda: start_bases(open_system(name)[0][0], SETS), conv=dict(CONV, rate=OPEN_ROWS[name]),
                   build=build, loop=loop, at=at, snapshot=open_snapshot, loop_tol=EXACT_LOOP, read_tol=OPEN_READ, full_again=True)


# ---- the table ------------------------------------------------------------------------------------------------------------------------------------

TABLE = [(g['name'], glue_adapter) for g in GLUE_ROWS] + [(f['row']['name'], family_adapter) for f in FAMILY_ROWS] + \
        [(name, sparse_adapter) for name in SPARSE_ROWS] + [(name, open_adapter) for name in OPEN_ROWS]
IDS = [name for name, _ in TABLE]


@pytest.mark.parametrize('rule', RULES)
@pytest.mark.parametrize('name,adapter', TABLE, ids=IDS)
def test_stop_values_meet_the_conditions(name, adapter, rule):
    """CPU: the row's reference loops admit a stop value with a relative margin above 1e-8 that meets accept_conv_target (>= 3 distinct stop counts, one
    set runs to the end, a finished set between two that run longer) or accept_min_grad, and a polling period that divides none of the stops.  A row
    that misses gets another seed, rate or start HERE."""
    check_stop_values(name, adapter(name), rule)


def test_rows_cover_every_glue_kernel():
    """CPU: the table names every kernel with a skip branch of its own and every kernel that has none on purpose, both vector homes, both sparse
    thread counts, both widths of k_shape_reduce (by the lines' own column spans against QOC_SHAPE_WAVE_FROM = 32), a fleet with R > 1, and every
    family of tests/test_robust_families.py: LOOP_ROWS."""
    named = set().union(*(g['kernels'] for g in GLUE_ROWS)) | set().union(*(f['kernels'] for f in FAMILY_ROWS)) | SP_ALL | LB
    for kernel in ('k_ens_reduce', 'k_ens_tilt', 'k_ens_reduce_risk', 'k_shape_reduce<1>', 'k_shape_reduce<64>', 'k_shape_reduce_risk', 'k_sp_forward',
                   'k_sp_backward', 'k_sp_grad', 'k_lb_forward', 'k_lb_backward', 'k_lb_reduce', 'k_ens_expand', 'k_shape_expand', 'k_map_expand', 'k_map_reduce',
                   'k_exact_grad', 'k_bwd_store'):
        assert kernel in named, kernel
    assert len(set(IDS)) == len(IDS)
    for g in GLUE_ROWS:                                     # what a row says it runs is what it is built from
        ks = g['kernels']
        assert ('k_shape_expand' in ks) == bool(g['line']) and ('k_map_expand' in ks) == bool(g['mapped']) and ('k_exact_grad' in ks) == g['exact'], g['name']
        assert (('k_ens_tilt' in ks) == (g['beta'] > 0 and g['Eq'][0] > 1)) and ('fleet' in ks) == bool(g['fleet']), g['name']
        if g['line']:
            T = tf.hold(g['steps'], g['line']).matrix
            span = max(int(np.ptp(np.nonzero(T[:, j])[0])) + 1 for j in range(T.shape[1]))
            assert ('k_shape_reduce<64>' in ks) == (span > 32 and g['beta'] == 0) and ('k_shape_reduce<1>' in ks) == (span <= 32 and g['beta'] == 0), (g['name'], span)
    assert any(g['fleet'] and g['fleet'][1] > 1 and g['fleet'][0] * g['fleet'][1] == SETS for g in GLUE_ROWS)
    assert {g['kind'] for g in GLUE_ROWS if g['exact']} == {'unitary', 'state'}
    assert {g['plan']['path'] for g in GLUE_ROWS if g['kernels'] >= ALL} == {'generic', 'mfma', 'gemm'}
    assert {home for _, home, _, _ in SPARSE_ROWS.values()} == {'lds', 'global'} and {threads for _, _, threads, _ in SPARSE_ROWS.values()} == {256, 1024}
    for args, _, threads, _ in SPARSE_ROWS.values():       # tests/test_sparse_gpu.py: 1024 threads past n = 256; n > 1024: a second pass over the rows
        assert threads == (1024 if args['n'] > 256 else 256)
    assert any(args['n'] > 1024 for args, _, _, _ in SPARSE_ROWS.values())
    assert any(args.get('forbidden') and args.get('reg_coeffs') and args.get('m', 1) > 1 for args, _, _, _ in SPARSE_ROWS.values())
    assert set(OPEN_ROWS) == {'n4_c2', 'st_n16_c1', 'regs'}
    want = {(r['problem'], tuple(sorted(r['plan'].items()))) for r, _, _ in rf.LOOP_ROWS}
    assert {(f['row']['problem'], tuple(sorted(f['row']['plan'].items()))) for f in FAMILY_ROWS} == want and all((f['row']['E'], f['row']['q']) == (3, 1) for f in FAMILY_ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize('rule', RULES)
@pytest.mark.parametrize('name,adapter', TABLE, ids=IDS)
def test_finished_sets_stay_as_they_finished(name, adapter, rule):
    check_row(name, adapter(name), rule)


# ---- 5. finished sets under the L-BFGS loop -------------------------------------------------------------------------------------------------------
# qoc_iterate_lbfgs evaluates with mode 0, hence skip_done = 0: a finished set is evaluated again at every iteration, on every path, and k_lbfgs_step
# returns for it.  Everything it can read back must come out of those evaluations with the bits it had when its done flag rose.

LBFGS_J, LBFGS_MAX_IT = 14, 10


def head_start(evaluate, x0, lead):
    """x0 after `lead` evaluations of tests/lbfgs_reference.py on the kind's reference (CPU): a start for ONE control set on problems whose sets would
    otherwise fall in step, so that it reaches a target evaluations before the others can."""
    return x0 if not lead else lb.run(evaluate, x0, dict(lg.BASE, conv_target=-1.0), lead)['x']


def lbfgs_plain(name, sp, path, variant=0, words=None, lead=0, **kw):
    """A plain engine of tests/test_lbfgs_gpu.py: KINDS with three control sets (tests/test_lbfgs_gpu.py's three starts; lead: head_start of the first), read
    back against the oracle."""
    def build(n_sets):
        eng = lg.make_engine(sp, n_sets, path, variant, **kw)
        for key, word in (words or {}).items():
            assert eng.plan[key].startswith(word), (name, key, word, eng.plan)
        return eng

    def at(base, b):
        o = go.evaluate(sp, base, want_grad=False, want_inter=True)
        return dict(inter=o['inter_vecs']) if sp.state_transfer else dict(inter=o['inter_vecs'], final=o['U_final'])

    return Adapter(key=('lbfgs', name), batch=3, starts=lambda: np.stack([head_start(lg.oracle_evaluator(sp), sp.base0, lead), 0.6 * sp.base0 + 0.1, -0.8 * sp.base0 + 0.05]), conv=None, build=build,
                   loop=None, at=at, snapshot=lambda eng: snapshot(eng, not sp.state_transfer), loop_tol=None, read_tol=dict(inter=U_ATOL, final=U_ATOL))


def _lbfgs_state_transfer():
    from tests.golden import cases
    from tests.helpers import oracle_system
    c = cases.case_c3(n=4, k=2, steps=30, taylor=(6, 0), seed=43)                      # tests/test_lbfgs_gpu.py: _state_transfer
    c['reg_coeffs'] = {'forbidden_coeff_list': [50.0], 'states_forbidden_list': [3]}
    c['total_time'] = 0.02 * 30
    return oracle_system(c)


def _part_a(adapter, name, n_sets, lead=0, pick=None):
    a = adapter(name)

    def starts():
        xs = np.array(a.starts())[list(pick or range(n_sets))]
        if lead:                                               # (a composed kind: the row's own reference drives the head start of set 0)
            g, c, ref_map, _, members, _, T = glue_parts(name)
            xs[0] = head_start(lambda x: ref.evaluate(c, ref_map, members[0], x, T=T, exact=g['exact'], beta=g['beta']), xs[0], lead)
        return xs
    return Adapter(key=a.key, batch=n_sets, starts=starts, conv=None, build=a.build, loop=None, at=a.at, snapshot=a.snapshot,
                   loop_tol=None, read_tol=a.read_tol)


# every engine kind of tests/test_lbfgs_gpu.py: KINDS (the plain ones on that file's problems; ensemble, line and open system on the rows of part A),
# then a mapped engine, a fleet (six control sets) and a sparse engine
LBFGS_KINDS = {
    'generic': lambda: lbfgs_plain('generic', lg.system(2, 30, 44, 5, 3), P.PATH_GENERIC, words=dict(path='generic'), lead=8),
    'mfma_batch8': lambda: lbfgs_plain('mfma_batch8', lg.system(2, 24, 44, 17, 3), P.PATH_MFMA, 8, words=dict(path='mfma', expm='8'), lead=8),
    'mfma_latency5': lambda: lbfgs_plain('mfma_latency5', lg.system(4, 40, 44), P.PATH_MFMA, 5, words=dict(path='mfma', expm='5', sweeps='latency')),
    'gemm': lambda: lbfgs_plain('gemm', lg.system(4, 40, 44), P.PATH_GEMM, words=dict(path='gemm')),
    'st_fused': lambda: lbfgs_plain('st_fused', _lbfgs_state_transfer(), P.PATH_ST_FUSED, words=dict(path='st_fused')),
    'small': lambda: lbfgs_plain('small', lg.system(4, 40, 44), P.PATH_SMALL, words=dict(path='small')),
    'exact_gradient': lambda: lbfgs_plain('exact_gradient', lg.system(4, 40, 44), P.PATH_AUTO, words=dict(path='generic', gradient='exact'), exact_gradient=True),
    'ensemble_E3': lambda: _part_a(glue_adapter, 'ensemble_E3_q1', 3),
    'shaped_P4': lambda: _part_a(glue_adapter, 'line_hold_8_4', 3),
    'open_n4_c2': lambda: _part_a(open_adapter, 'n4_c2', 3),
    'mapped': lambda: _part_a(glue_adapter, 'map_k2_r3_D3_MF', 3, pick=(0, 2, 4)),     # (its first three starts fall in step, on tests/lbfgs_reference.py over the row's reference)
    'fleet_F3_R2': lambda: _part_a(glue_adapter, 'fleet_F3_R2_E2_q1', SETS),
    'sparse_n24': lambda: _part_a(sparse_adapter, 'n24_m2_regs_forbidden_lds', 3),
}


def test_lbfgs_kinds_cover_the_loop_tests_kinds():
    """CPU: every kind of tests/test_lbfgs_gpu.py: KINDS has a row here (ensemble, line and open system at the shapes of part A), beside the three more."""
    base = {'shaped_P10': 'shaped_P4', 'open_n3_c1': 'open_n4_c2'}
    assert {base.get(kind, kind) for kind in lg.KINDS} | {'mapped', 'fleet_F3_R2', 'sparse_n24'} == set(LBFGS_KINDS)


def choose_single_target(losses, dones, max_it):
    """tests/test_lbfgs_gpu.py: test_three_control_sets_stop_on_their_own -- a target that one control set reaches at an evaluation f, at least three
    evaluations before max_iterations can end the others, between two neighbouring losses of all evaluations of a free run (losses[evaluation][set],
    dones[evaluation][set]: the free run's done flags).  Preferred: a target no other set reaches at all; the six fast problems here fall together,
    so that where there is none the others may reach it too, but not before f + 4 -- either way some other set is evaluated, and steps, at the
    three evaluations after f at least.  Of those the candidate that keeps every loss furthest away.  (target, the set, f, relative margin)."""
    J, B = len(losses), len(losses[0])
    flat = np.sort(np.unique(np.asarray(losses).ravel()))
    best = None
    for lo, hi in zip(flat[:-1], flat[1:]):
        t = 0.5 * (lo + hi)
        first = [next((j for j in range(J) if losses[j][b] < t), J) for b in range(B)]
        free_end = [next((j for j in range(J) if dones[j][b]), J) for b in range(B)]
        end = [min(a, e) for a, e in zip(first, free_end)]
        b = int(np.argmin(first))
        f = first[b]
        others = [end[g] for g in range(B) if g != b]
        margin = float(np.min(np.abs(flat - t))) / abs(t)
        key = (all(first[g] == J for g in range(B) if g != b), margin)
        if 1 <= f <= max_it - 3 and f < free_end[b] and max(others) - 1 - f >= 3 and min(others) > f and (best is None or key > best[0]):
            best = (key, t, b, f, margin)
    return None if best is None else best[1:]


@pytest.mark.gpu
@pytest.mark.parametrize('kind', list(LBFGS_KINDS))
def test_a_finished_set_keeps_its_bits_under_the_lbfgs_loop(kind):
    """Three control sets (a fleet: six), one iteration per call.  The target is chosen on a twin engine's own free run (14 evaluations without a
    target: the device loop is deterministic -- tests/test_lbfgs_gpu.py -- so the set reaches it at the same evaluation, by a margin of at least 1e-6
    where evaluations agree to 1e-12; choose_single_target).  From the evaluation at which the set's done flag rises its whole snapshot stays as it was, bit for bit,
    through every later evaluation while the others run on; and it is the reference's at the set's own base, at the kind's evaluation tolerance."""
    a = LBFGS_KINDS[kind]()
    bases = a.starts()
    B = len(bases)
    free = dict(lg.BASE, conv_target=-1.0, max_iterations=LBFGS_MAX_IT)
    twin = a.build(B)
    try:
        twin.set_base(bases)
        losses, dones = [], []
        for _ in range(LBFGS_J):
            twin.iterate_lbfgs(lg.lbfgs_params(free), 1)
            sc = twin.scalars()
            losses.append(sc['loss'].copy())
            dones.append(sc['done'].copy())
    finally:
        twin.close()
    best = choose_single_target(losses, dones, LBFGS_MAX_IT)
    assert best is not None and best[3] > 1e-6, (best, np.asarray(losses))
    target, b, f, margin = best
    p = lg.lbfgs_params(dict(free, conv_target=target))
    eng = a.build(B)
    try:
        print('%s: plan %s' % (kind, ' '.join('%s=%s' % kv for kv in eng.plan.items())))
        print('  conv_target %.6e (margin %.2e): set %d finishes at evaluation %d of %d' % (target, margin, b, f, LBFGS_J))
        eng.set_base(bases)
        snaps = []
        for _ in range(LBFGS_J):
            eng.iterate_lbfgs(p, 1)
            snaps.append(a.snapshot(eng))
        done = [[int(s['done'][g]) for s in snaps] for g in range(B)]
        assert done[b] == [0] * f + [1] * (LBFGS_J - f), (b, f, done)
        running = [j for j in range(f + 1, LBFGS_J) if any(not done[g][j] for g in range(B))]
        assert len(running) >= 3, done                         # the others are evaluated, and step, at least three more times
        for j in range(f + 1, LBFGS_J):
            for key in snaps[f]:
                np.testing.assert_array_equal(snaps[j][key][b], snaps[f][key][b], err_msg='%s of the finished set %d at evaluation %d (finished at %d)' % (key, b, j, f))
        for j in range(f + 1, f + 4):                          # ... while they move
            assert any(not np.array_equal(snaps[j]['base'][g], snaps[j - 1]['base'][g]) for g in range(B) if g != b), j
        worst = {}
        for key, want in a.at(snaps[f]['base'][b], b).items():
            worst[key] = fs.relative_error(snaps[-1][key][b], want)
            assert worst[key] <= a.read_tol[key], (key, worst[key], a.read_tol[key])
        print('  worst |device - reference| of the finished set\'s read-backs after the last evaluation: %s' % ', '.join('%s %.2e' % kv for kv in worst.items()))
    finally:
        eng.close()


RESTORE_ROW = 'gemm_stepwise_m12'                          # tests/test_finished_sets_gpu.py: the GEMM unitary route that forms its final state lazily


@functools.lru_cache(maxsize=None)
def restore_reference(max_it):
    """Two control sets of the row's problem under c1 = 0.9 and a small max_iterations (tests/test_lbfgs_gpu.py: max_it4), by tests/lbfgs_reference.py on
    the oracle: (system, bases, parameters, the records)."""
    sp = fs.plain_system(next(r for r in fs.ROWS if r['name'] == RESTORE_ROW)['problem'])
    bases = start_bases(sp, 2)
    p = dict(lg.BASE, c1=0.9, max_iterations=max_it)
    return sp, bases, p, [lb.run(lg.oracle_evaluator(sp), x0, p) for x0 in bases]


@pytest.mark.parametrize('max_it', [3, 4])
def test_restore_reference_ends_by_restore(max_it):
    """CPU: at max_iterations = 3 set 0 ends by RESTORE one evaluation after set 1 has stopped on an accepted trial; at 4 both end by RESTORE.  Margins
    as tests/test_lbfgs_gpu.py asserts them, and the refused trial's final unitary is far from the accepted point's."""
    sp, bases, p, recs = restore_reference(max_it)
    want = {3: ([lb.ACCEPT, lb.ACCEPT, lb.REJECT, lb.RESTORE, lb.STOP], [lb.ACCEPT, lb.ACCEPT, lb.REJECT, lb.STOP]),
            4: ([lb.ACCEPT, lb.ACCEPT, lb.REJECT, lb.REJECT, lb.RESTORE, lb.STOP], [lb.ACCEPT, lb.ACCEPT, lb.REJECT, lb.ACCEPT, lb.RESTORE, lb.STOP])}[max_it]
    for rec, branches in zip(recs, want):
        lg.assert_margins(rec)
        assert rec['branch'] == branches, rec['branch']


@pytest.mark.gpu
@pytest.mark.parametrize('max_it', [3, 4])
def test_a_run_ended_by_restore_reads_back_the_accepted_point(max_it):
    """A refused trial at the limit sends the variable back to x_acc, takes one more evaluation, then stops: the read-backs after the stop -- the lazily
    formed final unitary first -- are those of x_acc (U_ATOL against the oracle at the device's own base), and the oracle AT THE REFUSED TRIAL is far
    from them (asserted: more than 1e6 U_ATOL), so the row cannot pass on what the refused evaluation left behind."""
    sp, bases, p, recs = restore_reference(max_it)
    r = next(r for r in fs.ROWS if r['name'] == RESTORE_ROW)
    J = max(len(rec['branch']) for rec in recs) + 2
    eng = fs.engine(r, sp, 2)
    try:
        got = lg.step_engine(eng, lg.lbfgs_params(p), bases, J)
        first = snapshot(eng, True)
        assert list(first['done']) == [1, 1], first['done']
        for b, rec in enumerate(recs):
            n = len(rec['branch'])
            branches = lg.infer_branches([q[b] for q in got['points']], [q[b] for q in got['next']], [int(s['iterations'][b]) for s in got['scalars']],
                                         [int(s['done'][b]) for s in got['scalars']], p)
            assert branches == rec['branch'], (b, branches, rec['branch'])
            np.testing.assert_allclose(first['base'][b], rec['x'], rtol=0, atol=LOOP_ATOL)
            for j in range(n, J):                              # finished: evaluated where it stands, nothing moves
                assert np.array_equal(got['next'][j][b], got['next'][n - 1][b])
                for key in SCALARS + ('iterations', 'done'):
                    assert got['scalars'][j][key][b] == got['scalars'][n - 1][key][b], (b, j, key)
            o = go.evaluate(sp, first['base'][b], want_grad=False, want_inter=True)
            for key, want in (('final', o['U_final']), ('final_again', o['U_final']), ('inter', o['inter_vecs'])):
                err = fs.relative_error(first[key][b], want)
                print('set %d (%s): %s against the oracle at the accepted point %.2e' % (b, ' '.join(rec['branch']), key, err))
                assert err <= U_ATOL, (b, key, err)
            for key in ('loss', 'reg_loss', 'unitary_scale'):
                assert abs(first[key][b] - o[key]) <= S_RTOL * max(1.0, abs(o[key])), (b, key, first[key][b], o[key])
            if lb.RESTORE in rec['branch']:
                j = rec['branch'].index(lb.RESTORE)
                np.testing.assert_array_equal(first['base'][b], got['next'][j][b])          # back at x_acc, to the bit
                assert np.max(np.abs(got['points'][j][b] - first['base'][b])) > 1e-3       # ... which is not where the refused trial stood
                t = go.evaluate(sp, got['points'][j][b], want_grad=False, want_inter=True)
                for key, far in (('final', t['U_final']), ('inter', t['inter_vecs'])):
                    gap = fs.relative_error(first[key][b], far)
                    print('set %d: %s against the oracle at the refused trial %.2e' % (b, key, gap))
                    assert gap > 1e6 * U_ATOL, (b, key, gap)
        assert any(lb.RESTORE in rec['branch'] for rec in recs)
    finally:
        eng.close()
