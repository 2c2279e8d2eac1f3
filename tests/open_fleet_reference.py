"""The expected values of an open ensemble or fleet engine, composed from what exists (TEST INFRASTRUCTURE ONLY).

A member of such an engine is the open problem of tests/lindblad_reference.py on the member's Hamiltonians and on its collapse operators
sqrt(s_j) C_j: lindblad_reference.evaluate on a go.OracleSystem with the member's drift, run -- as tests/control_map_reference.py: trajectory runs the
closed oracle -- at given coefficients c (r x steps) through the amplitude bound S_i = 2 max_t |c_i| and the base arcsin(c / S), with no
regulariser of its own.  From it come the member's loss, unitary_scale, final density operators, populations and dL_du = dJ/dc.  The members are then
combined by tests/composed_reference.py: combine, as tests/control_map_reference.py: evaluate combines the closed ones.  A fleet picks rows:
device f is Fleet.device(f) (tests/fleet_reference.py: control_sets, swapped_apart)."""
import numpy as np

from oracle import grape_oracle as go
from quantum_optimal_control.helper_functions import fleet as fl_mod
from quantum_optimal_control.helper_functions import robust as rb
from quantum_optimal_control.helper_functions.synthetic_systems import herm
from tests import control_map_reference as ref
from tests import lindblad_reference as lr
from tests.composed_reference import at_coefficients, combine, split_regs
from tests.composed_reference import run_adam                          # noqa: F401  (re-exported for the tests)
from tests.fleet_reference import control_sets, swapped_apart          # noqa: F401  (re-exported for the tests)


def problem(n, k, steps, m, c, r=None, state_transfer=False, taylor=(6, 1), seed=0, regs=None):
    """tests/control_map_reference.py: problem with c collapse operators (lindblad_reference.collapse_list) and the open engine's (T, s), which holds
    in both modes."""
    p = ref.problem(n, k if r is None else r, k, steps, m, state_transfer=state_transfer, taylor=taylor, seed=300 + seed, regs=regs)
    p['Taylor_terms'] = list(taylor)
    return dict(p, collapse_ops=lr.collapse_list(n, c, seed), Hnames=['p%d' % j for j in range(k)])


def make_fleet(p, F, E, q, seed=5, risk=0.0, zero=True):
    """F devices of E members: every offset, amplitude scale and rate scale distinct, and (zero) one rate scale exactly 0."""
    rng = np.random.default_rng(seed + 100 * F + 10 * E + q)
    n, k, c = len(p['H0']), len(p['maxA']), len(p['collapse_ops'])
    ops = [0.3 * 2 * np.pi * herm(rng, n) for _ in range(q)]
    off = rng.uniform(-0.2, 0.2, size=(F, E, q))
    amp = rng.uniform(0.9, 1.1, size=(F, E, k)) + 0.05 * np.arange(F)[:, None, None]
    rates = rng.uniform(0.4, 2.5, size=(F, E, c)) + 0.3 * np.arange(F)[:, None, None]
    if zero and c:
        rates[F - 1, E - 1, c - 1] = 0.0
    w = rng.uniform(0.5, 1.5, size=E) if E > 1 else None
    return fl_mod.validate(fl_mod.Fleet(ops, off, amp, weights=w, risk=risk, collapse_ops=p['collapse_ops'], rate_scales=rates), n, k)


def member_system(p, H0e, bound):
    """The OracleSystem of one member: its drift, the problem's operators, the amplitude bound `bound`, no regulariser."""
    np.random.seed(p['np_seed'])
    return go.OracleSystem(H0e, p['Hops'], p['U'], p['total_time'], p['steps'], p['states_concerned_list'], U0=p['U0'], reg_coeffs={}, maxA=bound,
                           state_transfer=p['state_transfer'], Taylor_terms=p['Taylor_terms'])


def trajectory(p, H0e, coeff, ops, want_grad=True):
    """lindblad_reference.evaluate at the coefficients coeff (r x steps) under the collapse operators ops: its dict, with dL_du = dJ/dc."""
    S, base = at_coefficients(coeff)
    return lr.evaluate(member_system(p, H0e, S), ops, base, want_grad=want_grad)


def read_backs(out):
    """combine's dict with the read-backs of an open engine: member_rho (E, m, m, n, n), rho_final and populations of member 0."""
    rs = out['members']
    out.update(rho_final=rs[0]['rho_final'], populations=rs[0]['populations'], member_rho=np.stack([r['rho_final'] for r in rs]))
    return out


def evaluate(p, cm, ens, x, T=None, beta=None, want_grad=True):
    """The expected values at the variable x (k x steps, or k x P behind the line T (steps x P)) for the members of `ens` (a validated robust dict
    with collapse_ops and rate_scales): tests/composed_reference.py: combine over the members' trajectories (an open member has no state
    regulariser), with the read-backs above.  cm None: no map (the coefficients are the member's pulses).  beta None: the ensemble's own risk."""
    run = lambda e, coeff: trajectory(p, rb.member_hamiltonians(p['H0'], [], ens, e)[0], coeff, rb.member_collapse_ops(ens, e), want_grad)
    return read_backs(combine(x, p['maxA'], ens, p['total_time'], split_regs(p['reg_coeffs'])[1], run, cm=cm, T=T, beta=beta, want_grad=want_grad))


def evaluate_device(p, cm, fl, f, x, T=None, want_grad=True):
    """evaluate with device f's rows and the fleet's risk."""
    return evaluate(p, cm, fl.device(f), x, T=T, beta=float(fl.risk), want_grad=want_grad)


def engine_system(p):
    """What the engine is given beside the ensemble, the fleet, the line and the map: the oracle's arrays for the problem's operators."""
    return member_system(p, p['H0'], np.ones(len(p['Hops'])))
