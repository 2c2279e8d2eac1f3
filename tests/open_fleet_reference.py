"""The expected values of an open ensemble or fleet engine, composed from what exists (TEST INFRASTRUCTURE ONLY).

A member of such an engine is the open problem of tests/lindblad_reference.py on the member's Hamiltonians and on its collapse operators
sqrt(s_j) C_j: lindblad_reference.evaluate on a go.OracleSystem with the member's drift, run -- as tests/control_map_reference.py: trajectory runs the
closed oracle -- at given coefficients c (r x steps) through the amplitude bound S_i = 2 max_t |c_i| and the base arcsin(c / S), with no
regulariser of its own.  From it come the member's loss, unitary_scale, final density operators, populations and dL_du = dJ/dc.  The members are then
combined exactly as tests/control_map_reference.py: evaluate combines the closed ones: the weighted mean or its tilt (the soft worst case), the
map's pullback, the member's amplitude scales, the line's T^T, and go.pulse_regularisers on the k pulses (on the P samples behind a line).  A fleet
picks rows: device f is Fleet.device(f) (tests/fleet_reference.py: control_sets, swapped_apart)."""
from types import SimpleNamespace

import numpy as np

from oracle import grape_oracle as go
from quantum_optimal_control.helper_functions import control_map as cmap
from quantum_optimal_control.helper_functions import fleet as fl_mod
from quantum_optimal_control.helper_functions import robust as rb
from quantum_optimal_control.helper_functions.synthetic_systems import herm
from tests import control_map_reference as ref
from tests import lindblad_reference as lr
from tests.fleet_reference import control_sets, swapped_apart          # noqa: F401  (re-exported for the tests)
from tests.test_open_system import collapse_list


def problem(n, k, steps, m, c, r=None, state_transfer=False, taylor=(6, 1), seed=0, regs=None):
    """tests/control_map_reference.py: problem with c collapse operators (tests/test_open_system.py: collapse_list) and the open engine's (T, s), which
    holds in both modes."""
    p = ref.problem(n, k if r is None else r, k, steps, m, state_transfer=state_transfer, taylor=taylor, seed=300 + seed, regs=regs)
    p['Taylor_terms'] = list(taylor)
    return dict(p, collapse_ops=collapse_list(n, c, seed), Hnames=['p%d' % j for j in range(k)])


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
    S = 2.0 * np.max(np.abs(coeff), axis=1)
    S[S == 0.0] = 1.0
    return lr.evaluate(member_system(p, H0e, S), ops, np.arcsin(coeff / S[:, None]), want_grad=want_grad)


def evaluate(p, cm, ens, x, T=None, beta=None, want_grad=True):
    """The expected values at the variable x (k x steps, or k x P behind the line T (steps x P)) for the members of `ens` (a validated robust dict
    with collapse_ops and rate_scales): loss, reg_loss, grad, grad_squared, unitary_scale, member_loss, weights, member_rho (E, m, m, n, n), rho_final
    and populations of member 0, coefficients of member 0, pulse, uks.  cm None: no map (the coefficients are the member's pulses).  beta None: the
    ensemble's own risk."""
    maxA = np.asarray(p['maxA'], dtype=np.float64)
    k = len(maxA)
    x = np.asarray(x, dtype=np.float64).reshape(k, -1)
    beta = float(ens.get('risk', 0.0)) if beta is None else float(beta)
    _, pulse_rc = ref.split_regs(p['reg_coeffs'])
    ws = np.sin(x)
    wf = ws if T is None else ws @ T.T
    u = maxA[:, None] * wf
    w = np.asarray(ens['weights'], dtype=np.float64)
    E = len(w)
    rs, vs = [], []
    for e in range(E):
        H0e, _ = rb.member_hamiltonians(p['H0'], [], ens, e)
        v = ens['amp_scales'][e][:, None] * u
        vs.append(v)
        rs.append(trajectory(p, H0e, v if cm is None else cmap.apply(cm, v), rb.member_collapse_ops(ens, e), want_grad))
    loss_e = np.array([r['loss'] for r in rs])
    Pn = x.shape[1]
    omg = None
    if 'envelope' in pulse_rc:
        grid = np.linspace(-2, 2, Pn)
        shape = np.ones(Pn) - np.exp(-np.power(grid, 2.) / 2.)
        omg = np.tile(shape * (shape > 0) + 0.01 * np.ones(Pn), (k, 1))
    view = SimpleNamespace(reg_coeffs=pulse_rc, steps=Pn, dt=p['total_time'] / Pn, k=k, total_time=p['total_time'], use_gpu=True, one_minus_gauss=omg)
    val, dR = go.pulse_regularisers(view, ws)
    if beta > 0 and E > 1:
        loss, pi = ref.tilt(loss_e, w, beta)                      # (the state regulariser of an open member is zero)
    else:
        pi, loss = w, float(np.sum(w * loss_e))
    out = dict(loss=float(loss), reg_loss=float(loss) + val, unitary_scale=float(np.sum(w * np.array([r['unitary_scale'] for r in rs]))),
               member_loss=loss_e, weights=pi, pulse=u, uks=maxA[:, None] * ws, coefficients=vs[0] if cm is None else cmap.apply(cm, vs[0]),
               rho_final=rs[0]['rho_final'], populations=rs[0]['populations'], member_rho=np.stack([r['rho_final'] for r in rs]))
    if not want_grad:
        return out
    back = (lambda v, g: g) if cm is None else (lambda v, g: cmap.pullback(cm, v, g))
    dJdu = sum(pi[e] * ens['amp_scales'][e][:, None] * back(vs[e], rs[e]['dL_du']) for e in range(E))
    grad = np.cos(x) * (maxA[:, None] * (dJdu if T is None else dJdu @ T) + dR)
    out.update(grad=grad, grad_squared=0.5 * float(np.sum(grad * grad)))
    return out


def evaluate_device(p, cm, fl, f, x, T=None, want_grad=True):
    """evaluate with device f's rows and the fleet's risk."""
    return evaluate(p, cm, fl.device(f), x, T=T, beta=float(fl.risk), want_grad=want_grad)


def engine_system(p):
    """What the engine is given beside the ensemble, the fleet, the line and the map: the oracle's arrays for the problem's operators."""
    return member_system(p, p['H0'], np.ones(len(p['Hops'])))


def run_adam(evaluate_at, x0, conv):
    """tests/control_map_reference.py: run_adam, which also returns the evaluation that ended the loop and every evaluation's scalars."""
    x = np.array(x0, dtype=np.float64)
    opt = go.Adam(x.shape)
    iterations, hist = 0, []
    while True:
        r = evaluate_at(x)
        hist.append((r['loss'], r['reg_loss'], r['grad_squared'], r['unitary_scale']))
        if r['loss'] < conv['conv_target'] or r['grad_squared'] < conv['min_grad'] or iterations >= conv['max_iterations']:
            return dict(base=x, iterations=iterations, last=r, history=np.array(hist))
        iterations += 1
        x = opt.step(x, r['grad'], float(conv['rate']) * np.exp(-float(iterations) / conv['learning_rate_decay']))
