"""The expected values of an engine with a table of noise traces, composed from the unchanged oracle (TEST INFRASTRUCTURE ONLY).

With a table, frozen row q' of member e has at slice t the value offsets[e, q'] + traces[e, q', t].  A perturbation no longer folds into the
member's drift, so a member's trajectory is what tests/control_map_reference.py: trajectory already runs -- the oracle at given COEFFICIENTS --
on the problem c' whose operators are Hops + the perturbation operators, at the coefficients
    coeff = [ the member's control rows (its pulses a[e, j] u_j, or apply(map, them)) ; offsets[e][:, None] + traces[e] ]
through that function's arcsin(coeff / S) device, with the nominal drift H0 and the state regularisers only.  Of its dL_du = dJ/dcoeff the first r
rows are the member's dJ/dc; the frozen rows have no reader.  The members are then combined exactly as tests/control_map_reference.py: evaluate
combines them: the weighted mean or its tilt, the map's pullback, the member's amplitude scales, the line's T^T, and the pulse regularisers once on
the group view (split_regs), never on the frozen rows.  Open members run through tests/running_cost_reference.py: trajectory (which is
tests/open_fleet_reference.py: trajectory when there is no cost), sparse ones through tests/sparse_ensemble_reference.py: trajectory."""
from types import SimpleNamespace

import numpy as np

from oracle import grape_oracle as go
from quantum_optimal_control.helper_functions import control_map as cmap
from quantum_optimal_control.helper_functions import robust as rb
from tests import control_map_reference as ref


def member_rows(ens, e, steps):
    """offsets[e][:, None] + traces[e]: the q frozen rows of member e, (q, steps).  No table: the constant rows."""
    off = np.asarray(ens['offsets'], dtype=np.float64)[e][:, None]
    tr = ens.get('traces')
    return off + (np.zeros((off.shape[0], steps)) if tr is None else np.asarray(tr, dtype=np.float64)[e])


def _combine(k, maxA, total_time, steps, pulse_rc, ens, x, cm, T, beta, run, want_grad=True):
    """The control set's values from the members' trajectories run(e, coeff) (coeff: (r + q) x steps)."""
    maxA = np.asarray(maxA, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64).reshape(k, -1)
    ws = np.sin(x)
    wf = ws if T is None else ws @ T.T
    u = maxA[:, None] * wf
    w = np.asarray(ens['weights'], dtype=np.float64)
    E = len(w)
    rs, vs, cs = [], [], []
    for e in range(E):
        v = ens['amp_scales'][e][:, None] * u
        c = v if cm is None else cmap.apply(cm, v)
        vs.append(v)
        cs.append(c)
        rs.append(run(e, np.vstack([c, member_rows(ens, e, steps)])))
    r_rows = cs[0].shape[0]
    loss_e = np.array([r['loss'] for r in rs])
    state_e = np.array([r['reg_state'] if 'reg_state' in r else r['reg_loss'] - r['loss'] for r in rs])
    Pn = x.shape[1]
    omg = None
    if 'envelope' in pulse_rc:
        grid = np.linspace(-2, 2, Pn)
        shape = np.ones(Pn) - np.exp(-np.power(grid, 2.) / 2.)
        omg = np.tile(shape * (shape > 0) + 0.01 * np.ones(Pn), (k, 1))
    view = SimpleNamespace(reg_coeffs=pulse_rc, steps=Pn, dt=total_time / Pn, k=k, total_time=total_time, use_gpu=True, one_minus_gauss=omg)
    val, dR = go.pulse_regularisers(view, ws)
    if beta > 0 and E > 1:
        J, pi = ref.tilt(loss_e + state_e, w, beta)
        reg_state = float(np.sum(pi * state_e))
        loss, reg_loss = J - reg_state, J + val
    else:
        pi = w
        loss, reg_loss = float(np.sum(w * loss_e)), float(np.sum(w * (loss_e + state_e))) + val
    out = dict(loss=float(loss), reg_loss=float(reg_loss), unitary_scale=float(np.sum(w * np.array([r['unitary_scale'] for r in rs]))),
               member_loss=loss_e, member_reg_state=state_e, weights=pi, pulse=u, uks=maxA[:, None] * ws, coefficients=cs[0], members=rs)
    if not want_grad:
        return out
    back = (lambda v, g: g) if cm is None else (lambda v, g: cmap.pullback(cm, v, g))
    dJdu = sum(pi[e] * ens['amp_scales'][e][:, None] * back(vs[e], rs[e]['dL_du'][:r_rows]) for e in range(E))
    grad = np.cos(x) * (maxA[:, None] * (dJdu if T is None else dJdu @ T) + dR)
    out.update(grad=grad, grad_squared=0.5 * float(np.sum(grad * grad)))
    return out


def evaluate(c, ens, x, cm=None, T=None, exact=False, beta=None, want_grad=True):
    """A dense closed engine (c: a case dict of tests/control_map_reference.py: problem style, `maxA` of k entries; ens: a validated robust dict with
    or without traces) at the variable x (k x steps, or k x P behind the line T): loss, reg_loss, grad, grad_squared, unitary_scale, member_loss,
    weights, pulse, uks, coefficients (member 0's r rows), U_final / member_U / inter_vecs as tests/control_map_reference.py: evaluate gives them."""
    state_rc, pulse_rc = ref.split_regs(c['reg_coeffs'])
    cp = dict(c, Hops=list(c['Hops']) + [np.asarray(p, dtype=np.complex128) for p in ens['operators']])
    beta = float(ens.get('risk', 0.0)) if beta is None else float(beta)
    out = _combine(len(c['maxA']), c['maxA'], c['total_time'], c['steps'], pulse_rc, ens, x, cm, T, beta,
                   lambda e, coeff: ref.trajectory(cp, state_rc, c['H0'], coeff, exact, want_grad), want_grad)
    rs = out['members']
    out.update(U_final=rs[0]['U_final'], member_U=None if c['state_transfer'] else np.stack([r['U_final'] for r in rs]))
    if want_grad:
        out['inter_vecs'] = rs[0]['inter_vecs']
    return out


def evaluate_open(p, ens, x, cm=None, T=None, beta=None, costs=(), want_grad=True):
    """An open engine (p: tests/open_fleet_reference.py: problem; ens with collapse_ops and rate_scales; costs: running-cost records): the dict of
    evaluate with rho_final and populations of member 0, member_rho, and -- with costs -- expectations of member 0."""
    from tests import running_cost_reference as rcr
    _, pulse_rc = ref.split_regs(p['reg_coeffs'])
    pp = dict(p, Hops=list(p['Hops']) + [np.asarray(op, dtype=np.complex128) for op in ens['operators']])
    beta = float(ens.get('risk', 0.0)) if beta is None else float(beta)
    out = _combine(len(p['maxA']), p['maxA'], p['total_time'], p['steps'], pulse_rc, ens, x, cm, T, beta,
                   lambda e, coeff: rcr.trajectory(pp, p['H0'], coeff, rb.member_collapse_ops(ens, e), list(costs), want_grad), want_grad)
    rs = out['members']
    out.update(rho_final=rs[0]['rho_final'], populations=rs[0]['populations'], expectations=rs[0]['expectations'],
               member_rho=np.stack([r['rho_final'] for r in rs]))
    return out


def evaluate_sparse(p, ens, x, cm=None, T=None, beta=None):
    """A sparse engine (p: tests/sparse_ensemble_reference.py: Problem; the operators of ens may be scipy.sparse): the dict of evaluate with member
    0's inter_vecs."""
    from tests import sparse_ensemble_reference as ser
    state_rc = {key: v for key, v in p.reg_coeffs.items() if key not in ser.PULSE_KEYS}
    pulse_rc = {key: v for key, v in p.reg_coeffs.items() if key in ser.PULSE_KEYS}
    pp = ser.Problem(p.H0, list(p.Hops) + list(ens['operators']), p.V, p.W, p.total_time, p.steps, p.T, p.maxA, p.reg_coeffs)
    beta = float(ens.get('risk', 0.0)) if beta is None else float(beta)
    out = _combine(p.k, p.maxA, p.total_time, p.steps, pulse_rc, ens, x, cm, T, beta, lambda e, coeff: ser.trajectory(pp, state_rc, p.H0, coeff))
    out['inter_vecs'] = out['members'][0]['inter_vecs']
    return out


def with_traces(ens, traces):
    """The validated robust dict `ens` with the table `traces` (E, q, steps), or without one (None)."""
    out = {key: v for key, v in ens.items() if key != 'traces'}
    if traces is not None:
        out['traces'] = np.array(traces, dtype=np.float64)
    return out


def make_traces(E, q, steps, seed=0, F=None, scale=0.3):
    """Random traces in which one (member, operator) row is zero except at a single slice, so that a transposed index cannot pass; F given: a leading
    device axis, every device with a draw (and a lone slice) of its own."""
    rng = np.random.default_rng(9000 + seed)
    tr = rng.uniform(-scale, scale, size=((F or 1), E, q, steps))
    for f in range(tr.shape[0]):
        e, qq, t = (f + 1) % E, (f + q - 1) % q, (2 + 3 * f) % steps
        tr[f, e, qq, :] = 0.0
        tr[f, e, qq, t] = scale * (1.0 + 0.1 * f)
    return tr if F else tr[0]
