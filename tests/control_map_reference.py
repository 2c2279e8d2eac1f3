"""The expected values of a mapped engine, composed from the unchanged oracle.

A trajectory of a mapped engine is the oracle's problem on the r operators the map feeds, run at the coefficients c = apply(map, v) in place of a
pulse: a go.OracleSystem with those operators (a member's perturbations folded into its drift, as tests/test_robust_gpu.py does), the amplitude
bound S_i = 2 max_t |c_i| (so that arcsin is far from its end points) and only the state regularisers, evaluated at arcsin(c / S).  From it come
loss, inter_vecs and dL_du = dJ/dc -- the oracle's first-order gradient, or the exact one of tests/exact_gradient_reference.py.  The chain rule
    dJ/dv_j[t] = sum_i dJ/dc_i[t] M[i, j, t] p_ij'(v_j[t])
is then applied in NumPy (control_map.pullback), the members are weighted as tests/test_robust_gpu.py does (or tilted, tests/test_risk.py's
formula), a line applied as tests/test_transfer_gpu.py does, and the pulse part is go.pulse_regularisers on the k pulses (on the P samples behind a
line)."""
from types import SimpleNamespace

import numpy as np

from oracle import grape_oracle as go
from quantum_optimal_control.helper_functions import control_map as cmap
from quantum_optimal_control.helper_functions import robust as rb
from quantum_optimal_control.helper_functions.synthetic_systems import herm, random_unitary
from tests import exact_gradient_reference as xr

PULSE_KEYS = ('amplitude', 'envelope', 'dwdt', 'd2wdt2', 'bandpass', 'band')


def problem(n, r, k, steps, m, state_transfer=False, taylor=(6, 1), seed=0, total_time=None, regs=None):
    """A synthetic problem with r operators and k pulses (tests/golden/cases.py style, with `maxA` of k entries)."""
    rng = np.random.default_rng(1000 + seed)
    H0 = 2 * np.pi * 0.3 * herm(rng, n)
    Hops = [2 * np.pi * 0.15 * herm(rng, n) for _ in range(r)]
    if state_transfer:
        vec = lambda: (lambda v: v / np.linalg.norm(v))(rng.normal(size=n) + 1j * rng.normal(size=n))
        states = [vec() for _ in range(m)]
        U = [vec() for _ in range(m)]
        taylor = (taylor[0], 0)
    else:
        states = list(range(m))
        U = random_unitary(rng, n)
    return dict(H0=H0, Hops=Hops, U=U, total_time=0.25 * steps if total_time is None else total_time, steps=steps, states_concerned_list=states,
                U0=None if state_transfer else random_unitary(rng, n), maxA=rng.uniform(0.8, 1.6, size=k), state_transfer=state_transfer,
                Taylor_terms=list(taylor), reg_coeffs=dict(regs or {}), np_seed=seed)


def make_map(k, r, D, steps, mix=False, fixed=False, seed=0):
    """A dense random map: every polynomial coefficient nonzero, a signed slice-dependent M and an F where asked for."""
    rng = np.random.default_rng(2000 + 17 * seed + 100 * k + 10 * r + D)
    alpha = rng.uniform(0.3, 1.0, size=(r, k, D)) * rng.choice([-1.0, 1.0], size=(r, k, D)) / np.arange(1, D + 1)
    M = rng.uniform(-1.0, 1.0, size=(r, k, steps)) if mix else None
    F = rng.uniform(-0.5, 0.5, size=(r, steps)) if fixed else None
    return cmap.validate(cmap.ControlMap(alpha, M, F), k=k, r=r, steps=steps)


def nominal_ensemble(k):
    return dict(operators=[], offsets=np.zeros((1, 0)), amp_scales=np.ones((1, k)), weights=np.ones(1), risk=0.0)


def ensemble(c, E, q, seed=5):
    """tests/test_robust_gpu.py: ensemble, on the k pulses of a mapped problem."""
    rng = np.random.default_rng(seed)
    n, k = len(c['H0']), len(c['maxA'])
    if E == 1 and q == 0:
        return rb.validate(nominal_ensemble(k), n, k)
    ops = [0.3 * 2 * np.pi * herm(rng, n) for _ in range(q)]
    return rb.validate(dict(operators=ops, offsets=rng.uniform(-0.2, 0.2, size=(E, q)), amp_scales=rng.uniform(0.9, 1.1, size=(E, k)),
                            weights=rng.uniform(0.5, 1.5, size=E)), n, k)


def split_regs(rc):
    """(state regularisers, pulse regularisers) of a reg_coeffs dict."""
    return {key: v for key, v in rc.items() if key not in PULSE_KEYS}, {key: v for key, v in rc.items() if key in PULSE_KEYS}


def engine_system(c):
    """What the engine is given beside the map, the ensemble and the line: the oracle's arrays for the r operators (Hs, U0, V, W, T, s); its maxA and
    base0 belong to no pulse and are not used."""
    np.random.seed(c['np_seed'])
    return go.OracleSystem(c['H0'], c['Hops'], c['U'], c['total_time'], c['steps'], c['states_concerned_list'], U0=c['U0'], reg_coeffs=c['reg_coeffs'],
                           maxA=np.ones(len(c['Hops'])), state_transfer=c['state_transfer'], Taylor_terms=c['Taylor_terms'])


def trajectory(c, state_rc, H0e, coeff, exact=False, want_grad=True):
    """The oracle at the coefficients coeff (r x steps): its evaluation dict, with dL_du = dJ/dc."""
    S = 2.0 * np.max(np.abs(coeff), axis=1)
    S[S == 0.0] = 1.0
    np.random.seed(c['np_seed'])
    sp = go.OracleSystem(H0e, c['Hops'], c['U'], c['total_time'], c['steps'], c['states_concerned_list'], U0=c['U0'], reg_coeffs=state_rc, maxA=S,
                         state_transfer=c['state_transfer'], Taylor_terms=c['Taylor_terms'])
    base = np.arcsin(coeff / S[:, None])
    if not want_grad:
        return go.evaluate(sp, base, want_grad=False)
    return xr.evaluate(sp, base) if exact else go.evaluate(sp, base, want_inter=True)


def tilt(costs, w, beta):
    """(J, pi) of the soft worst case over member costs (include/qoc.h, qoc_set_risk)."""
    cmax = np.max(costs[w > 0])
    S = np.sum(np.where(w > 0, w * np.expm1(beta * (costs - cmax)), 0.0))
    pi = np.where(w > 0, w * np.exp(beta * (costs - cmax)), 0.0) / (1.0 + S)
    return cmax + np.log1p(S) / beta, pi


def evaluate(c, cm, ens, x, T=None, exact=False, beta=0.0, want_grad=True):
    """The mapped engine's expected values at the variable x (k x steps, or k x P behind the line T (steps x P)) for the members of `ens` (a validated
    robust dict): loss, reg_loss, grad, grad_squared, unitary_scale, member_loss, coefficients / inter_vecs / U_final of member 0, member_U (every
    member's final unitary; None in state-transfer mode), pulse, uks."""
    maxA = np.asarray(c['maxA'], dtype=np.float64)
    k = len(maxA)
    x = np.asarray(x, dtype=np.float64).reshape(k, -1)
    state_rc, pulse_rc = split_regs(c['reg_coeffs'])
    ws = np.sin(x)
    wf = ws if T is None else ws @ T.T
    u = maxA[:, None] * wf
    w = np.asarray(ens['weights'], dtype=np.float64)
    E = len(w)
    rs, vs = [], []
    for e in range(E):
        H0e = np.asarray(c['H0'], dtype=np.complex128)
        for qq, p in enumerate(ens['operators']):
            H0e = H0e + ens['offsets'][e, qq] * p
        v = ens['amp_scales'][e][:, None] * u
        vs.append(v)
        rs.append(trajectory(c, state_rc, H0e, cmap.apply(cm, v), exact, want_grad))
    loss_e = np.array([r['loss'] for r in rs])
    state_e = np.array([r['reg_loss'] - r['loss'] for r in rs])
    Pn = x.shape[1]
    omg = None
    if 'envelope' in pulse_rc:
        grid = np.linspace(-2, 2, Pn)
        shape = np.ones(Pn) - np.exp(-np.power(grid, 2.) / 2.)
        omg = np.tile(shape * (shape > 0) + 0.01 * np.ones(Pn), (k, 1))
    view = SimpleNamespace(reg_coeffs=pulse_rc, steps=Pn, dt=c['total_time'] / Pn, k=k, total_time=c['total_time'], use_gpu=True, one_minus_gauss=omg)
    val, dR = go.pulse_regularisers(view, ws)
    if beta > 0 and E > 1:
        J, pi = tilt(loss_e + state_e, w, beta)
        reg_state = float(np.sum(pi * state_e))
        loss, reg_loss = J - reg_state, J + val
    else:
        pi = w
        loss, reg_loss = float(np.sum(w * loss_e)), float(np.sum(w * (loss_e + state_e))) + val
    out = dict(loss=loss, reg_loss=reg_loss, unitary_scale=float(np.sum(w * np.array([r['unitary_scale'] for r in rs]))), member_loss=loss_e,
               weights=pi, pulse=u, uks=maxA[:, None] * ws, coefficients=cmap.apply(cm, vs[0]), U_final=rs[0]['U_final'],
               member_U=None if c['state_transfer'] else np.stack([r['U_final'] for r in rs]))
    if not want_grad:
        return out
    dJdu = sum(pi[e] * ens['amp_scales'][e][:, None] * cmap.pullback(cm, vs[e], rs[e]['dL_du']) for e in range(E))
    grad = np.cos(x) * (maxA[:, None] * (dJdu if T is None else dJdu @ T) + dR)
    out.update(grad=grad, grad_squared=0.5 * float(np.sum(grad * grad)), inter_vecs=rs[0]['inter_vecs'])
    return out


def central_differences(f, x, h=1e-6):
    g = np.zeros_like(x)
    for idx in np.ndindex(*x.shape):
        xp, xm = x.copy(), x.copy()
        xp[idx] += h
        xm[idx] -= h
        g[idx] = (f(xp) - f(xm)) / (2 * h)
    return g


def variables(k, Pn, G, seed=0):
    return np.random.default_rng(3000 + Pn + seed).normal(0.0, 0.7, size=(3, k, Pn))[:G]


def run_adam(evaluate_at, x0, conv):
    """The device loop's semantics (oracle.grape_oracle.run_adam) over any evaluation: dict(base, iterations, loss)."""
    x = np.array(x0, dtype=np.float64)
    opt = go.Adam(x.shape)
    iterations = 0
    while True:
        r = evaluate_at(x)
        if r['loss'] < conv['conv_target'] or r['grad_squared'] < conv['min_grad'] or iterations >= conv['max_iterations']:
            return dict(base=x, iterations=iterations, loss=r['loss'], reg_loss=r['reg_loss'])
        iterations += 1
        x = opt.step(x, r['grad'], float(conv['rate']) * np.exp(-float(iterations) / conv['learning_rate_decay']))
