"""The exact gradient in NumPy, in forward mode, written against the unchanged oracle: the derivative of the loss oracle.grape_oracle.evaluate
reports, truncation included ("Exact gradient").

    unitary mode     A = (H0' + sum_k u_k H_k') / 2^s,  P = sum_{j <= T} A^j / j!,  K = P^(2^s)
                     dP[E] = sum_{j=1..T} (1/j!) sum_{a < j} A^a E A^(j-1-a),  E = H_k' / 2^s;  each squaring X -> X^2 carries dX -> dX X + X dX
    state transfer   K = sum_{j <= T-1} B^j / j! (no scaling, as matvecexp),  dK[E] likewise with E = H_k'
    dL_du[k, t] = Re <Lambda_{t+1}, dK_t[E_k] Psi_t>   in place of the oracle's   Re <Lambda_{t+1}, H_k' Psi_{t+1}>

Psi_t enters slice t (Psi_0 = U0 V; the oracle's inter_vecs[0] holds V), Lambda_{t+1} is the costate of the oracle's own backward recursion (forbidden
levels and speed_up sources included).  Regularisers and the chain rule cos(base) (maxA dL_du + dR/dw) are the oracle's.  The composed versions
for an ensemble and for a pulse response are tests/robust_reference.py: composed / composed_shaped with this `evaluate` in the oracle's place."""
import numpy as np

from oracle import grape_oracle as go


def poly_and_derivative(A, E, degree):
    """P = sum_{j <= degree} A^j / j! and its derivative along E."""
    n = len(A)
    term = np.eye(n, dtype=complex)
    dterm = np.zeros((n, n), dtype=complex)
    P, dP, f = term.copy(), dterm.copy(), 1.0
    for j in range(1, degree + 1):
        dterm = dterm @ A + term @ E
        term = term @ A
        f *= j
        P = P + term / f
        dP = dP + dterm / f
    return P, dP


def exact_dL_du(sp, base, o):
    """dL_du (k x steps) of the exact gradient, from the oracle's evaluation `o` (want_inter=True) at `base`."""
    k, steps, m = sp.k, sp.steps, sp.m
    T, s = sp.exp_terms, sp.scaling
    u, inter, Hs = o['uks'], o['inter_vecs'], sp.Hs
    need = ('forbidden_coeff_list' in sp.reg_coeffs) or ('speed_up' in sp.reg_coeffs)
    S = go.state_regularisers(sp, inter)[1] if need else None
    z = np.sum(inter[steps] * np.conj(sp.W))
    lam = (-2.0 / m ** 2) * z * sp.W
    if S is not None:
        lam = lam + S[steps]
    dL = np.zeros((k, steps))
    for t in range(steps - 1, -1, -1):
        if not sp.state_transfer:
            A = (Hs[0] + np.tensordot(u[:, t], Hs[1:], axes=1)) / 2.0 ** s
            psi_in = inter[t] if t > 0 else sp.U0 @ sp.V
            X = None
            for kk in range(k):
                X, dX = poly_and_derivative(A, Hs[kk + 1] / 2.0 ** s, T)
                for _ in range(s):
                    dX = dX @ X + X @ dX
                    X = X @ X
                dL[kk, t] = np.real(np.sum(np.conj(lam) * (dX @ psi_in)))
            lam = X.conj().T @ lam                               # X = K_t
        else:
            B = Hs[0] + np.tensordot(u[:, t], Hs[1:], axes=1)
            for kk in range(k):
                _, dK = poly_and_derivative(B, Hs[kk + 1], T - 1)
                dL[kk, t] = np.real(np.sum(np.conj(lam) * (dK @ inter[t])))
            lam = go.matvecexp(B, lam, T, sign=-1.0)
        if S is not None and t > 0:
            lam = lam + S[t]
    return dL


def evaluate(sp, base):
    """go.evaluate's dict with `grad`, `dL_du` and `grad_squared` replaced by the exact gradient's; `first_order_grad` keeps the oracle's."""
    base = np.asarray(base, dtype=np.float64).reshape(sp.k, sp.steps)
    o = go.evaluate(sp, base, want_inter=True)
    dL = exact_dL_du(sp, base, o)
    _, dR_dw = go.pulse_regularisers(sp, np.sin(base))
    grad = np.cos(base) * (sp.maxA[:, None] * dL + dR_dw)
    out = dict(o, first_order_grad=o['grad'])
    out.update(grad=grad, dL_du=dL, grad_squared=float(0.5 * np.sum(grad ** 2)))
    return out


def central_differences(sp, base, h=1e-6):
    g = np.zeros_like(base)
    for idx in np.ndindex(*base.shape):
        bp, bm = base.copy(), base.copy()
        bp[idx] += h
        bm[idx] -= h
        g[idx] = (go.evaluate(sp, bp, want_grad=False)['reg_loss'] - go.evaluate(sp, bm, want_grad=False)['reg_loss']) / (2 * h)
    return g


# ---- the rows of the issue's table (recipes of tests/test_hip_parity.py: parity_cases unless spelled out) ---------------------------------

ALLREG_N4 = {'dwdt': 0.1, 'forbidden_coeff_list': [5.0, 5.0], 'states_forbidden_list': [2, 3], 'speed_up': 0.3, 'amplitude': 0.2}
ALLREG_ST = {'dwdt': 0.1, 'forbidden_coeff_list': [5.0, 5.0], 'states_forbidden_list': [4, 5], 'speed_up': 0.3, 'amplitude': 0.2}


def table_rows():
    from tests.golden import cases
    rows = []
    c = cases.case_c2(n=4, k=2, steps=12, m=3, taylor=(6, 1), seed=2); c['total_time'] = 2.0; rows.append(('n4_T6s1', c))
    c = cases.case_c2(n=4, k=2, steps=12, m=3, taylor=(6, 1), seed=2); c['total_time'] = 2.0; c['reg_coeffs'] = dict(ALLREG_N4)
    rows.append(('n4_allreg', c))
    rows.append(('n8_T3s2', cases.case_c2(n=8, k=3, steps=10, m=4, taylor=(3, 2), seed=3)))
    rows.append(('n17_T6s2', cases.case_c2(n=17, k=3, steps=9, m=5, taylor=(6, 2), seed=4)))
    rows.append(('small_auto_U0', cases.case_small_auto()))
    rows.append(('dressed', cases.case_dressed()))
    c = cases.case_c3(n=6, k=3, steps=15, taylor=(8, 0)); c['total_time'] = 1.0; c['reg_coeffs'] = dict(ALLREG_ST)
    rows.append(('state_transfer_allreg', c))
    c = cases.case_c3(n=6, k=3, steps=15, taylor=(4, 0)); c['total_time'] = 1.0; rows.append(('st_T4', c))
    rows.append(('state_small', cases.case_state_small()))
    return rows


def perturbed_base(sp):
    """The second base of tests/test_hip_parity.py: test_eval_parity."""
    return 2.5 * np.random.default_rng(123).normal(size=sp.base0.shape) / np.sqrt(sp.steps) + 0.3
