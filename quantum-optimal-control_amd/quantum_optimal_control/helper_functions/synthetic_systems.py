"""Synthetic benchmark systems of SURVEY.md 8(d): seeded random Hamiltonians with the reference's problem shapes.

The reference ships no benchmark inputs (its examples are notebooks); these recipes produce the dicts of `Grape()` keyword
inputs that bench.py, tools/ and the parity tests all share.  Only INPUT construction lives here.
"""
import numpy as np


def herm(rng, n):
    A = rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))
    H = (A + A.conj().T) / 2
    return H / np.linalg.norm(H, 2)


def random_unitary(rng, n):
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n)))
    return Q


def case_c2(n=32, k=4, steps=500, m=8, taylor=(5, 3), seed=0):
    """SURVEY 8(d) C2 recipe (also used, scaled down, for quick parity cases)."""
    rng = np.random.default_rng(seed)
    H0 = 2 * np.pi * 2 * herm(rng, n)
    Hops = [0.2 * 2 * np.pi * 2 * herm(rng, n) for _ in range(k)]
    U = random_unitary(rng, n)
    return dict(H0=H0, Hops=Hops, Hnames=['h%d' % i for i in range(k)], U=U, total_time=100.0 * steps / 500.0,
                steps=steps, states_concerned_list=list(range(m)), maxA=[4.0] * k, reg_coeffs={},
                Taylor_terms=list(taylor) if taylor is not None else None, state_transfer=False, initial_guess=None,
                dressed_info=None, U0=None, np_seed=seed)


def case_c3(n=64, k=6, steps=1000, taylor=(10, 0), seed=3):
    """state transfer e_0 -> e_1 with dwdt + forbidden regularisers."""
    rng = np.random.default_rng(seed)
    H0 = 2 * np.pi * 2 * herm(rng, n)
    Hops = [0.2 * 2 * np.pi * 2 * herm(rng, n) for _ in range(k)]
    e0 = np.zeros(n, dtype=complex); e0[0] = 1
    e1 = np.zeros(n, dtype=complex); e1[1] = 1
    return dict(H0=H0, Hops=Hops, Hnames=['h%d' % i for i in range(k)], U=[e1], total_time=200.0 * steps / 1000.0,
                steps=steps, states_concerned_list=[e0], maxA=[4.0] * k,
                reg_coeffs={'dwdt': 1e-3, 'forbidden_coeff_list': [100, 100], 'states_forbidden_list': [n - 2, n - 1]},
                Taylor_terms=list(taylor) if taylor is not None else None, state_transfer=True, initial_guess=None,
                dressed_info=None, U0=None, np_seed=seed)


def xx_chain(spins, coupling=1.0, control_sites=None):
    """An XX spin chain as scipy.sparse operators built from Kronecker products (n = 2^spins; the sparse state-transfer route):
    H0 = (coupling / 2) sum_i (X_i X_{i+1} + Y_i Y_{i+1}), one control Z_i / 2 per site of `control_sites` (default: every site).
    Returns (H0, Hops, Hnames, excitation) with excitation(i) the basis state that has spin i up and the others down.  Site 0 is the
    leftmost Kronecker factor; no dense n x n array is formed."""
    import scipy.sparse as sps
    X = sps.csr_matrix(np.array([[0, 1], [1, 0]], dtype=np.complex128))
    Y = sps.csr_matrix(np.array([[0, -1j], [1j, 0]], dtype=np.complex128))
    Z = sps.csr_matrix(np.array([[1, 0], [0, -1]], dtype=np.complex128))

    def at(ops):
        """kron of identities with ops[i] at site i"""
        out = sps.identity(1, dtype=np.complex128, format='csr')
        for i in range(spins):
            out = sps.kron(out, ops.get(i, sps.identity(2, dtype=np.complex128, format='csr')), format='csr')
        return out

    n = 2 ** spins
    H0 = sps.csr_matrix((n, n), dtype=np.complex128)
    for i in range(spins - 1):
        H0 = H0 + (coupling / 2.0) * (at({i: X, i + 1: X}) + at({i: Y, i + 1: Y}))
    H0 = sps.csr_matrix(H0)
    H0.eliminate_zeros()                       # XX + YY cancels on the aligned pairs
    sites = list(range(spins)) if control_sites is None else list(control_sites)
    Hops = [sps.csr_matrix(0.5 * at({i: Z})) for i in sites]
    Hnames = ['z%d' % i for i in sites]

    def excitation(i):
        v = np.zeros(n, dtype=np.complex128)
        v[2 ** (spins - 1 - i)] = 1.0
        return v

    return H0, Hops, Hnames, excitation


def xx_bonds(spins, coupling=1.0):
    """The bonds of xx_chain one by one: spins - 1 scipy.sparse operators (coupling / 2) (X_i X_{i+1} + Y_i Y_{i+1}) whose sum is its H0 -- the
    perturbation operators of a chain whose couplings are known to a few percent (one offset per bond).  Built with scipy.sparse.kron; no dense
    n x n array is formed."""
    import scipy.sparse as sps
    X = sps.csr_matrix(np.array([[0, 1], [1, 0]], dtype=np.complex128))
    Y = sps.csr_matrix(np.array([[0, -1j], [1j, 0]], dtype=np.complex128))
    eye = lambda d: sps.identity(d, dtype=np.complex128, format='csr')
    bonds = []
    for i in range(spins - 1):
        pair = sps.kron(X, X, format='csr') + sps.kron(Y, Y, format='csr')
        op = sps.csr_matrix((coupling / 2.0) * sps.kron(sps.kron(eye(2 ** i), pair, format='csr'), eye(2 ** (spins - 2 - i)), format='csr'))
        op.eliminate_zeros()
        bonds.append(op)
    return bonds
