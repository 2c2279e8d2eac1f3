"""Host-side pre-processing of a GRAPE problem whose Hamiltonians are scipy.sparse matrices (the sparse state-transfer route).

A sibling of core/system_parameters.py with the same public attributes where they make sense, and the one rule of this route: no dense n x n array is
ever formed -- not the operators, not an identity, not a real-embedded copy.  What the reference's SystemParameters keeps as dense derived views
(``matrix_list``, ``H0``, ``ops``, ``initial_unitary``, ``identity``) does not exist here; the engine consumes ``ops_sparse``.

Taylor order: the reference's rule for n >= 10 (core/system_parameters.py:139-141) needs only max |(-i dt) H_max| over the entries of
H_max = H0 + sum_k maxA_k H_k, which a sparse sum gives over the stored entries.  This route uses that scalar rule at every n (the matrix rule of
n < 10 would densify); state transfer takes no squarings.
"""
import numpy as np
import scipy.sparse as sps

from quantum_optimal_control.core.system_parameters import MAX_TAYLOR_TERMS, MIN_TAYLOR_TERMS, SystemParameters, taylor_scalar
from quantum_optimal_control.helper_functions.grape_functions import c_to_r_vec


def is_sparse_problem(H0, Hops):
    """True when the drift or any control operator is a scipy.sparse matrix: the problem then takes the sparse route."""
    try:
        return bool(sps.issparse(H0) or any(sps.issparse(h) for h in Hops))
    except TypeError:
        return False


def as_csr(op):
    """One operator as complex CSR, whatever it came as (a dense control next to a sparse drift is converted once; it stays O(n^2) only if it was)."""
    return sps.csr_matrix(op, dtype=np.complex128)


def max_abs_entry(H0, Hops, maxA):
    """max |H_max| over the stored entries of H_max = H0 + sum_k maxA_k H_k (0 for an empty pattern)."""
    H_max = as_csr(H0)
    for amp, op in zip(maxA, Hops):
        H_max = H_max + float(amp) * as_csr(op)
    H_max = sps.csr_matrix(H_max)
    return float(np.max(np.abs(H_max.data))) if H_max.nnz else 0.0


def member_max_abs_entry(H0, Hops, amps, perturbations=(), offsets=()):
    """The rule above for one member of an ensemble: the largest stored entry of |H0 + sum_k amps_k H_k| + sum_q |offsets_q| |P_q|.  The
    perturbations enter by their absolute values, entry for entry, so the figure bounds the largest entry of the member's H_max whatever the signs
    of its offsets (and equals max_abs_entry without perturbations).  Sparse sums only: no n x n array."""
    H_max = as_csr(H0)
    for amp, op in zip(amps, Hops):
        H_max = H_max + float(amp) * as_csr(op)
    bound = abs(sps.csr_matrix(H_max))
    for off, p in zip(offsets, perturbations):
        bound = bound + abs(float(off)) * abs(as_csr(p))
    bound = sps.csr_matrix(bound)
    return float(np.max(np.abs(bound.data))) if bound.nnz else 0.0


def choose_taylor_members(H0, Hops, maxA, devices, dt, steps, unitary_error, control_map=None):
    """The Taylor order of a sparse ensemble, fleet or mapped problem: choose_taylor_terms on every member's own operators, the largest order wins
    (as robust.choose_taylor and fleet.choose_taylor take it for dense members).  devices: a list of validated ensemble dicts (one for
    Grape(robust=), one per device of a fleet), or [None]: the nominal member alone.  Member e runs the controls amp_scales[e, j] maxA_j -- under a
    control map the coefficient bounds control_map.coefficient_bounds gives for those pulse bounds, one per operator the map feeds -- and the
    perturbations |offsets[e, q]| |P_q|."""
    maxA = np.asarray(maxA, dtype=np.float64).reshape(-1)
    best = 0
    for dev in devices:
        members = 1 if dev is None else dev['weights'].shape[0]
        for e in range(members):
            scale = np.ones_like(maxA) if dev is None else np.abs(dev['amp_scales'][e])
            amps = scale * maxA
            if control_map is not None:
                from quantum_optimal_control.helper_functions.control_map import coefficient_bounds
                amps = coefficient_bounds(control_map, amps)
            perts = [] if dev is None else dev['operators']
            offs = [] if dev is None else dev['offsets'][e]
            x = dt * member_max_abs_entry(H0, Hops, amps, perts, offs)
            best = max(best, int(choose_taylor_terms(x, steps, unitary_error)))
    return best


def choose_taylor_terms(x, steps, unitary_error):
    """The reference's downward search (Choose_exp_terms) with the scalar metric, no squarings: the first term count that fails."""
    n_terms = MAX_TAYLOR_TERMS
    while True:
        metric = 1 + steps * np.abs((taylor_scalar(x, n_terms, 0) - np.exp(x)) / np.exp(x))
        if n_terms == MIN_TAYLOR_TERMS or not (np.abs(metric - 1.0) < unitary_error):
            return n_terms
        n_terms -= 1


class SparseSystemParameters(SystemParameters):
    """SystemParameters for scipy.sparse Hamiltonians, state transfer only."""

    sparse_route = True

    def __init__(self, H0, Hops, Hnames, U, total_time, steps, states_concerned_list, maxA, draw, initial_guess, show_plots, Unitary_error,
                 reg_coeffs, save, file_path, Taylor_terms, use_gpu, use_inter_vecs, members=None):
        # members: the validated ensemble dicts whose members the Taylor order has to serve (choose_taylor_members), or None: the nominal problem
        self.members = members
        self.sparse_U = self.sparse_H = self.sparse_K = False        # the reference's flags stay ignored under use_gpu
        self.use_inter_vecs = use_inter_vecs
        self.use_gpu = use_gpu
        self.Taylor_terms = Taylor_terms
        self.dressed_info = None
        self.reg_coeffs = reg_coeffs
        self.file_path = file_path
        self.state_transfer = True
        self.no_scaling = True
        self.save = save
        self.H0_c = as_csr(H0)
        self.ops_c = [as_csr(op) for op in Hops]
        self.ops_max_amp = maxA
        self.Hnames = Hnames
        self.Hnames_original = Hnames
        self.total_time = total_time
        self.steps = steps
        self.show_plots = show_plots
        self.Unitary_error = Unitary_error
        self.states_concerned_list = states_concerned_list
        self.U0_c = None
        self.draw_list, self.draw_names = (draw[0], draw[1]) if draw is not None else ([], [])
        self.state_num = self.H0_c.shape[0]
        for op in [self.H0_c] + self.ops_c:
            if op.shape != (self.state_num, self.state_num):
                raise ValueError('Grape: every operator must be %d x %d, got %s' % (self.state_num, self.state_num, op.shape))

        self._transform_guess(initial_guess)
        self._unpack_dressed(None)
        self.target_vectors = [c_to_r_vec(np.asarray(vec)) for vec in U]
        self.dt = float(total_time) / steps
        self._build_initial_vectors()
        self._build_operators()
        self._build_envelope()
        self._build_guess()
        if save:
            self._log_setup()

    def _build_operators(self):
        """-i dt H for the drift and every control as CSR, and the Taylor order by the scalar rule."""
        self.ops_len = len(self.ops_c)
        self.ops_sparse = [sps.csr_matrix(-1j * self.dt * op) for op in [self.H0_c] + self.ops_c]
        self.scaling = 0
        if self.Taylor_terms is None and self.members is not None:
            self.exp_terms = choose_taylor_members(self.H0_c, self.ops_c, self.ops_max_amp, self.members, self.dt, self.steps, self.Unitary_error)
        elif self.Taylor_terms is None:
            x = self.dt * max_abs_entry(self.H0_c, self.ops_c, self.ops_max_amp)
            self.exp_terms = choose_taylor_terms(x, self.steps, self.Unitary_error)
        else:
            self.exp_terms = self.Taylor_terms[0]
        print("Using " + str(self.exp_terms) + " Taylor terms and " + str(self.scaling) + " Scaling & Squaring terms")

    def engine_inputs(self):
        """(sparse operators, None, V, W, None): the engine's inputs on the sparse route."""
        n = self.state_num
        V = np.stack([np.asarray(v, dtype=np.complex128) for v in self.initial_vectors_c], axis=1)
        W = np.stack([tv[:n] + 1j * tv[n:] for tv in self.target_vectors], axis=1)
        return self.ops_sparse, None, V, W, None
