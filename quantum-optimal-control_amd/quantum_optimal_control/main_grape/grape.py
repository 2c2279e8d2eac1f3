"""Grape() -- drop-in entry point of the MI355X-native GRAPE engine.

Signature, defaults, return value and error behaviour follow the reference's main_grape/grape.py:19-139; the
TensorFlow graph + session underneath are replaced by libqoc_hip.so (hand-written HIP kernels, complex fp64).
Differences that a caller can observe are listed in INTEGRATION.md (no live matplotlib figure; `use_gpu=False`
still runs on the MI355X because there is no CPU engine; HDF5 logging needs h5py).
"""
import os
import time

import numpy as np

from quantum_optimal_control.core.convergence import Convergence
from quantum_optimal_control.core.hip_state import HipState
from quantum_optimal_control.core.run_session import run_session
from quantum_optimal_control.core.system_parameters import SystemParameters

_TIME_UNITS = {"GHz": "ns", "MHz": "us", "KHz": "ms", "Hz": "s"}


def _next_free_log(data_path, file_name):
    number = 0
    while os.path.exists(os.path.join(data_path, str(number).zfill(5) + "_" + file_name + ".h5")):
        number += 1
    return os.path.join(data_path, str(number).zfill(5) + "_" + file_name + ".h5")


def _dump_inputs(file_path, H0, Hops, Hnames, U, total_time, steps, states_concerned_list, use_gpu, sparse_H,
                 sparse_U, sparse_K, maxA, initial_guess, method, convergence, reg_coeffs, dressed_info, control_map=None):
    from quantum_optimal_control.helper_functions.data_management import H5File
    with H5File(file_path) as hf:
        if _is_sparse(H0, Hops):
            # the sparse route: every operator as CSR arrays <name>_data / _indices / _indptr, never as an n x n dataset
            import scipy.sparse as sps
            for name, op in [('H0', H0)] + [('Hops_%d' % i, h) for i, h in enumerate(Hops)]:
                csr = sps.csr_matrix(op)
                for part in ('data', 'indices', 'indptr'):
                    hf.add(name + '_' + part, data=getattr(csr, part))
            hf.add('state_num', data=sps.csr_matrix(H0).shape[0])
            H0 = Hops = None
        for key, val in (('H0', H0), ('Hops', Hops), ('Hnames', Hnames), ('U', U), ('total_time', total_time),
                         ('steps', steps), ('states_concerned_list', states_concerned_list), ('use_gpu', use_gpu),
                         ('sparse_H', sparse_H), ('sparse_U', sparse_U), ('sparse_K', sparse_K)):
            if val is not None:
                hf.add(key, data=val)
        if maxA is not None:
            hf.add('maxA', data=maxA)
        if initial_guess is not None:
            hf.add('initial_guess', data=initial_guess)
        hf.add('method', method)
        if control_map is not None:
            # a control map (Hops are then the operators it feeds): alpha always, mix and fixed where the map has them
            hf.add('control_map_alpha', data=control_map.alpha)
            for key in ('mix', 'fixed'):
                if getattr(control_map, key) is not None:
                    hf.add('control_map_' + key, data=getattr(control_map, key))
        group = hf.create_group('convergence')
        for key, val in convergence.items():          # like the reference this needs a dict when save=True
            group.create_dataset(key, data=val)
        for name, mapping in (('reg_coeffs', reg_coeffs), ('dressed_info', dressed_info)):
            if mapping is not None:
                group = hf.create_group(name)
                for key, val in mapping.items():
                    group.create_dataset(key, data=val)


def _is_sparse(H0, Hops):
    """The drift or a control operator is a scipy.sparse matrix: the call takes the sparse state-transfer route."""
    from quantum_optimal_control.core.sparse_parameters import is_sparse_problem
    return is_sparse_problem(H0, Hops)


def _sparse_call(args, kwargs):
    """Whether a Grape call, by its positional and keyword arguments, takes the sparse route."""
    H0 = kwargs['H0'] if 'H0' in kwargs else (args[0] if len(args) > 0 else None)
    Hops = kwargs['Hops'] if 'Hops' in kwargs else (args[1] if len(args) > 1 else [])
    return H0 is not None and _is_sparse(H0, Hops)


def _is_lbfgs(args, kwargs):
    """method='LBFGS' (the device-resident L-BFGS loop) among the arguments of a Grape call, by keyword or by position."""
    method = kwargs['method'] if 'method' in kwargs else (args[20] if len(args) > 20 else 'Adam')
    return str(method).upper() == 'LBFGS'


def Grape(H0, Hops, Hnames, U, total_time, steps, states_concerned_list, convergence=None, U0=None, reg_coeffs=None,
          dressed_info=None, maxA=None, use_gpu=True, sparse_H=True, sparse_U=False, sparse_K=False, draw=None,
          initial_guess=None, show_plots=True, unitary_error=1e-4, method='Adam', state_transfer=False,
          no_scaling=False, freq_unit='GHz', file_name=None, save=True, data_path=None, Taylor_terms=None,
          use_inter_vecs=True, restarts=1, plan_seeds=None, time_comm=None, robust=None, *, transfer=None, exact_gradient=False, collapse_ops=None, control_map=None, fleet=None, running_costs=None, _first_seed=0, _device=0, _return_session=False, _restart_info=None):
    """Reference signature (main_grape/grape.py:19) plus one optional extension: ``restarts=B`` optimises B control sets at
    once on the GPU -- the first is the reference's own initial guess (same NumPy RNG draw / ``initial_guess``), the others
    are independent N(0, 1/sqrt(steps)) restarts -- and returns the (uks, U_final) of the best final fidelity.

    ``method='LBFGS'`` (extension): the device-resident L-BFGS loop -- every control set runs its own quasi-Newton search (history of
    ``convergence['lbfgs_history']`` = 8 curvature pairs, backtracking Armijo line search with ``lbfgs_c1`` = 1e-4, direction reset after
    ``lbfgs_max_ls`` = 20 rejected trials) on the GPU, objective reg_loss, stop rule and progress rows as for ``'Adam'``; ``max_iterations``
    bounds the evaluations (at most two more are spent on ending at an accepted point).  With ``restarts=R`` these are R independent runs and the
    best is returned.  No bounds, no strong-Wolfe search: ``'L-BFGS-B'`` and ``'BFGS'`` remain scipy's, one control set, one host round trip per
    evaluation.  The default first-order gradient differs by O(dt) from the derivative of the reported loss, so that for few, long
    slices the Armijo test starts refusing steps before the target is reached: pass ``exact_gradient=True`` there.  Works with ``restarts``,
    ``robust``, ``transfer``, ``exact_gradient`` and ``collapse_ops``; not with ``time_comm`` or the sharded entry points.

    ``robust`` (robust GRAPE): a dict with keys ``operators`` (q Hermitian n x n matrices P_q), ``offsets`` (E x q), ``amp_scales``
    (E x k, default ones) and ``weights`` (E, default uniform; normalised to sum 1), e.g. from helper_functions.robust.ensemble_grid.
    Member e has the drift H0 + sum_q offsets[e, q] P_q and the controls amp_scales[e, j] Hops[j]; the pulse is optimised for the
    weighted mean of the members' objectives, or, with an optional key ``risk`` (beta > 0), for their soft worst case (DESIGN.md 6b'):
    the reported loss and the stop rule then read that soft worst-case infidelity.  U_final is member 0's.

    ``transfer`` (transfer-function GRAPE): a helper_functions.transfer.Transfer (or a steps x P matrix): the variable is then the k x P
    samples an AWG plays, and the pulse the Hamiltonian sees is their response ``samples @ T.T``.  ``initial_guess`` is k x P sample
    amplitudes; the returned uks is the k x steps pulse, ``transfer.samples`` the k x P samples behind it.  The pulse regularisers
    (amplitude, dwdt, d2wdt2, bandpass) act on the samples; ``envelope`` is rejected.  Composes with ``robust``.

    ``exact_gradient`` (default False: the reference's first-order GRAPE gradient): True differentiates the slice propagators the engine
    computes -- truncated Taylor series and squarings included -- so that the loss and the gradient a driver sees belong to one function.
    It pays for few, long slices and for the scipy drivers, whose line searches assume exactly that; it costs more per evaluation
    (DESIGN.md).  Works with every ``method``, with ``restarts``, ``robust``, ``transfer`` and GrapeSharded; not with ``time_comm``.

    scipy.sparse Hamiltonians (sparse state transfer): when ``H0`` or any of ``Hops`` is a scipy.sparse matrix the call takes the sparse route --
    ``state_transfer=True`` is required (ValueError otherwise), every operator is kept sparse from here to the GPU (no n x n array is formed: spin chains
    and cavity arrays of n = 2^10 .. 2^14 levels run at their natural size), the Taylor order comes from the reference's rule for n >= 10 on the stored
    entries, and ``save=True`` logs the operators as ``<name>_data / _indices / _indptr``.  Works with every ``method`` and with ``restarts``; not with
    ``robust``, ``transfer``, ``exact_gradient``, ``collapse_ops``, ``time_comm``, ``dressed_info``, ``U0`` or the sharded entry points.  Dense inputs
    behave as before (``sparse_H`` / ``sparse_U`` / ``sparse_K`` stay ignored under ``use_gpu``).

    ``collapse_ops`` (open-system GRAPE): a list of n x n collapse operators that carry the square root of their rates, e.g. from
    helper_functions.open_system (``relaxation``, ``dephasing``).  The pulse is then scored and optimised under the Lindblad master equation
    d rho/dt = -i [H, rho] + sum_j (C_j rho C_j^dagger - 1/2 {C_j^dagger C_j, rho}): the loss is 1 - (1/m^2) sum_ij Re Tr(sigma_ij^dagger rho_ij(T)) over
    the operators rho_ij(0) = psi_i psi_j^dagger of the states of interest and sigma_ij = w_i w_j^dagger of their targets -- the closed loss when the
    list is empty.  Returns ``(uks, rho_final)`` with ``rho_final`` of shape (m, m, n, n): ``rho_final[i, i]`` is the density matrix that state i
    ends in, ``rho_final[i, j]`` the propagated coherence psi_i psi_j^dagger.  Taylor order and sub-steps come from
    open_system.choose_taylor unless ``Taylor_terms=(T, s)`` is given (degree T, 2^s sub-steps per slice, in both modes).  Works with every
    ``method`` (``'EVOLVE'`` with ``initial_guess=uks`` scores an existing pulse under decay) and with ``restarts``; not with ``robust``,
    ``transfer``, ``exact_gradient``, ``time_comm``, forbidden-level / ``speed_up`` regularisers, ``dressed_info`` or the sharded entry points.

    ``control_map`` (control maps): a helper_functions.control_map.ControlMap -- the coefficients of the Hamiltonian as functions of the pulses,
    c_i[t] = F[i, t] + sum_j M[i, j, t] p_ij(v_j[t]) with polynomials p_ij: crosstalk between lines, carriers, fixed drives, a compressing amplifier
    (``linear``, ``carriers``, ``fixed``, ``polynomial`` and their combinations).  ``Hops`` are then the r operators the map feeds, while ``Hnames``,
    ``maxA`` and ``initial_guess`` have one entry per pulse (k of them, r need not equal k) and the returned uks is k x steps; afterwards
    ``control_map.coefficients`` holds the r x steps coefficients the nominal Hamiltonian ran on.  The pulse regularisers act on the pulses, the
    Taylor order is chosen for the largest coefficients the map can deliver.  Works with every ``method``, with ``restarts``, ``robust``,
    ``transfer`` and ``exact_gradient``; not with ``collapse_ops``, scipy.sparse Hamiltonians, ``time_comm`` or the sharded entry points.

    ``fleet`` (device fleets): a helper_functions.fleet.Fleet (``fleet.devices``, ``fleet.around``) -- F devices that differ in their drift offsets and
    drive scales, each an ensemble of E members (E = 1: one Hamiltonian per device).  One engine then optimises a pulse for every device, ``restarts=R``
    control sets each, and the call returns ``(uks, U_final)`` with a leading device axis: ``uks[f]`` is the k x steps pulse of device f's best control
    set (the smallest loss of its R, the first of equals), ``U_final[f]`` member 0's final unitary under it.  Control set (f, r) starts where control
    set r of the same call without a fleet starts; ``initial_guess`` may also be (F, k, steps), one guess per device.  Afterwards the fleet carries
    ``losses`` (F,), ``best`` (F,), ``member_losses`` (F, E) and ``iterations`` (F,); ``transfer.samples`` is (F, k, P) and ``control_map.coefficients``
    (F, r, steps).  The Taylor order is the largest any member of any device would get.  ``method`` is ``'Adam'``, ``'LBFGS'`` or ``'EVOLVE'`` (the
    scan of one pulse over the devices).  Works with ``transfer``, ``control_map`` and ``exact_gradient``; not with ``robust`` (a fleet carries its own
    members: ``fleet.around``), ``collapse_ops``, scipy.sparse Hamiltonians, ``time_comm``, ``plan_seeds`` or the sharded entry points.

    Decay per member (open-system ensembles and fleets): a member of an ensemble, or a device of a fleet, is a Hamiltonian AND its decay.  A ``robust``
    dict may carry the keys ``collapse_ops`` (as the keyword above takes them) and ``rate_scales`` (E x c, default ones), a fleet ``collapse_ops`` and
    ``rate_scales`` (F x E x c; ``fleet.devices(..., collapse_ops=, rate_scales=)``, ``fleet.around``): member e of device f then decays through
    sqrt(rate_scales[f, e, j]) C_j (a scale of 0 switches the channel off), every member is scored under its own master equation as ``collapse_ops``
    defines it, and the members are combined as ``robust`` and ``fleet`` define it.  ``Grape(robust=ens)`` then returns ``(uks, rho_final)`` of member 0,
    (m, m, n, n); ``Grape(fleet=fl)`` returns them with a leading device axis and fills ``fl.losses``, ``best``, ``member_losses`` and ``iterations`` as
    without decay.  Taylor order and sub-steps: the largest that open_system.choose_taylor gives any member, unless ``Taylor_terms=(T, s)``.  Methods:
    ``'Adam'``, ``'LBFGS'``, ``'EVOLVE'`` and, on a robust call, scipy's.  Works with ``transfer``, ``control_map`` and ``restarts``; not with the
    ``collapse_ops`` keyword itself, ``exact_gradient``, ``dressed_info``, forbidden-level / ``speed_up`` / ``forbid_dressed`` regularisers,
    ``time_comm``, scipy.sparse Hamiltonians or the sharded entry points (ValueError, before the library is loaded).

    ``running_costs`` (open-system running costs): a list of at most 16 records from helper_functions.open_system -- ``level_cost(n, level, coeff)``,
    ``subspace_cost(n, levels, coeff)``, ``observable_cost(O, coeff)``, ``dressed_level_cost(v, coeff)``, each with ``power=2`` (or 1).  With
    x_i(tau) = Re Tr(O rho_ii(tau)) of every state of interest at every slice boundary tau = 0 .. steps, a record adds
    (coeff / steps) sum_tau sum_i x_i(tau)^power / power to the objective (reg_loss; the stop rule keeps reading the loss): "keep the resonator empty",
    "stay out of everything above the computational subspace", a truncation guard on the top level.  ``level_cost`` with power 2 is what
    ``reg_coeffs['forbidden_coeff_list']`` is on a closed engine.  Needs an open engine: ``collapse_ops=`` (``[]`` is the closed limit), or a ``robust``
    dict or a ``fleet`` that carries ``collapse_ops``; it then works with whatever that call works with.  Anything else: ValueError, before the library
    is loaded.  The gradient of the term is first order in dt, as the engine's is.

    Noise traces (time-dependent perturbations): a ``robust`` dict may carry the key ``traces`` (E x q x steps), a fleet ``traces`` (F x E x q x steps;
    ``fleet.devices(..., traces=)``, ``fleet.around``): at slice t member e then has the drift H0 + sum_q (offsets[e, q] + traces[e, q, t]) P_q --
    sampled noise trajectories whose correlation time is comparable to the gate (helper_functions.noise: ``ornstein_uhlenbeck``, ``one_over_f``,
    ``colored``, and ``noise.ensemble`` for the dict), which neither a constant offset nor a collapse operator models.  The pulse is optimised for the
    sample average (with ``risk``: the soft worst case) over this fixed set of traces; fresh draws during a run are an engine-level matter
    (``HipEngine.set_traces`` between bursts of ``iterate``).  The number of slices is checked before the library is loaded; the Taylor order uses,
    per member and operator, the value of offsets + traces[t] of largest magnitude over t; ``save=True`` logs ``robust_traces`` (``fleet_traces``).
    Works with whatever the robust or fleet call works with: ``restarts``, ``transfer``, ``control_map``, ``exact_gradient``, risk, decay per member,
    ``running_costs``, ``'Adam'``, ``'LBFGS'``, ``'EVOLVE'`` and, on a robust call, scipy's methods."""
    grape_start_time = time.time()
    time_unit = _TIME_UNITS[freq_unit]                  # KeyError on an unknown unit, as in the reference
    sparse = _is_sparse(H0, Hops)
    fleet_guess = None
    if fleet is not None:
        # device fleets: refused before anything is built (and before the library is loaded)
        for name, given in (('robust (a fleet carries its own members: fleet.around)', robust is not None),
                            ('scipy.sparse Hamiltonians (sparse state transfer)', sparse), ('collapse_ops (open-system GRAPE)', collapse_ops is not None),
                            ('time_comm', time_comm is not None)):
            if given:
                raise ValueError('Grape: fleet does not combine with %s' % name)
        if _first_seed != 0 or plan_seeds is not None:
            raise ValueError('Grape: fleet does not run sharded (plan_seeds, _first_seed, GrapeSharded)')
        if str(method).upper() not in ('ADAM', 'LBFGS', 'EVOLVE'):
            raise ValueError("Grape: fleet runs under method='Adam', 'LBFGS' or 'EVOLVE'; %r is scipy's, one control set" % (method,))
        if initial_guess is not None and np.ndim(initial_guess) == 3:
            # one guess per device: device 0's goes the way of every guess, the others follow it below
            fleet_guess = np.asarray(initial_guess, dtype=np.float64)
            initial_guess = fleet_guess[0]
    if sparse:
        # the sparse state-transfer route: refused before anything is built (and before the library is loaded)
        if not state_transfer:
            raise ValueError('Grape: scipy.sparse Hamiltonians need state_transfer=True (unitary mode propagates an n x n matrix)')
        for name, given in (('robust', robust is not None), ('transfer', transfer is not None), ('exact_gradient', bool(exact_gradient)),
                            ('collapse_ops', collapse_ops is not None), ('time_comm', time_comm is not None), ('dressed_info', dressed_info is not None)):
            if given:
                raise ValueError('Grape: scipy.sparse Hamiltonians (sparse state transfer) do not combine with %s' % name)
        if U0 is not None:
            raise ValueError('Grape: scipy.sparse Hamiltonians take no U0 (state transfer starts from the given vectors)')
        if _first_seed != 0 or plan_seeds is not None:
            raise ValueError('Grape: scipy.sparse Hamiltonians do not run sharded (GrapeSharded)')
    if collapse_ops is not None:
        from quantum_optimal_control.helper_functions import open_system as _open
        for name, given in (('robust', robust is not None), ('transfer', transfer is not None), ('exact_gradient', bool(exact_gradient)),
                            ('time_comm', time_comm is not None), ('dressed_info', dressed_info is not None),
                            ('the forbidden-level regulariser', reg_coeffs is not None and 'forbidden_coeff_list' in reg_coeffs),
                            ('the speed_up regulariser', reg_coeffs is not None and 'speed_up' in reg_coeffs),
                            ('forbid_dressed', reg_coeffs is not None and 'forbid_dressed' in reg_coeffs)):
            if given:
                raise ValueError('Grape: collapse_ops (open-system GRAPE) does not combine with %s' % name)
        if _first_seed != 0 or plan_seeds is not None:
            raise ValueError('Grape: collapse_ops (open-system GRAPE) does not run sharded (GrapeSharded)')
        collapse_ops = _open.validate(collapse_ops, len(H0))
    n_pulses = len(Hops)
    if control_map is not None:
        # control maps: refused before anything is built (and before the library is loaded)
        from quantum_optimal_control.helper_functions import control_map as _cmap
        for name, given in (('collapse_ops (open-system GRAPE)', collapse_ops is not None), ('scipy.sparse Hamiltonians (sparse state transfer)', sparse),
                            ('time_comm', time_comm is not None)):
            if given:
                raise ValueError('Grape: control_map does not combine with %s' % name)
        if _first_seed != 0 or plan_seeds is not None:
            raise ValueError('Grape: control_map does not run sharded (GrapeSharded)')
        _given_map = control_map                       # (validate returns a normalised copy: the caller's object gets .coefficients)
        control_map = _cmap.validate(control_map, r=len(Hops), steps=steps)
        n_pulses = control_map.n_pulses
        for name, seq in (('Hnames', Hnames), ('maxA', maxA), ('initial_guess', None if transfer is not None else initial_guess)):
            if seq is not None and len(seq) != n_pulses:
                raise ValueError('Grape: with a control map %s has one entry per pulse (%d), got %d' % (name, n_pulses, len(seq)))
    if fleet is not None:
        from quantum_optimal_control.helper_functions import fleet as _fleet
        _given_fleet = fleet                           # (validate returns a normalised copy: the caller's object gets the results)
        fleet = _fleet.validate(fleet, len(H0), n_pulses, steps=steps)
        if fleet_guess is not None and (fleet_guess.shape[0] != fleet.n_devices or fleet_guess.shape[1] != n_pulses):
            raise ValueError('Grape: a per-device initial guess of a fleet is (%d, %d, ...), got %s' % (fleet.n_devices, n_pulses, fleet_guess.shape))
    if str(method).upper() == 'LBFGS' and time_comm is not None:
        raise ValueError("Grape: method='LBFGS' cannot be time-sharded (time_comm)")
    if exact_gradient and time_comm is not None:
        raise ValueError('Grape: the exact gradient cannot be time-sharded (time_comm)')
    if robust is not None:
        from quantum_optimal_control.helper_functions import robust as _robust
        if time_comm is not None:
            raise ValueError('Grape: robust ensembles cannot be time-sharded (time_comm)')
        robust = _robust.validate(robust, len(H0), n_pulses, steps=steps)
    decay_devices = None                               # decay per member: the validated member dicts, one per device
    if fleet is not None and fleet.has_decay:
        decay_devices, _who = [fleet.device(f) for f in range(fleet.n_devices)], 'a fleet with decay'
    elif robust is not None and _robust.has_decay(robust):
        decay_devices, _who = [robust], 'a robust ensemble with decay'
    if decay_devices is not None:
        # what collapse_ops= refuses, refused here too: before anything is built (and before the library is loaded)
        from quantum_optimal_control.helper_functions import open_system as _open
        for name, given in (('exact_gradient', bool(exact_gradient)), ('time_comm', time_comm is not None), ('dressed_info', dressed_info is not None),
                            ('scipy.sparse Hamiltonians (sparse state transfer)', sparse),
                            ('the forbidden-level regulariser', reg_coeffs is not None and 'forbidden_coeff_list' in reg_coeffs),
                            ('the speed_up regulariser', reg_coeffs is not None and 'speed_up' in reg_coeffs),
                            ('forbid_dressed', reg_coeffs is not None and 'forbid_dressed' in reg_coeffs)):
            if given:
                raise ValueError('Grape: %s (open-system GRAPE) does not combine with %s' % (_who, name))
        if _first_seed != 0 or plan_seeds is not None:
            raise ValueError('Grape: %s (open-system GRAPE) does not run sharded (GrapeSharded)' % _who)
    if running_costs is not None:
        # running costs: an open engine's term, refused everywhere else before anything is built (and before the library is loaded)
        from quantum_optimal_control.helper_functions import open_system as _open
        if collapse_ops is None and decay_devices is None:
            raise ValueError("Grape: running_costs need an open engine (collapse_ops=, or a robust dict or a fleet that carries collapse_ops); closed "
                             "engines take reg_coeffs['forbidden_coeff_list']")
        running_costs = _open.validate_costs(running_costs, len(H0))
    if transfer is not None:
        from quantum_optimal_control.helper_functions import transfer as _transfer
        if time_comm is not None:
            raise ValueError('Grape: a transfer function cannot be time-sharded (time_comm)')
        transfer = _transfer.validate(transfer, steps)
        if reg_coeffs is not None and 'envelope' in reg_coeffs:
            raise ValueError('Grape: the envelope regulariser is defined per time slice; it cannot act on the samples of a transfer function')
    if use_gpu:
        sparse_H = sparse_U = sparse_K = False          # dense kernels only

    file_path = None
    if save:
        if file_name is None:
            raise ValueError('Grape function input: file_name, is not specified.')
        if data_path is None:
            raise ValueError('Grape function input: data_path, is not specified.')
        file_path = _next_free_log(data_path, file_name)
        print("data saved at: " + str(file_path))
        _dump_inputs(file_path, H0, Hops, Hnames, U, total_time, steps, states_concerned_list, use_gpu, sparse_H,
                     sparse_U, sparse_K, maxA, initial_guess, method, convergence, reg_coeffs, dressed_info, control_map=control_map)
        if robust is not None:
            from quantum_optimal_control.helper_functions.data_management import H5File
            with H5File(file_path) as hf:
                q = len(robust['operators'])
                hf.add('robust_operators', data=np.array(robust['operators']).reshape(q, len(H0), len(H0)))
                for key in ('offsets', 'amp_scales', 'weights'):
                    hf.add('robust_' + key, data=robust[key])
                if robust['risk'] > 0:
                    hf.add('robust_risk', data=np.array([robust['risk']]))
                if _robust.has_decay(robust):
                    c = len(robust['collapse_ops'])
                    hf.add('robust_collapse_ops', data=np.array(robust['collapse_ops'], dtype=np.complex128).reshape(c, len(H0), len(H0)))
                    hf.add('robust_rate_scales', data=robust['rate_scales'])
                if 'traces' in robust:
                    hf.add('robust_traces', data=robust['traces'])
        if transfer is not None:
            from quantum_optimal_control.helper_functions.data_management import H5File
            with H5File(file_path) as hf:
                hf.add('transfer_matrix', data=transfer.matrix)
        if exact_gradient:
            from quantum_optimal_control.helper_functions.data_management import H5File
            with H5File(file_path) as hf:
                hf.add('exact_gradient', data=np.array(1))
        if fleet is not None:
            from quantum_optimal_control.helper_functions.data_management import H5File
            with H5File(file_path) as hf:
                hf.add('fleet_offsets', data=fleet.offsets)
                hf.add('fleet_amp_scales', data=fleet.amp_scales)
                if fleet.has_decay:
                    c = len(fleet.collapse_ops)
                    hf.add('fleet_collapse_ops', data=np.array(fleet.collapse_ops, dtype=np.complex128).reshape(c, len(H0), len(H0)))
                    hf.add('fleet_rate_scales', data=fleet.rate_scales)
                if fleet.traces is not None:
                    hf.add('fleet_traces', data=fleet.traces)
        if collapse_ops is not None:
            from quantum_optimal_control.helper_functions.data_management import H5File
            with H5File(file_path) as hf:
                hf.add('collapse_ops', data=np.array(collapse_ops, dtype=np.complex128).reshape(len(collapse_ops), len(H0), len(H0)))
        if running_costs is not None:
            from quantum_optimal_control.helper_functions.data_management import H5File
            with H5File(file_path) as hf:
                hf.add('running_cost_observables', data=np.array([r[0] for r in running_costs], dtype=np.complex128).reshape(len(running_costs), len(H0), len(H0)))
                hf.add('running_cost_coeffs', data=np.array([r[1] for r in running_costs], dtype=np.float64))
                hf.add('running_cost_powers', data=np.array([r[2] for r in running_costs], dtype=np.int32))

    if U0 is None and not sparse:
        U0 = np.identity(len(H0))
    if convergence is None:
        convergence = {'rate': 0.01, 'update_step': 100, 'max_iterations': 5000, 'conv_target': 1e-8,
                       'learning_rate_decay': 2500}
    if maxA is None:
        if initial_guess is None:
            maxAmp = 4 * np.ones(n_pulses)
        else:
            maxAmp = 1.5 * np.max(np.abs(initial_guess if fleet_guess is None else fleet_guess)) * np.ones(n_pulses)
    else:
        maxAmp = maxA

    if decay_devices is not None and Taylor_terms is None:
        # the largest degree and sub-step count that the Lindblad rule gives any member, with its own Hamiltonians and scaled collapse operators
        from quantum_optimal_control.helper_functions.robust import taylor_view as _taylor_view
        Taylor_terms = _open.choose_taylor_members(H0, Hops, maxAmp, [_taylor_view(d) for d in decay_devices], float(total_time) / steps, steps, unitary_error,
                                                   control_map=control_map)

    if fleet is not None and Taylor_terms is None:
        # the largest Taylor order and squaring count any member of any device would get
        Taylor_terms = _fleet.choose_taylor(fleet, H0, Hops, control_map, maxAmp, U0, total_time, steps, unitary_error, state_transfer, no_scaling)

    if control_map is not None and Taylor_terms is None:
        # the chooser on (H0, Hops, cmax): the largest coefficients the map can deliver stand where maxA stands (every member's, with a robust ensemble)
        Taylor_terms = _cmap.choose_taylor(control_map, H0, Hops, None if robust is None else _robust.taylor_view(robust), maxAmp, U0, total_time, steps, unitary_error, state_transfer, no_scaling)

    if robust is not None and Taylor_terms is None:
        # the largest Taylor order and squaring count any member's own problem would get (both only lower the truncation error)
        Taylor_terms = _robust.choose_taylor(H0, Hops, robust, maxAmp, U0, total_time, steps, unitary_error, state_transfer, no_scaling)

    if collapse_ops is not None and Taylor_terms is None:
        Taylor_terms = _open.choose_taylor(H0, Hops, maxAmp, collapse_ops, float(total_time) / steps, steps, unitary_error)

    sample_base = None
    if transfer is not None and initial_guess is not None:
        # sample amplitudes -> the variable, by the reference's rule for a pulse (core/system_parameters.py: base = arcsin(u / maxA))
        guess = np.asarray(initial_guess, dtype=np.float64)
        if guess.shape != (n_pulses, transfer.n_samples):
            raise ValueError('Grape: with a transfer function the initial guess is (%d, %d) sample amplitudes, got %s'
                             % (n_pulses, transfer.n_samples, guess.shape))
        ratio = guess / np.asarray(maxAmp, dtype=np.float64)[:, None]
        for row in range(len(ratio)):
            if max(ratio[row]) > 1.0:
                raise ValueError('Initial guess has strength > max_amp for op %d' % (row))
        sample_base = np.arcsin(ratio)

    if sparse:
        from quantum_optimal_control.core.sparse_parameters import SparseSystemParameters
        sys_para = SparseSystemParameters(H0, Hops, Hnames, U, total_time, steps, states_concerned_list, maxAmp, draw, initial_guess, show_plots,
                                          unitary_error, reg_coeffs, save, file_path, Taylor_terms, use_gpu, use_inter_vecs)
    elif control_map is not None:
        # SystemParameters counts controls by the operators; with a map the variable, maxA, the envelope and the names belong to the k pulses.  It is
        # built for the r operators (Taylor order fixed above, no guess, the NumPy RNG left where it was) and the pulse side is then set in its place
        rng_state = np.random.get_state()
        sys_para = SystemParameters(H0, Hops, Hnames, U, U0, total_time, steps, states_concerned_list, dressed_info,
                                    _cmap.coefficient_bounds(control_map, maxAmp), draw, None, show_plots, unitary_error, state_transfer, no_scaling,
                                    reg_coeffs, save, file_path, Taylor_terms, use_gpu, use_inter_vecs, sparse_H, sparse_U, sparse_K)
        np.random.set_state(rng_state)
        sys_para.ops_max_amp = maxAmp
        sys_para.ops_len = n_pulses
        sys_para._build_envelope()
        sys_para._transform_guess(None if transfer is not None else initial_guess)
        sys_para._build_guess()
    else:
        sys_para = SystemParameters(H0, Hops, Hnames, U, U0, total_time, steps, states_concerned_list, dressed_info,
                                    maxAmp, draw, None if transfer is not None else initial_guess, show_plots, unitary_error, state_transfer, no_scaling,
                                    reg_coeffs, save, file_path, Taylor_terms, use_gpu, use_inter_vecs, sparse_H, sparse_U,
                                    sparse_K)
    # plan_seeds (extension): the batch size the engine plans its path / kernels / chunking for instead of `restarts` (None: its own batch,
    # the fastest choice for this process).  GrapeSharded passes hip_engine.plan_seeds_for(all restarts), so that a restart evolves
    # bit-identically under any rank count; Grape(restarts=R, plan_seeds=hip_engine.plan_seeds_for(R)) reproduces a sharded run in one process.
    # time_comm (extension): a hip_engine.QocComm whose ranks share ONE large trajectory along the time axis (GrapeTimeSharded below)
    if transfer is not None:
        # the variable is k x P; drawn after SystemParameters' own draw, so that calls without a transfer keep their RNG stream
        P = transfer.n_samples
        if sample_base is None:
            sample_base = np.random.normal(0, 1. / np.sqrt(P), [n_pulses, P])
        sys_para.ops_weight_base = sample_base
        sys_para.raw_shape = np.shape(sample_base)
    fleet_base = None
    if fleet_guess is not None:
        # every device's own first start point, by the rule its guess alone would go through (base = arcsin(u / maxA))
        width = steps if transfer is None else transfer.n_samples
        if fleet_guess.shape[2] != width:
            raise ValueError('Grape: a per-device initial guess of this fleet is (%d, %d, %d), got %s' % (fleet.n_devices, n_pulses, width, fleet_guess.shape))
        ratio = fleet_guess / np.asarray(maxAmp, dtype=np.float64)[None, :, None]
        for row in range(n_pulses):
            if np.max(ratio[:, row]) > 1.0:
                raise ValueError('Initial guess has strength > max_amp for op %d' % (row))
        fleet_base = np.arcsin(ratio)
    n_sets = max(1, int(restarts)) * (1 if fleet is None else fleet.n_devices)
    tfs = HipState(sys_para, n_seeds=n_sets, device=_device if time_comm is None else time_comm.device, first_seed=_first_seed,
                   plan_seeds=0 if plan_seeds is None else int(plan_seeds), time_comm=time_comm, ensemble=robust if fleet is None else fleet.device(0),
                   transfer=None if transfer is None else transfer.matrix, exact_gradient=bool(exact_gradient),
                   collapse_ops=collapse_ops, control_map=control_map, fleet=fleet, fleet_base=fleet_base, running_costs=running_costs)   # constants -> HBM
    graph = tfs.build_graph()
    conv = Convergence(sys_para, time_unit, convergence)
    try:
        SS = run_session(tfs, graph, conv, sys_para, method, show_plots=sys_para.show_plots, use_gpu=use_gpu)
        if fleet is not None:
            return _fleet_results(tfs.engine, sys_para, fleet, _given_fleet, transfer, control_map, _given_map if control_map is not None else None,
                                  tfs.start_base if str(method).upper() == 'EVOLVE' and fleet_base is not None else None, save, file_path,
                                  grape_start_time)
        if transfer is not None:
            transfer.samples = np.array(SS.samples)
        if control_map is not None:
            _given_map.coefficients = control_map.coefficients = np.array(tfs.engine.get_coefficients()[int(SS.seed)])
        if _restart_info is not None:
            # (a dict to fill: every control set's final scalars and variable, read before the engine goes -- examples/lbfgs_restarts.py)
            _restart_info.update(tfs.engine.scalars(), base=tfs.engine.get_base(), best=int(SS.seed))
            if robust is not None:
                # (a robust call: every member's loss at every control set's last evaluation, (restarts, E) -- examples/qubit_pi_pulse_under_noise.py)
                _restart_info.update(member_losses=tfs.engine.member_scalars()['loss'])
            if running_costs:
                # (with running costs: x_l,i(tau) of every control set's last evaluation, (restarts, steps + 1, L, m) -- examples/guarded_transmon_under_decay.py)
                _restart_info.update(expectations=tfs.engine.get_expectations())
        if save:
            from quantum_optimal_control.helper_functions.data_management import H5File
            with H5File(file_path) as hf:
                hf.add('wall_clock_time', data=np.array(time.time() - grape_start_time))
            print("data saved at: " + str(file_path))
        if _return_session:
            return SS.uks, SS.Uf, float(SS.l)
        return SS.uks, SS.Uf
    except KeyboardInterrupt:
        if save:
            from quantum_optimal_control.helper_functions.data_management import H5File
            with H5File(file_path) as hf:
                hf.add('wall_clock_time', data=np.array(time.time() - grape_start_time))
            print("data saved at: " + str(file_path))
        return None
    finally:
        tfs.close()


def _fleet_results(engine, sys_para, fleet, given_fleet, transfer, control_map, given_map, own_points, save, file_path, start_time):
    """The per-device selection after run_session: every device's best control set (helper_functions.fleet.select_best on the final losses), its pulse
    and member 0's final unitary, and the fleet's result fields (on the caller's object too)."""
    from quantum_optimal_control.helper_functions.fleet import select_best
    if own_points is not None:
        # method='EVOLVE' scored one shared point; with a guess per device every device is scored at its own
        engine.set_base(own_points)
        engine.evaluate(want_grad=False)
    s = engine.scalars()
    best, sets = select_best(s['loss'], fleet.n_devices)
    evaluated = engine.get_uks(evaluated=True)[sets]
    uks = engine.get_pulse()[sets] if engine.samples is not None else evaluated
    if getattr(engine, 'open_system', False):
        Uf = engine.get_final_density()[sets]              # (F, m, m, n, n): member 0's final density operators, in both modes
    else:
        Uf = [[] for _ in sets] if sys_para.state_transfer else engine.get_final_unitary()[sets]
    member_losses = engine.member_scalars()['loss'][sets]
    for fl in (fleet, given_fleet):
        fl.losses, fl.best, fl.member_losses, fl.iterations = np.array(s['loss'][sets]), np.array(best), np.array(member_losses), np.array(s['iterations'][sets])
    if transfer is not None:
        transfer.samples = np.array(evaluated)
    if control_map is not None:
        given_map.coefficients = control_map.coefficients = np.array(engine.get_coefficients()[sets])
    if save:
        from quantum_optimal_control.helper_functions.data_management import H5File
        with H5File(file_path) as hf:
            hf.add('fleet_uks', data=np.array(uks))
            hf.add('fleet_losses', data=np.array(fleet.losses))
            hf.add('wall_clock_time', data=np.array(time.time() - start_time))
        print("data saved at: " + str(file_path))
    return uks, Uf


def GrapeTimeSharded(*args, comm=None, **kwargs):
    """`Grape(...)` for ONE large control problem (hundreds of levels, thousands of slices: BASELINE config 5) on all GPUs of a node: the pulse is
    cut along the TIME axis, rank r of `comm` (parallel_seeds.open_comm(): RCCL over xGMI behind the C ABI) forms the propagators, sweeps and
    gradients of its run of time chunks, and two small collectives per iteration -- an all-gather of one n x n product per rank, an all-reduce of the
    gradient array -- keep the ranks in lock step (csrc/qoc_gemm_ts.h).  Every rank runs the same optimiser on the whole pulse and returns
    the same (uks, U_final); only rank 0 writes the run log.  comm = None: a plain Grape call.  Unitary mode, no forbidden-level / speed_up term,
    n > 96, at most 8 states of interest; the reference has no counterpart (one device: main_grape/grape.py:106-109)."""
    if _is_lbfgs(args, kwargs):
        raise ValueError("GrapeTimeSharded: method='LBFGS' is not supported; run Grape(method='LBFGS') on one GPU")
    if kwargs.get('collapse_ops') is not None:
        raise ValueError('GrapeTimeSharded: collapse_ops (open-system GRAPE) is not supported; run Grape(collapse_ops=...) on one GPU')
    if kwargs.get('running_costs') is not None:
        raise ValueError('GrapeTimeSharded: running_costs (open-system running costs) are not supported; run Grape(running_costs=...) on one GPU')
    if kwargs.get('control_map') is not None:
        raise ValueError('GrapeTimeSharded: control_map (control maps) is not supported; run Grape(control_map=...) on one GPU')
    if kwargs.get('fleet') is not None:
        raise ValueError('GrapeTimeSharded: fleet (device fleets) is not supported; run Grape(fleet=...) on one GPU')
    if isinstance(kwargs.get('robust'), dict) and kwargs['robust'].get('collapse_ops') is not None:
        raise ValueError('GrapeTimeSharded: a robust ensemble with decay (open-system GRAPE) is not supported; run Grape(robust=...) on one GPU')
    if _sparse_call(args, kwargs):
        raise ValueError('GrapeTimeSharded: scipy.sparse Hamiltonians (sparse state transfer) are not supported; run Grape(...) on one GPU')
    if comm is None:
        return Grape(*args, **kwargs)
    from quantum_optimal_control.core import hip_engine
    if not isinstance(comm, hip_engine.QocComm):
        # parallel_seeds.open_comm() falls back to a host file transport when RCCL cannot start; that transport cannot carry the two collectives
        # every iteration enqueues on the engine's stream.  Say so before any rank builds an engine (open it with require_rccl=True to fail earlier).
        raise TypeError('GrapeTimeSharded needs an RCCL communicator (hip_engine.QocComm, e.g. parallel_seeds.open_comm(require_rccl=True)); got %s%s'
                        % (type(comm).__name__, (': ' + str(getattr(comm, 'fallback_reason', ''))) if getattr(comm, 'fallback_reason', None) else ''))
    if comm.rank != 0:
        kwargs['save'] = False
        kwargs['show_plots'] = False
    return Grape(*args, time_comm=comm, **kwargs)


def GrapeSharded(*args, restarts=8, dist=None, comm=None, **kwargs):
    """`Grape(...)` with `restarts` control sets block-partitioned over the ranks of a one-node job (one process per GPU).
    Transport: `comm` = a `hip_engine.QocComm` (RCCL over xGMI behind the C ABI; `parallel_seeds.open_comm()` builds it from the
    launcher's RANK/LOCAL_RANK/WORLD_SIZE) or `dist` = an initialised `torch.distributed` module (gloo in the CPU tests); neither
    = a single process.  Every rank optimises its own restarts on its own GPU -- no data-path collective --, the best final
    losses are all-gathered once, and the winner's (uks, U_final) is broadcast, so every rank returns the same pair.
    Global restart g starts from the same point whatever the number of ranks (restart 0 = the reference's own draw), and every engine of the
    launch plans its kernels for the same batch: `plan_seeds`, default = the LARGEST shard of this launch, ceil(restarts / ranks) -- identical on all
    ranks, and never smaller than what an engine holds, so AUTO picks what is fastest for the launch at hand.  Bit-identity ACROSS launches with
    different rank counts is opt-in: pass the same `plan_seeds` to each of them (`hip_engine.plan_seeds_for(restarts)` = restarts / GPUs of the
    node is the natural choice) -- the result is then bit for bit that of `Grape(restarts=restarts, plan_seeds=<the same>)` in one process
    (tests/sharded_script.py checks array_equal); an engine that holds more control sets than it plans for says so on stderr when that changes
    the kernels it runs."""
    from quantum_optimal_control.parallel_seeds import SeedShard
    if _is_lbfgs(args, kwargs):
        # (before any rank builds an engine: every rank raises alike)
        raise ValueError("GrapeSharded: method='LBFGS' is not supported; run Grape(method='LBFGS', restarts=R) on one GPU")
    if kwargs.get('robust') is not None:
        # (before any rank builds an engine: every rank raises alike)
        raise ValueError('GrapeSharded: robust ensembles are not supported; run Grape(robust=..., restarts=R) on one GPU')
    if kwargs.get('transfer') is not None:
        raise ValueError('GrapeSharded: transfer functions are not supported; run Grape(transfer=..., restarts=R) on one GPU')
    if kwargs.get('collapse_ops') is not None:
        raise ValueError('GrapeSharded: collapse_ops (open-system GRAPE) is not supported; run Grape(collapse_ops=..., restarts=R) on one GPU')
    if kwargs.get('running_costs') is not None:
        raise ValueError('GrapeSharded: running_costs (open-system running costs) are not supported; run Grape(running_costs=..., restarts=R) on one GPU')
    if kwargs.get('control_map') is not None:
        raise ValueError('GrapeSharded: control_map (control maps) is not supported; run Grape(control_map=..., restarts=R) on one GPU')
    if kwargs.get('fleet') is not None:
        raise ValueError('GrapeSharded: fleet (device fleets) is not supported; run Grape(fleet=..., restarts=R) on one GPU')
    if _sparse_call(args, kwargs):
        raise ValueError('GrapeSharded: scipy.sparse Hamiltonians (sparse state transfer) are not supported; run Grape(..., restarts=R) on one GPU')
    if comm is not None:
        world, rank = comm.world, comm.rank
    elif dist is not None:
        world, rank = dist.get_world_size(), dist.get_rank()
    else:
        world, rank = 1, 0
    shard = SeedShard(total_seeds=int(restarts), rank=rank, world=world)
    if min(shard.counts) == 0:           # the same verdict on EVERY rank: nobody is left waiting in a collective
        raise ValueError('GrapeSharded: more ranks (%d) than restarts (%d)' % (world, restarts))
    default_device = comm.device if comm is not None else (os.environ.get('LOCAL_RANK', 0) if dist is not None else 0)
    device = int(kwargs.pop('device', default_device))
    if rank != 0:
        kwargs['save'] = False                                       # only rank 0 may write the run log
    kwargs.setdefault('plan_seeds', max(shard.counts))
    out = Grape(*args, restarts=shard.count, _first_seed=shard.first, _device=device, _return_session=True, **kwargs)
    if world == 1:
        return None if out is None else out[:2]
    # one value per RANK (its best restart): gather, pick the winner, broadcast its pulse and unitary.  A rank whose run was
    # interrupted still takes part (loss = +inf), so the others are not left waiting.
    ranks = SeedShard(total_seeds=world, rank=rank, world=world)     # one slot per rank
    loss = np.inf if out is None else out[2]
    losses = ranks.all_gather(np.array([loss]), dist=dist, comm=comm)
    if not np.all(np.isfinite(losses)):
        return None
    best = int(np.argmin(losses))
    uks, Uf = out[0], out[1]
    uks = ranks.broadcast_from_owner(best, lambda i: np.asarray(uks, dtype=np.float64), np.shape(uks), dist=dist, comm=comm)
    if not isinstance(Uf, list):
        shape = np.shape(Uf)
        flat = ranks.broadcast_from_owner(best, lambda i: np.ascontiguousarray(Uf, dtype=np.complex128).view(np.float64),
                                          shape[:-1] + (2 * shape[-1],), dist=dist, comm=comm)
        Uf = np.ascontiguousarray(flat).view(np.complex128)
    return uks, Uf
