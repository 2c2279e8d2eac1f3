"""ctypes binding of libqoc_hip.so (C ABI declared in include/qoc.h).

This is the only place the Python host touches the device: the engine object plays the role the TensorFlow
graph + session play in the reference (core/tensorflow_state.py + the session.run fetches of
core/run_session.py:53-54,66-69,119-127 and core/analysis.py:26-41).  There is NO CPU fallback: if the shared
library or a HIP device is missing, construction raises.
"""
import ctypes as C
import os

import numpy as np

from quantum_optimal_control.helper_functions import control_map as _cmap, open_system

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('QOC_HIP_LIBRARY') or os.path.normpath(os.path.join(_HERE, '..', '..', 'lib', 'libqoc_hip.so'))   # override: A/B builds

PATH_AUTO, PATH_GENERIC, PATH_MFMA, PATH_ST_FUSED, PATH_GEMM, PATH_SMALL = 0, 1, 2, 3, 4, 5
PATH_LINDBLAD = 6          # open engines only (HipEngine(collapse_ops=...))
PATH_SPARSE = 7            # sparse engines only (HipEngine(sparse_ops=...))
PATH_LINDBLAD_TILED = 8    # open engines past PATH_LINDBLAD's size rule, up to 128 levels (helper_functions/open_system.choose_path)


class QocConfig(C.Structure):
    _fields_ = [('n', C.c_int32), ('k', C.c_int32), ('steps', C.c_int32), ('m', C.c_int32),
                ('taylor_terms', C.c_int32), ('scaling', C.c_int32), ('state_transfer', C.c_int32),
                ('n_seeds', C.c_int32), ('dt', C.c_double), ('total_time', C.c_double),
                ('has_amplitude', C.c_int32), ('has_envelope', C.c_int32), ('has_dwdt', C.c_int32),
                ('has_d2wdt2', C.c_int32), ('has_speed_up', C.c_int32), ('has_bandpass', C.c_int32),
                ('c_amplitude', C.c_double), ('c_envelope', C.c_double), ('c_dwdt', C.c_double),
                ('c_d2wdt2', C.c_double), ('c_speed_up', C.c_double), ('c_bandpass', C.c_double),
                ('band_lo', C.c_int32), ('band_hi', C.c_int32), ('n_forbidden', C.c_int32),
                ('forbid_dressed', C.c_int32), ('device', C.c_int32), ('path', C.c_int32), ('chunks', C.c_int32),
                ('variant', C.c_int32), ('plan_seeds', C.c_int32), ('time_shards', C.c_int32), ('time_rank', C.c_int32), ('gradient', C.c_int32),
                ('reserved', C.c_int32 * 2)]


class QocEnsemble(C.Structure):
    _fields_ = [('members', C.c_int32), ('n_perturb', C.c_int32), ('P', C.POINTER(C.c_double)), ('offsets', C.POINTER(C.c_double)),
                ('amp_scales', C.POINTER(C.c_double)), ('weights', C.POINTER(C.c_double))]


class QocTransfer(C.Structure):
    _fields_ = [('n_samples', C.c_int32), ('T', C.POINTER(C.c_double))]


class QocControlMap(C.Structure):
    _fields_ = [('n_terms', C.c_int32), ('degree', C.c_int32), ('poly', C.POINTER(C.c_double)), ('mix', C.POINTER(C.c_double)),
                ('fixed', C.POINTER(C.c_double))]


class QocFleet(C.Structure):
    _fields_ = [('devices', C.c_int32), ('offsets', C.POINTER(C.c_double)), ('amp_scales', C.POINTER(C.c_double))]


class QocOpen(C.Structure):
    _fields_ = [('n_collapse', C.c_int32), ('C', C.POINTER(C.c_double))]


class QocDecay(C.Structure):
    _fields_ = [('n_collapse', C.c_int32), ('C', C.POINTER(C.c_double)), ('rate_scales', C.POINTER(C.c_double))]


class QocRunningCosts(C.Structure):
    _fields_ = [('n_obs', C.c_int32), ('O', C.POINTER(C.c_double)), ('coeffs', C.POINTER(C.c_double)), ('powers', C.POINTER(C.c_int32))]


class QocSparse(C.Structure):
    _fields_ = [('indptr', C.POINTER(C.c_int64)), ('row', C.POINTER(C.c_int32)), ('col', C.POINTER(C.c_int32)), ('val', C.POINTER(C.c_double)),
                ('vector_home', C.c_int32)]


class QocSparsePlan(C.Structure):
    _fields_ = [('row_layout', C.c_int32)]


class QocAdamParams(C.Structure):
    _fields_ = [('rate', C.c_double), ('learning_rate_decay', C.c_double), ('conv_target', C.c_double),
                ('min_grad', C.c_double), ('max_iterations', C.c_int32), ('poll_every', C.c_int32)]


class QocLbfgsParams(C.Structure):
    _fields_ = [('conv_target', C.c_double), ('min_grad', C.c_double), ('c1', C.c_double), ('shrink', C.c_double),
                ('max_iterations', C.c_int32), ('history', C.c_int32), ('max_ls', C.c_int32), ('poll_every', C.c_int32)]


_DP = C.POINTER(C.c_double)
_IP = C.POINTER(C.c_int32)
_lib = None

_SIGNATURES = {
    'qoc_create': (C.c_int, [C.POINTER(QocConfig), _DP, _DP, _DP, _DP, _DP, _DP, _IP, _DP, _DP, C.POINTER(C.c_void_p)]),
    'qoc_create_ensemble': (C.c_int, [C.POINTER(QocConfig), C.POINTER(QocEnsemble), _DP, _DP, _DP, _DP, _DP, _DP, _IP, _DP, _DP,
                                      C.POINTER(C.c_void_p)]),
    'qoc_create_shaped': (C.c_int, [C.POINTER(QocConfig), C.POINTER(QocEnsemble), C.POINTER(QocTransfer), _DP, _DP, _DP, _DP, _DP, _DP, _IP, _DP,
                                    _DP, C.POINTER(C.c_void_p)]),
    'qoc_create_mapped': (C.c_int, [C.POINTER(QocConfig), C.POINTER(QocEnsemble), C.POINTER(QocTransfer), C.POINTER(QocControlMap), _DP, _DP, _DP,
                                    _DP, _DP, _DP, _IP, _DP, _DP, C.POINTER(C.c_void_p)]),
    'qoc_get_coefficients': (C.c_int, [C.c_void_p, _DP]),
    'qoc_create_fleet': (C.c_int, [C.POINTER(QocConfig), C.POINTER(QocEnsemble), C.POINTER(QocFleet), C.POINTER(QocTransfer),
                                   C.POINTER(QocControlMap), _DP, _DP, _DP, _DP, _DP, _DP, _IP, _DP, _DP, C.POINTER(C.c_void_p)]),
    'qoc_create_open': (C.c_int, [C.POINTER(QocConfig), C.POINTER(QocOpen), _DP, _DP, _DP, _DP, _DP, _DP, C.POINTER(C.c_void_p)]),
    'qoc_create_open_fleet': (C.c_int, [C.POINTER(QocConfig), C.POINTER(QocDecay), C.POINTER(QocEnsemble), C.POINTER(QocFleet), C.POINTER(QocTransfer),
                                        C.POINTER(QocControlMap), _DP, _DP, _DP, _DP, _DP, _DP, C.POINTER(C.c_void_p)]),
    'qoc_get_member_final_density': (C.c_int, [C.c_void_p, _DP]),
    'qoc_create_open_costs': (C.c_int, [C.POINTER(QocConfig), C.POINTER(QocDecay), C.POINTER(QocRunningCosts), C.POINTER(QocEnsemble), C.POINTER(QocFleet),
                                        C.POINTER(QocTransfer), C.POINTER(QocControlMap), _DP, _DP, _DP, _DP, _DP, _DP, C.POINTER(C.c_void_p)]),
    'qoc_get_expectations': (C.c_int, [C.c_void_p, _DP]),
    'qoc_create_sparse': (C.c_int, [C.POINTER(QocConfig), C.POINTER(QocSparse), _DP, _DP, _DP, _DP, _IP, _DP, C.POINTER(C.c_void_p)]),
    'qoc_create_sparse_fleet': (C.c_int, [C.POINTER(QocConfig), C.POINTER(QocSparse), C.POINTER(QocSparsePlan), C.POINTER(QocEnsemble),
                                          C.POINTER(QocFleet), C.POINTER(QocTransfer), C.POINTER(QocControlMap), _DP, _DP, _DP, _DP, _IP, _DP,
                                          C.POINTER(C.c_void_p)]),
    'qoc_get_final_density': (C.c_int, [C.c_void_p, _DP]),
    'qoc_get_populations': (C.c_int, [C.c_void_p, _DP]),
    'qoc_get_pulse': (C.c_int, [C.c_void_p, _DP]),
    'qoc_get_member_scalars': (C.c_int, [C.c_void_p, _DP, _DP]),
    'qoc_get_member_final_unitary': (C.c_int, [C.c_void_p, _DP]),
    'qoc_get_trajectory_gradient': (C.c_int, [C.c_void_p, _DP]),
    'qoc_set_risk': (C.c_int, [C.c_void_p, C.c_double]),
    'qoc_get_member_weights': (C.c_int, [C.c_void_p, _DP]),
    'qoc_set_traces': (C.c_int, [C.c_void_p, _DP]),
    'qoc_destroy': (C.c_int, [C.c_void_p]),
    'qoc_set_base': (C.c_int, [C.c_void_p, _DP]),
    'qoc_get_base': (C.c_int, [C.c_void_p, _DP]),
    'qoc_eval': (C.c_int, [C.c_void_p, _DP, _DP, _DP, _DP, _DP]),
    'qoc_adam_step': (C.c_int, [C.c_void_p, _DP]),
    'qoc_run_adam': (C.c_int, [C.c_void_p, C.POINTER(QocAdamParams), _IP]),
    'qoc_iterate': (C.c_int, [C.c_void_p, C.POINTER(QocAdamParams), C.c_int32]),
    'qoc_iterate_lbfgs': (C.c_int, [C.c_void_p, C.POINTER(QocLbfgsParams), C.c_int32]),
    'qoc_run_lbfgs': (C.c_int, [C.c_void_p, C.POINTER(QocLbfgsParams), _IP]),
    'qoc_sync': (C.c_int, [C.c_void_p]),
    'qoc_get_scalars': (C.c_int, [C.c_void_p, _DP, _DP, _DP, _DP, _IP, _IP]),
    'qoc_get_uks': (C.c_int, [C.c_void_p, _DP]),
    'qoc_get_uks_evaluated': (C.c_int, [C.c_void_p, _DP]),
    'qoc_get_final_unitary': (C.c_int, [C.c_void_p, _DP]),
    'qoc_get_inter_vecs': (C.c_int, [C.c_void_p, _DP]),
    'qoc_profile_enable': (C.c_int, [C.c_void_p, C.c_int32]),
    'qoc_profile_read': (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), _DP]),
    'qoc_time_iterations': (C.c_int, [C.c_void_p, C.POINTER(QocAdamParams), C.c_int32, _DP]),
    'qoc_path_in_use': (C.c_int, [C.c_void_p]),
    'qoc_chunks_in_use': (C.c_int, [C.c_void_p]),
    'qoc_plan_describe': (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32]),
    'qoc_set_time_comm': (C.c_int, [C.c_void_p, C.c_void_p]),
    'qoc_comm_unique_id': (C.c_int, [C.c_void_p]),
    'qoc_comm_probe': (C.c_int, [C.c_int32]),
    'qoc_comm_create': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    'qoc_comm_destroy': (C.c_int, [C.c_void_p]),
    'qoc_comm_world': (C.c_int, [C.c_void_p]),
    'qoc_comm_rank': (C.c_int, [C.c_void_p]),
    'qoc_comm_library': (C.c_char_p, []),
    'qoc_comm_all_gather_scalar': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, _DP]),
    'qoc_comm_all_gather_f64': (C.c_int, [C.c_void_p, _DP, C.c_int32, _DP]),
    'qoc_comm_all_reduce_max_f64': (C.c_int, [C.c_void_p, _DP, C.c_int32]),
    'qoc_comm_broadcast_f64': (C.c_int, [C.c_void_p, _DP, C.c_int64, C.c_int32]),
    'qoc_comm_barrier': (C.c_int, [C.c_void_p]),
    'qoc_device_count': (C.c_int, []),
    'qoc_device_info': (C.c_int, [C.c_int32, C.c_char_p, C.c_int32, _IP, C.POINTER(C.c_int64)]),
    'qoc_device_peer_access': (C.c_int, [C.c_int32, C.c_int32, _IP]),
    'qoc_last_error': (C.c_char_p, []),
    'qoc_version': (C.c_char_p, []),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def load_library():
    """dlopen the in-tree libqoc_hip.so and declare every prototype of include/qoc.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError('libqoc_hip.so not found at %s -- build it with `python -c "import __graft_entry__ as g; '
                          'g.build()"` (hipcc --offload-arch=gfx950); there is no CPU fallback.' % LIB_PATH)
    # one process per GPU under a launcher: RCCL shares device memory between the ranks through dmabuf IPC handles, the only kind this host
    # driver supports, and the HIP runtime reads the switch when it starts -- i.e. possibly at the first call into the library loaded here
    if int(os.environ.get('WORLD_SIZE', '1') or 1) > 1:
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def library_loaded():
    return _lib is not None


class QocError(RuntimeError):
    pass


def _check(rc):
    if rc != 0:
        raise QocError('libqoc_hip: status %d: %s' % (rc, load_library().qoc_last_error().decode()))


def _dp(a):
    return None if a is None else a.ctypes.data_as(_DP)


def _c128(a, shape):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.complex128))
    assert a.shape == tuple(shape), (a.shape, shape)
    return a


def device_count():
    return load_library().qoc_device_count()


def device_info(device=0):
    lib = load_library()
    name = C.create_string_buffer(256)
    cus = C.c_int32()
    mem = C.c_int64()
    _check(lib.qoc_device_info(device, name, 256, C.byref(cus), C.byref(mem)))
    return dict(name=name.value.decode(), compute_units=cus.value, hbm_bytes=mem.value)


def device_peer_access(device, peer):
    """True when HIP device `device` can address the memory of device `peer` directly (hipDeviceCanAccessPeer)."""
    lib = load_library()
    can = C.c_int32()
    _check(lib.qoc_device_peer_access(int(device), int(peer), C.byref(can)))
    return bool(can.value)


def reg_config(reg_coeffs, total_time):
    """Translate the reference's reg_coeffs dict (core/regularization_functions.py:15-88) into qoc_config fields."""
    rc = {} if reg_coeffs is None else reg_coeffs
    out = {}
    for key, name in (('amplitude', 'amplitude'), ('envelope', 'envelope'), ('dwdt', 'dwdt'), ('d2wdt2', 'd2wdt2'),
                      ('speed_up', 'speed_up'), ('bandpass', 'bandpass')):
        out['has_' + name] = int(key in rc)
        out['c_' + name] = float(rc[key]) if key in rc else 0.0
    if 'bandpass' in rc:
        band_id = (np.array(rc['band']) * total_time).astype(int)              # regularization_functions.py:59-61
        out['band_lo'], out['band_hi'] = int(band_id[0]), int(band_id[1])
    if 'forbidden_coeff_list' in rc:
        pairs = list(zip(rc['forbidden_coeff_list'], rc['states_forbidden_list']))   # zip truncation as in :81
        out['forbidden_coeffs'] = np.array([float(c) for c, _ in pairs], dtype=np.float64)
        out['forbidden_states'] = np.array([int(s) for _, s in pairs], dtype=np.int32)
    return out


COMM_ID_BYTES = 128
SCALAR_LOSS, SCALAR_REG_LOSS, SCALAR_GRAD_SQUARED, SCALAR_UNITARY_SCALE = 0, 1, 2, 3


def comm_unique_id():
    """128-byte RCCL id (rank 0 creates it, the launcher hands it to the other ranks: parallel_seeds.rendezvous)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(load_library().qoc_comm_unique_id(buf))
    return buf.raw


def plan_seeds_for(total_restarts):
    """The batch size AUTO should plan for when `total_restarts` control sets may be sharded over the GPUs of this node: what a
    full-node run gives each GPU.  It depends on the node, not on how many ranks a launch uses, so a restart evolves bit-identically
    under any rank count (and a full-node run keeps every GPU's 1024 SIMDs busy)."""
    return max(1, -(-int(total_restarts) // max(1, device_count())))


def comm_probe(device=0):
    """Local preconditions of QocComm (librccl loadable, device usable); raises QocError with the reason.  No collective."""
    _check(load_library().qoc_comm_probe(int(device)))


class QocComm(object):
    """One RCCL communicator per process (one process per GPU) behind the C ABI (include/qoc.h, multi-GPU section).
    No torch involved: the collectives run from the engine's device buffers on the engine's HIP stream."""

    def __init__(self, unique_id, world, rank, device=0):
        assert len(unique_id) == COMM_ID_BYTES
        self._lib = load_library()
        self._h = C.c_void_p()
        self.world, self.rank, self.device = int(world), int(rank), int(device)
        _check(self._lib.qoc_comm_create(C.create_string_buffer(bytes(unique_id), COMM_ID_BYTES), self.world, self.rank,
                                         self.device, C.byref(self._h)))
        self.library = self._lib.qoc_comm_library().decode()

    def _attach(self, engine):
        import weakref
        if not hasattr(self, '_engines'):
            self._engines = weakref.WeakSet()
        self._engines.add(engine)

    def _detach(self, engine):
        if hasattr(self, '_engines'):
            self._engines.discard(engine)

    def close(self):
        """Destroys the communicator.  Time-sharded engines that still hold it (HipEngine(time_comm=...)) are closed FIRST -- the C ABI refuses to destroy a
        communicator an engine still uses, and a close() in a caller's finally block after an engine-side exception must neither leak the communicator nor
        mask that exception with a second one."""
        if getattr(self, '_h', None) is not None and self._h.value:
            for eng in list(getattr(self, '_engines', ())):
                eng.close()
            _check(self._lib.qoc_comm_destroy(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def all_gather_scalar(self, engine, which, width):
        """[world][width] rows of one per-seed scalar array of `engine` (device to device on the engine's stream)."""
        out = np.empty((self.world, int(width)))
        _check(self._lib.qoc_comm_all_gather_scalar(self._h, engine._h, int(which), int(width), _dp(out)))
        return out

    def all_gather(self, values):
        values = np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(-1))
        out = np.empty((self.world, values.shape[0]))
        _check(self._lib.qoc_comm_all_gather_f64(self._h, _dp(values), values.shape[0], _dp(out)))
        return out

    def all_reduce_max(self, values):
        buf = np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(-1)).copy()
        _check(self._lib.qoc_comm_all_reduce_max_f64(self._h, _dp(buf), buf.shape[0]))
        return buf

    def broadcast(self, array, root):
        buf = np.ascontiguousarray(np.asarray(array, dtype=np.float64)).copy()
        _check(self._lib.qoc_comm_broadcast_f64(self._h, _dp(buf.reshape(-1)), buf.size, int(root)))
        return buf

    def barrier(self):
        _check(self._lib.qoc_comm_barrier(self._h))


def _getter(holder):
    """key -> value or None, whatever carries the keys: a dict, an object with attributes (helper_functions.fleet.Fleet) or None."""
    return holder.get if isinstance(holder, dict) else lambda key, default=None: getattr(holder, key, default)


def ensemble_arrays(ensemble, n, k, dt, dense=True):
    """The C ABI's qoc_ensemble arrays from a dict with keys `operators` (q Hermitian n x n matrices P_q), `offsets` (E x q), `amp_scales`
    (E x k) and `weights` (E, used as given): (P = -i dt P_q stacked, offsets, amp_scales, weights), all C-contiguous.  dense=False (the sparse
    route: the operators travel with the sparse operators, sparse_perturbations): the operators are only counted, and P is None."""
    ops = [np.asarray(_densified(p), dtype=np.complex128) for p in ensemble.get('operators', [])] if dense else list(ensemble.get('operators', []))
    q = len(ops)
    amp = np.ascontiguousarray(np.asarray(ensemble['amp_scales'], dtype=np.float64))
    E = amp.shape[0]
    assert amp.shape == (E, k), amp.shape
    off = np.ascontiguousarray(np.asarray(ensemble.get('offsets', np.zeros((E, 0))), dtype=np.float64).reshape(E, q))
    wt = np.ascontiguousarray(np.asarray(ensemble['weights'], dtype=np.float64))
    assert wt.shape == (E,), wt.shape
    if not dense:
        return None, off, amp, wt
    P = np.ascontiguousarray(np.stack([-1j * float(dt) * p for p in ops]) if q else np.zeros((0, n, n), dtype=np.complex128))
    assert P.shape == (q, n, n), P.shape
    return P, off, amp, wt


def fleet_arrays(fleet, E, q, k):
    """The C ABI's qoc_fleet arrays from a helper_functions.fleet.Fleet or a dict with keys `offsets` (F x E x q, optional when q = 0) and
    `amp_scales` (F x E x k): (offsets, amp_scales), both C-contiguous."""
    get = _getter(fleet)
    amp = np.ascontiguousarray(np.asarray(get('amp_scales'), dtype=np.float64))
    if amp.ndim != 3 or amp.shape[1:] != (E, k):
        raise ValueError('HipEngine: fleet amp_scales have shape %s, expected (F, %d, %d)' % (amp.shape, E, k))
    F = amp.shape[0]
    off = get('offsets')
    off = np.zeros((F, E, q)) if off is None or (q == 0 and np.size(off) == 0) else np.ascontiguousarray(np.asarray(off, dtype=np.float64))
    if off.shape != (F, E, q):
        raise ValueError('HipEngine: fleet offsets have shape %s, expected (%d, %d, %d)' % (off.shape, F, E, q))
    return off, amp


def decay_arrays(ensemble, fleet, n, E, dt):
    """The decay an ensemble dict (keys collapse_ops, rate_scales (E, c)) or a fleet (attributes or keys collapse_ops, rate_scales (F, E, c)) carries,
    as the C ABI's qoc_decay arrays: (D = sqrt(dt) C_j stacked (c, n, n), rate_scales (F, E, c) with F = 1 for an ensemble), or None without decay.
    The fleet's decay stands in front of the ensemble's (Grape hands device 0 of a fleet over as its ensemble)."""
    get = _getter(fleet)
    ops, rates, lead = get('collapse_ops'), get('rate_scales'), 'fleet'
    if ops is None:
        if get('rate_scales') is not None:
            raise ValueError('HipEngine: fleet rate_scales given without collapse_ops')
        if ensemble is None or ensemble.get('collapse_ops') is None:
            if ensemble is not None and ensemble.get('rate_scales') is not None:
                raise ValueError('HipEngine: ensemble rate_scales given without collapse_ops')
            return None
        ops, rates, lead = ensemble['collapse_ops'], ensemble.get('rate_scales'), 'ensemble'
        if rates is not None:
            rates = np.asarray(rates, dtype=np.float64)[None]
    ops = open_system.validate(list(ops), n)
    c = len(ops)
    if rates is None:
        F = 1 if (fleet is None or lead == 'ensemble') else np.shape(get('amp_scales'))[0]
        rates = np.ones((F, E, c))
    rates = np.ascontiguousarray(np.asarray(rates, dtype=np.float64))
    if rates.ndim != 3 or rates.shape[1:] != (E, c):
        raise ValueError('HipEngine: %s rate_scales have shape %s, expected (%s%d, %d)' % (lead, rates.shape[1:] if lead == 'ensemble' else rates.shape,
                                                                                          '' if lead == 'ensemble' else 'F, ', E, c))
    if not np.all(np.isfinite(rates)) or np.any(rates < 0):
        raise ValueError('HipEngine: %s rate_scales must be finite and >= 0' % lead)
    D = np.ascontiguousarray(np.sqrt(float(dt)) * np.array(ops, dtype=np.complex128).reshape(c, n, n))
    return D, rates


VECTOR_HOME = {None: 0, 'auto': 0, 'lds': 1, 'global': 2}
ROW_LAYOUT = {0: 0, 'auto': 0, 1: 1, 'per_operator': 1, 2: 2, 'merged': 2}


def _densified(op):
    """A perturbation operator for a dense route: a scipy.sparse matrix becomes an array, anything else passes."""
    return op.toarray() if hasattr(op, 'toarray') else op


def sparse_perturbations(ensemble, dt):
    """The perturbation operators of an ensemble dict as the sparse route takes them: -i dt P_q as complex CSR, a dense P_q converted once and a
    scipy.sparse one never densified.  They stand behind the controls in HipEngine's sparse_ops (include/qoc.h, qoc_create_sparse_fleet)."""
    import scipy.sparse as sps
    return [sps.csr_matrix(-1j * float(dt) * sps.csr_matrix(p, dtype=np.complex128)) for p in (ensemble or {}).get('operators', [])]


def sparse_arrays(sparse_ops):
    """The C ABI's qoc_sparse arrays from a list of k + 1 scipy.sparse matrices (already -i dt H_j): (n, indptr, row, col, val), the entries of the
    operators one after the other in COO form.  No operator is densified; duplicates and explicit zeros go through as they are (the library sums the
    former and keeps the latter)."""
    import scipy.sparse as sps
    coos = [sps.coo_matrix(a) for a in sparse_ops]
    n = coos[0].shape[0]
    for a in coos:
        if a.shape != (n, n):
            raise ValueError('HipEngine: sparse operators must all be (%d, %d), got %s' % (n, n, a.shape))
    indptr = np.zeros(len(coos) + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([a.nnz for a in coos])
    row = np.ascontiguousarray(np.concatenate([a.row for a in coos]).astype(np.int32))
    col = np.ascontiguousarray(np.concatenate([a.col for a in coos]).astype(np.int32))
    val = np.ascontiguousarray(np.concatenate([a.data for a in coos]).astype(np.complex128))
    return n, indptr, row, col, val


# what a refusal asks of HipEngine's arguments `a`, when its block is reached (a key that is not here: that argument is not None)
_GIVEN = {
    'member collapse_ops': lambda a: _getter(a['ensemble'])('collapse_ops') is not None or _getter(a['fleet'])('collapse_ops') is not None,
    'member rate_scales': lambda a: _getter(a['ensemble'])('rate_scales') is not None or _getter(a['fleet'])('rate_scales') is not None,
    'exact_gradient': lambda a: bool(a['exact_gradient']),
    'time sharding': lambda a: a['time_comm'] is not None or int(a['time_shards']) > 0,
    'sparse_ops beside Hs': lambda a: a['sparse_ops'] is not None and a['Hs'] is not None,
    'another path': lambda a: int(a['path']) not in (PATH_AUTO, PATH_SPARSE),
}
_NOT_ON_GLUE = (('collapse_ops', 'collapse_ops (open-system GRAPE)'), ('sparse_ops beside Hs', 'sparse_ops (sparse state transfer) beside a dense Hs'),
                ('time sharding', 'time sharding'))
# What does not combine with what: block -> (the feature as the message names it, ((what is asked, the partner as the message names it), ...)).
# HipEngine looks at the blocks in this order, each when its feature is there, and at the partners in theirs; the first one given is the ValueError
# 'HipEngine: <feature> does not combine with <partner>', before the library is loaded.  (Between the blocks stand the checks with messages of
# their own: row_layout without sparse_ops, the validators of the helper modules, running_costs on a closed engine.)
_REFUSALS = {
    # (decay per member needs the open engine, which the sparse route does not have: named before anything is built)
    'sparse_ops with decay': ('sparse_ops (sparse state transfer)', (('member collapse_ops', 'decay per member (collapse_ops)'),
                                                                     ('member rate_scales', 'decay per member (rate_scales)'))),
    # (before the fleet's own refusal of collapse_ops=: decay that the members carry is named as such)
    'decay': ('an ensemble or fleet with decay', (('collapse_ops', 'the collapse_ops= keyword (the members carry the decay)'),
                                                  ('exact_gradient', 'exact_gradient'), ('time sharding', 'time sharding'))),
    'fleet': ('fleet', _NOT_ON_GLUE),
    'control_map': ('control_map', _NOT_ON_GLUE),
    # (transfer: the line runs on sparse operators behind the C ABI, qoc_create_sparse_fleet; this binding keeps its refusal)
    'sparse_ops': ('sparse_ops (sparse state transfer)', (('transfer', 'transfer'), ('exact_gradient', 'exact_gradient'), ('collapse_ops', 'collapse_ops'),
                                                          ('time sharding', 'time sharding'), ('Vs', 'Vs (dressed forbidden levels)'), ('Hs', 'a dense Hs'),
                                                          ('U0', 'U0'), ('another path', 'path %(path)s'))),
    'collapse_ops': ('collapse_ops (open-system GRAPE)', (('ensemble', 'ensemble'), ('transfer', 'transfer'), ('exact_gradient', 'exact_gradient'),
                                                          ('time sharding', 'time sharding'))),
}


def _refuse(block, a):
    """ValueError for the first partner of `block` (_REFUSALS) that HipEngine's arguments `a` hold."""
    feature, partners = _REFUSALS[block]
    for asked, partner in partners:
        if _GIVEN[asked](a) if asked in _GIVEN else a[asked] is not None:
            raise ValueError('HipEngine: %s does not combine with %s' % (feature, partner % a))


# One builder per struct of the C ABI: (the struct, the arrays it points into -- to be kept alive across the call).
def _ensemble_struct(ensemble, n, k, dt, dense):
    P, off, amp, wt = ensemble_arrays(ensemble, n, k, dt, dense=dense)
    return QocEnsemble(members=amp.shape[0], n_perturb=off.shape[1], P=_dp(P.view(np.float64)) if (P is not None and P.shape[0]) else None,
                       offsets=_dp(off) if off.shape[1] else None, amp_scales=_dp(amp), weights=_dp(wt)), (P, off, amp, wt)


def _transfer_struct(transfer, steps):
    T = np.ascontiguousarray(np.asarray(transfer, dtype=np.float64))
    if T.ndim != 2 or T.shape[0] != steps:
        raise ValueError('HipEngine: the transfer matrix has shape %s, expected (%d, P)' % (T.shape, steps))
    return QocTransfer(n_samples=T.shape[1], T=_dp(T)), T


def _map_struct(cm):
    return QocControlMap(n_terms=cm.n_terms, degree=cm.degree, poly=_dp(cm.alpha), mix=_dp(cm.mix), fixed=_dp(cm.fixed)), cm


def _fleet_struct(fleet, ens, k):
    foff, famp = fleet_arrays(fleet, ens.members if ens is not None else 1, ens.n_perturb if ens is not None else 0, k)
    return QocFleet(devices=famp.shape[0], offsets=_dp(foff) if foff.shape[2] else None, amp_scales=_dp(famp)), (foff, famp)


def _costs_struct(running_costs, n):
    L = len(running_costs)
    cO = np.ascontiguousarray(np.array([r[0] for r in running_costs], dtype=np.complex128).reshape(L, n, n))
    ca = np.ascontiguousarray(np.array([r[1] for r in running_costs], dtype=np.float64).reshape(L))
    cp = np.ascontiguousarray(np.array([r[2] for r in running_costs], dtype=np.int32).reshape(L))
    return QocRunningCosts(n_obs=L, O=_dp(cO.view(np.float64)) if L else None, coeffs=_dp(ca) if L else None,
                           powers=cp.ctypes.data_as(_IP) if L else None), (cO, ca, cp)


def _sparse_structs(sparse, vector_home, row_layout):
    """(qoc_sparse, qoc_sparse_plan): the plan of the sparse ensemble entry point (row_layout None: 0, as on that entry point without the keyword)."""
    _, indptr, row, col, val = sparse
    sp = QocSparse(indptr=indptr.ctypes.data_as(C.POINTER(C.c_int64)), row=row.ctypes.data_as(_IP), col=col.ctypes.data_as(_IP),
                   val=_dp(val.view(np.float64)), vector_home=VECTOR_HOME[vector_home])
    return (sp, QocSparsePlan(row_layout=ROW_LAYOUT[0 if row_layout is None else row_layout])), sparse


def _decay_struct(D, rates=None, fl=None, kind=QocDecay):
    """qoc_decay from D_j = sqrt(dt) C_j and the members' table of rate scales (None, the collapse_ops= keyword: no table; kind=QocOpen: qoc_open)."""
    if rates is not None and fl is not None and rates.shape[0] != fl.devices:
        raise ValueError('HipEngine: rate_scales are for %d devices, the fleet has %d' % (rates.shape[0], fl.devices))
    if rates is not None and fl is None and rates.shape[0] != 1:
        raise ValueError('HipEngine: rate_scales with a device axis need a fleet')
    dc = kind(n_collapse=D.shape[0], C=_dp(D.view(np.float64)) if D.shape[0] else None)
    if rates is not None:
        dc.rate_scales = _dp(rates) if D.shape[0] else None
    return dc, (D, rates)


def _entry_point(cfg, args, s, row_layout_given):
    """The creation symbol of include/qoc.h that serves the structs `s` (a dict: ensemble, fleet, transfer, control_map, decay -- carried by the
    members --, open -- the collapse_ops= keyword --, costs, sparse, plan; None where there is none), and its arguments."""
    ref = lambda x: None if x is None else C.byref(x)
    glue = ens, fl, tr, cmap = tuple(ref(s[name]) for name in ('ensemble', 'fleet', 'transfer', 'control_map'))
    dc, op, costs, sp, pl = (ref(s[name]) for name in ('decay', 'open', 'costs', 'sparse', 'plan'))
    lean, lean_sparse = args[:6] + args[-1:], args[2:8] + args[-1:]     # (no forbidden lists or Vs on an open engine; no Hs, U0 or Vs on a sparse one)
    composed = row_layout_given or any(g is not None for g in glue)    # (a plain sparse engine stays on qoc_create_sparse)
    table = (   # (what is there, the symbol, its arguments): the first row whose condition holds
        (sp and composed, 'qoc_create_sparse_fleet', (cfg, sp, pl) + glue + lean_sparse),
        (dc and costs, 'qoc_create_open_costs', (cfg, dc, costs) + glue + lean),
        (dc, 'qoc_create_open_fleet', (cfg, dc) + glue + lean),
        (fl, 'qoc_create_fleet', (cfg,) + glue + args),
        (cmap, 'qoc_create_mapped', (cfg, ens, tr, cmap) + args),
        (sp, 'qoc_create_sparse', (cfg, sp) + lean_sparse),
        # (the plain open problem with running costs: every glue pointer NULL -- in the library an ensemble engine of one nominal member)
        (op and costs, 'qoc_create_open_costs', (cfg, op, costs, None, None, None, None) + lean),
        (op, 'qoc_create_open', (cfg, op) + lean),       # (the state regularisers and Vs stay behind: the library refuses them by name)
        (tr, 'qoc_create_shaped', (cfg, ens, tr) + args),
        (ens, 'qoc_create_ensemble', (cfg, ens) + args),
        (True, 'qoc_create', (cfg,) + args))
    return next((symbol, call) for given, symbol, call in table if given)


class HipEngine(object):
    """Device-resident GRAPE problem: constants in HBM, n_seeds control sets, one HIP stream.  What does not combine with what is the table
    _REFUSALS above: a ValueError before the library is loaded.

    ensemble (robust GRAPE, include/qoc.h qoc_create_ensemble): a dict with keys `operators`, `offsets`, `amp_scales`, `weights` (see
    ensemble_arrays); every control set is then optimised for the weighted objective over the members, and the read-backs keep their
    per-control-set shapes (member 0 for the final unitary and inter_vecs; member_scalars / member_final_unitary give every member).
    An optional key `risk` (beta > 0) selects the soft worst case over the members in place of their mean (set_risk, member_weights).

    transfer (transfer-function GRAPE, include/qoc.h qoc_create_shaped): a real steps x P response matrix.  The variable, the gradient and
    get_uks are then (n_seeds, k, P) -- the AWG's samples --, get_pulse() gives the (n_seeds, k, steps) pulse the trajectories ran on, and the
    pulse regularisers act on the samples.  Composes with ensemble.

    exact_gradient (include/qoc.h qoc_config.gradient): False = the reference's first-order GRAPE gradient; True = the derivative of the slice
    propagators the engine computes (truncated Taylor series and squarings), so that loss and gradient belong to one function.  Generic path
    only (AUTO resolves to it; any other explicit path and time sharding raise QocError).  Composes with ensemble and transfer.

    collapse_ops (open-system GRAPE, include/qoc.h qoc_create_open): a list of n x n collapse operators that carry the square root of their
    rates (helper_functions/open_system.py builds the usual ones; an empty list is the closed limit).  The engine then propagates the operators
    psi_i psi_j^dagger of the states of interest under the Lindblad master equation, with degree taylor_terms and 2^scaling sub-steps per slice in
    both modes; loss, gradient and the optimiser entry points keep their shapes, get_final_density() and get_populations() take the place of
    get_final_unitary() and get_inter_vecs().  Given path=PATH_AUTO, an open engine (this keyword, or decay carried by ensemble or fleet) runs on
    PATH_LINDBLAD where its size rule holds (n <= 32 within 159 KiB of LDS) and on PATH_LINDBLAD_TILED up to n = 128
    (helper_functions/open_system.choose_path); an explicit path= is passed through.

    sparse_ops (sparse state transfer, include/qoc.h qoc_create_sparse): a list of k + 1 scipy.sparse matrices -i dt H0, -i dt H_1 .. in place of Hs
    (pass Hs=None, U0=None).  State transfer only, on path AUTO or PATH_SPARSE; the engine keeps every operator in ELLPACK and never forms an n x n
    array, so n = 2^14 and more fit.  vector_home: None / 'auto', 'lds' or 'global' (where the Taylor chain's two vectors live; A/B runs and tests).
    Every other entry point works as on a dense state-transfer engine.
    Sparse ensembles, fleets and maps (include/qoc.h qoc_create_sparse_fleet): with ensemble, fleet, control_map or row_layout the engine is made by
    the sparse ensemble entry point (a line, transfer=, is served by that entry point in C only).  The ensemble's `operators` (Hermitian P_q, scipy.sparse or dense; never densified here) go
    behind the controls as -i dt P_q; with a control_map sparse_ops holds the drift and the r operators the map feeds.  row_layout: None (a plain
    sparse engine stays on qoc_create_sparse), 0 / 'auto', 1 / 'per_operator' (the kernels of a plain sparse engine) or 2 / 'merged' (one list per
    row over all operators; the same numbers, fewer passes per Taylor term); self.plan['rows'] names what ran.

    noise traces (include/qoc.h qoc_set_traces): an `ensemble` dict with the key `traces` (E x q x steps), or a `fleet` with traces (F x E x q x steps):
    frozen row q' of member e then runs offsets[e, q'] + traces[e, q', t] at slice t -- sampled noise trajectories (helper_functions/noise.py) in place
    of errors that are constant over the pulse.  The table is uploaded after creation (the fleet's stands in front of the ensemble's, as its other rows
    do), set_traces() replaces or removes it between evaluations or bursts of iterations, and self.plan['traces'] is '1' while one is set.  Works on
    every engine with members and q >= 1, open and sparse ones included; taylor_terms and scaling are the caller's (robust.choose_taylor's rule).

    control_map (include/qoc.h qoc_create_mapped): a helper_functions.control_map.ControlMap (or a dict alpha / mix / fixed).  Hs then holds the drift
    and the r operators the map feeds, maxA (and one_minus_gauss, the variable, the gradient, get_uks) the k pulses: self.k is the number of pulses,
    self.terms the number of operators.  get_coefficients() gives the (n_seeds, r, steps) coefficients the nominal member's trajectories ran on.
    Composes with ensemble, transfer, exact_gradient and sparse_ops.

    fleet (device fleets, include/qoc.h qoc_create_fleet): a helper_functions.fleet.Fleet, or a dict with keys `offsets` (F x E x q) and `amp_scales`
    (F x E x k).  n_seeds = F R control sets, device-major: control set g is optimised on device g // R's members.  `ensemble` then supplies the
    operators, the weights and the risk (its offsets and amp_scales are not read; a Fleet brings its own when `ensemble` is None; neither: one
    member per device, no perturbation).  self.devices is F; every read-back keeps its (n_seeds, ...) shape.  Composes with transfer, control_map
    and exact_gradient.

    decay per member (open-system ensembles and fleets, include/qoc.h qoc_create_open_fleet): an `ensemble` dict with the keys `collapse_ops` (c
    operators as collapse_ops= takes them) and `rate_scales` (E x c, default ones), or a `fleet` with collapse_ops and rate_scales (F x E x c).  Member
    e of device f is then the open problem with the collapse operators sqrt(rate_scales[f, e, j]) C_j; self.open_system is True, get_final_density()
    and get_populations() give member 0 of each control set, member_final_density() every member, and everything an ensemble engine offers (risk,
    member read-backs, transfer, control_map, the loops) works as it does there.

    running_costs (open-system running costs, include/qoc.h qoc_create_open_costs): a list of at most 16 records (O, coeff, power) as
    helper_functions/open_system.py builds them (level_cost, subspace_cost, observable_cost, dressed_level_cost).  Every trajectory's state regulariser is
    then sum_l (coeff_l / steps) sum_tau sum_i x_l,i(tau)^power_l / power_l over the expectation values x_l,i(tau) = Re Tr(O_l rho_ii(tau)), tau = 0 ..
    steps; get_expectations() gives them, member_scalars()['reg_state'] every member's sum.  Needs an open engine -- collapse_ops= (an empty list is the
    closed limit) or decay carried by ensemble or fleet -- and composes with whatever that engine composes with; on a closed engine: ValueError, before
    the library is loaded (closed engines take reg_coeffs['forbidden_coeff_list'])."""

    def __init__(self, Hs, U0, V, W, maxA, dt, total_time, steps, taylor_terms, scaling, state_transfer=False,
                 reg_coeffs=None, one_minus_gauss=None, Vs=None, n_seeds=1, device=0, path=PATH_AUTO, chunks=0, variant=0, plan_seeds=0,
                 time_shards=0, time_rank=-1, time_comm=None, ensemble=None, transfer=None, exact_gradient=False, collapse_ops=None,
                 sparse_ops=None, vector_home=None, control_map=None, fleet=None, row_layout=None, running_costs=None):
        # 1. what the arguments refuse, before the library is loaded (_REFUSALS, and the checks between its blocks)
        a = dict(Hs=Hs, U0=U0, Vs=Vs, path=path, time_shards=time_shards, time_comm=time_comm, ensemble=ensemble, transfer=transfer,
                 exact_gradient=exact_gradient, collapse_ops=collapse_ops, sparse_ops=sparse_ops, fleet=fleet)
        sparse = decay = None
        if sparse_ops is not None:
            _refuse('sparse_ops with decay', a)
        elif row_layout is not None:
            raise ValueError('HipEngine: row_layout belongs to sparse_ops (sparse state transfer)')
        if (ensemble is not None or fleet is not None) and sparse_ops is None:
            if fleet is not None and ensemble is None and not isinstance(fleet, dict):
                E_members = int(np.shape(fleet.amp_scales)[1])
            else:
                E_members = 1 if ensemble is None else int(np.shape(ensemble['amp_scales'])[0])
            decay = decay_arrays(ensemble, fleet, int(np.shape(Hs)[1]), E_members, dt)
        if decay is not None:
            _refuse('decay', a)
        if fleet is not None:
            _refuse('fleet', a)
            if ensemble is None and not isinstance(fleet, dict):
                ensemble = fleet.device(0)
        if control_map is not None:
            _refuse('control_map', a)
            control_map = _cmap.validate(control_map, k=np.shape(maxA)[0], r=(len(sparse_ops) if sparse_ops is not None else np.shape(Hs)[0]) - 1, steps=steps)
        if sparse_ops is not None:
            _refuse('sparse_ops', a)
            if not state_transfer:
                raise ValueError('HipEngine: sparse_ops needs state_transfer=True (unitary mode propagates an n x n matrix)')
            if vector_home not in VECTOR_HOME:
                raise ValueError("HipEngine: vector_home is None, 'auto', 'lds' or 'global', got %r" % (vector_home,))
            if ensemble is not None and ensemble.get('amp_scales') is None:
                raise ValueError('HipEngine: an ensemble on sparse_ops needs amp_scales (E x k) and weights (helper_functions.robust.validate)')
            if row_layout is not None and row_layout not in ROW_LAYOUT:
                raise ValueError("HipEngine: row_layout is None, 0 / 'auto', 1 / 'per_operator' or 2 / 'merged', got %r" % (row_layout,))
            # (the ensemble's perturbation operators stand behind the controls, kept sparse)
            sparse = sparse_arrays(list(sparse_ops) + sparse_perturbations(ensemble, dt))
        if collapse_ops is not None:
            _refuse('collapse_ops', a)       # (a fleet has refused collapse_ops by now: the ensemble asked about is the caller's)
            collapse_ops = open_system.validate(collapse_ops, np.shape(Hs)[1])
        if running_costs is not None:
            if collapse_ops is None and decay is None:
                raise ValueError("HipEngine: running_costs need an open engine (collapse_ops=, or decay carried by ensemble or fleet); closed engines take "
                                 "reg_coeffs['forbidden_coeff_list']")
            running_costs = open_system.validate_costs(running_costs, np.shape(Hs)[1])
        if int(path) == PATH_AUTO and (collapse_ops is not None or decay is not None):
            # an open engine: PATH_LINDBLAD wherever its size rule holds (every engine that ran before this path existed), the tiled path above.  The
            # library's AUTO IS PATH_LINDBLAD, so where the rule holds the configuration goes over as it always did, with AUTO in it
            if open_system.choose_path(int(np.shape(Hs)[1]), len(collapse_ops) if collapse_ops is not None else int(decay[0].shape[0])) == PATH_LINDBLAD_TILED:
                path = PATH_LINDBLAD_TILED
        lib = load_library()
        self._lib = lib
        self._h = C.c_void_p()
        # 2. the configuration, the caller's arrays and one struct per feature
        if sparse is None:
            Hs = np.ascontiguousarray(np.asarray(Hs, dtype=np.complex128))
            k = Hs.shape[0] - 1 if control_map is None else control_map.n_pulses
            n = Hs.shape[1]
        else:
            k, n = (len(sparse_ops) - 1 if control_map is None else control_map.n_pulses), sparse[0]
        V = np.ascontiguousarray(np.asarray(V, dtype=np.complex128))
        m = V.shape[1]
        self.n, self.k, self.m, self.steps, self.n_seeds = n, k, m, int(steps), int(n_seeds)
        self.terms = k if control_map is None else control_map.n_terms      # operators beside the drift (a control map: what it feeds)
        self.state_transfer = bool(state_transfer)
        W = _c128(W, (n, m))
        U0a = None if U0 is None else _c128(U0, (n, n))
        maxA = np.ascontiguousarray(np.asarray(maxA, dtype=np.float64))
        assert maxA.shape == (k,)
        rcfg = reg_config(reg_coeffs, total_time)
        fs, fc = rcfg.pop('forbidden_states', None), rcfg.pop('forbidden_coeffs', None)
        use_vs = Vs is not None and fs is not None and len(fs) > 0
        # time_shards: one trajectory sharded along the time axis (csrc/qoc_gemm_ts.h); time_rank -1: emulated in this engine
        # plan_seeds 0: plan for n_seeds; > 0: the batch AUTO plans for (sharded restarts: see plan_seeds_for)
        cfg = QocConfig(n=n, k=k, steps=int(steps), m=m, taylor_terms=int(taylor_terms), scaling=int(scaling), state_transfer=int(bool(state_transfer)),
                        n_seeds=int(n_seeds), dt=float(dt), total_time=float(total_time), n_forbidden=0 if fs is None else len(fs),
                        forbid_dressed=int(use_vs), device=int(device), path=int(path), chunks=int(chunks), variant=int(variant),
                        time_shards=int(time_shards), time_rank=int(time_rank), gradient=int(bool(exact_gradient)), plan_seeds=int(plan_seeds),
                        **rcfg)       # (what is left of rcfg: the pulse regularisers' has_.. and c_.., band_lo and band_hi)
        self.exact_gradient = bool(exact_gradient)
        omg = None
        if one_minus_gauss is not None:
            omg = np.ascontiguousarray(np.asarray(one_minus_gauss, dtype=np.float64))
            assert omg.shape == (k, int(steps))
        Vsa = _c128(Vs, (n, n)) if use_vs else None
        args = (None if sparse is not None else _dp(Hs.view(np.float64)), None if U0a is None else _dp(U0a.view(np.float64)), _dp(V.view(np.float64)), _dp(W.view(np.float64)),
                _dp(maxA), _dp(omg), None if fs is None else fs.ctypes.data_as(_IP), _dp(fc), None if Vsa is None else _dp(Vsa.view(np.float64)),
                C.byref(self._h))
        none = (None, None)
        ens, a_ens = _ensemble_struct(ensemble, n, k, dt, sparse is None) if ensemble is not None else none
        tr, a_tr = _transfer_struct(transfer, int(steps)) if transfer is not None else none
        cmap, a_map = _map_struct(control_map) if control_map is not None else none
        fl, a_fl = _fleet_struct(fleet, ens, k) if fleet is not None else none
        rcs, a_rcs = _costs_struct(running_costs, n) if running_costs is not None else none
        (sp, pl), a_sp = _sparse_structs(sparse, vector_home, row_layout) if sparse is not None else (none, None)
        dc, a_dc = _decay_struct(decay[0], decay[1], fl) if decay is not None else none
        # (the collapse_ops= keyword: qoc_open, and with running costs the qoc_decay of qoc_create_open_costs without a table of rate scales)
        D = None if collapse_ops is None else np.ascontiguousarray(np.sqrt(float(dt)) * np.array(collapse_ops, dtype=np.complex128).reshape(len(collapse_ops), n, n))
        op, a_op = _decay_struct(D, kind=QocOpen if rcs is None else QocDecay) if collapse_ops is not None else none
        # 3. the one call (a_..: the arrays behind the structs, alive across it), and what the structs say about the engine it made
        symbol, call_args = _entry_point(C.byref(cfg), args, dict(ensemble=ens, fleet=fl, transfer=tr, control_map=cmap, decay=dc, open=op, costs=rcs,
                                                                  sparse=sp, plan=pl), row_layout is not None)
        _check(getattr(lib, symbol)(*call_args))
        by_sparse_fleet = symbol == 'qoc_create_sparse_fleet'
        self.open_system = op is not None or dc is not None
        self.samples = None if tr is None else int(tr.n_samples)          # transfer-function GRAPE: P, the length of the variable's rows
        self.devices = 0 if fl is None else int(fl.devices)                 # device fleets: F, the devices the n_seeds control sets are spread over
        self.n_costs = 0 if rcs is None else int(rcs.n_obs)                 # running costs: L, the observables behind get_expectations()
        self.row_layout = int(pl.row_layout) if by_sparse_fleet else None
        self.perturbations = 0 if ens is None else int(ens.n_perturb)     # q: the frozen control rows behind the `terms` rows of every trajectory
        # (without ensemble: one nominal member on a fleet and on a sparse engine of the ensemble entry point; collapse_ops= with running costs stays 0)
        self.members = int(ens.members) if ens is not None else int(fl is not None or by_sparse_fleet)
        self.risk = 0.0
        if ensemble is not None and float(ensemble.get('risk', 0.0)) > 0:
            self.set_risk(ensemble['risk'])
        self.path = lib.qoc_path_in_use(self._h)
        self.chunks = lib.qoc_chunks_in_use(self._h)
        self._read_plan()
        # noise traces: the fleet's table, else the ensemble's (Grape hands device 0 of a fleet over as its ensemble)
        traces = _getter(fleet)('traces') if fleet is not None else None
        if traces is None and fleet is None and ensemble is not None:
            traces = ensemble.get('traces')
        if traces is not None:
            self.set_traces(traces)
        if time_comm is not None:
            _check(lib.qoc_set_time_comm(self._h, time_comm._h))
            self._time_comm = time_comm                # keep it alive as long as the engine
            time_comm._attach(self)                    # ... and let it close this engine before it goes (QocComm.close)

    # -- lifetime ---------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self._lib.qoc_destroy(self._h)
            self._h = C.c_void_p()
            tc = getattr(self, '_time_comm', None)
            if tc is not None:
                tc._detach(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- trainable variable ---------------------------------------------------------------------------------------
    def _seed_shape(self):
        return (self.n_seeds, self.k, self.steps if self.samples is None else self.samples)

    def set_base(self, base):
        base = np.ascontiguousarray(np.asarray(base, dtype=np.float64)).reshape(self._seed_shape())
        _check(self._lib.qoc_set_base(self._h, _dp(base)))

    def get_base(self):
        out = np.empty(self._seed_shape())
        _check(self._lib.qoc_get_base(self._h, _dp(out)))
        return out

    # -- evaluation / optimisation ------------------------------------------------------------------------------
    def evaluate(self, want_grad=True):
        B = self.n_seeds
        loss, reg, g2, us = (np.empty(B) for _ in range(4))
        grad = np.empty(self._seed_shape()) if want_grad else None
        _check(self._lib.qoc_eval(self._h, _dp(loss), _dp(reg), _dp(g2), _dp(us), _dp(grad)))
        return dict(loss=loss, reg_loss=reg, grad_squared=g2, unitary_scale=us, grad=grad)

    def adam_step(self, lr):
        lr = np.ascontiguousarray(np.broadcast_to(np.asarray(lr, dtype=np.float64), (self.n_seeds,)))
        _check(self._lib.qoc_adam_step(self._h, _dp(lr)))

    @staticmethod
    def adam_params(rate=0.01, learning_rate_decay=2500, conv_target=1e-8, min_grad=1e-25, max_iterations=5000,
                    poll_every=100):
        p = QocAdamParams()
        p.rate, p.learning_rate_decay = float(rate), float(learning_rate_decay)
        p.conv_target, p.min_grad = float(conv_target), float(min_grad)
        p.max_iterations, p.poll_every = int(max_iterations), int(poll_every)
        return p

    def run_adam(self, params):
        its = np.empty(self.n_seeds, dtype=np.int32)
        _check(self._lib.qoc_run_adam(self._h, C.byref(params), its.ctypes.data_as(_IP)))
        return its

    def iterate(self, params, iters):
        _check(self._lib.qoc_iterate(self._h, C.byref(params), int(iters)))

    @staticmethod
    def lbfgs_params(conv_target=1e-8, min_grad=1e-25, max_iterations=5000, history=8, c1=1e-4, shrink=0.5, max_ls=20, poll_every=100):
        """Parameters of the device-resident L-BFGS loop (include/qoc.h, qoc_lbfgs_params): `history` curvature pairs per control set (1 .. 16),
        the Armijo constant `c1`, the factor `shrink` of a rejected trial step and the `max_ls` rejected trials after which the direction is reset."""
        p = QocLbfgsParams()
        p.conv_target, p.min_grad, p.c1, p.shrink = float(conv_target), float(min_grad), float(c1), float(shrink)
        p.max_iterations, p.history, p.max_ls, p.poll_every = int(max_iterations), int(history), int(max_ls), int(poll_every)
        return p

    def run_lbfgs(self, params):
        """The L-BFGS loop to the end of every control set (the host polls the done flags every params.poll_every iterations); the iteration counters."""
        its = np.empty(self.n_seeds, dtype=np.int32)
        _check(self._lib.qoc_run_lbfgs(self._h, C.byref(params), its.ctypes.data_as(_IP)))
        return its

    def iterate_lbfgs(self, params, iters):
        """Exactly `iters` iterations of the L-BFGS loop (one evaluation and one step each), no host synchronisation."""
        _check(self._lib.qoc_iterate_lbfgs(self._h, C.byref(params), int(iters)))

    def sync(self):
        _check(self._lib.qoc_sync(self._h))

    def scalars(self):
        B = self.n_seeds
        loss, reg, g2, us = (np.empty(B) for _ in range(4))
        its = np.empty(B, dtype=np.int32)
        done = np.empty(B, dtype=np.int32)
        _check(self._lib.qoc_get_scalars(self._h, _dp(loss), _dp(reg), _dp(g2), _dp(us), its.ctypes.data_as(_IP),
                                         done.ctypes.data_as(_IP)))
        return dict(loss=loss, reg_loss=reg, grad_squared=g2, unitary_scale=us, iterations=its, done=done)

    # -- read-back ------------------------------------------------------------------------------------------------
    def get_uks(self, evaluated=False):
        """maxA*sin(base) of the current variable, or (evaluated=True) the controls the last evaluation ran on."""
        out = np.empty(self._seed_shape())
        fn = self._lib.qoc_get_uks_evaluated if evaluated else self._lib.qoc_get_uks
        _check(fn(self._h, _dp(out)))
        return out

    def get_pulse(self):
        """Transfer-function engines: the (n_seeds, k, steps) pulse u_f = maxA T sin(base) the last evaluation ran on."""
        out = np.empty((self.n_seeds, self.k, self.steps))
        _check(self._lib.qoc_get_pulse(self._h, _dp(out)))
        return out

    def get_coefficients(self):
        """Mapped engines: the (n_seeds, r, steps) coefficients c of the operators, as member 0's trajectories ran them in the last evaluation."""
        out = np.empty((self.n_seeds, self.terms, self.steps))
        _check(self._lib.qoc_get_coefficients(self._h, _dp(out)))
        return out

    def get_final_unitary(self):
        out = np.empty((self.n_seeds, self.n, self.n), dtype=np.complex128)
        _check(self._lib.qoc_get_final_unitary(self._h, _dp(out.view(np.float64))))
        return out

    def get_final_density(self):
        """Open engines: rho_ij(T) of the last evaluation, (n_seeds, m, m, n, n); [g, i, i] is the density matrix state i ends in."""
        out = np.empty((self.n_seeds, self.m, self.m, self.n, self.n), dtype=np.complex128)
        _check(self._lib.qoc_get_final_density(self._h, _dp(out.view(np.float64))))
        return out

    def member_final_density(self):
        """Open ensemble and fleet engines: rho_ij(T) of every member at the last evaluation, (n_seeds, members, m, m, n, n)."""
        out = np.empty((self.n_seeds, max(self.members, 1), self.m, self.m, self.n, self.n), dtype=np.complex128)
        _check(self._lib.qoc_get_member_final_density(self._h, _dp(out.view(np.float64))))
        return out

    def get_populations(self):
        """Open engines: Re rho_ii(tau)[l, l] of the last evaluation, (n_seeds, steps + 1, n, m); tau = 0 is the start."""
        out = np.empty((self.n_seeds, self.steps + 1, self.n, self.m))
        _check(self._lib.qoc_get_populations(self._h, _dp(out)))
        return out

    def get_expectations(self):
        """Open engines with running_costs: x_l,i(tau) = Re Tr(O_l rho_ii(tau)) of the last evaluation, (n_seeds, steps + 1, L, m); tau = 0 is the start
        (member 0 of each control set)."""
        out = np.empty((self.n_seeds, self.steps + 1, self.n_costs, self.m))
        _check(self._lib.qoc_get_expectations(self._h, _dp(out)))
        return out

    def member_scalars(self):
        """Ensemble engines: dict(loss, reg_state) of the last evaluation, each [n_seeds][members].  An engine of collapse_ops= with running_costs is, in
        the library, an ensemble of one nominal member (qoc_create_open_costs with every glue pointer NULL): self.members stays 0, as on every engine
        made without ensemble or fleet (the run summary of a robust call keys on it), and the arrays are [n_seeds][1] -- reg_state is each control set's
        running cost R."""
        loss = np.empty((self.n_seeds, max(self.members, 1)))      # (collapse_ops= with running_costs: one nominal member)
        reg = np.empty((self.n_seeds, max(self.members, 1)))
        _check(self._lib.qoc_get_member_scalars(self._h, _dp(loss), _dp(reg)))
        return dict(loss=loss, reg_state=reg)

    def set_risk(self, beta):
        """Ensemble engines: the risk parameter beta >= 0 of the soft worst-case objective (include/qoc.h qoc_set_risk); 0 is the weighted
        mean.  Holds from the next evaluation, so a caller may anneal it between evaluations or bursts of iterations."""
        _check(self._lib.qoc_set_risk(self._h, float(beta)))
        self.risk = float(beta)

    def _read_plan(self):
        buf = C.create_string_buffer(1024)
        _check(self._lib.qoc_plan_describe(self._h, buf, 1024))
        self.plan = dict(kv.split('=', 1) for kv in buf.value.decode().split())

    def set_traces(self, traces):
        """Ensemble engines with q >= 1: the table of noise traces (include/qoc.h qoc_set_traces), (E, q, steps) -- with a fleet (F, E, q, steps) --
        added per slice to the frozen perturbation rows; None removes it.  Holds from the next evaluation and resets nothing (Adam moments, L-BFGS
        history, done flags), so a caller may draw fresh traces between bursts of iterate(); self.plan['traces'] follows."""
        if traces is None:
            _check(self._lib.qoc_set_traces(self._h, None))
        else:
            shape = ((self.devices,) if self.devices else ()) + (max(self.members, 1), self.perturbations, self.steps)
            tr = np.ascontiguousarray(np.asarray(traces, dtype=np.float64))
            if self.perturbations >= 1 and tr.shape != shape:
                raise ValueError('HipEngine: traces have shape %s, expected %s' % (tr.shape, shape))
            _check(self._lib.qoc_set_traces(self._h, _dp(tr)))
        self._read_plan()

    def member_weights(self):
        """Ensemble engines: the tilted weights pi_e of the last evaluation, [n_seeds][members] (the members' own weights at risk 0)."""
        out = np.empty((self.n_seeds, max(self.members, 1)))
        _check(self._lib.qoc_get_member_weights(self._h, _dp(out)))
        return out

    def trajectory_gradient(self):
        """Ensemble engines: the trajectories' gradient array of the last evaluation, before the member reduction:
        (n_seeds, members, terms + perturbations, steps).  On a sparse ensemble engine the frozen perturbation rows are exact zeros."""
        out = np.empty((self.n_seeds, max(self.members, 1), self.terms + self.perturbations, self.steps))
        _check(self._lib.qoc_get_trajectory_gradient(self._h, _dp(out)))
        return out

    def member_final_unitary(self):
        """Ensemble engines: every member's final unitary of the last evaluation, [n_seeds][members][n][n]."""
        out = np.empty((self.n_seeds, self.members, self.n, self.n), dtype=np.complex128)
        _check(self._lib.qoc_get_member_final_unitary(self._h, _dp(out.view(np.float64))))
        return out

    def get_inter_vecs(self):
        out = np.empty((self.n_seeds, self.steps + 1, self.n, self.m), dtype=np.complex128)
        _check(self._lib.qoc_get_inter_vecs(self._h, _dp(out.view(np.float64))))
        return out

    # -- measurement ----------------------------------------------------------------------------------------------
    def profile_enable(self, on=True):
        _check(self._lib.qoc_profile_enable(self._h, int(on)))

    def profile_read(self):
        name = C.c_char_p()
        launches = C.c_int64()
        ms = C.c_double()
        _check(self._lib.qoc_profile_read(self._h, C.byref(name), C.byref(launches), C.byref(ms)))
        return dict(kernel=name.value.decode(), launches=launches.value, total_ms=ms.value)

    def time_iterations(self, params, iters):
        ms = C.c_double()
        _check(self._lib.qoc_time_iterations(self._h, C.byref(params), int(iters), C.byref(ms)))
        return ms.value
