"""HipState -- the engine-side counterpart of the reference's TensorflowState (core/tensorflow_state.py:11-394).

TensorflowState builds a static TF graph whose tensors run_session fetches; HipState uploads the same constants
to the MI355X once (``build_graph`` keeps the reference's method name) and exposes the same fetch set as plain
methods backed by the C ABI of libqoc_hip.so.
"""
import numpy as np

from quantum_optimal_control.core import hip_engine


class HipState(object):

    def __init__(self, sys_para, n_seeds=1, device=0, path=hip_engine.PATH_AUTO, chunks=0, first_seed=0, plan_seeds=0, time_comm=None, ensemble=None, transfer=None,
                 exact_gradient=False, collapse_ops=None, control_map=None, fleet=None, fleet_base=None, running_costs=None):
        self.sys_para = sys_para
        self.n_seeds = n_seeds
        self.first_seed = first_seed      # global index of this engine's first restart (seed-sharded runs)
        self.device = device
        self.path = path
        self.chunks = chunks
        self.plan_seeds = plan_seeds      # batch size AUTO plans for (0 = n_seeds): qoc_config.plan_seeds
        self.time_comm = time_comm        # hip_engine.QocComm of a time-sharded run (one trajectory over the GPUs of a node), or None
        self.ensemble = ensemble          # robust GRAPE: the validated robust dict of Grape (helper_functions/robust.py), or None
        self.transfer = transfer          # transfer-function GRAPE: the steps x P response matrix, or None (sys_para.ops_weight_base is then k x P)
        self.exact_gradient = bool(exact_gradient)   # qoc_config.gradient: the derivative of the computed propagators instead of the first-order formula
        self.collapse_ops = collapse_ops  # open-system GRAPE: the validated list of collapse operators (helper_functions/open_system.py), or None
        self.control_map = control_map    # control map: the validated helper_functions.control_map.ControlMap, or None (sys_para.ops_c are then the r operators it feeds)
        self.fleet = fleet                # device fleet: the validated helper_functions.fleet.Fleet, or None; n_seeds is then F x restarts, device-major
        self.fleet_base = fleet_base      # ... and each device's own first start point (F, k, P), or None: sys_para.ops_weight_base for every device
        self.running_costs = running_costs   # open-system running costs: the validated (O, coeff, power) records (helper_functions/open_system.py), or None
        self.engine = None

    def build_graph(self):
        sp = self.sys_para
        rc = sp.reg_coeffs
        if rc is None:
            # the reference evaluates `'amplitude' in None` here (regularization_functions.py:15)
            raise TypeError("argument of type 'NoneType' is not iterable")
        if 'd2wdt2' in rc and 'dwdt' not in rc:
            raise NameError("name 'new_weights' is not defined")         # regularization_functions.py:38-45
        if 'bandpass' in rc and not sp.use_gpu:
            raise ValueError('currently does not support bandpass reg for CPU (no CPU kernel for FFT)')
        needs_inter = ('forbidden_coeff_list' in rc) or ('speed_up' in rc)
        if needs_inter and not sp.state_transfer and not sp.use_inter_vecs:
            raise TypeError("'NoneType' object is not iterable")         # tfs.inter_vecs is None (:71, :381)
        Hs, U0, V, W, Vs = sp.engine_inputs()
        # the sparse route (core/sparse_parameters.py): Hs is then the list of scipy.sparse operators, and no dense array stands in for it
        sparse_ops = Hs if getattr(sp, 'sparse_route', False) else None
        self.engine = hip_engine.HipEngine(
            None if sparse_ops is not None else Hs, U0, V, W, sp.ops_max_amp, sp.dt, sp.total_time, sp.steps, sp.exp_terms, sp.scaling,
            state_transfer=sp.state_transfer, reg_coeffs=rc,
            one_minus_gauss=sp.one_minus_gauss if 'envelope' in rc else None, Vs=Vs,
            n_seeds=self.n_seeds, device=self.device, path=self.path, chunks=self.chunks, plan_seeds=self.plan_seeds,
            time_shards=0 if self.time_comm is None else self.time_comm.world, time_rank=-1 if self.time_comm is None else self.time_comm.rank,
            time_comm=self.time_comm, ensemble=self.ensemble, transfer=self.transfer, exact_gradient=self.exact_gradient,
            collapse_ops=self.collapse_ops, sparse_ops=sparse_ops, control_map=self.control_map, fleet=self.fleet,
            running_costs=self.running_costs)
        base = np.asarray(sp.ops_weight_base, dtype=np.float64)
        if self.fleet is not None:
            # control set (f, r) starts where control set r of the same call without a fleet starts (or, r = 0, from device f's own point)
            from quantum_optimal_control.helper_functions.fleet import tile_bases
            from quantum_optimal_control.parallel_seeds import restart_guesses
            F = self.fleet.n_devices
            R = self.n_seeds // F
            extra = restart_guesses(base.shape[0], base.shape[1], 1, R - 1)
            if self.fleet_base is None:
                base = tile_bases(np.concatenate([base[None], extra], axis=0), F)
            else:
                first = np.asarray(self.fleet_base, dtype=np.float64).reshape((F, 1) + base.shape)
                base = tile_bases(np.concatenate([first, np.broadcast_to(extra[None], (F,) + extra.shape)], axis=1), F)
        elif base.ndim == 2 and (self.n_seeds > 1 or self.first_seed > 0):
            # global restart 0 = the reference's own starting point; restart g > 0 = the reproducible stream of index g,
            # whatever rank / batch it lands in
            from quantum_optimal_control.parallel_seeds import restart_guesses
            if self.first_seed == 0:
                extra = restart_guesses(base.shape[0], base.shape[1], 1, self.n_seeds - 1)
                base = np.concatenate([base[None], extra], axis=0)
            else:
                base = restart_guesses(base.shape[0], base.shape[1], self.first_seed, self.n_seeds)
        elif base.ndim == 2:
            base = base[None]
        self.engine.set_base(base)
        self.start_base = base            # (n_seeds, k, P): where every control set starts
        print("Graph built!")
        return self.engine

    def close(self):
        if self.engine is not None:
            self.engine.close()
            self.engine = None
