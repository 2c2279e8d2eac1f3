"""Body of the run-log test of Grape(collapse_ops=...).  h5py is optional; tests/test_open_system_gpu.py runs this file in an interpreter that
has it (as tests/test_h5_log.py does with tests/h5_scripts.py).  Usage: python open_system_h5_script.py <tmpdir>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'quantum-optimal-control_amd'))


def grape_open_system_save(tmp):
    """The run log of an open run holds collapse_ops, the final density operators and the populations in place of final_state and inter_vecs_*;
    the log of a closed run holds none of them."""
    import h5py
    from quantum_optimal_control.helper_functions import open_system
    from quantum_optimal_control.main_grape.grape import Grape
    SX = np.array([[0, 1], [1, 0]], dtype=complex)
    SY = np.array([[0, -1j], [1j, 0]], dtype=complex)
    conv = {'rate': 0.02, 'update_step': 5, 'max_iterations': 10, 'conv_target': 1e-10, 'learning_rate_decay': 1000}
    ops = [open_system.relaxation(2, 50.0), open_system.dephasing(2, 80.0)]
    for is_open, name in ((True, 'open'), (False, 'closed')):
        np.random.seed(3)
        uks, final = Grape(0.0 * SX, [2 * np.pi * SX / 2, 2 * np.pi * SY / 2], ['x', 'y'], SX, 20.0, 10, [0, 1], convergence=conv, reg_coeffs={},
                           maxA=[0.1, 0.1], show_plots=False, save=True, file_name=name, data_path=tmp, collapse_ops=ops if is_open else None)
        with h5py.File(os.path.join(tmp, '00000_%s.h5' % name), 'r') as f:
            for key in ('collapse_ops', 'final_density_real', 'final_density_imag', 'populations'):
                assert (key in f) == is_open, key
            for key in ('final_state', 'inter_vecs_raw_real', 'inter_vecs_mag_squared'):
                assert (key in f) != is_open, key
            for key in ('error', 'reg_error', 'uks', 'iteration', 'run_time', 'unitary_scale', 'taylor_terms'):
                assert key in f, key
            assert f['uks'].shape[1:] == (2, 10)
            if is_open:
                assert f['collapse_ops'].shape == (2, 2, 2) and np.allclose(f['collapse_ops'][()], np.array(ops))
                assert f['final_density_real'].shape[1:] == (2, 2, 2, 2) and f['populations'].shape[1:] == (2, 2, 11)
                rho = f['final_density_real'][-1] + 1j * f['final_density_imag'][-1]
                assert np.allclose(rho, final) and final.shape == (2, 2, 2, 2)
                assert np.allclose(f['populations'][-1][:, :, -1], np.real(np.einsum('iill->il', final)))
    print('OK grape_open_system_save')


if __name__ == '__main__':
    grape_open_system_save(sys.argv[1])
