"""Body of the run-log test of Grape(transfer=...).  h5py is optional; tests/test_transfer_gpu.py runs this file in an interpreter that has it
(as tests/test_h5_log.py does with tests/h5_scripts.py).  Usage: python transfer_h5_script.py <tmpdir>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'quantum-optimal-control_amd'))


def grape_transfer_save(tmp):
    """The run log of a shaped run: the response matrix, and a uks_samples row (k x P) beside every uks row (k x steps)."""
    import h5py
    from quantum_optimal_control.helper_functions import transfer as tf
    from quantum_optimal_control.main_grape.grape import Grape
    SX = np.array([[0, 1], [1, 0]], dtype=complex)
    SY = np.array([[0, -1j], [1j, 0]], dtype=complex)
    line = tf.gaussian_filter(40, 8, 20.0, 0.6)
    conv = {'rate': 0.02, 'update_step': 5, 'max_iterations': 10, 'conv_target': 1e-10, 'learning_rate_decay': 1000}
    np.random.seed(3)
    uks, _ = Grape(0.0 * SX, [2 * np.pi * SX / 2, 2 * np.pi * SY / 2], ['x', 'y'], SX, 20.0, 40, [0, 1], convergence=conv, reg_coeffs={},
                   maxA=[0.1, 0.1], show_plots=False, save=True, file_name='shaped', data_path=tmp, transfer=line)
    with h5py.File(os.path.join(tmp, '00000_shaped.h5'), 'r') as f:
        assert np.array_equal(f['transfer_matrix'][()], line.matrix)
        assert f['uks'].shape[1:] == (2, 40) and f['uks_samples'].shape[1:] == (2, 8) and f['uks'].shape[0] == f['uks_samples'].shape[0] >= 3
        assert np.array_equal(f['uks'][-1], uks) and np.array_equal(f['uks_samples'][-1], line.samples)
        for row in range(f['uks'].shape[0]):
            assert np.max(np.abs(f['uks'][row] - tf.apply(line, f['uks_samples'][row]))) <= 1e-14
    print('OK grape_transfer_save')


if __name__ == '__main__':
    grape_transfer_save(sys.argv[1])
