"""The reference of every set-pair interaction matrix test (tests/test_pair_matrix_restatement.py on the CPU,
tests/test_gpu_pair_matrix.py on the device): a NumPy restatement of M[S][S] of include/agbnp_hip.h (agbnp_hip_pair_matrix_*),
built from the per-atom terms of tests/decomposition_restatement.py and the CPU oracle's Born radii:

    a != b   M[a][b] = k sum_{i in a, j in b} q_i q_j f_ij
    a == b   M[a][a] = sum_{i in a} (T0 + T1 + T2)_i + k sum_{i != j, both in a} q_i q_j f_ij      (ordered pairs)

with f_ij = 1 / sqrt(d^2 + B_i B_j exp(-d^2 / (4 B_i B_j))) (d^2 < cutoff^2 with a cutoff).  The block sums of k q_i q_j f_ij are
formed over row chunks with a one-hot matrix of the sets on both sides.  Version 0 has the cavity term on the diagonal only.  A
plain module like tests/decomposition_restatement.py: the test files import what they use."""
import numpy as np

from tests.decomposition_restatement import CHUNK, DIEL, restate


def pair_values(pos, charge, born, lo, hi, cutoff=None):
    """k q_i q_j f_ij for the rows lo..hi - 1 and every column; 0 for i == j and beyond the cutoff."""
    d2 = ((pos[lo:hi, None, :] - pos[None, :, :]) ** 2).sum(axis=-1)
    bb = born[lo:hi, None] * born[None, :]
    f = 1.0 / np.sqrt(d2 + bb * np.exp(-0.25 * d2 / bb))
    f[np.arange(hi - lo), np.arange(lo, hi)] = 0.0
    if cutoff is not None:
        f[d2 >= cutoff * cutoff] = 0.0
    return DIEL * charge[lo:hi, None] * charge[None, :] * f


def restate_matrix(params, pos, sets, num_sets, version=1, cutoff=None, method=1):
    """(energy of Oracle.execute, M[num_sets, num_sets], terms[4, N]) at `pos` for the partition `sets` (one index per atom)."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    sets = np.asarray(sets, dtype=np.int64)
    if method == 0:
        cutoff = None
    energy, terms, o = restate(params, pos, version=version, cutoff=cutoff, method=method)
    n = len(sets)
    matrix = np.zeros((num_sets, num_sets))
    np.add.at(matrix, (sets, sets), terms[0] + terms[1] + terms[2])
    if version == 1:
        onehot = np.zeros((n, num_sets))
        onehot[np.arange(n), sets] = 1.0
        born, q = o.vector("born"), np.asarray(params[3], dtype=np.float64)
        for lo in range(0, n, CHUNK):
            hi = min(n, lo + CHUNK)
            matrix += onehot[lo:hi].T @ (pair_values(pos, q, born, lo, hi, cutoff) @ onehot)
    return energy, matrix, terms
