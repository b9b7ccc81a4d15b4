"""The reference of the set-pair matrix of a binding energy (include/agbnp_hip.h: agbnp_hip_binding_pair_matrix_*;
tests/test_binding_pair_matrix_restatement.py on the CPU, tests/test_gpu_binding_pair_matrix.py on the device): the matrix
restatement (tests/pair_matrix_restatement.py) of the complex, of subset(receptor) and of subset(ligand), each with the
partition restricted to its atoms under the SAME set numbering and the SAME number of sets, and

    D[a][b] = M_RL[a][b] - M_R[a][b] - M_L[a][b],      u = E_RL - E_R - E_L = sum_{a,b} D[a][b].

A plain module like tests/binding_decomposition_restatement.py: the test files import what they use."""
import numpy as np

from tests.binding_restatement import partition, system_of
from tests.pair_matrix_restatement import restate_matrix


def restate(params, ligand_atoms, pos, sets, num_sets, version=1, cutoff=None, method=1):
    """(D[num_sets, num_sets], u) at `pos`; u from the three members' oracle energies, formed as
    tests/binding_decomposition_restatement.py forms it."""
    d, u, _ = restate_members(params, ligand_atoms, pos, sets, num_sets, version, cutoff, method)
    return d, u


def restate_members(params, ligand_atoms, pos, sets, num_sets, version=1, cutoff=None, method=1):
    """(D, u, (M_RL, M_R, M_L)): the members' matrices as well, for the tests that look at one of them."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    sets = np.asarray(sets, dtype=np.int64)
    n = len(params[0])
    receptor, ligand = partition(n, ligand_atoms)
    s = system_of(params, pos)
    kw = dict(version=version, cutoff=cutoff, method=method)
    e_rl, m_rl, _ = restate_matrix(s.params(), s.pos, sets, num_sets, **kw)
    d = m_rl.copy()
    u = float(e_rl)  # (E_RL - E_R - E_L in that order, as tests/binding_restatement.py forms it)
    members = [m_rl]
    for atoms in (receptor, ligand):
        sub = s.subset(atoms)
        e, m, _ = restate_matrix(sub.params(), sub.pos, sets[atoms], num_sets, **kw)
        d -= m
        u -= float(e)
        members.append(m)
    return d, u, tuple(members)
