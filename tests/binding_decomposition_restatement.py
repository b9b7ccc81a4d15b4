"""The reference of the per-atom decomposition of a binding energy (include/agbnp_hip.h: agbnp_hip_binding_decompose_*;
tests/test_binding_decomposition_restatement.py on the CPU, tests/test_gpu_binding_decomposition.py on the device): the
decomposition restatement (tests/decomposition_restatement.py) of the complex, of subset(receptor) and of subset(ligand), the two
sub-systems' planes scattered back to the complex's atom order through the partition of tests/binding_restatement.py, and

    D[t][i] = T_RL[t][i] - T_own[t][own(i)],      u = E_RL - E_R - E_L = sum_{t,i} D[t][i].

A plain module like tests/gpu_helpers.py: the test files import what they use."""
import numpy as np

from tests.binding_restatement import partition, system_of
from tests.decomposition_restatement import TERMS, restate as restate_member


def restate(params, ligand_atoms, pos, version=1, cutoff=None, method=1):
    """(D[4, N], u) at `pos`; u from the three members' oracle energies."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n = len(params[0])
    receptor, ligand = partition(n, ligand_atoms)
    s = system_of(params, pos)
    kw = dict(version=version, cutoff=cutoff, method=method)
    e_rl, t_rl, _ = restate_member(s.params(), s.pos, **kw)
    own = np.zeros((len(TERMS), n))
    u = float(e_rl)  # (E_RL - E_R - E_L in that order, as tests/binding_restatement.py forms it)
    for atoms in (receptor, ligand):
        sub = s.subset(atoms)
        e, t, _ = restate_member(sub.params(), sub.pos, **kw)
        own[:, atoms] = t
        u -= float(e)
    return t_rl - own, u
