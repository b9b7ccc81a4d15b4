"""The reference of every binding-energy test (tests/test_binding_restatement.py on the CPU, tests/test_gpu_binding.py on the
device): three CPU oracles -- the complex, the receptor and the ligand, the latter two made from AGBNPSystem.subset() -- combined
in NumPy by the formulas of include/agbnp_hip.h (agbnp_hip_binding_*):

    u        = E_RL(x) - E_R(x_R) - E_L(x_L)
    E_lam    = E_R + E_L + lam u = (1 - lam)(E_R + E_L) + lam E_RL
    F_lam,i  = lam F^RL_i + (1 - lam) F^R_r(i)   (i a receptor atom)     = lam F^RL_i + (1 - lam) F^L_l(i)   (i a ligand atom)

The ligand is a set of atom indices of the complex, in any order; the receptor is the rest; both keep ascending complex order.
A plain module like tests/gpu_helpers.py: the test files import what they use."""
import numpy as np

import openmm_agbnp_plugin_amd as P
from oracle import Oracle


def partition(n, ligand_atoms):
    """(receptor atoms, ligand atoms), both ascending."""
    ligand = np.array(sorted(int(a) for a in ligand_atoms), dtype=np.int64)
    assert 1 <= len(ligand) < n and len(set(ligand.tolist())) == len(ligand) and ligand[0] >= 0 and ligand[-1] < n
    receptor = np.setdiff1d(np.arange(n), ligand)
    return receptor, ligand


def system_of(params, pos):
    radius, gamma, alpha, charge, ish = params
    return P.AGBNPSystem("complex", pos, radius, gamma, alpha, charge, ish)


class BindingRestatement:
    """The three oracles of one partition; evaluate(pos) runs them at one geometry of the complex."""

    def __init__(self, params, ligand_atoms, version=1, cutoff=None, method=1):
        n = len(params[0])
        self.receptor, self.ligand = partition(n, ligand_atoms)
        s = system_of(params, np.zeros((n, 3)))
        kw = dict(version=version, cutoff=cutoff, method=method)
        self.oracles = (Oracle(*s.params(), **kw), Oracle(*s.subset(self.receptor).params(), **kw),
                        Oracle(*s.subset(self.ligand).params(), **kw))

    def evaluate(self, pos):
        """((E_RL, E_R, E_L), F_RL[N, 3], F_own[N, 3]): F_own holds every atom's force in its own sub-system."""
        pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
        e_rl, f_rl = self.oracles[0].execute(pos)
        e_r, f_r = self.oracles[1].execute(np.ascontiguousarray(pos[self.receptor]))
        e_l, f_l = self.oracles[2].execute(np.ascontiguousarray(pos[self.ligand]))
        f_own = np.zeros_like(pos)
        f_own[self.receptor] = np.asarray(f_r).reshape(-1, 3)
        f_own[self.ligand] = np.asarray(f_l).reshape(-1, 3)
        return (float(e_rl), float(e_r), float(e_l)), np.asarray(f_rl, dtype=np.float64).reshape(-1, 3).copy(), f_own


def combine(energies, f_rl, f_own, lam):
    """(E_lam, u, F_lam) of one evaluate()."""
    e_rl, e_r, e_l = energies
    u = e_rl - e_r - e_l
    return (1.0 - lam) * (e_r + e_l) + lam * e_rl, u, lam * f_rl + (1.0 - lam) * f_own


def restate(params, ligand_atoms, pos, lam, version=1, cutoff=None, method=1):
    """(E_lam, u, F_lam[N, 3], (E_RL, E_R, E_L)) at `pos`."""
    energies, f_rl, f_own = BindingRestatement(params, ligand_atoms, version, cutoff, method).evaluate(pos)
    return combine(energies, f_rl, f_own, lam) + (energies,)
