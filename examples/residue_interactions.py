#!/usr/bin/env python3
"""Residue-by-residue table of the AGBNP energy of a structure on the MI355X (include/agbnp_hip.h, agbnp_hip_pair_matrix_host):
the set-pair interaction matrix M over a partition of the atoms -- M[a][b] + M[b][a] is the GB pair energy between sets a and b,
M[a][a] what set a holds in itself (cavity, van der Waals, GB self, its own pairs) -- the ten strongest interactions between
sets, the ten largest diagonal entries, and the matrix's sum beside the energy.  The pairwise table of an MM-GBSA-style
decomposition: average pair_matrix_device() over the frames of a trajectory.

  python examples/residue_interactions.py trpcage tests/golden/residues_trpcage.txt   # one line per atom: its residue
  python examples/residue_interactions.py 1dwc tests/golden/residues_1dwc.txt
  python examples/residue_interactions.py trpcage     # no file: a heavy atom and the hydrogens that follow it form a set
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd.AGBNPplugin import AGBNPForce


def heavy_atom_groups(system):
    """Every heavy atom with the hydrogens that follow it (hydrogens in front of the first heavy atom join it)."""
    sets = np.maximum(np.cumsum(system.ishydrogen == 0) - 1, 0).astype(np.int32)
    first = [int(np.flatnonzero(sets == k)[0]) for k in range(int(sets.max()) + 1)]
    return sets, [f"atom {i}" for i in first]


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "trpcage"
    system = P.load_dms(name) if name.endswith(".dms") else P.load_system(name)
    sets, labels = P.load_sets(sys.argv[2]) if len(sys.argv) > 2 else heavy_atom_groups(system)
    if len(labels) > 2048:  # AGBNP_HIP_MAX_SETS
        raise SystemExit(f"{len(labels)} sets: a partition has at most 2048 (give a sets file with coarser sets)")

    force = AGBNPForce()
    force.setVersion(1)
    for r, g, a, q, h in zip(*system.params()):
        force.addParticle(r, g, a, q, bool(h))

    context = P.AGBNPContext(force)
    context.setPositions(system.pos)
    energy, m = context.getInteractionMatrix(sets, num_sets=len(labels))
    print(f"{system.name}: {system.n} atoms in {len(labels)} sets")

    between = m + m.T  # the GB pair energy between two sets
    np.fill_diagonal(between, 0.0)
    upper = np.triu(np.abs(between), 1)
    print("the ten strongest interactions between sets (kJ/mol):")
    for flat in np.argsort(-upper, axis=None)[:10]:
        a, b = np.unravel_index(flat, m.shape)
        if upper[a, b] > 0.0:
            print(f"  {labels[a]:>14s} - {labels[b]:<14s} {between[a, b]:12.4f}")
    print("the ten largest diagonal entries (kJ/mol):")
    for a in np.argsort(-np.abs(np.diag(m)))[:10]:
        print(f"  {labels[a]:>14s} {m[a, a]:12.4f}")
    print(f"sum of the {m.size} entries: {m.sum():.6f} kJ/mol   energy: {energy:.6f} kJ/mol")


if __name__ == "__main__":  # (importing the script -- a test collector, say -- runs nothing)
    main()
