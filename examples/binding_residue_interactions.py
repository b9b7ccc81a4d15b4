#!/usr/bin/env python3
"""Which receptor residue pays how much against which ligand residue, on the MI355X (include/agbnp_hip.h,
agbnp_hip_binding_set_atom_sets and agbnp_hip_binding_pair_matrix_*): atoms FIRST..LAST of a structure are the ligand, the rest
is the receptor, a sets file partitions the atoms of the complex (one line per atom: its residue), and one call tabulates

    D[a][b] = M_RL[a][b] - M_R[a][b] - M_L[a][b],      sum over a, b of D[a][b] = u = E_RL - E_R - E_L

with M the set-pair interaction matrices of the complex, the receptor and the ligand at the complex's positions.  Between a
receptor set and a ligand set D[a][b] + D[b][a] is their direct GB pair interaction; between two receptor sets it is how much
the ligand's arrival changes their interaction.  Prints the ten strongest receptor-set x ligand-set entries, the ten largest
receptor-receptor changes, and the matrix's sum beside u.  A set that holds atoms of both sides (a ligand that cuts a residue)
is listed with the ligand.  The pairwise table of an MM-GBSA decomposition: average pair_matrix_device() over frames.

  python examples/binding_residue_interactions.py trpcage tests/golden/residues_trpcage.txt 0 15
  python examples/binding_residue_interactions.py 1dwc tests/golden/residues_1dwc.txt 4122 4151
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd.AGBNPplugin import AGBNPForce


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("system")
    ap.add_argument("sets", help="one line per atom of the complex: atoms whose lines are equal form a set")
    ap.add_argument("first", type=int)
    ap.add_argument("last", type=int)
    ap.add_argument("--version", type=int, default=1)
    args = ap.parse_args()
    system = P.load_dms(args.system) if args.system.endswith(".dms") else P.load_system(args.system)
    sets, labels = P.load_sets(args.sets)
    if len(labels) > 2048:  # AGBNP_HIP_MAX_SETS
        raise SystemExit(f"{len(labels)} sets: a partition has at most 2048 (give a sets file with coarser sets)")

    force = AGBNPForce()
    force.setVersion(args.version)
    for r, g, a, q, h in zip(*system.params()):
        force.addParticle(r, g, a, q, bool(h))
    binding = P.BindingEnergy(force, range(args.first, args.last + 1))
    binding.set_atom_sets(sets, len(labels))
    ligand_sets = np.zeros(len(labels), dtype=bool)
    ligand_sets[np.asarray(sets)[binding.ligand_atoms]] = True
    print(f"{system.name}: {system.n} atoms in {len(labels)} sets, ligand {args.first}..{args.last} ({len(binding.ligand_atoms)} atoms in "
          f"{int(ligand_sets.sum())} sets), AGBNP version {args.version}")

    d, u = binding.pair_matrix(system.pos)
    between = d + d.T  # what a pair of sets contributes to u
    np.fill_diagonal(between, 0.0)
    across = np.abs(between) * np.outer(~ligand_sets, ligand_sets)
    print("the ten strongest receptor set - ligand set entries (kJ/mol):")
    for flat in np.argsort(-across, axis=None)[:10]:
        a, b = np.unravel_index(flat, d.shape)
        if across[a, b] > 0.0:
            print(f"  {labels[a]:>14s} - {labels[b]:<14s} {between[a, b]:12.4f}")
    inside = np.triu(np.abs(between) * np.outer(~ligand_sets, ~ligand_sets), 1)
    print("the ten largest changes between two receptor sets when the ligand arrives (kJ/mol):")
    for flat in np.argsort(-inside, axis=None)[:10]:
        a, b = np.unravel_index(flat, d.shape)
        if inside[a, b] > 0.0:
            print(f"  {labels[a]:>14s} - {labels[b]:<14s} {between[a, b]:12.4f}")
    print(f"sum of the {d.size} entries: {d.sum():.6f} kJ/mol   u: {u:.6f} kJ/mol")


if __name__ == "__main__":  # (importing the script -- a test collector, say -- runs nothing)
    main()
