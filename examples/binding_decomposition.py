#!/usr/bin/env python3
"""Which atoms carry the solvation part of a binding energy, on the MI355X (include/agbnp_hip.h, agbnp_hip_binding_decompose_*):
atoms FIRST..LAST of a structure are the ligand, the rest is the receptor, and one call decomposes the complex and both parts at
the complex's positions:

    u = E_RL - E_R - E_L = sum over terms t and atoms i of D[t][i],      D[t][i] = T_RL[t][i] - T_own[t][own(i)]

with T the four per-atom planes of an evaluation (cavity, vdW, GB self, GB pair).  Prints the four plane totals of u, u itself,
and the ten receptor atoms and the ten ligand atoms with the largest |sum_t D[t][i]|.  The planes are per atom: a per-residue
table is a sum over each residue's atoms.

  python examples/binding_decomposition.py trpcage 0 15       # bundled structure
  python examples/binding_decomposition.py 1dwc 4122 4151
  python examples/binding_decomposition.py /path/to/file.dms 2500 2530 --version 0
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
    ap.add_argument("first", type=int)
    ap.add_argument("last", type=int)
    ap.add_argument("--version", type=int, default=1)
    args = ap.parse_args()
    system = P.load_dms(args.system) if args.system.endswith(".dms") else P.load_system(args.system)

    force = AGBNPForce()
    force.setVersion(args.version)
    for r, g, a, q, h in zip(*system.params()):
        force.addParticle(r, g, a, q, bool(h))
    binding = P.BindingEnergy(force, range(args.first, args.last + 1))
    print(f"{system.name}: {system.n} atoms, ligand {args.first}..{args.last} ({len(binding.ligand_atoms)} atoms), receptor "
          f"{len(binding.receptor_atoms)} atoms, AGBNP version {args.version}")

    terms, u = binding.decompose(system.pos)
    for name, plane in zip(P.DECOMPOSITION_TERMS, terms):
        print(f"  {name:8s} {plane.sum():16.6f} kJ/mol")
    print(f"  u        {u:16.6f} kJ/mol   (the planes sum to {terms.sum():.6f})")

    per_atom = terms.sum(axis=0)
    for side, atoms in (("receptor", binding.receptor_atoms), ("ligand", binding.ligand_atoms)):
        print(f"the ten {side} atoms with the largest |sum_t D[t][i]| (kJ/mol):")
        print("  atom      total     cavity        vdW    GB self    GB pair")
        for k in np.argsort(-np.abs(per_atom[atoms]))[:10]:
            i = int(atoms[k])
            print(f"  {i:5d} {per_atom[i]:10.4f} " + " ".join(f"{terms[t, i]:10.4f}" for t in range(len(terms))))


if __name__ == "__main__":  # (importing the script -- a test collector, say -- runs nothing)
    main()
