#!/usr/bin/env python3
"""Per-atom decomposition of the AGBNP energy of a structure on the MI355X (include/agbnp_hip.h, agbnp_hip_decompose_host): the
four totals -- cavity, van der Waals, GB self, GB pair -- and their sum, the GaussVol surface area of every heavy atom
(A_i = cavity term / gamma_i), and the ten atoms that carry the most solvation energy.  The starting point of a per-residue
MM-GBSA-style table: sum the columns over a residue's atoms, average decompose_device() over the frames of a trajectory.

  python examples/decompose_agbnp.py 1dwc                # bundled structure (openmm_agbnp_plugin_amd/data/1dwc.dat)
  python examples/decompose_agbnp.py /path/to/file.dms   # Desmond .dms with an agbnp2 table
  python examples/decompose_agbnp.py trpcage 0           # version 0: the cavity term alone
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd.AGBNPplugin import AGBNPForce


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "1dwc"
    version = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    system = P.load_dms(name) if name.endswith(".dms") else P.load_system(name)

    force = AGBNPForce()
    force.setVersion(version)
    for r, g, a, q, h in zip(*system.params()):
        force.addParticle(r, g, a, q, bool(h))

    context = P.AGBNPContext(force)
    context.setPositions(system.pos)
    energy, terms = context.getEnergyDecomposition()
    print(f"{system.name}: {system.n} atoms ({system.nheavy} heavy), AGBNP version {version}")
    for term, plane in zip(P.DECOMPOSITION_TERMS, terms):
        print(f"  {term:8s} {plane.sum():16.6f} kJ/mol")
    print(f"  {'total':8s} {energy:16.6f} kJ/mol   (sum of the {terms.size} terms: {terms.sum():.6f})")

    gamma = np.asarray(system.gamma, dtype=np.float64)
    area = np.divide(terms[0], gamma, out=np.zeros(system.n), where=gamma != 0.0)
    print(f"surface area: {area.sum():.4f} nm^2 over {int((gamma != 0.0).sum())} atoms with a surface tension")
    print("  atom   area/nm^2")
    for i in np.flatnonzero(gamma != 0.0):
        print(f"  {i:5d} {area[i]:10.5f}")

    per_atom = terms.sum(axis=0)
    print("the ten atoms with the largest |sum of terms| (kJ/mol):")
    print("  atom      total " + " ".join(f"{t:>10s}" for t in P.DECOMPOSITION_TERMS))
    for i in np.argsort(-np.abs(per_atom))[:10]:
        print(f"  {i:5d} {per_atom[i]:10.4f} " + " ".join(f"{terms[t, i]:10.4f}" for t in range(len(P.DECOMPOSITION_TERMS))))


if __name__ == "__main__":  # (importing the script -- a test collector, say -- runs nothing)
    main()
