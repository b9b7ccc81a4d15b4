#!/usr/bin/env python3
"""Perturbation energies on the MI355X (include/agbnp_hip.h, agbnp_hip_perturbed_energies_host): what ONE conformation costs under
M parameter sets, from one evaluation.  Builds a charge-scaling ladder q (1 - 0.05 m), m = 0 .. M - 1, prints E_m from one call
beside the energies of M separately created kernels (what the same answer costs without the call), and the one-sample Zwanzig
estimate between neighbouring rungs, dF(m -> m + 1) ~ E_{m+1} - E_m at this single conformation -- over the frames of a
trajectory a caller averages exp(-(E_{m+1} - E_m) / kT) instead, and the rows E_m of every frame are an MBAR matrix's.

  python examples/perturbation_energies.py trpcage 8     # bundled structure, 8 rungs
  python examples/perturbation_energies.py 1dwc 16
  python examples/perturbation_energies.py /path/to/file.dms 4
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd.AGBNPplugin import AGBNPForce


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "trpcage"
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    system = P.load_dms(name) if name.endswith(".dms") else P.load_system(name)
    radius, gamma, alpha, charge, ishydrogen = system.params()
    scales = 1.0 - 0.05 * np.arange(count)

    context = P.AGBNPContext(AGBNPForce.from_arrays(radius, gamma, alpha, charge, ishydrogen))
    context.setPositions(system.pos)
    energy, energies = context.getPerturbedEnergies(np.tile(gamma, (count, 1)), np.tile(alpha, (count, 1)), np.outer(scales, charge))

    print(f"{system.name}: {system.n} atoms, {count} charge-scaling rungs; the context's own energy {energy:.6f} kJ/mol")
    print("  rung  scale   one call, kJ/mol   its own kernel, kJ/mol   difference")
    for m, scale in enumerate(scales):
        kernel = P.HipCalcAGBNPForceKernel()
        kernel.initialize(AGBNPForce.from_arrays(radius, gamma, alpha, scale * np.asarray(charge), ishydrogen))
        alone = kernel.energy(system.pos)
        kernel.release()
        print(f"  {m:4d}  {scale:5.2f} {energies[m]:18.6f} {alone:24.6f} {energies[m] - alone:12.2e}")
    print("Zwanzig estimate between neighbouring rungs from this one conformation, kJ/mol:")
    for m in range(count - 1):
        print(f"  {m:2d} -> {m + 1:2d} {energies[m + 1] - energies[m]:14.6f}")


if __name__ == "__main__":  # (importing the script -- a test collector, say -- runs nothing)
    main()
