#!/usr/bin/env python3
"""The solvation part of a binding energy on the MI355X (include/agbnp_hip.h, agbnp_hip_binding_*): atoms FIRST..LAST of a
structure are the ligand, the rest is the receptor, and one call evaluates the complex and both parts at the complex's positions:

    u = E_RL - E_R - E_L        E_lambda = E_R + E_L + lambda u        F_lambda = lambda F_RL + (1 - lambda) F_(R|L)

Prints the three energies, u, and the ten ligand atoms with the largest hybrid force; with --frames K it then scores K jittered
frames with the energy-only call and prints the mean and the standard deviation of u -- the solvation term of an MM-GBSA score
over a trajectory.

  python examples/binding_energy.py trpcage 0 15            # bundled structure, lambda = 0.5
  python examples/binding_energy.py 1dwc 4122 4151 0.35 --frames 100
  python examples/binding_energy.py /path/to/file.dms 2500 2530 1.0 --version 0
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import openmm_agbnp_plugin_amd as P
from openmm_agbnp_plugin_amd.AGBNPplugin import AGBNPForce

COMPONENTS = ("e_vol1", "e_vol2", "e_atom", "e_gb_pair")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("system")
    ap.add_argument("first", type=int)
    ap.add_argument("last", type=int)
    ap.add_argument("lam", type=float, nargs="?", default=0.5, metavar="LAMBDA")
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--version", type=int, default=1)
    args = ap.parse_args()
    system = P.load_dms(args.system) if args.system.endswith(".dms") else P.load_system(args.system)

    force = AGBNPForce()
    force.setVersion(args.version)
    for r, g, a, q, h in zip(*system.params()):
        force.addParticle(r, g, a, q, bool(h))
    binding = P.BindingEnergy(force, range(args.first, args.last + 1))
    ligand = binding.ligand_atoms
    print(f"{system.name}: {system.n} atoms, ligand {args.first}..{args.last} ({len(ligand)} atoms), receptor {len(binding.receptor_atoms)} atoms, "
          f"AGBNP version {args.version}")

    e_lam, u, forces = binding.execute(system.pos, args.lam)
    # (every member's last evaluation is complete and read back: its four energy components are its energy)
    e_rl, e_r, e_l = [sum(binding.member(which).scalar(c) for c in COMPONENTS) for which in ("complex", "receptor", "ligand")]
    print(f"  E_RL     {e_rl:16.6f} kJ/mol")
    print(f"  E_R      {e_r:16.6f} kJ/mol")
    print(f"  E_L      {e_l:16.6f} kJ/mol")
    print(f"  u        {u:16.6f} kJ/mol   (E_RL - E_R - E_L = {e_rl - e_r - e_l:.6f})")
    print(f"  E_lambda {e_lam:16.6f} kJ/mol   at lambda = {args.lam} (E_R + E_L + lambda u = {e_r + e_l + args.lam * u:.6f})")

    size = np.linalg.norm(forces[ligand], axis=1)
    print("the ten ligand atoms with the largest |F_lambda| (kJ/mol/nm):")
    print("  atom        |F|         Fx         Fy         Fz")
    for k in np.argsort(-size)[:10]:
        i = int(ligand[k])
        print(f"  {i:5d} {size[k]:10.4f} {forces[i, 0]:10.4f} {forces[i, 1]:10.4f} {forces[i, 2]:10.4f}")

    if args.frames > 0:
        us = np.array([binding.energy(system.jittered(step), args.lam)[1] for step in range(args.frames)])
        print(f"u over {args.frames} jittered frames: mean {us.mean():.6f} kJ/mol, standard deviation {us.std():.6f} kJ/mol")


if __name__ == "__main__":  # (importing the script -- a test collector, say -- runs nothing)
    main()
