#!/usr/bin/env python3
"""The first stages of a standard MD protocol on the MI355X engine: energy of the start structure, minimisation, Langevin
equilibration -- what the reference's example/test_agbnp.py does through simulation.minimizeEnergy() (example/test_agbnp.py:49)
and a LangevinIntegrator (300 K, 1/ps, 0.5 fs: example/test_agbnp.py:37).  The minimiser is FIRE on the device
(openmm_agbnp_plugin_amd/md.py, DeviceMD.minimise); examples/test_agbnp.py, the counterpart of the whole
reference script, still relaxes with 200 capped steps along the force.  AGBNP1 + tethers (the OPLS terms of the reference's
system come from OpenMM and are outside this repository).

  python examples/minimise_agbnp.py [system=trpcage] [tolerance=10.0 kJ/mol/nm] [equilibration steps=1000]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import openmm_agbnp_plugin_amd as P
from AGBNPplugin import AGBNPForce, HipCalcAGBNPForceKernel
from openmm_agbnp_plugin_amd.md import DeviceMD


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "trpcage"
    tolerance = float(sys.argv[2]) if len(sys.argv) > 2 else 10.0
    n_equil = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    system = P.load_dms(name) if name.endswith(".dms") else P.load_system(name)
    print("Started at: " + str(time.asctime()))

    force = AGBNPForce()
    force.setNonbondedMethod(AGBNPForce.NoCutoff)  # example/test_agbnp.py:17
    force.setVersion(1)                            # implicitSolvent='AGBNP'
    for r, g, a, q, h in zip(*system.params()):
        force.addParticle(r, g, a, q, bool(h))
    kernel = HipCalcAGBNPForceKernel()
    kernel.initialize(force)

    md = DeviceMD(system, kernel, dt=0.0005, temperature=300.0, friction=1.0)
    md.settle()
    md.forces()
    kernel.finish()
    print(f"{float(md.ene):.4f} kJ/mol")

    print("Minimization ...")
    start = time.perf_counter()
    relaxed = md.minimise(tolerance=tolerance)[0]
    elapsed = time.perf_counter() - start
    print(f"minimised in {int(relaxed['iterations'])} iterations{'' if relaxed['converged'] else ' (not converged)'}: "
          f"{relaxed['energy']:.4f} kJ/mol, largest force {relaxed['fmax']:.2f} kJ/mol/nm, {elapsed:.3f} s")
    if relaxed["voids"] or relaxed["withheld"]:
        print(f"({int(relaxed['voids'])} void iteration(s), {int(relaxed['withheld'])} withheld evaluation(s): repeated in place)")

    print("Equilibration ...")
    print('#"Step","Potential Energy (kJ/mole)","Total Energy (kJ/mole)","Temperature (K)"')

    def report(m):
        pot, kin = m.energies(last=1)
        print(f"{m.steps_done},{pot[0]:.4f},{pot[0] + kin[0]:.4f},{2.0 * kin[0] / (3 * system.n * 0.0083144626):.2f}")

    missed = md.run(n_equil, "langevin", check_every=max(min(n_equil, 1000), 1), on_report=report) if n_equil > 0 else 0
    if missed:
        print(f"WARNING: {missed} step(s) ran without the AGBNP term (tree capacity exceeded)")


if __name__ == "__main__":  # (importing the script -- a test collector, say -- runs nothing)
    main()
