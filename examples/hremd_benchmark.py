#!/usr/bin/env python3
"""Hamiltonian replica exchange on the MI355X engine: R rungs of one system, all at 300 K, the charges of rung k scaled by
1 - 0.05 k (which tempers the GB term), Langevin (1/ps friction, 1 fs step, as examples/1dwc_benchmark.py), AGBNP1 + tethers,
all rungs advanced by one set of launches per step (agbnp_hip_execute_group between the group forms of the integrator kernels)
and an exchange attempt between neighbouring rungs every `exchange_every` steps: cross energies by agbnp_hip_energy_group,
the decision and the exchange of the conformations on the device (openmm_agbnp_plugin_amd/md.py, HamiltonianReplicaMD).
Prints every rung's potential energy and the walker it holds at every report, the elapsed time / aggregate ns/day and the
acceptance per rung pair at the end.

  python examples/hremd_benchmark.py [system=trpcage] [replicas=4] [steps=10000] [exchange_every=100] [minimise=0]

A non-zero `minimise` relaxes every rung with FIRE (md.minimise()) before the first step.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import openmm_agbnp_plugin_amd as P
from AGBNPplugin import AGBNPForce, HipCalcAGBNPForceKernel
from openmm_agbnp_plugin_amd.md import HamiltonianReplicaMD

CHARGE_STEP = 0.05  # the charges of rung k are scaled by 1 - CHARGE_STEP k


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "trpcage"
    replicas = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    nsteps = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
    exchange_every = int(sys.argv[4]) if len(sys.argv) > 4 else 100
    minimise = bool(int(sys.argv[5])) if len(sys.argv) > 5 else False
    system = P.load_dms(name) if name.endswith(".dms") else P.load_system(name)

    kernels = []
    for k in range(replicas):  # one context per rung
        force = AGBNPForce()
        force.setNonbondedMethod(AGBNPForce.CutoffNonPeriodic)
        force.setCutoffDistance(1.0)
        force.setVersion(1)
        for r, g, a, q, h in zip(*system.params()):
            force.addParticle(r, g, a, q * (1.0 - CHARGE_STEP * k), bool(h))
        kernel = HipCalcAGBNPForceKernel()
        kernel.initialize(force)
        kernels.append(kernel)

    md = HamiltonianReplicaMD(system, kernels, [300.0] * replicas, k_tether=1.0e5, dt=0.001, friction=1.0)
    md.settle()
    md.forces()
    md.finish()
    if minimise:
        for r, rec in enumerate(md.minimise()):
            print(f"rung {r}: minimised in {int(rec['iterations'])} iterations{'' if rec['converged'] else ' (not converged)'}: "
                  f"{rec['energy']:.4f} kJ/mol, largest force {rec['fmax']:.2f} kJ/mol/nm")
    print(f"{system.name}: {system.n} atoms x {replicas} rungs, AGBNP1 + tethers, Langevin 300 K, 1 fs, charges x 1-{1.0 - CHARGE_STEP * (replicas - 1):.2f}, "
          f"exchange every {exchange_every} steps, engine on {torch.cuda.get_device_name(0)}")
    print('#"Step",' + ",".join(f'"Potential Energy {k} (kJ/mole)","Walker {k}"' for k in range(replicas)))

    def report(m):
        pot, walkers = m.last[:, 0].cpu().numpy(), m.walkers()
        print(f"{m.steps_done}," + ",".join(f"{pot[k]:.4f},{walkers[k]}" for k in range(replicas)))

    md.run(20, "langevin", check_every=20)  # first steps outside the timed region
    torch.cuda.synchronize()
    start = time.perf_counter()
    # every 1000 steps the host reads every member's overflow log: an evaluation whose trees outgrew their store gave NO AGBNP
    # term for that rung (outputs are withheld, never partial) and is counted; a withheld cross energy makes its pair void.
    missed = md.run(nsteps, "langevin", exchange_every=exchange_every, check_every=1000, on_report=report)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - start
    if missed.any():
        print(f"WARNING: evaluation(s) ran without the AGBNP term, per rung {missed.tolist()} (tree capacity exceeded)")
    print(f"elapsed time={elapsed:.3f}s   {1e3 * elapsed / nsteps:.4f} ms/step   {86.4 * nsteps * replicas / (elapsed * 1e3):.1f} ns/day "
          f"aggregate ({replicas} rungs)")
    print("acceptance k<->k+1: " + " ".join("-" if a != a else f"{a:.2f}" for a in md.acceptance()))


if __name__ == "__main__":  # (importing the script -- a test collector, say -- runs nothing)
    main()
