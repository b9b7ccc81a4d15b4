#!/usr/bin/env python3
"""Temperature replica exchange on the MI355X engine: R replicas of one system on a geometric temperature ladder from
300 K, Langevin (1/ps friction, 1 fs step, as examples/1dwc_benchmark.py), AGBNP1 + tethers, all replicas advanced by one
set of launches per step (agbnp_hip_execute_group between the group forms of the integrator kernels) and an exchange
attempt between neighbouring rungs every `exchange_every` steps, decided on the device (openmm_agbnp_plugin_amd/md.py,
ReplicaMD).  Prints every replica's potential energy and rung at every report, the elapsed time / aggregate ns/day and
the acceptance per rung pair at the end.

  python examples/remd_benchmark.py [system=trpcage] [replicas=8] [steps=10000] [exchange_every=100] [minimise=0]

A non-zero `minimise` relaxes every replica with FIRE (md.minimise()) before the first step.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import openmm_agbnp_plugin_amd as P
from AGBNPplugin import AGBNPForce, HipCalcAGBNPForceKernel
from openmm_agbnp_plugin_amd.md import ReplicaMD

RATIO = 1.05  # neighbouring rungs: T_{k+1} / T_k


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "trpcage"
    replicas = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    nsteps = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
    exchange_every = int(sys.argv[4]) if len(sys.argv) > 4 else 100
    minimise = bool(int(sys.argv[5])) if len(sys.argv) > 5 else False
    system = P.load_dms(name) if name.endswith(".dms") else P.load_system(name)

    kernels = []
    for _ in range(replicas):  # one context per replica
        force = AGBNPForce()
        force.setNonbondedMethod(AGBNPForce.CutoffNonPeriodic)
        force.setCutoffDistance(1.0)
        force.setVersion(1)
        for r, g, a, q, h in zip(*system.params()):
            force.addParticle(r, g, a, q, bool(h))
        kernel = HipCalcAGBNPForceKernel()
        kernel.initialize(force)
        kernels.append(kernel)

    ladder = [300.0 * RATIO ** k for k in range(replicas)]
    md = ReplicaMD(system, kernels, ladder, k_tether=1.0e5, dt=0.001, friction=1.0)
    md.settle()
    md.forces()
    md.finish()
    if minimise:
        for r, rec in enumerate(md.minimise()):
            print(f"replica {r}: minimised in {int(rec['iterations'])} iterations{'' if rec['converged'] else ' (not converged)'}: "
                  f"{rec['energy']:.4f} kJ/mol, largest force {rec['fmax']:.2f} kJ/mol/nm")
    print(f"{system.name}: {system.n} atoms x {replicas} replicas, AGBNP1 + tethers, Langevin {ladder[0]:.0f}-{ladder[-1]:.0f} K, 1 fs, "
          f"exchange every {exchange_every} steps, engine on {torch.cuda.get_device_name(0)}")
    print('#"Step",' + ",".join(f'"Potential Energy {r} (kJ/mole)","Rung {r}"' for r in range(replicas)))

    def report(m):
        pot, rungs = m.last[:, 0].cpu().numpy(), m.rungs()
        print(f"{m.steps_done}," + ",".join(f"{pot[r]:.4f},{rungs[r]}" for r in range(replicas)))

    md.run(20, "langevin", check_every=20)  # first steps outside the timed region
    torch.cuda.synchronize()
    start = time.perf_counter()
    # every 1000 steps the host reads every member's overflow log: a step whose trees outgrew their store got NO AGBNP force
    # for that replica (outputs are withheld, never partial) and is counted; a production driver would roll back.
    missed = md.run(nsteps, "langevin", exchange_every=exchange_every, check_every=1000, on_report=report)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - start
    if missed.any():
        print(f"WARNING: step(s) ran without the AGBNP term, per replica {missed.tolist()} (tree capacity exceeded)")
    print(f"elapsed time={elapsed:.3f}s   {1e3 * elapsed / nsteps:.4f} ms/step   {86.4 * nsteps * replicas / (elapsed * 1e3):.1f} ns/day "
          f"aggregate ({replicas} replicas)")
    print("acceptance k<->k+1: " + " ".join("-" if a != a else f"{a:.2f}" for a in md.acceptance()))


if __name__ == "__main__":  # (importing the script -- a test collector, say -- runs nothing)
    main()
