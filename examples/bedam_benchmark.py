#!/usr/bin/env python3
"""Lambda replica exchange over a binding ladder (BEDAM / single decoupling) on the MI355X engine: R replicas of one complex
under E_lambda = E_R + E_L + lambda u, u = E_RL - E_R - E_L, on an even lambda ladder from 0 to 1, all at 300 K, Langevin
(1/ps friction, 1 fs step), AGBNP1 + tethers.  All replicas are advanced by one binding group per step
(agbnp_hip_binding_execute_group between the group forms of the integrator kernels: one gather launch, the members' evaluations
as replica groups, one combine launch that reads every lambda from device memory) and an exchange attempt between neighbouring
rungs every EVERY steps: one small launch that swaps lambdas on the device from the u words the steps' last evaluation left
(openmm_agbnp_plugin_amd/md.py, BindingReplicaMD).  The ligand is the atoms FIRST .. LAST of the system.  Prints the acceptance
per rung pair, the mean u per rung over the attempts and ms per step.

  python examples/bedam_benchmark.py [SYSTEM=trpcage] [FIRST=0] [LAST=15] [RUNGS=4] [STEPS=2000] [EVERY=50]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import openmm_agbnp_plugin_amd as P
from AGBNPplugin import AGBNPForce, BindingEnergy
from openmm_agbnp_plugin_amd.md import BindingReplicaMD


def main():
    arg = lambda i, default: type(default)(sys.argv[i]) if len(sys.argv) > i else default  # noqa: E731
    name, first, last, rungs, nsteps, every = arg(1, "trpcage"), arg(2, 0), arg(3, 15), arg(4, 4), arg(5, 2000), arg(6, 50)
    system = P.load_dms(name) if name.endswith(".dms") else P.load_system(name)
    ligand = list(range(first, last + 1))

    bindings = []
    for _ in range(rungs):  # one binding (complex, receptor and ligand contexts) per replica
        force = AGBNPForce()
        force.setVersion(1)
        for r, g, a, q, h in zip(*system.params()):
            force.addParticle(r, g, a, q, bool(h))
        bindings.append(BindingEnergy(force, ligand))
    ladder = np.linspace(0.0, 1.0, rungs) if rungs > 1 else np.array([1.0])

    md = BindingReplicaMD(system, bindings, ladder, 300.0, k_tether=1.0e5, dt=0.001, friction=1.0)
    md.settle()
    md.forces()
    md.finish()
    print(f"{system.name}: {system.n} atoms, ligand {first}..{last}, {rungs} rungs lambda = " + " ".join(f"{x:.3f}" for x in ladder) +
          f", AGBNP1 + tethers, Langevin 300 K, 1 fs, exchange every {every} steps, engine on {torch.cuda.get_device_name(0)}")
    md.run(20, "langevin", check_every=20)  # first steps outside the timed region
    torch.cuda.synchronize()
    start = time.perf_counter()
    # every 1000 steps the host reads every binding's log: a withheld evaluation gave NO AGBNP term for that replica (outputs are
    # withheld, never partial) and is counted; if it was the one an attempt reads u from, the replica's pair is void
    missed = md.run(nsteps, "langevin", exchange_every=every, check_every=1000)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - start
    if missed.any():
        print(f"WARNING: evaluation(s) ran without the AGBNP term, per replica {missed.tolist()}")
    log = md.exchange_log()
    print("acceptance k<->k+1: " + " ".join("-" if a != a else f"{a:.2f}" for a in md.acceptance()))
    judged = log[log["accepted"] >= 0]
    mean_u = []
    for k in range(rungs):  # rung k is the `lo` of the pairs (k, k + 1) and the `hi` of the pairs (k - 1, k)
        u = np.concatenate([judged["u_lo"][judged["rung"] == k], judged["u_hi"][judged["rung"] == k - 1]])
        mean_u.append("-" if len(u) == 0 else f"{u.mean():.3f}")
    print("mean u per rung (kJ/mol): " + " ".join(mean_u))
    print(f"void pairs: {int((log['accepted'] < 0).sum())} of {len(log)}   lambda of every replica now: " + " ".join(f"{x:.3f}" for x in md.lambdas()))
    print(f"elapsed time={elapsed:.3f}s   {1e3 * elapsed / max(nsteps, 1):.4f} ms/step   {86.4 * nsteps * rungs / (elapsed * 1e3):.1f} ns/day "
          f"aggregate ({rungs} replicas)")


if __name__ == "__main__":  # (importing the script -- a test collector, say -- runs nothing)
    main()
