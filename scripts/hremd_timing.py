#!/usr/bin/env python3
"""What a Hamiltonian exchange attempt costs (openmm_agbnp_plugin_amd/md.py: HamiltonianReplicaMD), timed in one process: (a) ms
per step of a steady run without attempts, beside ReplicaMD's on contexts of its own (the same launches: the yardstick); (b) ms
per attempt -- cross round, the two launches, refresh -- as the difference between a run with an attempt every
`--exchange-every` steps and the run without, over the number of attempts.  Charges scaled by 1 - 0.05 k, all rungs at 300 K,
Langevin, 1 fs; every repeat is timed with a host clock around work that ends in a synchronise and checked for withheld
evaluations.  Prints a table and one JSON line with the library's build id.

  python scripts/hremd_timing.py [--steps 2000] [--warmup 40] [--repeats 3] [--exchange-every 20] [--cases trpcage:4,trpcage:8]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--exchange-every", type=int, default=20)
    ap.add_argument("--cases", default="trpcage:4,trpcage:8", help="system:replicas, comma-separated")
    args = ap.parse_args()
    import torch

    import openmm_agbnp_plugin_amd as P
    from openmm_agbnp_plugin_amd import _lib
    from openmm_agbnp_plugin_amd.md import HamiltonianReplicaMD, ReplicaMD

    def kernel(s, q=1.0):
        radius, gamma, alpha, charge, ish = s.params()
        k = P.HipCalcAGBNPForceKernel(device=0)
        k.initialize(P.AGBNPForce.from_arrays(radius, gamma, alpha, charge * q, ish, version=1))
        return k

    def timed(md, **kw):
        torch.cuda.synchronize()
        start = time.perf_counter()
        withheld = int(md.run(args.steps, "langevin", check_every=1000, **kw).sum())
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - start), withheld

    out = {"build_id": _lib.build_id(), "steps": args.steps, "warmup": args.warmup, "exchange_every": args.exchange_every, "results": []}
    print("| system | R | ReplicaMD, ms/step | HamiltonianReplicaMD, ms/step | ms/attempt | accepted |")
    print("|---|---|---|---|---|---|")
    for name, R in [(c.split(":")[0], int(c.split(":")[1])) for c in args.cases.split(",")]:
        s = P.load_system(name)
        rep = ReplicaMD(s, [kernel(s) for _ in range(R)], [300.0] * R, k_tether=1.0e5)
        ham = HamiltonianReplicaMD(s, [kernel(s, 1.0 - 0.05 * k) for k in range(R)], [300.0] * R, k_tether=1.0e5)
        for md in (rep, ham):
            md.settle()
            md.forces()
            md.finish()
            md.run(args.warmup, "langevin", exchange_every=args.exchange_every, check_every=args.warmup)
        attempts = args.steps // args.exchange_every
        t = {"replica_step": [], "hamiltonian_step": [], "attempt": []}
        withheld = 0
        for _ in range(args.repeats):
            ms, w = timed(rep)
            t["replica_step"].append(ms / args.steps)
            withheld += w
            plain, w = timed(ham)
            t["hamiltonian_step"].append(plain / args.steps)
            withheld += w
            ms, w = timed(ham, exchange_every=args.exchange_every)
            t["attempt"].append((ms - plain) / max(attempts, 1))
            withheld += w
        log = ham.exchange_log()
        mean = {key: sum(v) / len(v) for key, v in t.items()}
        out["results"].append(dict(system=name, replicas=R, withheld=withheld, attempted=int(len(log)), accepted=int((log["accepted"] == 1).sum()),
                                   void=int((log["accepted"] < 0).sum()), **{key + "_ms": v for key, v in t.items()}))
        cell = lambda key: f"{mean[key]:.4f} ({' / '.join(f'{x:.4f}' for x in t[key])})"  # noqa: E731
        print(f"| {name} | {R} | {cell('replica_step')} | {cell('hamiltonian_step')} | {cell('attempt')} | "
              f"{int((log['accepted'] == 1).sum())} of {len(log)} |" + (f"  WITHHELD {withheld}" if withheld else ""), flush=True)
        del rep, ham
    print(json.dumps(out))


if __name__ == "__main__":
    main()
