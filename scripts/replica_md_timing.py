#!/usr/bin/env python3
"""Replica-exchange MD (openmm_agbnp_plugin_amd/md.py: ReplicaMD) against what the repository could do before it, timed in one
process: (a) R DeviceMD graph-replay loops, one context each, run one after another; (b) one ReplicaMD over R contexts of its
own, with an exchange attempt every `--exchange-every` steps.  Langevin, 1 fs; `--steps` timed steps after a warm-up (graph
capture, first group calls); the two ways alternate, `--repeats` times each, every repeat timed with a host clock around work
that ends in a synchronise and checked for withheld steps.  Prints a table and one JSON line: aggregate steps per second
(R x steps / elapsed), every repeat, with the library's build id.

  python scripts/replica_md_timing.py [--steps 2000] [--warmup 40] [--repeats 3] [--exchange-every 100]
                                      [--cases trpcage:1,trpcage:2,trpcage:4,trpcage:8,1dwc:4]
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
    ap.add_argument("--exchange-every", type=int, default=100)
    ap.add_argument("--cases", default="trpcage:1,trpcage:2,trpcage:4,trpcage:8,1dwc:4", help="system:replicas, comma-separated")
    args = ap.parse_args()
    import torch

    import openmm_agbnp_plugin_amd as P
    from openmm_agbnp_plugin_amd import _lib
    from openmm_agbnp_plugin_amd.md import DeviceMD, ReplicaMD

    def kernel(s):
        k = P.HipCalcAGBNPForceKernel(device=0)
        k.initialize(P.AGBNPForce.from_arrays(*s.params(), version=1))
        return k

    out = {"build_id": _lib.build_id(), "steps": args.steps, "warmup": args.warmup, "exchange_every": args.exchange_every, "results": []}
    print("| system | R | (a) R x DeviceMD, steps/s | (b) ReplicaMD, steps/s | b / a | accepted |")
    print("|---|---|---|---|---|---|")
    for name, R in [(c.split(":")[0], int(c.split(":")[1])) for c in args.cases.split(",")]:
        s = P.load_system(name)
        ladder = [300.0 * 1.03 ** r for r in range(R)]
        singles = [DeviceMD(s, kernel(s), k_tether=1.0e5, temperature=ladder[r], seed=r) for r in range(R)]
        for md in singles:
            md.settle()
            md.forces()
            md.kernel.finish()
            md.run(args.warmup, "langevin", check_every=args.warmup)
        rep = ReplicaMD(s, [kernel(s) for _ in range(R)], ladder, k_tether=1.0e5)
        rep.settle()
        rep.forces()
        rep.finish()
        rep.run(args.warmup, "langevin", exchange_every=args.exchange_every, check_every=args.warmup)
        torch.cuda.synchronize()
        rate = {"a": [], "b": []}
        withheld = 0
        for _ in range(args.repeats):
            start = time.perf_counter()
            for md in singles:
                withheld += md.run(args.steps, "langevin", check_every=1000)
            torch.cuda.synchronize()
            rate["a"].append(R * args.steps / (time.perf_counter() - start))
            start = time.perf_counter()
            withheld += int(rep.run(args.steps, "langevin", exchange_every=args.exchange_every, check_every=1000).sum())
            torch.cuda.synchronize()
            rate["b"].append(R * args.steps / (time.perf_counter() - start))
        log = rep.exchange_log()
        mean = {w: sum(v) / len(v) for w, v in rate.items()}
        spread = {w: (max(v) - min(v)) / mean[w] for w, v in rate.items()}
        out["results"].append({"system": name, "replicas": R, "a_steps_per_s": rate["a"], "b_steps_per_s": rate["b"], "withheld": withheld,
                               "attempted": int(len(log)), "accepted": int(log["accepted"].sum())})
        cell = lambda w: f"{mean[w]:.0f} ({' / '.join(f'{x:.0f}' for x in rate[w])}; spread {100 * spread[w]:.1f} %)"  # noqa: E731
        print(f"| {name} | {R} | {cell('a')} | {cell('b')} | {mean['b'] / mean['a']:.2f} | {int(log['accepted'].sum())} of {len(log)} |"
              + (f"  WITHHELD {withheld}" if withheld else ""), flush=True)
        del singles, rep
    print(json.dumps(out))


if __name__ == "__main__":
    main()
