#!/usr/bin/env python3
"""What the FIRE minimiser costs and buys (openmm_agbnp_plugin_amd/md.py: DeviceMD.minimise), for all systems in
ONE process: (a) ms per FIRE iteration -- `--iterations` of them with a tolerance that is never met, one host check at the end;
(b) ms per step of run(..., "descent"), the capped move along the force that examples/test_agbnp.py runs
(replayed graphs); (c) the largest per-atom force norm after 200 descent steps from the file's coordinates beside the
iterations FIRE needs from there for tolerance 10 kJ/mol/nm, and the energies both end at.  Version 1, NoCutoff, k_tether 2e4
(the settings of examples/test_agbnp.py); every repeat is timed with a host clock around work that ends in a synchronise.
Prints a table and one JSON line with the library's build id.

  python scripts/minimise_timing.py [--iterations 1000] [--repeats 3] [--systems trpcage,1dwc]
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
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--systems", default="trpcage,1dwc")
    args = ap.parse_args()
    import torch

    import openmm_agbnp_plugin_amd as P
    from openmm_agbnp_plugin_amd import _lib
    from openmm_agbnp_plugin_amd.md import DeviceMD

    out = {"build_id": _lib.build_id(), "iterations": args.iterations, "results": []}
    print("| system | atoms | FIRE, ms/iteration | descent, ms/step | fmax after 200 descent steps | E after them | FIRE iterations to fmax < 10 | E there |")
    print("|---|---|---|---|---|---|---|---|")
    for name in args.systems.split(","):
        s = P.load_system(name)
        k = P.HipCalcAGBNPForceKernel(device=0)
        k.initialize(P.AGBNPForce.from_arrays(*s.params(), version=1))
        md = DeviceMD(s, k, k_tether=2.0e4, dt=0.0005)
        md.settle()

        def restart():
            md.x.copy_(md.x0)
            md.forces()
            md.forces()  # (the first one behind a jump back to the start may be withheld)
            k.finish()

        def fmax():
            return float(md.frc.square().sum(dim=1).max().sqrt())

        restart()
        md.minimise(tolerance=1e-9, max_iterations=20, check_every=20)
        md.run(20, "descent", check_every=20)  # (captures the graphs)
        fire, descent, withheld = [], [], 0
        for _ in range(args.repeats):
            restart()
            torch.cuda.synchronize()
            start = time.perf_counter()
            rec = md.minimise(tolerance=1e-9, max_iterations=args.iterations, check_every=args.iterations)
            torch.cuda.synchronize()
            fire.append(1e3 * (time.perf_counter() - start) / args.iterations)
            withheld += int(rec["withheld"].sum())
            restart()
            torch.cuda.synchronize()
            start = time.perf_counter()
            withheld += md.run(args.iterations, "descent", check_every=args.iterations)
            torch.cuda.synchronize()
            descent.append(1e3 * (time.perf_counter() - start) / args.iterations)
        restart()
        missed = md.run(200, "descent", check_every=200)
        f_descent, e_descent = fmax(), float(md.ene)
        restart()
        rec = md.minimise(tolerance=10.0)[0]
        cell = lambda v: f"{sum(v) / len(v):.4f} ({' / '.join(f'{x:.4f}' for x in v)})"  # noqa: E731
        out["results"].append(dict(system=name, atoms=int(s.n), fire_ms=fire, descent_ms=descent, withheld=withheld, descent_200_fmax=f_descent,
                                   descent_200_energy=e_descent, descent_200_withheld=int(missed), fire_iterations=int(rec["iterations"]),
                                   fire_converged=int(rec["converged"]), fire_fmax=float(rec["fmax"]), fire_energy=float(rec["energy"]),
                                   fire_voids=int(rec["voids"]), fire_withheld=int(rec["withheld"])))
        print(f"| {name} | {int(s.n)} | {cell(fire)} | {cell(descent)} | {f_descent:.1f} | {e_descent:.4f} | {int(rec['iterations'])}"
              f"{'' if rec['converged'] else ' (NOT converged)'} | {float(rec['energy']):.4f} |"
              + (f"  WITHHELD {withheld + int(missed) + int(rec['withheld'])}" if withheld + int(missed) + int(rec["withheld"]) else ""), flush=True)
        del md, k
    print(json.dumps(out))


if __name__ == "__main__":
    main()
