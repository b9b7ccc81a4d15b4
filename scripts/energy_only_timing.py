#!/usr/bin/env python3
"""Energy-only against full evaluations (include/agbnp_hip.h: agbnp_hip_energy_device / agbnp_hip_execute_device), timed in one
process: 1dwc (version 1) and trpcage (versions 0 and 1), the two kinds alternating on the device-resident path in blocks of 16
queued evaluations, each block timed with device events, after a warm-up.  Prints one JSON line with the medians in ms and the library's build id.

  python scripts/energy_only_timing.py [--steps 200] [--warmup 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import torch

    import openmm_agbnp_plugin_amd as P
    from openmm_agbnp_plugin_amd import _lib

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)  # (not the default stream: its handle is NULL, which the engine reads as its own stream)
    sp = stream.cuda_stream
    out = {"build_id": _lib.build_id(), "steps": args.steps, "warmup": args.warmup, "results": []}
    for name, version in (("1dwc", 1), ("trpcage", 1), ("trpcage", 0)):
        s = P.load_system(name)
        k = P.HipCalcAGBNPForceKernel(device=0)
        k.initialize(P.AGBNPForce.from_arrays(*s.params(), version=version))
        # a handful of nearby geometries, visited in turn (the trees are rebuilt every evaluation, no jump between them)
        geoms = torch.tensor(np.stack([s.jittered(i) for i in range(8)]), dtype=torch.float64, device=dev).contiguous()
        frc = torch.zeros((s.n, 3), dtype=torch.float64, device=dev)
        ene = torch.zeros((2,), dtype=torch.float64, device=dev)
        k.execute(s.jittered(0), np.zeros((s.n, 3)))
        torch.cuda.synchronize()
        # blocks of `block` evaluations of one kind, the kinds alternating block by block; device events around each block
        # (an event pair around a single evaluation measured far less than its kernels take)
        block = 16
        times = {"full": [], "energy": []}
        for rnd in range((args.warmup + args.steps) // block + 1):
            for kind in ("full", "energy"):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                for i in range(block):
                    g = geoms[i % len(geoms)]
                    if kind == "full":
                        k.execute_device(g.data_ptr(), frc.data_ptr(), ene[0:1].data_ptr(), sp)
                    else:
                        k.energy_device(g.data_ptr(), ene[1:2].data_ptr(), sp)
                b.record(stream)
                assert k.finish(sp) == 0, "an evaluation was withheld"
                if rnd * block >= args.warmup:
                    times[kind].append(a.elapsed_time(b) / block)
        torch.cuda.synchronize()
        ms = {kind: float(np.median(v)) for kind, v in times.items()}
        out["results"].append({"system": name, "version": version, "atoms": s.n, "full_ms": round(ms["full"], 5),
                               "energy_only_ms": round(ms["energy"], 5), "ratio": round(ms["energy"] / ms["full"], 4),
                               "energy_only_launches": int(k.scalar("energy_only_launches")),
                               "full_launches": int(k.scalar("launches"))})
        k.release()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
