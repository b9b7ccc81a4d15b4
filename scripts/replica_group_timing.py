#!/usr/bin/env python3
"""Replica groups (include/agbnp_hip.h: agbnp_hip_execute_group) against the single-context paths, timed in one process:
trpcage (versions 1 and 0) and 1dwc (version 1) with R = 1, 2, 4, 8 contexts, three ways -- (a) R evaluations back to back on
one stream, (b) R contexts on R streams, (c) the group call -- in blocks of queued rounds timed with device events after a
warm-up, every block checked with finish() == 0.  Every member keeps one position buffer, as an MD loop does; a new geometry
is copied into it in front of every block (outside the timed region).  Prints one JSON line: ms per round, ms per
replica-evaluation and the aggregate ns/day (1 fs steps: 86.4 / ms per replica-evaluation), with the library's build id.
AGBNP_HIP_GROUP_LAUNCHES=0 in the environment makes (c) run every member alone (the A/B of the grouping itself).

  python scripts/replica_group_timing.py [--steps 200] [--warmup 24] [--replicas 1,2,4,8] [--systems trpcage:1,trpcage:0,1dwc:1]
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
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--replicas", default="1,2,4,8")
    ap.add_argument("--systems", default="trpcage:1,trpcage:0,1dwc:1", help="name:version, comma-separated")
    args = ap.parse_args()
    import torch

    import openmm_agbnp_plugin_amd as P
    from openmm_agbnp_plugin_amd import _lib

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)  # (not the default stream: its handle is NULL, which the engine reads as its own stream)
    sp = stream.cuda_stream
    replicas = [int(r) for r in args.replicas.split(",")]
    out = {"build_id": _lib.build_id(), "steps": args.steps, "warmup": args.warmup,
           "group_launches": os.environ.get("AGBNP_HIP_GROUP_LAUNCHES", "1") != "0", "results": []}
    block = 8  # rounds per timed block
    for name, version in [(x.split(":")[0], int(x.split(":")[1])) for x in args.systems.split(",")]:
        s = P.load_system(name)
        geoms = torch.tensor(np.stack([s.jittered(i) for i in range(8)]), dtype=torch.float64, device=dev).contiguous()
        for R in replicas:
            ks = []
            for m in range(R):
                k = P.HipCalcAGBNPForceKernel(device=0)
                k.initialize(P.AGBNPForce.from_arrays(*s.params(), version=version))
                k.execute(s.jittered(m), np.zeros((s.n, 3)))
                ks.append(k)
            pos = torch.zeros((R, s.n, 3), dtype=torch.float64, device=dev)
            frc = torch.zeros((R, s.n, 3), dtype=torch.float64, device=dev)
            ene = torch.zeros((R,), dtype=torch.float64, device=dev)
            side = [torch.cuda.Stream(device=dev) for _ in range(R)]
            torch.cuda.synchronize()
            times = {"a": [], "b": [], "c": []}
            for rnd in range((args.warmup + args.steps) // block + 1):
                for way in ("a", "b", "c"):
                    with torch.cuda.stream(stream):
                        for m in range(R):
                            pos[m].copy_(geoms[(rnd + m) % len(geoms)])
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(stream)
                    if way == "b":
                        for st in side:
                            st.wait_event(t0)
                    for i in range(block):
                        g = [pos[m] for m in range(R)]
                        if way == "c":
                            P.execute_group(ks, [x.data_ptr() for x in g], [frc[m].data_ptr() for m in range(R)],
                                            [ene[m:m + 1].data_ptr() for m in range(R)], sp)
                            continue
                        for m, k in enumerate(ks):
                            k.execute_device(g[m].data_ptr(), frc[m].data_ptr(), ene[m:m + 1].data_ptr(),
                                             side[m].cuda_stream if way == "b" else sp)
                    if way == "b":
                        for st in side:
                            e = torch.cuda.Event()
                            e.record(st)
                            stream.wait_event(e)
                    t1.record(stream)
                    for m, k in enumerate(ks):
                        assert k.finish(side[m].cuda_stream if way == "b" else sp) == 0, "an evaluation was withheld"
                    if rnd * block >= args.warmup:
                        times[way].append(t0.elapsed_time(t1) / block)
            torch.cuda.synchronize()
            row = {"system": name, "version": version, "atoms": s.n, "R": R,
                   "group_members": int(ks[0].scalar("group_members"))}
            for way, v in times.items():
                ms = float(np.median(v))
                row[way] = {"ms_per_round": round(ms, 5), "ms_per_replica_eval": round(ms / R, 5),
                            "ns_per_day": round(86.4 * R / ms, 1)}
            out["results"].append(row)
            for k in ks:
                k.release()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
