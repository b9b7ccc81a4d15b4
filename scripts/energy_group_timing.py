#!/usr/bin/env python3
"""Energy-only replica groups (include/agbnp_hip.h: agbnp_hip_energy_group) against the other ways to get R energies, timed in
one process: trpcage (versions 1 and 0) and 1dwc (version 1) with R = 1, 2, 4, 8 contexts, four ways, alternating -- (a) R
energy_device calls back to back on one stream, (b) the same on R streams, (c) the energy_group call, (d) the full execute_group
whose forces are thrown away -- in blocks of 8 queued rounds timed with device events after a warm-up, every block checked
with finish() == 0.  Every member keeps one position buffer; a new geometry is copied into it in front of every block
(outside the timed region).  A library without agbnp_hip_energy_group (the parent of that change) runs (a), (b) and (d): they
are the yardsticks.

Then, on trpcage version 1 with R = 4, a cross-evaluation round of an exchange matrix: every member evaluated at its
neighbour's conformation and then back at its own (conformations jittered(1000 + m, sigma=0.02): unrelated to each other), with
expect_jump() in front of both evaluations, and without it -- every evaluation withheld as a jump, read with finish() and
repeated, which is all a library without the hint can do.  Host wall-clock per round, finish() included in both.

Prints one JSON line with the library's build id.

  python scripts/energy_group_timing.py [--steps 200] [--warmup 24] [--replicas 1,2,4,8] [--systems trpcage:1,trpcage:0,1dwc:1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cross_rounds(P, torch, stream, rounds, warmup):
    """trpcage version 1, R = 4: ms of host wall-clock per cross-evaluation round, hinted and not."""
    R = 4
    sp = stream.cuda_stream
    dev = torch.device("cuda:0")
    s = P.load_system("trpcage")
    confs = [torch.tensor(s.jittered(1000 + m, sigma=0.02), dtype=torch.float64, device=dev) for m in range(R)]
    have_group, have_hint = hasattr(P, "energy_group"), hasattr(P.HipCalcAGBNPForceKernel, "expect_jump")
    result = {"R": R, "system": "trpcage", "version": 1, "call": "energy_group" if have_group else "energy_device"}
    for way in (["hint"] if have_hint else []) + ["repeat"]:
        ks = []
        for m in range(R):
            k = P.HipCalcAGBNPForceKernel(device=0)
            k.initialize(P.AGBNPForce.from_arrays(*s.params(), version=1))
            k.energy(s.jittered(1000 + m, sigma=0.02))
            ks.append(k)
        pos = torch.zeros((R, s.n, 3), dtype=torch.float64, device=dev)
        ene = torch.zeros((R,), dtype=torch.float64, device=dev)

        def evaluate(members):
            if have_group:
                P.energy_group([ks[m] for m in members], [pos[m].data_ptr() for m in members],
                               [ene[m:m + 1].data_ptr() for m in members], sp)
            else:
                for m in members:
                    ks[m].energy_device(pos[m].data_ptr(), ene[m:m + 1].data_ptr(), sp)

        times, repeats = [], 0
        for rnd in range(warmup + rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for shift in (1, 0):  # at the neighbour's conformation, then back at the member's own
                with torch.cuda.stream(stream):
                    for m in range(R):
                        pos[m].copy_(confs[(m + shift) % R])
                if way == "hint":
                    for k in ks:
                        k.expect_jump()
                todo = list(range(R))
                for attempt in range(4):
                    evaluate(todo)
                    todo = [m for m in todo if ks[m].finish(sp)]
                    if not todo:
                        break
                    repeats += len(todo) if rnd >= warmup else 0
                assert not todo, "an evaluation stayed withheld"
            if rnd >= warmup:
                times.append(1e3 * (time.perf_counter() - t0))
        result[way] = {"ms_per_round": round(float(np.median(times)), 4), "repeated_evaluations_per_round": repeats / rounds}
        for k in ks:
            k.release()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--replicas", default="1,2,4,8")
    ap.add_argument("--systems", default="trpcage:1,trpcage:0,1dwc:1", help="name:version, comma-separated")
    ap.add_argument("--cross-rounds", type=int, default=100, help="0: skip the cross-evaluation rounds")
    args = ap.parse_args()
    import torch

    import openmm_agbnp_plugin_amd as P
    from openmm_agbnp_plugin_amd import _lib

    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)  # (not the default stream: its handle is NULL, which the engine reads as its own stream)
    sp = stream.cuda_stream
    replicas = [int(r) for r in args.replicas.split(",")]
    ways = ("a", "b", "c", "d") if hasattr(P, "energy_group") else ("a", "b", "d")
    out = {"build_id": _lib.build_id(), "steps": args.steps, "warmup": args.warmup, "ways": list(ways),
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
            pp, fp, ep = [pos[m].data_ptr() for m in range(R)], [frc[m].data_ptr() for m in range(R)], [ene[m:m + 1].data_ptr() for m in range(R)]
            torch.cuda.synchronize()
            times = {w: [] for w in ways}
            kinds = {}
            for rnd in range((args.warmup + args.steps) // block + 1):
                for way in ways:
                    with torch.cuda.stream(stream):
                        for m in range(R):
                            pos[m].copy_(geoms[(rnd + m) % len(geoms)])
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record(stream)
                    if way == "b":
                        for st in side:
                            st.wait_event(t0)
                    for i in range(block):
                        if way == "c":
                            P.energy_group(ks, pp, ep, sp)
                        elif way == "d":
                            P.execute_group(ks, pp, fp, ep, sp)
                        else:
                            for m, k in enumerate(ks):
                                k.energy_device(pp[m], ep[m], side[m].cuda_stream if way == "b" else sp)
                    if way == "b":
                        for st in side:
                            e = torch.cuda.Event()
                            e.record(st)
                            stream.wait_event(e)
                    t1.record(stream)
                    for m, k in enumerate(ks):
                        assert k.finish(side[m].cuda_stream if way == "b" else sp) == 0, "an evaluation was withheld"
                    if way in ("c", "d"):
                        kinds[way] = int(ks[0].scalar("group_members"))
                    if rnd * block >= args.warmup:
                        times[way].append(t0.elapsed_time(t1) / block)
            torch.cuda.synchronize()
            row = {"system": name, "version": version, "atoms": s.n, "R": R, "group_members": kinds}
            if "group_block_writes" in P.HipCalcAGBNPForceKernel.SCALARS:
                row["group_block_writes"] = int(ks[0].scalar("group_block_writes"))
            for way, v in times.items():
                ms = float(np.median(v))
                row[way] = {"ms_per_round": round(ms, 5), "ms_per_replica_eval": round(ms / R, 5)}
            out["results"].append(row)
            for k in ks:
                k.release()
    if args.cross_rounds > 0:
        out["cross"] = cross_rounds(P, torch, stream, args.cross_rounds, 10)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
