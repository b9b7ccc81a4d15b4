#!/usr/bin/env python3
"""What the perturbation energies cost (include/agbnp_hip.h: agbnp_hip_perturbed_energies_device), beside what
gives the same answer without them, and that adding them has left the full evaluation alone.

(a) In one child process per system and number of sets M (1, 4, 8, 16: every compiled tier, and one set in the smallest):
    microseconds per call of
      perturbed    perturbed_energies_device() with M sets -- M energies from ONE evaluation
      decompose    decompose_device() on the same kernel: the same evaluation plus a launch of the same grid
      group        energy_group() over M separately created kernels, one per set, at the same position buffer: what gives the same
                   M energies without this call
    `--evaluations` calls enqueued on one stream at one geometry and ONE synchronise at the end, the kinds alternating over
    `--repeats` repeats, all three on ONE side stream (torch's default stream has the handle 0, which the library takes for a
    context's own stream: a group call on it joins every member's stream to the first one's, which the single-context calls do
    not pay).  The child also checks that `perturbed` and `group` agree to 1e-7 (scaled) before it times anything, and reports
    scalar 19 of the group's members behind a group call (M: they shared one launch set).
(b) With --parent-library (a libagbnp_hip.so built from the parent commit): execute_device() of this build and of the parent's,
    each in a fresh child process, alternating (timing_support.parent_table: nothing on the MD path may move).
Version 1, NoCutoff, Reference mode; every figure is a host clock around work that ends in a synchronise.  This process only
starts the children.  Prints a table and one JSON line with the library's build id.

  python scripts/perturbation_timing.py [--evaluations 1000] [--repeats 5] [--systems trpcage,1dwc] [--sets 1,4,8,16] [--parent-library PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from timing_support import cell, parent_table, run_child, timed  # noqa: E402


def ladder(s, count):
    """A charge-scaling ladder q (1 - 0.05 m); gamma and alpha are the system's own."""
    import numpy as np

    return [(s.gamma, s.alpha, (1.0 - 0.05 * m) * np.asarray(s.charge)) for m in range(count)]


def timed_calls(name, count, evaluations, repeats):
    import numpy as np
    import torch

    import openmm_agbnp_plugin_amd as P

    s = P.load_system(name)
    sets = ladder(s, count)
    k = P.HipCalcAGBNPForceKernel(device=0)
    k.initialize(P.AGBNPForce.from_arrays(*s.params(), version=1))
    k.set_parameter_sets(*[np.array([x[i] for x in sets]) for i in range(3)])
    members = []
    for g, a, q in sets:
        member = P.HipCalcAGBNPForceKernel(device=0)
        member.initialize(P.AGBNPForce.from_arrays(s.radius, g, a, q, s.ishydrogen, version=1))
        members.append(member)
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream()  # (see above: not the handle 0)
    stream = side.cuda_stream
    pos = torch.tensor(s.pos, dtype=torch.float64, device=dev).contiguous()
    ene = torch.zeros((1,), dtype=torch.float64, device=dev)
    out = torch.zeros((count,), dtype=torch.float64, device=dev)
    per_atom = torch.zeros((4, s.n), dtype=torch.float64, device=dev)
    words = torch.zeros((count,), dtype=torch.float64, device=dev)
    word_ptrs = [words.data_ptr() + 8 * m for m in range(count)]
    call = {
        "perturbed": lambda: k.perturbed_energies_device(pos.data_ptr(), out.data_ptr(), ene.data_ptr(), stream),
        "decompose": lambda: k.decompose_device(pos.data_ptr(), per_atom.data_ptr(), ene.data_ptr(), stream),
        "group": lambda: P.energy_group(members, [pos.data_ptr()] * count, word_ptrs, stream),
    }
    for kernel in [k] + members:  # (settles the capacity variant and the first masks)
        kernel.execute(s.pos, np.zeros((s.n, 3)))

    def finish_all(what):
        if any(kernel.finish(stream) != 0 for kernel in [k] + members):
            raise SystemExit(f"{name}: {what} evaluations were withheld")

    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        call["perturbed"]()
        call["group"]()
        torch.cuda.synchronize()
        finish_all("first")
        differ = float(((out - words).abs() / torch.clamp(1e-3 * words.abs(), min=1.0)).max())
        if differ > 1e-7:
            raise SystemExit(f"{name}: the perturbed energies differ from the {count} kernels' by {differ:.3e}")
        figures = timed(call, tuple(call), evaluations, repeats, finish_all)
        call["group"]()
        shared = [int(member.scalar("group_members")) for member in members]
        finish_all("closing")
    return int(s.n), figures, differ, shared


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--evaluations", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--systems", default="trpcage,1dwc")
    ap.add_argument("--sets", default="1,4,8,16")
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)  # one system's figures as a JSON line
    ap.add_argument("--count", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        from openmm_agbnp_plugin_amd import _lib

        n, figures, differ, shared = timed_calls(args.child, args.count, args.evaluations, args.repeats)
        print(json.dumps(dict(atoms=n, figures=figures, differ=differ, group_members=shared, build_id=_lib.build_id())))
        return
    out = {"build_id": None, "evaluations": args.evaluations, "results": []}
    print("| system | atoms | M | perturbed_energies_device, us | decompose_device, us | energy_group of M kernels, us | group / perturbed | scalar 19 of the group's members |")
    print("|---|---|---|---|---|---|---|---|")
    for name in args.systems.split(","):
        for count in [int(c) for c in args.sets.split(",")]:
            got = run_child("perturbation_timing.py", ["--child", name, "--count", str(count), "--repeats", str(args.repeats)], args.evaluations)
            f, out["build_id"] = got["figures"], got["build_id"]
            ratio = sum(f["group"]) / sum(f["perturbed"])
            out["results"].append(dict(system=name, atoms=got["atoms"], sets=count, differ=got["differ"], group_members=got["group_members"],
                                       **{k + "_us": v for k, v in f.items()}))
            shared = sorted(set(got["group_members"]))
            print(f"| {name} | {got['atoms']} | {count} | {cell(f['perturbed'])} | {cell(f['decompose'])} | {cell(f['group'])} | {ratio:.2f} | {shared} |", flush=True)
    if args.parent_library:
        parent_table(args.systems.split(","), args.parent_library, args.repeats, args.evaluations, out["results"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
