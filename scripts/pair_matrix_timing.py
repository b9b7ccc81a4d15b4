#!/usr/bin/env python3
"""What a set-pair interaction matrix costs (include/agbnp_hip.h: agbnp_hip_pair_matrix_device), and that adding it
has left the full evaluation alone.

(a) In one child process per case: microseconds per pair_matrix_device() call beside decompose_device() on the same build and
    context, `--evaluations` calls enqueued on one stream at one geometry and ONE synchronise at the end, the two kinds
    alternating over `--repeats` repeats.  The two calls differ in their last launch alone (k_pair_matrix, k_decompose), so the
    difference of the columns is the difference of those launches.  Cases: trpcage with its 20 residues and with every atom its
    own set (S = N = 272), 1dwc (thrombin) with its 258 residues (tests/golden/residues_*.txt).
(b) With --parent-library (a libagbnp_hip.so built from the parent commit): execute_device() of this build and of the parent's,
    each in a fresh child process, alternating, `--repeats` processes each, as scripts/decompose_timing.py does it (its code):
    the two must agree within the run-to-run spread.
Version 1, NoCutoff, Reference mode; every figure is a host clock around work that ends in a synchronise.  This process only
starts the children (it never opens the device itself).  Prints a table and one JSON line with the library's build id.

  python scripts/pair_matrix_timing.py [--evaluations 2000] [--repeats 5] [--parent-library PATH]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from decompose_timing import cell, timed_execute  # noqa: E402

CASES = {"trpcage residues": ("trpcage", "residues"), "trpcage S = N": ("trpcage", "atoms"), "1dwc residues": ("1dwc", "residues")}


def timed_calls(name, partition, evaluations, repeats):
    """(atoms, sets, {kind: [us per call, one figure per repeat]}) for one case, the kinds alternating."""
    import numpy as np
    import torch

    import openmm_agbnp_plugin_amd as P

    s = P.load_system(name)
    if partition == "residues":
        sets, labels = P.load_sets(os.path.join(ROOT, "tests", "golden", f"residues_{name}.txt"))
        num_sets = len(labels)
    else:
        sets, num_sets = np.arange(s.n), s.n
    k = P.HipCalcAGBNPForceKernel(device=0)
    k.initialize(P.AGBNPForce.from_arrays(*s.params(), version=1))
    k.set_atom_sets(sets, num_sets)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    pos = torch.tensor(s.pos, dtype=torch.float64, device=dev).contiguous()
    ene = torch.zeros((1,), dtype=torch.float64, device=dev)
    per_atom = torch.zeros((4, s.n), dtype=torch.float64, device=dev)
    matrix = torch.zeros((num_sets, num_sets), dtype=torch.float64, device=dev)
    call = {
        "decompose": lambda: k.decompose_device(pos.data_ptr(), per_atom.data_ptr(), ene.data_ptr(), stream),
        "pair_matrix": lambda: k.pair_matrix_device(pos.data_ptr(), matrix.data_ptr(), ene.data_ptr(), stream),
    }
    k.execute(s.pos, np.zeros((s.n, 3)))  # (settles the capacity variant and the first masks)
    for kind in call:  # warm-up: every kernel of every kind has run
        for _ in range(20):
            call[kind]()
    if k.finish(stream) != 0:
        raise SystemExit(f"{name}: warm-up evaluations were withheld")
    out = {kind: [] for kind in call}
    for _ in range(repeats):
        for kind in call:
            torch.cuda.synchronize()
            start = time.perf_counter()
            for _ in range(evaluations):
                call[kind]()
            torch.cuda.synchronize()
            out[kind].append(1e6 * (time.perf_counter() - start) / evaluations)
            if k.finish(stream) != 0:
                raise SystemExit(f"{name}: {kind} evaluations were withheld")
    return int(s.n), int(num_sets), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--evaluations", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)  # one case's figures as a JSON line
    ap.add_argument("--execute", default=None, help=argparse.SUPPRESS)  # one system's execute_device figures as a JSON line
    args = ap.parse_args()
    from openmm_agbnp_plugin_amd import _lib
    if args.child:
        n, sets, figures = timed_calls(*CASES[args.child], args.evaluations, args.repeats)
        print(json.dumps(dict(atoms=n, sets=sets, figures=figures, build_id=_lib.build_id())))
        return
    if args.execute:
        n, figures, build = timed_execute(args.execute, os.environ.get("AGBNP_HIP_LIBRARY") or _lib.LIB_PATH, args.evaluations)
        print(json.dumps(dict(atoms=n, figures=figures, build_id=build)))
        return

    def child(flag, what, library=None):
        env = dict(os.environ)
        env.pop("AGBNP_HIP_LIBRARY", None)
        if library:
            env["AGBNP_HIP_LIBRARY"] = os.path.abspath(library)
        done = subprocess.run([sys.executable, os.path.abspath(__file__), flag, what, "--evaluations", str(args.evaluations),
                               "--repeats", str(args.repeats)], env=env, capture_output=True, text=True, timeout=600)
        if done.returncode != 0:
            raise SystemExit(f"{what}: child ended with {done.returncode}\n{done.stderr[-2000:]}")
        return json.loads(done.stdout.strip().splitlines()[-1])

    out = {"build_id": None, "evaluations": args.evaluations, "results": []}
    print("| case | atoms | sets | decompose_device, us | pair_matrix_device, us | difference, us |")
    print("|---|---|---|---|---|---|")
    for case in CASES:
        got = child("--child", case)
        figures, out["build_id"] = got["figures"], got["build_id"]
        extra = (sum(figures["pair_matrix"]) - sum(figures["decompose"])) / args.repeats
        out["results"].append(dict(case=case, atoms=got["atoms"], sets=got["sets"], decompose_us=figures["decompose"],
                                   pair_matrix_us=figures["pair_matrix"]))
        print(f"| {case} | {got['atoms']} | {got['sets']} | {cell(figures['decompose'])} | {cell(figures['pair_matrix'])} | {extra:.1f} |",
              flush=True)
    if args.parent_library:
        print()
        print("| system | execute_device, this build, us | execute_device, parent build, us |")
        print("|---|---|---|")
        for name in ("trpcage", "1dwc"):
            sides, builds = {"new": [], "parent": []}, {}
            for _ in range(args.repeats):
                for side, library in (("new", None), ("parent", args.parent_library)):
                    got = child("--execute", name, library)
                    sides[side] += got["figures"]["execute"]
                    builds[side] = got["build_id"]
            out["results"].append(dict(system=name, execute_us=sides["new"], parent_execute_us=sides["parent"], parent_build_id=builds["parent"]))
            print(f"| {name} | {cell(sides['new'])} | {cell(sides['parent'])} |", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
