#!/usr/bin/env python3
"""Python's share of a call through the host mirror, measured on the CPU: `_lib.load` answers with the recording library of
tests/test_python_marshalling.py (recording off), so what is timed is argument checking and marshalling alone.  execute_device,
energy_device, execute_group (4 members) and binding_execute_group (4 bindings): the best of `--repeats` runs of `--calls` calls
each, in microseconds per call.  With `--against DIR` (a checkout of another commit) the same for that tree's package, in this
process, the repeats of the two alternating: on a busy host many short repeats (--calls 2000 --repeats 300) separate the two
trees where five long ones do not.  Prints one JSON line.

  python scripts/python_overhead.py [--calls 100000] [--repeats 5] [--against DIR]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ways(root, recorder, members):
    """The four calls through the package of the tree at `root`."""
    for name in [name for name in sys.modules if name.startswith("openmm_agbnp_plugin_amd")]:
        del sys.modules[name]
    sys.path.insert(0, root)
    P = importlib.import_module("openmm_agbnp_plugin_amd")
    sys.path.remove(root)
    assert os.path.samefile(os.path.dirname(os.path.dirname(P.__file__)), root)
    sys.modules["openmm_agbnp_plugin_amd._lib"].load = lambda: recorder

    def member(cls, handle):
        m = object.__new__(cls)
        m._h, m.numParticles = C.c_void_p(handle), 304
        members.append(m)
        return m
    k = member(P.HipCalcAGBNPForceKernel, 0x5000)
    ks = [member(P.HipCalcAGBNPForceKernel, 0x5000 + i) for i in range(4)]
    bs = [member(P.BindingEnergy, 0x6000 + i) for i in range(4)]
    pos, frc, ene, u = [1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12], [13, 14, 15, 16]
    return dict(execute_device=lambda: k.execute_device(1, 2, 3, 44),
                energy_device=lambda: k.energy_device(1, 3, 44),
                execute_group=lambda: P.execute_group(ks, pos, frc, ene, 44),
                binding_execute_group=lambda: P.binding_execute_group(bs, pos, 99, frc, ene, u, 44))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--against", default=None)
    args = ap.parse_args()
    from tests.test_python_marshalling import Recorder
    recorder, members = Recorder(record=False), []
    trees = {"this": ways(ROOT, recorder, members)}
    if args.against:
        trees["against"] = ways(os.path.abspath(args.against), recorder, members)
    best = {tree: dict.fromkeys(calls, float("inf")) for tree, calls in trees.items()}
    for _ in range(args.repeats):
        for tree, calls in trees.items():
            for name, call in calls.items():
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    call()
                best[tree][name] = min(best[tree][name], time.perf_counter() - t0)
    for m in members:  # (the handles were never the library's)
        m._h = None
    out = {tree: {name: round(1e6 * t / args.calls, 3) for name, t in row.items()} for tree, row in best.items()}
    print(json.dumps({"us_per_call": out, "calls": args.calls, "repeats": args.repeats}))


if __name__ == "__main__":
    main()
