#!/usr/bin/env python3
"""What a per-atom decomposition costs (include/agbnp_hip.h: agbnp_hip_decompose_device), and that adding it has
left the full evaluation alone.

(a) In one child process per system: microseconds per decompose_device() call beside energy_device() on the same build, `--evaluations`
    calls enqueued on one stream at one geometry and ONE synchronise at the end, the two kinds alternating over `--repeats`
    repeats.  The difference is the decomposition's one extra launch and the enlarged-radius self volumes of its cavity launch.
(b) With --parent-library (a libagbnp_hip.so built from the parent commit): execute_device() of this build and of the parent's,
    each in a fresh child process (AGBNP_HIP_LIBRARY names the library of a process), alternating, `--repeats` processes each;
    the table gives each side's mean and its run-to-run spread (max - min): the existing instantiations are untouched, so the
    two must agree within that spread.
Version 1, NoCutoff, Reference mode; every figure is a host clock around work that ends in a synchronise.  This process only
starts the children (it never opens the device itself).  Prints a table and one JSON line with the library's build id.

  python scripts/decompose_timing.py [--evaluations 2000] [--repeats 5] [--systems trpcage,1dwc] [--parent-library PATH]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed_calls(name, kinds, evaluations, repeats):
    """{kind: [us per call, one figure per repeat]} for one system, the kinds alternating."""
    import numpy as np
    import torch

    import openmm_agbnp_plugin_amd as P

    s = P.load_system(name)
    k = P.HipCalcAGBNPForceKernel(device=0)
    k.initialize(P.AGBNPForce.from_arrays(*s.params(), version=1))
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    pos = torch.tensor(s.pos, dtype=torch.float64, device=dev).contiguous()
    frc = torch.zeros((s.n, 3), dtype=torch.float64, device=dev)
    ene = torch.zeros((1,), dtype=torch.float64, device=dev)
    per_atom = torch.zeros((4, s.n), dtype=torch.float64, device=dev)
    call = {
        "execute": lambda: k.execute_device(pos.data_ptr(), frc.data_ptr(), ene.data_ptr(), stream),
        "energy": lambda: k.energy_device(pos.data_ptr(), ene.data_ptr(), stream),
        "decompose": lambda: k.decompose_device(pos.data_ptr(), per_atom.data_ptr(), ene.data_ptr(), stream),
    }
    k.execute(s.pos, np.zeros((s.n, 3)))  # (settles the capacity variant and the first masks)
    for kind in kinds:  # warm-up: every kernel of every kind has run
        for _ in range(20):
            call[kind]()
    if k.finish(stream) != 0:
        raise SystemExit(f"{name}: warm-up evaluations were withheld")
    out = {kind: [] for kind in kinds}
    for _ in range(repeats):
        for kind in kinds:
            torch.cuda.synchronize()
            start = time.perf_counter()
            for _ in range(evaluations):
                call[kind]()
            torch.cuda.synchronize()
            out[kind].append(1e6 * (time.perf_counter() - start) / evaluations)
            if k.finish(stream) != 0:
                raise SystemExit(f"{name}: {kind} evaluations were withheld")
    return int(s.n), out


def timed_execute(name, library, evaluations):
    """[us per execute_device call] through the C ABI alone (the symbols that the parent's library has too), for part (b)."""
    import ctypes as C

    import numpy as np
    import torch

    import openmm_agbnp_plugin_amd as P
    from openmm_agbnp_plugin_amd import _lib

    _lib._share_hip_runtime_with_torch()
    lib = C.CDLL(library)
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
    lib.agbnp_hip_create.argtypes = [C.POINTER(vp), C.c_int, dp, dp, dp, dp, ip, C.c_int, C.c_int, C.c_double, C.c_int]
    lib.agbnp_hip_execute_host.argtypes = [vp, dp, dp, dp]
    lib.agbnp_hip_execute_device.argtypes = [vp, vp, vp, vp, vp]
    lib.agbnp_hip_finish.argtypes = [vp, vp, ip]
    lib.agbnp_hip_destroy.argtypes = [vp]
    lib.agbnp_hip_build_id.restype = C.c_char_p
    s = P.load_system(name)
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in s.params()[:4]] + [np.ascontiguousarray(s.ishydrogen, dtype=np.int32)]
    h = vp()
    if lib.agbnp_hip_create(C.byref(h), s.n, *[a.ctypes.data_as(dp) for a in arrays[:4]], arrays[4].ctypes.data_as(ip), 1, 0, 1.0, 0) != 0:
        raise SystemExit(f"{name}: agbnp_hip_create failed")
    dev = torch.device("cuda:0")
    stream = vp(torch.cuda.current_stream().cuda_stream)
    pos = torch.tensor(s.pos, dtype=torch.float64, device=dev).contiguous()
    frc = torch.zeros((s.n, 3), dtype=torch.float64, device=dev)
    ene = torch.zeros((1,), dtype=torch.float64, device=dev)
    hpos, hfrc, e, rep = np.ascontiguousarray(s.pos, dtype=np.float64), np.zeros((s.n, 3)), C.c_double(0.0), C.c_int(0)
    lib.agbnp_hip_execute_host(h, hpos.ctypes.data_as(dp), hfrc.ctypes.data_as(dp), C.byref(e))
    figures = []
    for timed in (False, True):  # (the first round is the warm-up)
        torch.cuda.synchronize()
        start = time.perf_counter()
        for _ in range(evaluations if timed else 20):
            if lib.agbnp_hip_execute_device(h, vp(pos.data_ptr()), vp(frc.data_ptr()), vp(ene.data_ptr()), stream) != 0:
                raise SystemExit(f"{name}: agbnp_hip_execute_device failed")
        torch.cuda.synchronize()
        if timed:
            figures.append(1e6 * (time.perf_counter() - start) / evaluations)
        if lib.agbnp_hip_finish(h, stream, C.byref(rep)) != 0 or rep.value != 0:
            raise SystemExit(f"{name}: execute evaluations were withheld")
    build = lib.agbnp_hip_build_id().decode()
    lib.agbnp_hip_destroy(h)
    return int(s.n), {"execute": figures}, build


def cell(v):
    return f"{sum(v) / len(v):.1f} (spread {max(v) - min(v):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--evaluations", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--systems", default="trpcage,1dwc")
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)  # one system's figures of --kinds as a JSON line
    ap.add_argument("--kinds", default="execute", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        from openmm_agbnp_plugin_amd import _lib

        if args.kinds == "execute":
            n, figures, build = timed_execute(args.child, os.environ.get("AGBNP_HIP_LIBRARY") or _lib.LIB_PATH, args.evaluations)
        else:
            n, figures = timed_calls(args.child, args.kinds.split(","), args.evaluations, args.repeats)
            build = _lib.build_id()
        print(json.dumps(dict(atoms=n, figures=figures, build_id=build)))
        return

    def child(name, kinds, repeats, library=None):
        env = dict(os.environ)
        env.pop("AGBNP_HIP_LIBRARY", None)
        if library:
            env["AGBNP_HIP_LIBRARY"] = os.path.abspath(library)
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--kinds", kinds, "--evaluations", str(args.evaluations),
                               "--repeats", str(repeats)], env=env, capture_output=True, text=True, timeout=600)
        if done.returncode != 0:
            raise SystemExit(f"{name} {kinds}: child ended with {done.returncode}\n{done.stderr[-2000:]}")
        return json.loads(done.stdout.strip().splitlines()[-1])

    out = {"build_id": None, "evaluations": args.evaluations, "results": []}
    print("| system | atoms | energy_device, us | decompose_device, us | extra, us |")
    print("|---|---|---|---|---|")
    for name in args.systems.split(","):
        got = child(name, "energy,decompose", args.repeats)
        n, figures, out["build_id"] = got["atoms"], got["figures"], got["build_id"]
        extra = sum(figures["decompose"]) / args.repeats - sum(figures["energy"]) / args.repeats
        out["results"].append(dict(system=name, atoms=n, energy_us=figures["energy"], decompose_us=figures["decompose"]))
        print(f"| {name} | {n} | {cell(figures['energy'])} | {cell(figures['decompose'])} | {extra:.1f} |", flush=True)
    if args.parent_library:
        print()
        print("| system | execute_device, this build, us | execute_device, parent build, us |")
        print("|---|---|---|")
        for name in args.systems.split(","):
            sides, builds = {"new": [], "parent": []}, {}
            for _ in range(args.repeats):
                for side, library in (("new", None), ("parent", args.parent_library)):
                    got = child(name, "execute", 1, library)
                    sides[side] += got["figures"]["execute"]
                    builds[side] = got["build_id"]
            out["results"].append(dict(system=name, execute_us=sides["new"], parent_execute_us=sides["parent"], parent_build_id=builds["parent"]))
            print(f"| {name} | {cell(sides['new'])} | {cell(sides['parent'])} |", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
